"""CPU: the matching rule of closed-loop pose commands (tests/closed_loop_ref.py restates k_command_rows in float64), the cases
the GPU test runs, and the C boundary of infgen_command_rows."""
import ctypes as C
import os
import re

import numpy as np

import closed_loop_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_token_whose_integration_is_the_command_costs_nothing_and_wins():
    vocab = ref.vocabularies()[0]
    rng = np.random.default_rng(3)
    for ty in range(3):
        last = vocab[ty, :, 5]
        for k in rng.integers(0, last.shape[0], 8):
            pos, head = rng.uniform(-50, 50, 2), rng.uniform(-3, 3)
            # the command IS token k's world contour: its centre, its heading and the box it was made of
            w = ref.world_contours(last[k][None], pos, head)[0]
            x, y, h = ref.integrate(last[k], pos, head)
            length = np.hypot(*(w[0] - w[3])); width = np.hypot(*(w[0] - w[1]))
            assert np.abs(ref.box_contour(x, y, h, width, length) - w).max() < 1e-5          # (the tokens are rigid boxes)
            tok, cost, gap = ref.match(last, pos, head, (x, y, h), width, length)
            assert tok == k and cost < 1e-4 and gap > 1e-3, (ty, k, tok, cost, gap)


def test_ties_go_to_the_first_index():
    vocab = ref.vocabularies()[1]
    last = vocab[0, :, 5].copy()
    last[700] = last[40]; last[41] = last[40]           # three equal tokens
    x, y, h = ref.integrate(last[40], (3.0, -2.0), 0.4)
    tok, cost, gap = ref.match(last, (3.0, -2.0), 0.4, (x + 0.01, y, h), 2.0, 4.8)
    assert tok == 40 and gap == 0.0
    c = ref.costs(last, (3.0, -2.0), 0.4, (x + 0.01, y, h), 2.0, 4.8)
    assert c[40] == c[41] == c[700] == cost


def test_the_restatement_decides_the_gpu_cases():
    cases = ref.kernel_cases()
    share, n = ref.decided_share(cases)
    print(f'{n} matched rows, {100 * share:.1f} % decided beyond the margin; margins {sorted({k["margin"] for _, k in cases})}')
    assert n >= 100 and share >= 0.98
    sizes = {v.shape[1] for v, _ in cases}
    assert any(s % 256 for s in sizes) and 2048 in sizes
    for _, k in cases:
        assert set(np.unique(k['atype'])) == {0, 1, 2}
        f, w = k['flag'].astype(bool), k['written']
        assert f[0, 0] and f[1, 0] and f[0, 10] and f[1, 15] and f[0, 12] and not w[0, 12]        # first, last valid, beyond n_agents
        assert w[1, 3] and not k['matched'][1, 3] and w[1, 7] and not k['matched'][1, 7]            # no command / already invalid
        assert (k['exp_tok'][w & ~k['matched']] == -1).all() and (k['exp_state'][k['matched']] == ref.VALID).all()
        assert k['margin'] < 1e-3 and 0 < k['cost'][k['matched']].max() < 4 * 0.6


def test_header_and_binding_declare_the_entry_and_the_context_is_unchanged():
    from infgen_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    m = re.search(r'int infgen_command_rows\(([^;]*)\);', hdr)
    assert m, 'include/infgen_hip.h declares infgen_command_rows'
    args = m.group(1)
    for name in ('const InfgenRollout* r', 'int t', 'int kind', 'cmd_token', 'cmd_pose', 'cmd_mask', 'shape', 'cmd_cost', 'void* stream'):
        assert name in args, name
    lib = _lib.load()
    assert lib.infgen_command_rows.argtypes is not None and len(lib.infgen_command_rows.argtypes) == 9
    # InfgenRollout did not grow: the size the parent commit's binding had, and the ABI version the older tests pin
    assert C.sizeof(_lib.Rollout) == 1272 == lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT)
    assert lib.infgen_layout_query(_lib.Q_ABI_VERSION) == 1
    # refused without a plan to write (no launch happens: this runs without a GPU)
    r = _lib.Rollout()
    r.S, r.A_cap, r.T, r.token_size = 1, 16, 4, 8
    assert lib.infgen_command_rows(C.byref(r), 0, 0, None, None, None, None, None, None) != 0
    assert b'replay_row' in lib.infgen_last_error()
