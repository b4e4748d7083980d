"""CPU: the pure-torch side of the per-token log-probabilities (infgen_amd/logprob.py) and the ABI additions."""
import math
import os
import re

import numpy as np
import torch

from conftest import REPO


def test_mask_helper_on_a_hand_written_case():
    """4 rows x 5 columns, 2 history columns, 3 decode steps: a plain row, a row inserted at step 2 (bos column 3: decoded from
    column 4 on), a row whose second decoded token is -1, a replayed row"""
    from infgen_amd import logprob
    tok = torch.tensor([[5, 6, 7, 8, 9],
                        [-1, -1, -1, -1, 3],
                        [1, 2, 3, -1, 4],
                        [9, 9, 9, 9, 9]])
    first = torch.tensor([2, 4, 2, 2])
    forced = torch.tensor([False, False, False, True])
    m = logprob.logprob_mask(tok, first, 2, 3, forced)
    want = torch.tensor([[0, 0, 1, 1, 1],
                         [0, 0, 0, 0, 1],
                         [0, 0, 1, 0, 1],
                         [0, 0, 0, 0, 0]], dtype=torch.bool)
    assert m.dtype == torch.bool and torch.equal(m, want)
    # fewer decode steps than columns left: the columns beyond them are not decoded ones
    assert torch.equal(logprob.logprob_mask(tok, first, 2, 2, forced), want & torch.tensor([1, 1, 1, 1, 0], dtype=torch.bool))
    assert torch.equal(logprob.logprob_mask(tok, first, 2, 3), want | torch.tensor([[0] * 5] * 3 + [[0, 0, 1, 1, 1]], dtype=torch.bool))
    # a leading batch dimension
    mb = logprob.logprob_mask(tok[None].repeat(2, 1, 1), first[None].repeat(2, 1), 2, 3, forced[None].repeat(2, 1))
    assert torch.equal(mb[0], want) and torch.equal(mb[1], want)

    lp = -torch.arange(20, dtype=torch.float32).reshape(4, 5) / 7
    pp = logprob.pred_prob(lp, m, 2, 3)
    assert pp.shape == (4, 3)
    assert torch.equal(pp, torch.where(want[:, 2:], torch.exp(lp[:, 2:]), torch.zeros(())))
    total = logprob.rollout_logprob(lp, m)
    assert total.dtype == torch.float64 and total.shape == ()
    exact = math.fsum(float(v) for v in lp[want])
    assert abs(float(total) - exact) <= 5 * 2.0 ** -53 * float(lp[want].abs().double().sum())


def test_fixed_order_sum_ignores_trailing_padding():
    from infgen_amd import logprob
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(8, 18, generator=g) * -9).float()
    m = torch.rand(8, 18, generator=g) < 0.7
    a = logprob.rollout_logprob(x, m)
    xp = torch.cat([x, torch.full((24, 18), -3.0)])             # a padded layout: 24 more rows, masked out
    mp = torch.cat([m, torch.zeros(24, 18, dtype=torch.bool)])
    b = logprob.rollout_logprob(torch.stack([xp, xp]), torch.stack([mp, mp]))
    assert b.shape == (2,) and float(b[0]) == float(a) and float(b[1]) == float(a)       # bitwise
    assert abs(float(a) - math.fsum(float(v) for v in x[m])) <= 8 * 2.0 ** -53 * float(x[m].abs().double().sum())
    assert float(logprob.rollout_logprob(x, torch.zeros_like(m))) == 0.0


def test_rollout_struct_carries_the_new_field():
    """the new pointer is the last one the struct gained: only the two ablation switches, which an older test pins as the
    struct's final members, follow it; the library and the binding agree on the size"""
    from infgen_amd import _lib
    names = [f[0] for f in _lib.Rollout._fields_]
    assert names[-3:] == ['token_logprob', 'no_grid_token', 'no_state_token']
    assert dict(_lib.Rollout._fields_)['token_logprob'] is _lib._p
    assert _lib.Rollout.token_logprob.offset + 16 == _lib.C.sizeof(_lib.Rollout)
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT) == _lib.C.sizeof(_lib.Rollout)
    assert lib.infgen_layout_query(_lib.Q_ABI_VERSION) == 1
    for sym in ('infgen_token_logprob', 'infgen_heads_logprob'):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym)


def test_header_declares_the_new_entries():
    with open(os.path.join(REPO, 'include', 'infgen_hip.h')) as f:
        h = f.read()
    assert re.search(r'int\s+infgen_token_logprob\(const float\* logits, int rows, int n, const int\* token, float\* out, void\* stream\);', h)
    assert re.search(r'int\s+infgen_heads_logprob\([^;]*float\* token_logprob, void\* stream\);', h)
    body = h[h.index('typedef struct InfgenRollout {'):h.index('} InfgenRollout;')]
    decls = [d.strip() for d in re.sub(r'/\*.*?\*/', '', body, flags=re.S).split(';') if d.strip()]
    assert decls[-3:] == ['float* token_logprob', 'int no_grid_token', 'int no_state_token']


def test_argument_checks_need_no_device():
    """the entries refuse bad arguments before anything is launched"""
    from infgen_amd import _lib
    lib = _lib.load()
    x = np.zeros(8, np.float32)
    p = x.ctypes.data
    assert lib.infgen_token_logprob(None, 2, 4, p, p, None) != 0 and b'null pointer' in lib.infgen_last_error()
    assert lib.infgen_token_logprob(p, 2, 0, p, p, None) != 0 and b'n must be positive' in lib.infgen_last_error()
    assert lib.infgen_token_logprob(None, 0, 4, None, None, None) == 0            # no rows: nothing to do
    assert lib.infgen_heads_logprob(p, 4, p, p, 128, p, p, p, None, None) != 0 and b'token_logprob is NULL' in lib.infgen_last_error()
    # 4 rows take k_heads under the default by-size rule: without a logits buffer the call is refused, not launched
    assert lib.infgen_heads_logprob(p, 4, p, p, 128, None, p, p, p, None) != 0 and b'needs a logits buffer' in lib.infgen_last_error()
