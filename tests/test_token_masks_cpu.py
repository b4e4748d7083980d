"""CPU: the host side of constrained decoding (infgen_amd/constraints.py, the engine's argument checks, the C ABI's struct).
Everything here is checked before any launch, so none of it needs a GPU."""
import ctypes as C

import numpy as np
import pytest

from infgen_amd import constraints as tc
from infgen_amd import synth


@pytest.fixture(scope='module')
def vocab():
    return synth.make_agent_vocab(2048)


def test_bit_packing_round_trips():
    rng = np.random.default_rng(5)
    for n in (32, 128, 2048):
        a = rng.random((7, n)) < 0.4
        a[0] = True
        a[1] = False
        a[1, n - 1] = True
        w = tc.pack_bits(a)
        assert w.dtype == np.uint32 and w.shape == (7, n // 32)
        assert np.array_equal(tc.unpack_bits(w), a)
        # the documented bit order: token c is bit c % 32 of little-endian word c / 32
        for s, c in ((2, 0), (3, 31), (4, 32 % n), (5, n - 1), (6, 45 % n)):
            assert bool((int(w[s, c // 32]) >> (c % 32)) & 1) == bool(a[s, c])
        assert (w[0] == 0xffffffff).all() and int(w[1, -1]) == 1 << 31 and not w[1, :-1].any()
        m = tc.TokenMasks(a)
        assert np.array_equal(m.allowed, a) and m.n_sets == 7 and m.token_size == n
        bits = m.bits
        assert str(bits.dtype) == 'torch.uint32' and tuple(bits.shape) == (7, n // 32)
        assert np.array_equal(bits.view(dtype=__import__('torch').int32).numpy().view(np.uint32), w)


def _kinematics(vocab):
    """a plain restatement: the last contour's centre and heading (rear-left -> front-left corner) per type and token"""
    out = []
    for name in ('veh', 'ped', 'cyc'):
        last = vocab[name][:, 5].astype(np.float64)                    # [token][4][2]
        cx, cy = last[:, :, 0].mean(1), last[:, :, 1].mean(1)
        yaw = np.arctan2(last[:, 0, 1] - last[:, 3, 1], last[:, 0, 0] - last[:, 3, 0])
        out.append((cx / 0.5, np.sqrt(cx * cx + cy * cy) / 0.5, yaw / 0.5))
    return out


def test_from_vocab_against_numpy(vocab):
    kin = _kinematics(vocab)
    # the synthetic vocabulary is built from (displacement, yaw change) grids: the derived quantities are those, up to rounding
    k = np.arange(2048)
    dth = ((k % 32) / 31.0 - 0.5) * 2.0 * 0.9
    assert np.abs(kin[0][2] * 0.5 - dth).max() < 1e-5
    for rules, want in (
            ({'max_speed': 3.0}, [kin[t][1] <= 3.0 for t in range(3)]),
            ({'min_speed': 1.0}, [kin[t][1] >= 1.0 for t in range(3)]),
            ({'no_reverse': True}, [kin[t][0] >= 0.0 for t in range(3)]),
            ({'max_yaw_rate': 0.4}, [np.abs(kin[t][2]) <= 0.4 for t in range(3)]),
            ({'max_speed': 8.0, 'no_reverse': True, 'max_yaw_rate': 1.0},
             [(kin[t][1] <= 8.0) & (kin[t][0] >= 0.0) & (np.abs(kin[t][2]) <= 1.0) for t in range(3)])):
        m = tc.TokenMasks.from_vocab(vocab, rules)
        assert m.n_sets == 3 and m.type_sets == [0, 1, 2], rules
        for t in range(3):
            assert np.array_equal(m.allowed[t], want[t]), (rules, t)
            assert 0 < want[t].sum(), rules
        assert any(w.sum() < 2048 for w in want), (rules, 'the rule constrains something')
    # per type: only the named types get a set, a type's own rule wins over the one for all types
    m = tc.TokenMasks.from_vocab(vocab, {'ped': {'max_speed': 1.5}})
    assert m.n_sets == 1 and m.type_sets == [-1, 0, -1]
    assert np.array_equal(m.allowed[0], kin[1][1] <= 1.5)
    m = tc.TokenMasks.from_vocab(vocab, {'max_speed': 5.0, 'cyc': {'max_speed': 2.0, 'no_reverse': True}})
    assert m.type_sets == [0, 1, 2]
    assert np.array_equal(m.allowed[0], kin[0][1] <= 5.0) and np.array_equal(m.allowed[1], kin[1][1] <= 5.0)
    assert np.array_equal(m.allowed[2], (kin[2][1] <= 2.0) & (kin[2][0] >= 0.0))
    # the stacked [3][token_size][6][4][2] array the engine holds is accepted too
    stacked = np.stack([vocab[k_] for k_ in ('veh', 'ped', 'cyc')])
    assert np.array_equal(tc.TokenMasks.from_vocab(stacked, {'max_speed': 3.0}).words, tc.TokenMasks.from_vocab(vocab, {'max_speed': 3.0}).words)
    assert tc.TokenMasks.from_vocab(vocab, {'max_speed': 3.0}).key() != tc.TokenMasks.from_vocab(vocab, {'max_speed': 4.0}).key()


def test_errors_before_any_launch(vocab):
    with pytest.raises(ValueError, match=r"'ped'.*'min_speed'"):
        tc.TokenMasks.from_vocab(vocab, {'ped': {'min_speed': 50.0}})
    with pytest.raises(ValueError, match=r"'veh'.*'max_speed'"):
        tc.TokenMasks.from_vocab(vocab, {'max_speed': -1.0})
    with pytest.raises(ValueError, match='unknown rule'):
        tc.TokenMasks.from_vocab(vocab, {'max_jerk': 1.0})
    with pytest.raises(ValueError, match='no rule'):
        tc.TokenMasks.from_vocab(vocab, {})
    a = np.ones((2, 2048), bool)
    a[1] = False
    with pytest.raises(ValueError, match='set 1 allows no token'):
        tc.TokenMasks(a)
    with pytest.raises(ValueError, match='multiple of 32'):
        tc.TokenMasks(np.ones((1, 100), bool))
    with pytest.raises(ValueError, match='boolean'):
        tc.TokenMasks(np.ones((1, 128), np.int32))
    ok = tc.TokenMasks(np.ones((2, 128), bool))
    with pytest.raises(ValueError, match='outside the table'):
        tc.check_type_selectors([0, 2, -1], ok.n_sets)
    with pytest.raises(ValueError, match='outside the table'):
        tc.TokenMasks(np.ones((2, 128), bool), type_sets=[0, 1, 5])
    with pytest.raises(ValueError, match='three set indices'):
        tc.check_type_selectors([0, 1], ok.n_sets)
    with pytest.raises(ValueError, match='outside -1'):
        tc.check_row_selectors(np.array([[0, 1, 2]]), ok.n_sets)
    with pytest.raises(ValueError, match='outside -1'):
        tc.check_row_selectors(np.array([[0, -2]]), ok.n_sets)
    with pytest.raises(ValueError, match='integer'):
        tc.check_row_selectors(np.array([[0.5]]), ok.n_sets)
    assert tc.check_row_selectors(np.array([[-1, 0, 1]], np.int64), ok.n_sets).dtype == np.int32


def test_op_arguments_are_checked_on_the_host():
    """torch_ops._token_mask: a wrong width, selectors without a table and a per-type set without the rows' types raise before the
    library is called (no device is touched: the tensors are refused by shape)"""
    import torch
    from infgen_amd import torch_ops
    dev = torch.device('cpu')
    bits = tc.TokenMasks(np.ones((2, 128), bool)).bits
    with pytest.raises(ValueError, match='32-bit words'):
        torch_ops._token_mask(bits, None, None, None, 4, 2048, dev)                 # the table is 128 tokens wide
    with pytest.raises(ValueError, match='32-bit words'):
        torch_ops._token_mask(bits.view(dtype=torch.int32).float(), None, None, None, 4, 128, dev)
    with pytest.raises(ValueError, match='need mask_bits'):
        torch_ops._token_mask(None, torch.zeros(4, dtype=torch.int32), None, None, 4, 128, dev)
    with pytest.raises(ValueError, match="rows' types"):
        torch_ops._token_mask(bits, None, [0, -1, -1], None, 4, 128, dev)           # a table given without types
    with pytest.raises(ValueError, match='one entry per row'):
        torch_ops._token_mask(bits, torch.zeros(5, dtype=torch.int32), None, None, 4, 128, dev)
    with pytest.raises(ValueError, match='three set indices'):
        torch_ops._token_mask(bits, None, [0, 1], torch.zeros(4, dtype=torch.int32), 4, 128, dev)
    assert torch_ops._token_mask(None, None, None, None, 4, 128, dev) == ((None, 0, None, None, None), ())


def test_abi_follows_the_header():
    """the mask travels as parameters and as a handle in the context: no struct was added and InfgenRollout did not grow"""
    from infgen_amd import _lib
    r = dict(_lib.Rollout._fields_)
    assert r['token_mask'] is C.c_int and _lib.Rollout.token_mask.offset == _lib.Rollout.sample_k.offset + 4
    assert _lib.Rollout.sample_u.offset == _lib.Rollout.sample_k.offset + 8
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT) == C.sizeof(_lib.Rollout)
    for fn, n in (('infgen_heads_sample_mask', 19), ('infgen_sample_topk_mask', 15), ('infgen_token_mask_create', 5),
                  ('infgen_token_mask_destroy', 1)):
        assert fn in _lib.SYMBOLS and len(_lib.SYMBOLS[fn][1]) == n and hasattr(lib, fn), fn
    # the registry needs no device: handles are positive, reused after destroy, and refused where they name nothing
    mt = (C.c_int * 3)(0, -1, -1)
    h1 = lib.infgen_token_mask_create(None, 0, None, mt, None)
    h2 = lib.infgen_token_mask_create(None, 3, None, None, None)
    assert h1 >= 1 and h2 >= 1 and h1 != h2
    assert lib.infgen_token_mask_create(None, -1, None, None, None) == -1 and b'n_sets' in lib.infgen_last_error()
    assert lib.infgen_token_mask_destroy(h1) == 0 and lib.infgen_token_mask_destroy(h1) != 0
    assert lib.infgen_token_mask_create(None, 0, None, None, None) == h1
    assert lib.infgen_token_mask_destroy(h1) == 0 and lib.infgen_token_mask_destroy(h2) == 0
    assert lib.infgen_token_mask_destroy(0) != 0 and lib.infgen_token_mask_destroy(10 ** 6) != 0
    ctx = _lib.Rollout()
    ctx.S, ctx.A_cap, ctx.T, ctx.W, ctx.ring, ctx.num_layers, ctx.token_size = 1, 32, 4, 1, 2, 1, 2048
    ctx.token_mask = 10 ** 6
    assert lib.infgen_rollout_validate(C.byref(ctx)) != 0 and b'no handle' in lib.infgen_last_error()
    # what validate() refuses, from the pointers' values alone (nothing is dereferenced on the host)
    h = lib.infgen_token_mask_create(4096, 2, None, mt, None)
    ctx.token_mask = h
    assert lib.infgen_rollout_validate(C.byref(ctx)) != 0 and b"rows' types" in lib.infgen_last_error()      # (the context has no type array)
    ctx.type = 8192
    ctx.token_size = 2000
    assert lib.infgen_rollout_validate(C.byref(ctx)) != 0 and b'multiple of 32' in lib.infgen_last_error()
    assert lib.infgen_token_mask_destroy(h) == 0
    h = lib.infgen_token_mask_create(4100, 2, None, mt, None)
    ctx.token_mask, ctx.token_size = h, 2048
    assert lib.infgen_rollout_validate(C.byref(ctx)) != 0 and b'16-byte aligned' in lib.infgen_last_error()
    assert lib.infgen_token_mask_destroy(h) == 0


def test_handles_that_name_nothing_are_refused_with_these_words():
    """zero, a negative, one past the end and a destroyed handle: destroy and the three attach entries (turning a rider off or on)
    say 'no such token mask', a context says it is 'no handle' (0 in a context: no mask at all); an attach entry checks its own
    arguments before the handle; the next create takes the freed slot.  No device: every call returns before any launch"""
    from infgen_amd import _lib
    lib = _lib.load()
    t3 = (C.c_int * 3)(1, 0, 1)
    live = lib.infgen_token_mask_create(None, 0, None, None, None)
    dead = lib.infgen_token_mask_create(None, 0, None, None, None)
    assert live >= 1 and dead >= 1 and lib.infgen_token_mask_destroy(dead) == 0
    ctx = _lib.Rollout()
    ctx.S, ctx.A_cap, ctx.T, ctx.W, ctx.ring, ctx.num_layers, ctx.token_size = 1, 32, 4, 1, 2, 1, 2048
    for bad in (0, -3, 10 ** 6, dead):
        calls = (('infgen_token_mask_destroy', (bad,)),
                 ('infgen_token_mask_collision', (bad, None, None, None, None, 1, 0.0, None)),
                 ('infgen_token_mask_collision', (bad, 4096, 8192, 12288, 16384, 1, 0.0, None)),
                 ('infgen_token_mask_road', (bad, None, None, None, None, None, None, None, 0, 1, 1, 0.0, None, None)),
                 ('infgen_token_mask_road', (bad, 4096, 8192, 12288, 16384, 20480, 24576, 28672, 64, 1, 1, 0.0, t3, None)),
                 ('infgen_token_mask_score', (bad, None, 0, None, None, None, None, 0, 1, 1, 0.0, None, 0.5)),
                 ('infgen_token_mask_score', (bad, 4096, 4, None, 12288, None, None, 0, 1, 1, 0.0, t3, 0.5)))
        for fn, args in calls:
            assert getattr(lib, fn)(*args) == -1, (fn, bad)
            assert lib.infgen_last_error() == fn.encode() + b': no such token mask', (fn, bad)
        ctx.token_mask = bad
        if bad == 0:
            assert lib.infgen_rollout_validate(C.byref(ctx)) == 0
        else:
            assert lib.infgen_rollout_validate(C.byref(ctx)) == -1
            assert lib.infgen_last_error() == b'infgen_rollout_validate: token_mask is no handle of infgen_token_mask_create'
    assert lib.infgen_token_mask_collision(0, 4096, 8192, 12288, 16384, 2, 0.0, None) == -1
    assert lib.infgen_last_error() == b'infgen_token_mask_collision: collision mask: predict must be 0 or 1'
    assert lib.infgen_token_mask_road(0, 4096, 8192, 12288, 16384, 20480, 24576, 28672, 64, 1, 2, 0.0, t3, None) == -1
    assert lib.infgen_last_error() == b'infgen_token_mask_road: road mask: sweep must be 0 or 1'
    assert lib.infgen_token_mask_score(0, 4096, 0, None, 12288, None, None, 0, 1, 1, 0.0, t3, 0.5) == -1
    assert lib.infgen_last_error() == b'infgen_token_mask_score: step score: steps must be positive'
    assert lib.infgen_token_mask_create(None, 0, None, None, None) == dead
    assert lib.infgen_token_mask_destroy(dead) == 0 and lib.infgen_token_mask_destroy(live) == 0


def test_road_table_checks_fire_in_this_order_with_these_words():
    """what a road and a score configuration are asked alike - each argument set below is bad in everything not yet reported, so
    the message names the first check that fires (the scores' dt sits between the margin and the sweep)"""
    from infgen_amd import _lib
    lib = _lib.load()
    t3 = (C.c_int * 3)(1, 0, 1)
    h = lib.infgen_token_mask_create(None, 0, None, None, None)

    def road(rec_cap, copies, sweep, margin, shape=None, end_pose=None, types=None):
        assert lib.infgen_token_mask_road(h, 4096, 8192, shape, end_pose, 20480, 24576, 28672, rec_cap, copies, sweep, margin,
                                          types, None) == -1
        return lib.infgen_last_error()

    def score(rec_cap, copies, sweep, margin, dt, shape=None, types=None):
        assert lib.infgen_token_mask_score(h, 4096, 4, None, shape, None, None, rec_cap, copies, sweep, margin, types, dt) == -1
        return lib.infgen_last_error()

    assert road(-1, 0, 2, -1.0) == b'infgen_token_mask_road: road mask: margin must be finite and >= 0'
    assert road(-1, 0, 2, 0.0) == b'infgen_token_mask_road: road mask: sweep must be 0 or 1'
    assert road(-1, 0, 1, 0.0) == b'infgen_token_mask_road: road mask: copies must be at least 1'
    assert road(-1, 1, 1, 0.0) == b'infgen_token_mask_road: road mask: negative record capacity'
    assert road(0, 1, 1, 0.0) == b"infgen_token_mask_road: road mask: needs the rows' shape array [S][A_cap][3]"
    assert road(0, 1, 1, 0.0, 12288) == b'infgen_token_mask_road: road mask: needs the end-pose table of infgen_collision_end_poses'
    assert road(0, 1, 1, 0.0, 12288, 16384) == b'infgen_token_mask_road: road mask: needs the three-entry type switch'
    assert score(-1, 0, 2, float('nan'), 0.0) == b'infgen_token_mask_score: step score: road_margin must be finite and >= 0'
    assert score(-1, 0, 2, 0.0, 0.0) == b'infgen_token_mask_score: step score: dt must be finite and > 0'
    assert score(-1, 0, 2, 0.0, 0.5) == b'infgen_token_mask_score: step score: sweep must be 0 or 1'
    assert score(-1, 0, 1, 0.0, 0.5) == b'infgen_token_mask_score: step score: copies must be at least 1'
    assert score(-1, 1, 1, 0.0, 0.5) == b'infgen_token_mask_score: step score: negative record capacity'
    assert score(0, 1, 1, 0.0, 0.5) == b"infgen_token_mask_score: step score: needs the rows' shape array [S][A_cap][3]"
    assert score(0, 1, 1, 0.0, 0.5, 12288) == b'infgen_token_mask_score: step score: needs the three-entry type switch'
    assert lib.infgen_token_mask_road(h, 4096, 8192, 12288, 16384, 20480, 24576, 28672, 64, 1, 1, 0.0, t3, None) == 0
    assert lib.infgen_token_mask_destroy(h) == 0
