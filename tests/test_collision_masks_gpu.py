"""Collision-aware decoding on the GPU: k_collision_mask against the float64 restatement of tests/collision_ref.py, and
the engine / session / decoder plumbing on the fixtures c1_a8_m128 and ins_forced_a16_m256."""
import numpy as np
import pytest
import torch

import collision_ref as cr
from conftest import load_case
from rider_helpers import DEV, _emitted_in_sets, _make, _t, _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vocabs():
    from infgen_amd import synth
    full = synth.make_agent_vocab(2048)
    return {2048: full, 64: cr.thin_vocab(full, 64)}


def _op(case):
    """the operator on a case of collision_ref.make_case -> (bits bool [rows][K], raw words, count)"""
    from infgen_amd import torch_ops  # noqa: F401
    t = _t
    end = torch_ops.collision_end_poses(t(case['vocab']))
    kw = {}
    if case['base_rows'] is not None:
        from infgen_amd import constraints
        kw = dict(mask_bits=t(constraints.pack_bits(case['sets']).view(np.int32)), mask_row=t(case['mask_row']), mask_type=case['mask_type'])
    bits, count = torch.ops.infgen_hip.collision_mask(t(case['pos']), t(case['head']), t(case['state']), t(case['n_agents']),
                                                      t(case['atype']), t(case['shape']), case['c'], end, case['predict'],
                                                      case['margin'], **kw)
    return cr.unpack(bits.cpu().numpy(), case['token_size']), bits, count.cpu().numpy()


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize('name', list(cr.CASES))
def test_operator_equals_the_float64_restatement_outside_the_band(name, vocabs):
    case = cr.make_case(name, vocabs[cr.CASES[name]['token_size']])
    ref = cr.case_reference(case)
    got, words, count = _op(case)
    A, K = case['A'], case['token_size']
    live, base = ref['live'], ref['base']
    in_band = (ref['min_abs_sep'] <= cr.BAND) & live[:, None]
    print(f'{name}: {int(live.sum())} live rows, {int(in_band.sum())} (row, token) pairs inside the band, '
          f'{int((got != ref["allowed"]).sum())} bits differ')
    assert in_band.sum() <= 1e-3 * live.sum() * K
    # every (row, token) outside the band agrees exactly
    differ = (got != ref['allowed']) & ~in_band
    assert not differ.any(), np.argwhere(differ)[:10]
    # rows that are not in the scene at column c, and padding rows: base(i)
    assert np.array_equal(got[~live], base[~live]) and np.array_equal(count[~live], base[~live].sum(axis=1))
    # the count is the popcount of the set before the fallback; 0 means the fallback was taken and the row holds base(i)
    for r in np.flatnonzero(live):
        if count[r] > 0:
            assert count[r] == got[r].sum()
        else:
            assert np.array_equal(got[r], base[r]) and not (ref['pre'][r] & ~in_band[r]).any()
        assert abs(int(count[r]) - int(ref['count'][r])) <= int(in_band[r].sum())
    boxed = cr.BOXED_SCENE * A + cr.BOXED_ROW
    assert count[boxed] == 0 and np.array_equal(got[boxed], base[boxed]), 'the boxed-in row takes the fallback'
    # a second launch reproduces the bits exactly
    _, words2, count2 = _op(case)
    assert torch.equal(words, words2) and np.array_equal(count, count2)


def test_first_new_keeps_appended_rows_out(vocabs):
    """rows at or beyond first_new[s] are neither obstacles nor constrained: the sets equal those of a scene that ends there"""
    case = cr.make_case('k2048_a33_p0_m0', vocabs[2048])
    from infgen_amd import torch_ops
    t = _t
    end = torch_ops.collision_end_poses(t(case['vocab']))
    first_new = np.array([20, 1, 2, 1], np.int32)
    args = lambda n, fn: (t(case['pos']), t(case['head']), t(case['state']), t(n), t(case['atype']), t(case['shape']), case['c'], end,
                          case['predict'], case['margin'], None, None, None, fn)
    a, ca = torch.ops.infgen_hip.collision_mask(*args(case['n_agents'], t(first_new)))
    b, cb = torch.ops.infgen_hip.collision_mask(*args(np.minimum(case['n_agents'], first_new), None))
    assert torch.equal(a, b) and torch.equal(ca, cb)
    ref = cr.reference(case['pos'], case['head'], case['state'], case['n_agents'], case['atype'], case['shape'], case['vocab'], case['c'],
                       case['predict'], case['margin'], None, first_new)
    band = (ref['min_abs_sep'] <= cr.BAND)
    assert not ((cr.unpack(a.cpu().numpy(), 2048) != ref['allowed']) & ~band).any()


# ------------------------------------------------------------------------------------------ engine level
def _op_on_engine(eng, col, first_new=None, masks=None):
    """the operator applied to column col of the engine's state, with the engine's own shape array and end-pose table"""
    kw = {}
    if masks is not None:
        kw = dict(mask_bits=eng.mask_bits, mask_row=eng.mask_row, mask_type=list(eng.token_mask_type))
    conf = eng.avoid_collisions
    return torch.ops.infgen_hip.collision_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype,
                                               eng._coll['shape'].view(eng.S, eng.A_cap, 3), col, eng._coll_end, conf['predict'],
                                               conf['margin'], first_new=first_new, **kw)


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'k5'])
@pytest.mark.parametrize('mode', [1, 2], ids=['split', 'by-size'])
def test_session_bits_equal_the_operator_and_tokens_lie_in_their_sets(mode, sampled):
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    mask = np.zeros(8, bool)
    mask[0] = True
    kw = dict(options={'attn_mode': mode}, replay=[mask], avoid_collisions=True)
    if sampled:
        kw.update(sample_k=5, sample_uniforms=np.random.default_rng(3).random((cfg.num_decode_steps, 1, 8)).astype(np.float32))
    w = _weights(c)
    eng = _make(c, w, **kw)
    assert eng.collision_bits is not None and eng.collision_allowed is not None
    plan = eng.teacher_token.clone()
    ses = eng.session()
    hc, checked = cfg.hist_columns, 0
    for t in range(cfg.num_decode_steps):
        ses.command(tokens=plan[:, hc + t].clamp(min=0))
        ses.advance()
        col = hc - 1 + t
        bits, count = _op_on_engine(eng, col)
        assert torch.equal(eng.collision_bits, bits) and torch.equal(eng.collision_allowed, count), t
        assert torch.equal(ses.observe()['allowed_tokens'].reshape(-1), count)
        checked += _emitted_in_sets(eng, col, bits, skip=eng.replay_row.bool().cpu().numpy())
    assert checked > 20


def _parked_scene(c, w, q, m, steps_ahead):
    """the scene with row q parked (a replayed, stationary plan) where the free greedy rollout has row m after steps_ahead steps"""
    import copy
    free = _make(c, w)
    free.rollout()
    out = free.outputs()[0]
    hc = c['cfg'].hist_columns
    sc = copy.deepcopy(c['scene'])
    ag = sc['agent']
    ag['token_pos'] = np.array(ag['token_pos'], copy=True)
    ag['token_heading'] = np.array(ag['token_heading'], copy=True)
    ag['state_idx'] = np.array(ag['state_idx'], copy=True)
    ag['token_pos'][q, :, :2] = out['pos_a'][m, hc - 1 + steps_ahead, :2]
    ag['token_heading'][q, :] = out['head_a'][m, hc - 1 + steps_ahead]
    ag['state_idx'][q, :] = 1
    return sc


def _min_sep(out, shape, m, q, cols):
    """float64 separation of the boxes of rows m and q at the given columns of pos_a / head_a"""
    e = 0.5 * np.asarray(shape, np.float64)[:, :2]
    return np.array([cr.sat_sep(out['pos_a'][m, k, :2], out['head_a'][m, k], e[m], out['pos_a'][q, k, :2], out['head_a'][q, k], e[q])
                     for k in cols])


def test_a_parked_agent_in_the_greedy_path_is_avoided():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    probe = _make(c, w)
    probe.rollout()
    o = probe.outputs()[0]
    av = int(probe.av[0])
    # the moving row: the one that travels farthest in the free rollout; the parked row: another one that is not the ego
    travel = np.linalg.norm(o['pos_a'][:, hc - 1 + steps, :2] - o['pos_a'][:, hc - 1, :2], axis=1)
    travel[o['next_state_idx'][:, hc:hc + steps].min(axis=1) == 0] = -1
    m = int(np.argmax(travel))
    q = next(r for r in range(8) if r not in (m, av))
    shape = probe._shape10.cpu().numpy()[0]
    assert int(probe.n_agents[0]) == np.asarray(c['scene']['agent']['state_idx']).shape[0], 'engine rows are the scene\'s rows'
    mask = np.zeros(8, bool)
    mask[q] = True
    found = None
    for ahead in (3, 2, 4, 5, 1, 6):          # where along the free path the parked agent stands: the first placement the free rollout hits
        sc = _parked_scene(c, w, q, m, ahead)
        free = _make(c, w, scenes=[sc], replay=[mask])
        free.rollout()
        fo = free.outputs()[0]
        sep = _min_sep(fo, shape, m, q, range(hc, hc + steps + 0))
        if _min_sep(fo, shape, m, q, [hc - 1])[0] > 0.5 and (sep < -0.05).any():
            found = (sc, sep)
            break
    assert found is not None, 'the unconstrained rollout drives into the parked agent: the test constrains something'
    sc, free_sep = found
    eng = _make(c, w, scenes=[sc], replay=[mask], avoid_collisions=True)
    eng.prologue()
    eng._refresh_opts(groups=True)
    allowed = []
    for t in range(steps):
        eng.step(t)
        allowed.append(int(eng.collision_allowed[m]))
    co = eng.outputs()[0]
    sep = _min_sep(co, shape, m, q, range(hc, hc + steps))
    print('free sep', np.round(free_sep, 3), 'constrained sep', np.round(sep, 3), 'allowed', allowed)
    assert (np.array(allowed) > 0).any()
    for t in range(steps):
        if allowed[t] > 0 and co['next_state_idx'][m, hc + t] != 0:
            assert sep[t] >= -cr.BAND, (t, sep[t], allowed[t])


def test_graph_rollout_equals_the_stepwise_engine():
    c = load_case('c1_a8_m128')
    w = _weights(c)
    kw = dict(options={'attn_mode': 1}, avoid_collisions=dict(margin=0.5, predict=1), token_logprob=True)
    g = _make(c, w, use_graph=True, **kw)
    g.rollout()
    g.rollout()                       # (the first rollout runs eagerly, the second captures and replays)
    assert g._graph is not None
    a = g.outputs()[0]
    e = _make(c, w, **kw)
    e.prologue()
    e._refresh_opts(groups=True)
    for t in range(c['cfg'].num_decode_steps):
        e.step(t)
    b = e.outputs()[0]
    assert set(a) == set(b)
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=x.dtype.kind == 'f'), key
    assert torch.equal(g.collision_bits, e.collision_bits) and torch.equal(g.collision_allowed, e.collision_allowed)


@pytest.mark.parametrize('insertion', [False, True], ids=['c1', 'insertion'])
def test_off_is_the_engine_without_the_argument(insertion):
    c = load_case('ins_forced_a16_m256' if insertion else 'c1_a8_m128')
    cfg = c['cfg']
    kw = dict(token_logprob=True, store_logits=True)
    if insertion:
        cfg.disable_insertion = False
        kw.update(force_enter=True)
    w = _weights(c, cfg)
    a = _make(c, w, **kw)
    a.rollout()
    b = _make(c, w, avoid_collisions=False, **kw)
    b.rollout()
    assert b._coll is None and b.collision_bits is None and b._ctx.token_mask == 0, 'no buffers, no handle'
    x, y = a.outputs()[0], b.outputs()[0]
    assert set(x) == set(y)
    for key in x:
        p, q = np.asarray(x[key]), np.asarray(y[key])
        assert p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == 'f'), key
    # turned on and off again by reload: the same outputs once more
    b.reload([c['scene']], avoid_collisions=True)
    b.rollout()
    assert b._ctx.token_mask >= 1 and b.collision_bits is not None
    b.reload([c['scene']], avoid_collisions=False)
    b.rollout()
    z = b.outputs()[0]
    for key in x:
        p, q = np.asarray(x[key]), np.asarray(z[key])
        assert p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == 'f'), key


def test_inserted_rows_take_their_types_set_then_a_collision_set():
    from infgen_amd import constraints
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    masks = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 6.0})
    w = _weights(c, cfg)
    eng = _make(c, w, force_enter=True, token_masks=masks, avoid_collisions=True)
    eng.prologue()
    eng._refresh_opts(groups=True)
    A_cap, K = eng.A_cap, cfg.token_size
    words = torch.from_numpy(masks.words.view(np.int32).copy()).to(DEV)
    appended_before, later_live = None, 0
    for t in range(cfg.num_decode_steps):
        n_before = eng.n_agents.clone()
        for _ in eng._step_gen(t):
            pass
        col = cfg.hist_columns - 1 + t
        n_after = eng.n_agents.clone()
        bits, count = _op_on_engine(eng, col, first_new=n_before, masks=masks)
        assert torch.equal(eng.collision_bits, bits) and torch.equal(eng.collision_allowed, count), t
        types = eng.atype.reshape(-1)
        for r in range(int(n_before[0]), int(n_after[0])):          # appended inside this step: the type's static set
            assert torch.equal(bits[r], words[masks.type_sets[int(types[r])]]), (t, r)
        if appended_before:                                          # appended one step earlier: in the scene now, with a set of their own
            live = eng.state[0, col].cpu().numpy()
            later_live += sum(int(live[r] != 0) for r in appended_before)
        appended_before = list(range(int(n_before[0]), int(n_after[0])))
        _emitted_in_sets(eng, col, bits)
    out = eng.outputs()[0]
    assert out['num_inserted'] > 0 and later_live > 0


def test_speed_cap_and_collisions_combine():
    from infgen_amd import constraints
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    masks = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0})
    w = _weights(c)
    eng = _make(c, w, token_masks=masks, avoid_collisions=dict(margin=0.5), options={'attn_mode': 1})
    eng.prologue()
    eng._refresh_opts(groups=True)
    types = eng.atype.cpu().numpy()
    base = np.stack([masks.allowed[masks.type_sets[int(ty)]] for ty in types.reshape(-1)]).reshape(eng.S, eng.A_cap, -1)
    n = 0
    for t in range(cfg.num_decode_steps):
        eng.step(t)
        col = cfg.hist_columns - 1 + t
        bits, count = _op_on_engine(eng, col, masks=masks)
        assert torch.equal(eng.collision_bits, bits)
        sets = cr.unpack(bits.cpu().numpy(), cfg.token_size).reshape(base.shape)
        assert not (sets & ~base).any(), 'a collision set never leaves the static set'
        n += _emitted_in_sets(eng, col, bits)
        tok, st = eng.token[:, col + 1].cpu().numpy(), eng.state[:, col + 1].cpu().numpy()
        for s, r in zip(*np.nonzero((st != 0) & (tok >= 0))):
            assert base[s, r, tok[s, r]]
    assert n > 20
