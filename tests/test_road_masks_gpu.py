"""Road-aware decoding on the GPU: k_road_mask and k_road_records_* against the float64 restatement of
tests/road_ref.py, and the engine / session plumbing on the fixtures c1_a8_m128 and ins_forced_a16_m256."""
import functools

import numpy as np
import pytest
import torch

import collision_ref as cr
import road_ref as rr
from conftest import load_case
from rider_helpers import _emitted_in_sets, _make, _t, _weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def vocabs():
    from infgen_amd import synth
    full = synth.make_agent_vocab(2048)
    return {2048: full, 64: rr.thin_vocab(full, 64)}


@functools.lru_cache(maxsize=None)
def _ref(name):
    from infgen_amd import synth
    full = synth.make_agent_vocab(2048)
    K = rr.CASES[name]['token_size']
    case = rr.make_case(name, full if K == 2048 else rr.thin_vocab(full, K))
    return case, rr.case_reference(case)


def _op(case, first_new=None, n_agents=None):
    """segments -> k_road_records_seg -> k_road_mask on a case of road_ref.make_case -> (bits bool [rows][K], raw words, count)"""
    from infgen_amd import constraints, torch_ops
    end = torch_ops.collision_end_poses(_t(case['vocab']))
    paths = torch_ops.road_paths(end)
    rec, nrec = torch_ops.road_records_from_segments(_t(case['segments']), _t(case['n_segments']))
    kw = {}
    if case['base_rows'] is not None:
        kw = dict(mask_bits=_t(constraints.pack_bits(case['sets']).view(np.int32)), mask_row=_t(case['mask_row']), mask_type=case['mask_type'])
    bits, count = torch.ops.infgen_hip.road_mask(_t(case['pos']), _t(case['head']), _t(case['state']),
                                                 _t(case['n_agents'] if n_agents is None else n_agents), _t(case['atype']),
                                                 _t(case['shape']), case['c'], end, paths, rec, nrec, case['copies'], case['sweep'],
                                                 case['margin'], list(case['types']), first_new=first_new, **kw)
    return cr.unpack(bits.cpu().numpy(), case['token_size']), bits, count.cpu().numpy()


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize('name', list(rr.CASES))
def test_operator_equals_the_float64_restatement_outside_the_band(name):
    case, ref = _ref(name)
    got, words, count = _op(case)
    A, K, copies = case['A'], case['token_size'], case['copies']
    live, base = ref['live'], ref['base']
    in_band = (ref['min_abs_sep'] <= rr.BAND) & live[:, None]
    judged = live & ~ref['straddle_band']                      # rows whose straddle decisions all lie outside the band
    print(f'{name}: {int(live.sum())} ruled rows, {int(in_band.sum())} (row, token) pairs inside the band, '
          f'{int(ref["straddle_band"].sum())} rows with a straddle decision in it, {int((got != ref["allowed"]).sum())} bits differ')
    assert in_band.sum() <= 1e-3 * live.sum() * K and ref['straddle_band'].sum() <= 1
    differ = (got != ref['allowed']) & ~in_band & judged[:, None]
    assert not differ.any(), np.argwhere(differ)[:10]
    # rows the rule does not apply to (not in the scene, padding, pedestrians): base(i)
    assert np.array_equal(got[~live], base[~live]) and np.array_equal(count[~live], base[~live].sum(axis=1))
    # the count is the popcount of the set before the fallback; 0 means the fallback was taken and the row holds base(i)
    for r in np.flatnonzero(judged):
        if count[r] > 0:
            assert count[r] == got[r].sum()
        else:
            assert np.array_equal(got[r], base[r]) and not (ref['pre'][r] & ~in_band[r]).any()
        assert abs(int(count[r]) - int(ref['count'][r])) <= int(in_band[r].sum())
    walled = rr.WALLED * copies * A
    assert count[walled] == 0 and np.array_equal(got[walled], base[walled]), 'the walled-in row takes the fallback'
    ring = rr.RING * copies * A
    assert ref['kept'][ring] > 128 and 0 < count[ring] < base[ring].sum(), 'the row with more records than the list holds'
    # a second launch reproduces the bits exactly
    _, words2, count2 = _op(case)
    assert torch.equal(words, words2) and np.array_equal(count, count2)


def test_records_from_the_map_equal_the_numpy_records():
    from infgen_amd import synth, torch_ops
    cfg = synth.smart_config()
    mv = synth.make_map_vocab()
    scenes = [synth.make_scene(synth.scene_seed(3, k), 8, m, cfg)['pt_token'] for k, m in enumerate((128, 70, 1, 200))]
    M = 200
    pos, ori = np.zeros((4, M, 2), np.float32), np.zeros((4, M), np.float32)
    ty, tok = np.zeros((4, M), np.int64), np.zeros((4, M), np.int64)
    for s, p in enumerate(scenes):
        k = p['num_nodes']
        pos[s, :k], ori[s, :k] = p['position'][:, :2] + np.array([5000.0, -5000.0], np.float32), p['orientation']
        ty[s, :k], tok[s, :k] = p['type'], p['token_idx']
    ty[:, 150:] = 12                          # padding beyond n_map never counts
    tok[0, np.flatnonzero(ty[0] == 12)[0]] = 4000      # a token id outside the vocabulary contributes nothing
    n_map = np.array([p['num_nodes'] for p in scenes], np.int32)
    n_map[3] = 150
    for detail in (1, 2, 5, 10):
        want = rr.records_from_map(pos, ori, ty, tok, n_map, mv, detail)
        rec, n = torch_ops.road_records_from_map(_t(pos), _t(ori), _t(ty), _t(tok), _t(n_map), _t(mv), detail)
        rec, n = rec.cpu().numpy(), n.cpu().numpy()
        assert n.tolist() == [len(w) for w in want] and rec.shape[1] == max(max(n), 1)
        for s, w in enumerate(want):
            assert np.array_equal(rec[s, :n[s], :2], w[:, :2]), 'anchors are exact copies'
            assert np.allclose(rec[s, :n[s]], w, rtol=0, atol=2e-6), np.abs(rec[s, :n[s]] - w).max()
    assert n[2] in (0, 10) and n[0] > 0 and n[3] > 0


def test_first_new_keeps_appended_rows_out():
    """rows at or beyond first_new[s] keep base(i): the sets equal those of a scene that ends there"""
    case, _ = _ref('k2048_a33_c1_s0_m0')
    first_new = np.array([20, 1, 2, 1, 3, 0, 1], np.int32)
    a, wa, ca = _op(case, first_new=_t(first_new))
    b, wb, cb = _op(case, n_agents=np.minimum(case['n_agents'], first_new))
    assert torch.equal(wa, wb) and np.array_equal(ca, cb)
    ref = rr.case_reference(case, first_new)
    band = (ref['min_abs_sep'] <= rr.BAND) | ref['straddle_band'][:, None]
    assert not ((a != ref['allowed']) & ~band).any()
    assert not ref['live'].reshape(7, 33)[0, 20:].any() and ref['live'].reshape(7, 33)[0, :20].any()


# ------------------------------------------------------------------------------------------ engine level
def _road_op(eng, col, base=None, first_new=None):
    """the operator applied to column col of the engine's state, with the engine's own tables; base: (bits, ident) of a per-row base"""
    from infgen_amd import torch_ops  # noqa: F401  (registers torch.ops.infgen_hip)
    conf = eng.stay_on_road
    kw = {} if base is None else dict(mask_bits=base[0], mask_row=base[1])
    return torch.ops.infgen_hip.road_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, eng._road['shape'].view(eng.S, eng.A_cap, 3),
                                          col, eng._coll_end, eng._road_paths, eng.road_records, eng.road_n_records, eng.copies,
                                          conf['sweep'], conf['margin'], list(conf['types']), first_new=first_new, **kw)


def _same_outputs(x, y):
    assert set(x) == set(y)
    for key in x:
        p, q = np.asarray(x[key]), np.asarray(y[key])
        assert p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == 'f'), key


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'k5'])
def test_session_bits_equal_the_operator_and_tokens_lie_in_their_sets(sampled):
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    mask = np.zeros(8, bool)
    mask[0] = True
    kw = dict(options={'attn_mode': 1}, replay=[mask], stay_on_road=dict(margin=0.5, detail=5))
    if sampled:
        kw.update(sample_k=5, sample_uniforms=np.random.default_rng(3).random((cfg.num_decode_steps, 1, 8)).astype(np.float32))
    eng = _make(c, _weights(c), **kw)
    assert eng.road_bits is not None and eng.road_allowed is not None
    plan = eng.teacher_token.clone()
    ses = eng.session()
    pt = c['scene']['pt_token']
    edges = int((np.asarray(pt['type']) == rr.EDGE).sum())
    assert edges > 0 and eng.road_n_records.tolist() == [5 * edges] and eng.road_records.shape[1] >= 5 * edges
    hc, checked, bitten = cfg.hist_columns, 0, 0
    for t in range(cfg.num_decode_steps):
        ses.command(tokens=plan[:, hc + t].clamp(min=0))
        ses.advance()
        col = hc - 1 + t
        bits, count = _road_op(eng, col)
        assert torch.equal(eng.road_bits, bits) and torch.equal(eng.road_allowed, count), t
        assert torch.equal(ses.observe()['allowed_tokens'].reshape(-1), count)
        checked += _emitted_in_sets(eng, col, bits, skip=eng.replay_row.bool().cpu().numpy())
        bitten += int(((count > 0) & (count < cfg.token_size)).sum())
    assert checked > 20 and bitten > 0, 'the map\'s edges ban tokens of some row'


def _wall_sep(out, shape, m, wall, cols, margin=0.0):
    """float64 separation of row m's box at the given columns from the wall's obstacle rectangle"""
    p0, p1 = np.asarray(wall[:2], np.float64), np.asarray(wall[2:], np.float64)
    d = p1 - p0
    e = 0.5 * np.asarray(shape, np.float64)[m, :2]
    return np.array([cr.sat_sep(np.asarray(out['pos_a'][m, k, :2], np.float64), out['head_a'][m, k], e, (p0 + p1) / 2, np.arctan2(d[1], d[0]),
                                [0.5 * np.linalg.norm(d) + margin, margin]) for k in cols])


def test_a_wall_across_the_greedy_path_is_not_driven_through():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    free = _make(c, w)
    free.rollout()
    o = free.outputs()[0]
    shape, types = free._shape10.cpu().numpy()[0], free.atype.cpu().numpy()[0]
    travel = np.linalg.norm(o['pos_a'][:, hc - 1 + steps, :2] - o['pos_a'][:, hc - 1, :2], axis=1)
    travel[o['next_state_idx'][:, hc:hc + steps].min(axis=1) == 0] = -1
    travel[types[:len(travel)] == 1] = -1                       # (pedestrians are not ruled)
    m = int(np.argmax(travel))
    margin, found = 0.3, None
    for ahead in (3, 2, 4, 5, 6):          # a 12 m wall across the free path, through the row's position `ahead` steps on
        a, b = o['pos_a'][m, hc - 1 + ahead, :2].astype(np.float64), o['pos_a'][m, hc - 2 + ahead, :2].astype(np.float64)
        u = (a - b) / max(np.linalg.norm(a - b), 1e-9)
        nrm = np.array([-u[1], u[0]])
        wall = np.concatenate([a - 6.0 * nrm, a + 6.0 * nrm]).astype(np.float32)
        free_sep = _wall_sep(o, shape, m, wall, range(hc - 1, hc + steps), margin)
        if free_sep[0] > 0.5 and (free_sep[1:] < -0.05).any():
            found = wall
            break
    assert found is not None, 'the free rollout drives through the wall: the test constrains something'
    eng = _make(c, w, stay_on_road=dict(margin=margin, segments=[found[None]]))
    eng.prologue()
    eng._refresh_opts(groups=True)
    assert eng.road_n_records.tolist() == [1]
    allowed = []
    for t in range(steps):
        eng.step(t)
        allowed.append(int(eng.road_allowed[m]))
    co = eng.outputs()[0]
    sep = _wall_sep(co, shape, m, found, range(hc - 1, hc + steps), margin)
    print('free sep', np.round(free_sep, 3), 'constrained sep', np.round(sep, 3), 'allowed', allowed)
    assert (np.array(allowed) < cfg.token_size).any(), 'the wall bans tokens of the row'
    assert min(allowed) > 0, 'one wall never empties the row\'s set: no step took the fallback'
    assert (co['next_state_idx'][m, hc:hc + steps] != 0).all()
    # over the whole horizon neither the row's box nor the path of any step overlaps the wall
    assert (sep >= -rr.BAND).all(), sep
    psep = _path_sep(co, shape, m, found, range(hc - 1, hc - 1 + steps), margin)
    assert (psep >= -rr.BAND).all(), psep


def _path_sep(out, shape, m, wall, cols, margin=0.0):
    """float64 separation of row m's path rectangle of the step column k -> k + 1 (centre half way, heading of the displacement,
    half extents (|d| / 2, the row's half width)) from the wall's obstacle rectangle; inf where the row does not move"""
    p0, p1 = np.asarray(wall[:2], np.float64), np.asarray(wall[2:], np.float64)
    w = p1 - p0
    hw = 0.5 * float(np.asarray(shape, np.float64)[m, 1])
    res = []
    for k in cols:
        a, b = np.asarray(out['pos_a'][m, k, :2], np.float64), np.asarray(out['pos_a'][m, k + 1, :2], np.float64)
        d = b - a
        L = np.linalg.norm(d)
        res.append(np.inf if L == 0 else cr.sat_sep((a + b) / 2, np.arctan2(d[1], d[0]), [0.5 * L, hw], (p0 + p1) / 2,
                                                    np.arctan2(w[1], w[0]), [0.5 * np.linalg.norm(w) + margin, margin]))
    return np.array(res)


def test_a_thin_wall_is_jumped_without_the_sweep_and_not_with_it():
    """a zero-margin wall between two consecutive poses of the free greedy rollout, where a row moves farther in one step than its
    box is long: no free end box of any row touches the wall, so with sweep = 0 every row keeps its free token and the row lands
    beyond the wall; with sweep = 1 the path rectangle of that token crosses it and the row never gets across"""
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    free = _make(c, w)
    free.rollout()
    o = free.outputs()[0]
    n = int(free.n_agents[0])
    shape, types = free._shape10.cpu().numpy()[0], free.atype.cpu().numpy()[0]
    disp = np.linalg.norm(np.diff(o['pos_a'][:n, hc - 1:hc + steps, :2].astype(np.float64), axis=1), axis=2)      # [row][step]
    order = np.dstack(np.unravel_index(np.argsort(-disp, axis=None), disp.shape))[0]
    found, tried = None, []
    for m, t in order[:40]:
        if types[m] == 1 or disp[m, t] <= 0:
            continue
        a, b = o['pos_a'][m, hc - 1 + t, :2].astype(np.float64), o['pos_a'][m, hc + t, :2].astype(np.float64)
        u = (b - a) / disp[m, t]
        nrm = np.array([-u[1], u[0]])
        for frac in (0.5, 0.4, 0.6):
            mid = a + frac * (b - a)
            wall = np.concatenate([mid - 6.0 * nrm, mid + 6.0 * nrm]).astype(np.float32)
            # every row's free box, from the start to the landing column, stays clear of the wall; the step's path crosses it
            boxes = min(float(_wall_sep(o, shape, r, wall, range(hc - 1, hc + t + 1)).min()) for r in range(n))
            path = float(_path_sep(o, shape, m, wall, [hc - 1 + t])[0])
            tried.append((int(m), int(t), round(float(disp[m, t]), 2), float(shape[m, 0]), round(boxes, 3), round(path, 3)))
            if boxes > 0.05 and path < -0.05:
                found = (int(m), int(t), wall)
                break
        if found:
            break
    print('row, step, displacement, box length, min free box sep, path sep:', tried[:12])
    assert found is not None, f'no step of the free rollout is long enough to clear a wall: {tried}'
    m, t, wall = found
    side = lambda out, k: float(np.dot(np.asarray(out['pos_a'][m, k, :2], np.float64) - wall[:2], [-(wall[3] - wall[1]), wall[2] - wall[0]]))
    runs = {}
    for sweep in (0, 1):
        eng = _make(c, w, stay_on_road=dict(margin=0.0, sweep=sweep, segments=[wall[None]]))
        eng.prologue()
        eng._refresh_opts(groups=True)
        allowed = []
        for k in range(steps):
            eng.step(k)
            allowed.append(int(eng.road_allowed[m]))
        runs[sweep] = (eng.outputs()[0], allowed)
    jump, allowed0 = runs[0]
    # sweep = 0: the free tokens up to and including the jump, and the row is on the other side of the wall
    assert np.array_equal(jump['next_token_idx'][:n, hc:hc + t + 1], o['next_token_idx'][:n, hc:hc + t + 1])
    assert side(jump, hc - 1 + t) * side(jump, hc + t) < 0, 'the row jumped the wall'
    assert _wall_sep(jump, shape, m, wall, [hc + t])[0] > 0.05 and _path_sep(jump, shape, m, wall, [hc - 1 + t])[0] < -0.05
    kept, allowed1 = runs[1]
    psep = _path_sep(kept, shape, m, wall, range(hc - 1, hc - 1 + steps))
    print('sweep 1: path sep', np.round(psep, 3), 'allowed', allowed1)
    assert min(allowed1) > 0 and allowed1[t] < cfg.token_size
    assert (psep >= -rr.BAND).all() and (_wall_sep(kept, shape, m, wall, range(hc - 1, hc + steps)) >= -rr.BAND).all()
    # the step that jumped does not jump now (later the row may drive round the end of the 12 m wall: its path stays clear above)
    assert side(kept, hc - 1 + t) * side(kept, hc + t) > 0 and kept['next_token_idx'][m, hc + t] != o['next_token_idx'][m, hc + t]


def test_graph_rollout_equals_the_stepwise_engine():
    c = load_case('c1_a8_m128')
    w = _weights(c)
    kw = dict(options={'attn_mode': 1}, stay_on_road=dict(margin=0.5, detail=10), token_logprob=True)
    g = _make(c, w, use_graph=True, **kw)
    g.rollout()
    g.rollout()                       # (the first rollout runs eagerly, the second captures and replays)
    assert g._graph is not None
    e = _make(c, w, **kw)
    e.prologue()
    e._refresh_opts(groups=True)
    for t in range(c['cfg'].num_decode_steps):
        e.step(t)
    _same_outputs(g.outputs()[0], e.outputs()[0])
    assert torch.equal(g.road_bits, e.road_bits) and torch.equal(g.road_allowed, e.road_allowed)
    assert torch.equal(g.road_records, e.road_records) and torch.equal(g.road_n_records, e.road_n_records)


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
    b = _make(c, w, stay_on_road=False, **kw)
    b.rollout()
    assert b._road is None and b.road_bits is None and b.road_records is None and b._ctx.token_mask == 0, 'no buffers, no handle'
    x = a.outputs()[0]
    _same_outputs(x, b.outputs()[0])
    # turned on and off again by reload: the same outputs once more
    b.reload([c['scene']], stay_on_road=True)
    b.rollout()
    assert b._ctx.token_mask >= 1 and b.road_bits is not None and int(b.road_n_records[0]) > 0
    if insertion:
        assert b.outputs()[0]['num_inserted'] > 0
    b.reload([c['scene']], stay_on_road=False)
    b.rollout()
    _same_outputs(x, b.outputs()[0])


def test_collision_and_road_masks_compose():
    """the road kernel's base is the collision set: set = collision set AND NOT off-road, an empty one falls back to the collision
    set - checked on every row and step, and at the first step on a row that is both boxed in (a 400 m agent sits on it) and walled in"""
    import copy
    from infgen_amd import torch_ops  # noqa: F401
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps, K = cfg.hist_columns, cfg.num_decode_steps, cfg.token_size
    probe = _make(c, w)
    types = probe.atype.cpu().numpy()[0]
    here = probe.state[0, hc - 1].cpu().numpy() != 0                 # in the scene at the first decode step's column
    m = next(r for r in range(8) if types[r] == 0 and here[r])
    q = next(r for r in range(8) if r != m and here[r])
    sc = copy.deepcopy(c['scene'])
    ag = sc['agent']
    ag['shape'] = np.array(ag['shape'], copy=True)
    ag['shape'][q, :, :2] = 400.0                              # row q's box covers the scene: every token of every row collides
    # walls around row m's pose of the first decode step, a centimetre outside its box: every token ends on one
    assert int(probe.n_agents[0]) == np.asarray(ag['state_idx']).shape[0], 'engine rows are the scene\'s rows'
    shp = probe._shape10.cpu().numpy()[0, m]
    walls = rr.walls_around(probe.pos[0, hc - 1, m].cpu().numpy(), float(probe.head[0, hc - 1, m]), 0.5 * shp[0], 0.5 * shp[1], 0.0)
    walls = walls.astype(np.float32)
    eng = _make(c, w, scenes=[sc], avoid_collisions=True, stay_on_road=dict(segments=[walls], sweep=0), options={'attn_mode': 1})
    eng.prologue()
    eng._refresh_opts(groups=True)
    assert float(eng._coll['shape'][q, 0]) == 400.0 and eng.road_n_records.tolist() == [22]
    for t in range(steps):
        eng.step(t)
        col = hc - 1 + t
        cbits, ccount = torch.ops.infgen_hip.collision_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype,
                                                            eng._coll['shape'].view(eng.S, eng.A_cap, 3), col, eng._coll_end, 1, 0.0)
        assert torch.equal(eng.collision_bits, cbits) and torch.equal(eng.collision_allowed, ccount), t
        rbits, rcount = _road_op(eng, col, base=(cbits, eng._road['ident']))
        assert torch.equal(eng.road_bits, rbits) and torch.equal(eng.road_allowed, rcount), t
        free_bits, free_count = _road_op(eng, col)              # the road rule alone
        coll, road, alone = (cr.unpack(b.cpu().numpy(), K) for b in (cbits, rbits, free_bits))
        rc, fc = rcount.cpu().numpy(), free_count.cpu().numpy()
        for r in range(eng.S * eng.A_cap):
            off = ~alone[r] if fc[r] > 0 else np.ones(K, bool)
            want = coll[r] & ~off
            assert np.array_equal(road[r], want if want.any() else coll[r]), (t, r)
            assert rc[r] == want.sum()
        if t == 0:      # boxed in and walled in: both fallbacks, the row keeps its static set (every token)
            assert int(ccount[m]) == 0 and rc[m] == 0 and coll[m].all() and road[m].all()
        _emitted_in_sets(eng, col, rbits)


def test_copies_read_their_map_scenes_records():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    from infgen_amd import synth
    other = synth.make_scene(synth.scene_seed(1, 7), 8, 128, cfg, vocab=c['vocab'], grid=c['grid'])
    u = np.random.default_rng(4).random((cfg.num_decode_steps, 4, 8)).astype(np.float32)
    eng = _make(c, w, scenes=[c['scene'], other], copies=2, sample_k=5, sample_uniforms=u, stay_on_road=dict(margin=0.5, detail=5),
                options={'attn_mode': 1})
    assert eng.S == 4 and eng.road_n_records.shape[0] == 2
    eng.prologue()
    eng._refresh_opts(groups=True)
    n = eng.road_n_records.cpu().numpy()
    want = [5 * int((np.asarray(s['pt_token']['type']) == rr.EDGE).sum()) for s in (c['scene'], other)]
    assert n.tolist() == want and want[0] != want[1]
    for t in range(3):
        eng.step(t)
        col = cfg.hist_columns - 1 + t
        bits, count = _road_op(eng, col)
        assert torch.equal(eng.road_bits, bits) and torch.equal(eng.road_allowed, count), t
        # the operator on scene 2 alone (a one-scene call: row-scene 2 -> map scene 1) gives the same rows
        one = torch.ops.infgen_hip.road_mask(eng.pos[2:3], eng.head[2:3], eng.state[2:3], eng.n_agents[2:3], eng.atype[2:3],
                                             eng._road['shape'].view(4, eng.A_cap, 3)[2:3], col, eng._coll_end, eng._road_paths,
                                             eng.road_records[1:2], eng.road_n_records[1:2], 1, 1, 0.5, [1, 0, 1])
        assert torch.equal(one[0], bits.view(4, eng.A_cap, -1)[2]) and torch.equal(one[1], count.view(4, eng.A_cap)[2])
