"""Step scores on the GPU: k_step_score against the float64 restatement of tests/step_score_ref.py, and the engine /
session / branching plumbing on small synthetic scenes."""
import functools

import numpy as np
import pytest
import torch

import step_score_ref as R
from rider_helpers import DEV, _make, _t, _weights

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name):
    case = R.make_case(name)
    return case, R.case_reference(case)


def _op(case, records=True):
    from infgen_amd import torch_ops
    rec = nrec = None
    if records:
        rec, nrec = torch_ops.road_records_from_segments(_t(case['segments']), _t(case['n_segments']))
    return torch.ops.infgen_hip.step_score(_t(case['pos']), _t(case['head']), _t(case['state']), _t(case['n_agents']), _t(case['atype']),
                                           _t(case['shape']), case['c1'], rec, nrec, case['copies'], case['sweep'], case['margin'],
                                           list(case['types']), 0.5)


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize('name', list(R.CASES))
def test_operator_equals_the_float64_restatement(name):
    """flags and counts exactly (tests/test_step_scores_cpu.py asserts that no decision of a case lies inside the band); min_sep
    within the band, 1e-4 m (fp32 SAT at tens of metres); max_accel within 2e-4 m/s^2 (two displacement norms of up to ~30 m carry
    a few ulp, ~6e-6 m, each; their difference over dt^2 = 0.25 is <= ~5e-5, the bar is 4 x that); max_yaw_rate within 1e-5 rad/s
    (one ulp of 2 pi over 0.5 s is ~1e-6)"""
    case, ref = _ref(name)
    score, row = _op(case)
    score2, row2 = _op(case)
    torch.cuda.synchronize()
    assert torch.equal(score.view(torch.int32), score2.view(torch.int32)) and torch.equal(row, row2)      # identical bytes
    sc, rw, want = score.cpu().numpy().astype(np.float64), row.cpu().numpy(), ref['score']
    fin = np.isfinite(want[:, R.MIN_SEP])
    print(f'{name}: min_sep err {np.abs(sc[fin, R.MIN_SEP] - want[fin, R.MIN_SEP]).max() if fin.any() else 0:.3g}, max_accel err '
          f'{np.abs(sc[:, R.MAX_ACCEL] - want[:, R.MAX_ACCEL]).max():.3g}, max_yaw_rate err '
          f'{np.abs(sc[:, R.MAX_YAW_RATE] - want[:, R.MAX_YAW_RATE]).max():.3g}, flags differ {int((rw != ref["row"]).sum())}')
    assert np.array_equal(rw, ref['row']), np.argwhere(rw != ref['row'])[:10]
    for col in (R.N_LIVE, R.N_OVERLAP, R.N_OFFROAD):
        assert np.array_equal(sc[:, col], want[:, col]), (col, sc[:, col], want[:, col])
    assert np.array_equal(sc[:, R.N_LIVE], (rw & R.LIVE_BIT).astype(bool).sum(axis=1))
    assert np.array_equal(sc[:, R.N_OVERLAP], (rw & R.OVERLAP_BIT).astype(bool).sum(axis=1))
    assert np.array_equal(sc[:, R.N_OFFROAD], (rw & R.OFFROAD_BIT).astype(bool).sum(axis=1))
    assert np.array_equal(np.isinf(sc[:, R.MIN_SEP]), ~fin) and (sc[~fin, R.MIN_SEP] > 0).all()
    assert np.abs(sc[fin, R.MIN_SEP] - want[fin, R.MIN_SEP]).max(initial=0.0) <= 1e-4
    assert np.abs(sc[:, R.MAX_ACCEL] - want[:, R.MAX_ACCEL]).max() <= 2e-4
    assert np.abs(sc[:, R.MAX_YAW_RATE] - want[:, R.MAX_YAW_RATE]).max() <= 1e-5
    assert not sc[:, 6:].any()


def test_operator_without_a_record_table_and_its_refusals():
    from infgen_amd import _lib
    case, ref = _ref('a33_c2_s1_m05')
    score, row = _op(case, records=False)
    with_rec, _ = _op(case)
    sc = score.cpu().numpy()
    assert not sc[:, R.N_OFFROAD].any() and not (row.cpu().numpy() & R.OFFROAD_BIT).any()
    keep = [R.N_LIVE, R.N_OVERLAP, R.MIN_SEP, R.MAX_ACCEL, R.MAX_YAW_RATE]
    assert torch.equal(score[:, keep].view(torch.int32), with_rec[:, keep].view(torch.int32))
    args = [_t(case[k]) for k in ('pos', 'head', 'state', 'n_agents', 'atype', 'shape')]
    op = torch.ops.infgen_hip.step_score
    for kw in (dict(c1=4), dict(c1=-1), dict(road_margin=-1.0), dict(road_margin=float('nan')), dict(dt=0.0), dict(dt=-0.5), dict(sweep=2)):
        full = dict(dict(c1=3, copies=2, sweep=1, road_margin=0.0, dt=0.5), **kw)
        with pytest.raises(_lib.InfgenHipError):
            op(*args, full['c1'], None, None, full['copies'], full['sweep'], full['road_margin'], [1, 0, 1], full['dt'])
    with pytest.raises(ValueError):
        op(*args, 3, None, None, 4)                  # 6 slots are no multiple of 4 copies
    with pytest.raises(ValueError):
        op(*args, 3, None, None, 0)


# ------------------------------------------------------------------------------------------ engine level
def _op_on_engine(eng, t):
    """the operator applied to the engine's stored columns at c1 = 2 + t, with the engine's own shape array and road table"""
    sc = eng.step_scores
    return torch.ops.infgen_hip.step_score(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, eng._score_boxes().view(eng.S, eng.A_cap, 3),
                                           eng.hc + t, eng.road_records, eng.road_n_records, eng.copies, sc['sweep'], sc['road_margin'],
                                           list(sc['types']), sc['dt'])


def _log_equals_the_operator(eng, steps):
    for t in range(steps):
        score, row = _op_on_engine(eng, t)
        assert torch.equal(eng.step_score[:, t].view(torch.int32), score.view(torch.int32)), t
    assert torch.equal(eng.score_row, row)
    assert bool((eng.step_score[:, :, 0] > 0).any()), 'some row is live'


@pytest.mark.parametrize('mode', [1, 2], ids=['split', 'by-size'])
def test_graph_and_stepwise_logs_equal_the_operator_on_the_final_columns(mode):
    from conftest import load_case
    c = load_case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    w = _weights(c)
    kw = dict(options={'attn_mode': mode}, step_scores=True)
    g = _make(c, w, use_graph=True, **kw)
    assert g.step_score.shape == (g.S, steps, 8) and g.score_row.shape == (g.S, g.A_cap) and g.score_row.dtype == torch.uint8
    assert g.hc == 2, 'decode step t produces column 2 + t'
    g.rollout()
    g.rollout()                       # (the first rollout runs eagerly, the second captures and replays)
    assert g._graph is not None
    _log_equals_the_operator(g, steps)
    e = _make(c, w, **kw)
    e.prologue()
    e._refresh_opts(groups=True)
    for t in range(steps):
        e.step(t)
        assert torch.equal(e.score_row, _op_on_engine(e, t)[1]), t       # the flag bytes are those of the newest step
    _log_equals_the_operator(e, steps)
    assert torch.equal(e.step_score.view(torch.int32), g.step_score.view(torch.int32)) and torch.equal(e.score_row, g.score_row)


def test_on_is_the_engine_without_the_argument_and_insertion_is_refused():
    from conftest import load_case
    c = load_case('c1_a8_m128')
    w = _weights(c)
    kw = dict(token_logprob=True, store_logits=True)
    a = _make(c, w, **kw)
    a.rollout()
    assert a.step_score is None and a._ctx.token_mask == 0
    b = _make(c, w, step_scores=dict(road_margin=0.2, types=('veh', 'ped', 'cyc')), **kw)
    b.rollout()
    assert b._ctx.token_mask >= 1
    x, y = a.outputs()[0], b.outputs()[0]
    assert set(x) == set(y)
    for key in x:
        p, q = np.asarray(x[key]), np.asarray(y[key])
        assert p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == 'f'), key
    assert torch.equal(a.logits, b.logits) and torch.equal(a.pos, b.pos) and torch.equal(a.token, b.token)
    # off again by reload, on again: the outputs stay, the log comes back
    log = b.step_score.clone()
    b.reload([c['scene']], step_scores=False)
    assert b.step_scores is None
    b.rollout()
    b.reload([c['scene']], step_scores=dict(road_margin=0.2, types=('veh', 'ped', 'cyc')))
    b.step_score.zero_()
    b.rollout()
    assert torch.equal(b.step_score.view(torch.int32), log.view(torch.int32)) and torch.equal(a.pos, b.pos)
    ic = load_case('ins_forced_a16_m256')
    ic['cfg'].disable_insertion = False
    with pytest.raises(ValueError, match='insertion'):
        _make(ic, _weights(ic, ic['cfg']), force_enter=True, step_scores=True)
    with pytest.raises(ValueError, match='one road table'):
        _make(c, w, stay_on_road=dict(detail=5), step_scores=dict(detail=2))


def test_branch_copies_the_log_and_the_branched_rollout_still_equals_the_operator():
    from conftest import load_case
    c = load_case('c1_a8_m128')
    steps, tb = c['cfg'].num_decode_steps, 3
    u = np.random.default_rng(7).random((steps, 4, 8), dtype=np.float32)
    eng = _make(c, _weights(c), copies=4, sample_k=5, sample_uniforms=u, step_scores=True)
    eng.prologue()
    eng.run(0, tb)
    before = eng.step_score.clone()
    eng.branch([0, 0, 2, 2], tb)
    torch.cuda.synchronize()
    assert int(eng.branch_bad[0]) == 0
    for child, parent in ((1, 0), (3, 2)):
        assert torch.equal(eng.step_score[child, :tb].view(torch.int32), before[parent, :tb].view(torch.int32))
        assert torch.equal(eng.step_score[parent].view(torch.int32), before[parent].view(torch.int32))
    assert not torch.equal(before[1, :tb], before[0, :tb]) or not torch.equal(before[3, :tb], before[2, :tb]), 'the copies had diverged'
    eng.run(tb, steps)
    _log_equals_the_operator(eng, steps)


def test_observe_carries_the_scores():
    from conftest import load_case
    c = load_case('c1_a8_m128')
    mask = np.zeros(8, bool)
    mask[0] = True
    eng = _make(c, _weights(c), replay=[mask], step_scores=True)
    plan = eng.teacher_token.clone()
    ses = eng.session()
    first = ses.observe()
    assert 'step_score' not in first and first['score_row'].shape == (eng.S, eng.A_cap)
    for t in range(3):
        ses.command(tokens=plan[:, eng.hc + t].clamp(min=0))
        ses.advance()
        obs = ses.observe()
        score, row = _op_on_engine(eng, t)
        assert obs['step_score'].shape == (eng.S, 8) and torch.equal(obs['step_score'].view(torch.int32), score.view(torch.int32))
        assert torch.equal(obs['score_row'], row)


def _hand_loop(eng, every, weights, keep=None, u=None):
    """the guided rollout written out: run / score_log_weight / keep_best or systematic / branch -> the parent vectors used"""
    from infgen_amd import branching
    steps, used = eng.cfg.num_decode_steps, []
    eng.prologue()
    for b, t0 in enumerate(range(0, steps, every)):
        t1 = min(t0 + every, steps)
        eng.run(t0, t1)
        lw = branching.score_log_weight(eng.step_score, t0, t1, weights, copies=eng.copies)
        if keep is not None:
            parent = branching.keep_best(lw, keep)
        else:
            parent = branching.resample_parents(branching.systematic_ancestors(lw, u[b]), eng.copies)
        used.append(parent.reshape(-1).clone())
        eng.branch(parent, t1)
    return torch.stack(used)


@pytest.mark.parametrize('how', ['keep_best', 'systematic'])
def test_rollout_guided_equals_the_hand_written_loop(how):
    from conftest import load_case
    c = load_case('c1_a8_m128')
    steps, n, every = c['cfg'].num_decode_steps, 4, 4
    su = np.random.default_rng(11).random((steps, n, 8), dtype=np.float32)
    weights = dict(w_overlap=1.0, w_offroad=1.0, w_accel=0.05, w_yaw=0.1, w_gap=0.5, gap_limit=2.0)
    w = _weights(c)
    kw = dict(copies=n, sample_k=5, sample_uniforms=su, step_scores=True, token_logprob=True)
    n_blocks = -(-steps // every)
    u = torch.from_numpy(np.random.default_rng(12).random((n_blocks, 1))).float().to(DEV)
    arg = dict(keep=2) if how == 'keep_best' else dict(keep=None, u=u)
    g = _make(c, w, **kw)
    g.rollout_guided(every=every, weights=weights, **arg)
    h = _make(c, w, **kw)
    used = _hand_loop(h, every, weights, **arg)
    torch.cuda.synchronize()
    assert g.ancestry.shape == (n_blocks, g.S) and g.ancestry.dtype == torch.int32 and torch.equal(g.ancestry, used.to(torch.int32))
    assert int(g.branch_bad[0]) == 0
    for k in ('pos', 'head', 'state', 'token', 'token_logprob'):
        assert torch.equal(getattr(g, k), getattr(h, k)), k
    assert torch.equal(g.step_score.view(torch.int32), h.step_score.view(torch.int32))
    assert bool((g.ancestry != torch.arange(g.S, device=DEV, dtype=torch.int32)[None]).any()), 'some copy was replaced'
    _log_equals_the_operator(g, steps)
    # what the driver refuses
    with pytest.raises(ValueError, match='copies'):
        _make(c, w, step_scores=True).rollout_guided()
    with pytest.raises(ValueError, match='step_scores'):
        _make(c, w, copies=2).rollout_guided()
    with pytest.raises(ValueError, match='uniforms'):
        g.rollout_guided(keep=None)
    with pytest.raises(ValueError, match='keep'):
        g.rollout_guided(keep=5)


def test_a_parked_agent_in_the_greedy_path_is_reported():
    """n_overlap == 2 - the moving row and the parked one - from the step where their boxes meet"""
    from conftest import load_case
    from test_collision_masks_gpu import _min_sep, _parked_scene
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    probe = _make(c, w)
    probe.rollout()
    o = probe.outputs()[0]
    av = int(probe.av[0])
    travel = np.linalg.norm(o['pos_a'][:, hc - 1 + steps, :2] - o['pos_a'][:, hc - 1, :2], axis=1)
    travel[o['next_state_idx'][:, hc:hc + steps].min(axis=1) == 0] = -1
    m = int(np.argmax(travel))
    q = next(r for r in range(8) if r not in (m, av))
    shape = probe._shape10.cpu().numpy()[0]
    mask = np.zeros(8, bool)
    mask[q] = True
    found = None
    for ahead in (3, 2, 4, 5, 1, 6):
        sc = _parked_scene(c, w, q, m, ahead)
        eng = _make(c, w, scenes=[sc], replay=[mask], step_scores=True)
        eng.prologue()
        eng._refresh_opts(groups=True)
        rows = []
        for t in range(steps):
            eng.step(t)
            rows.append(eng.score_row[0].cpu().numpy().copy())
        fo = eng.outputs()[0]
        sep = _min_sep(fo, shape, m, q, range(hc, hc + steps))
        if _min_sep(fo, shape, m, q, [hc - 1])[0] > 0.5 and (sep < -0.05).any():
            found = (eng, sep, np.array(rows))
            break
    assert found is not None, 'the greedy rollout drives into the parked agent'
    eng, sep, rows = found
    log = eng.step_score[0].cpu().numpy()
    ref = [R.reference(eng.pos.cpu().numpy(), eng.head.cpu().numpy(), eng.state.cpu().numpy(), eng.n_agents.cpu().numpy(),
                       eng.atype.cpu().numpy(), eng._shape10.cpu().numpy(), hc + t) for t in range(steps)]
    print('sep of the pair', np.round(sep, 3), 'n_overlap', log[:, R.N_OVERLAP], 'restated', [r['score'][0, R.N_OVERLAP] for r in ref])
    meet = int(np.argmax(sep < -0.05))
    assert (sep[:meet] > R.BAND).all(), 'the boxes are apart before they meet'
    for t in range(steps):
        if abs(sep[t]) < R.BAND or ref[t]['band'] < R.BAND:
            continue
        assert log[t, R.N_OVERLAP] == ref[t]['score'][0, R.N_OVERLAP], t
        both = bool(rows[t][m] & R.OVERLAP_BIT) and bool(rows[t][q] & R.OVERLAP_BIT)
        if sep[t] < 0:
            assert both and log[t, R.N_OVERLAP] >= 2 and log[t, R.MIN_SEP] <= sep[t] + 1e-4, t
    others = ref[meet]['pair_sep'][0].copy()
    others[[m, q], :] = np.inf
    assert (others > 0).all(), 'no other pair overlaps at that step'
    assert log[meet, R.N_OVERLAP] == 2 and (log[:meet, R.N_OVERLAP] == [r['score'][0, R.N_OVERLAP] for r in ref[:meet]]).all()


def test_a_walled_scene_reports_off_road_rows_and_none_under_stay_on_road():
    """walls from road_ref.walls_around round a vehicle: the free rollout drives through them (n_offroad > 0); with stay_on_road on
    - the scores then read the road masks' own record table - nothing is off-road"""
    import road_ref as rr
    from conftest import load_case
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    probe = _make(c, w)
    probe.rollout()
    o = probe.outputs()[0]
    types = probe.atype.cpu().numpy()[0]
    travel = np.linalg.norm(o['pos_a'][:, hc - 1 + steps, :2] - o['pos_a'][:, hc - 1, :2], axis=1)
    travel[o['next_state_idx'][:, hc:hc + steps].min(axis=1) == 0] = -1
    travel[types[:len(travel)] != 0] = -1
    m = int(np.argmax(travel))
    shp = probe._shape10.cpu().numpy()[0, m]
    walls = rr.walls_around(probe.pos[0, hc - 1, m].cpu().numpy(), float(probe.head[0, hc - 1, m]), 0.5 * shp[0], 0.5 * shp[1], 1.0)
    # (walls a metre outside the box: a short token stays inside them, so the masks' empty-set fallback - after which the row would
    # sit on a wall, exempt for the masks as a straddled segment and off-road for the scores - is not what this test is about)
    seg = dict(segments=[walls.astype(np.float32)])
    free = _make(c, w, step_scores=seg)
    free.rollout()
    assert free.road_n_records.tolist() == [22]
    off = free.step_score[0, :, R.N_OFFROAD].cpu().numpy()
    kept = _make(c, w, stay_on_road=seg, step_scores=True)
    assert kept.step_scores['segments'] is not None and kept._score_shape is None, 'one road table, one shape array'
    kept.prologue()
    kept._refresh_opts(groups=True)
    allowed, rows = [], []
    for t in range(steps):
        kept.step(t)
        allowed.append(kept.road_allowed.view(-1).cpu().numpy().copy())
        rows.append(kept.score_row[0].cpu().numpy().copy())
    on = kept.step_score[0, :, R.N_OFFROAD].cpu().numpy()
    print('n_offroad free', off, 'under stay_on_road', on, 'smallest allowed set', np.min(allowed, axis=1))
    print('walled row', m, 'off-road rows per step', [np.flatnonzero(r & R.OFFROAD_BIT).tolist() for r in rows], 'their allowed sets',
          [[int(a[i]) for i in np.flatnonzero(r & R.OFFROAD_BIT)] for a, r in zip(allowed, rows)], 'types', types.tolist())
    assert (off > 0).any()
    assert min(int(a[m]) for a in allowed) > 0, 'the walled row never took the fallback'
    assert (on == 0).all(), on
    _log_equals_the_operator(kept, steps)


def test_decoder_returns_the_scores_and_runs_guided_rollouts():
    from infgen_amd import synth
    from conftest import load_case
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    dec = _decoder(cfg)
    _load(dec, c['sd'])
    dev = torch.device(DEV)
    dec = dec.to(dev).eval()
    scene = synth.make_scene(9301, 8, 128, cfg, vocab=c['vocab'], grid=c['grid'])
    steps = cfg.num_decode_steps
    free = dec.inference_rollouts(_to_data(scene, dev), 2)
    assert all('step_score' not in r for r in free)
    n0 = len(dec._engines)
    dec.step_scores = dict(road_margin=0.2)
    rolls = dec.inference_rollouts(_to_data(scene, dev), 2)
    assert len(dec._engines) == n0 + 1, 'a scoring call does not reuse the engine without scores'
    eng = _make(c, _weights(c), scenes=[scene], copies=2, step_scores=dict(road_margin=0.2))
    eng.rollout()
    for j, r in enumerate(rolls):
        assert r['step_score'].shape == (steps, 8) and torch.equal(r['step_score'].view(torch.int32), eng.step_score[j].view(torch.int32))
        assert torch.equal(r['next_token_idx'], free[j]['next_token_idx']), 'scoring changes no token'
    dec.guided_rollouts = dict(every=4, keep=1)
    guided = dec.inference_rollouts(_to_data(scene, dev), 2)
    eng.rollout_guided(every=4, keep=1)
    for j, r in enumerate(guided):
        assert torch.equal(r['step_score'].view(torch.int32), eng.step_score[j].view(torch.int32))
    assert torch.equal(guided[0]['next_token_idx'], guided[1]['next_token_idx']), 'keep = 1: both copies end as the best one'
    with pytest.raises(ValueError, match='copies'):
        dec.inference(_to_data(scene, dev))
    dec.step_scores = False
    with pytest.raises(ValueError, match='step_scores'):
        dec.inference_rollouts(_to_data(scene, dev), 2)
