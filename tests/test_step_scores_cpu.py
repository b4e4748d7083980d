"""Step scores without a GPU: the float64 restatement against a brute-force polygon test, the band condition the GPU
test's exact flag comparison rests on, ``branching.score_log_weight`` and the host-side argument checks."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_score_ref as R                                   # noqa: E402
from infgen_amd import branching, constraints                # noqa: E402
from infgen_amd.branching import score_log_weight            # noqa: E402
from infgen_amd.constraints import check_step_scores         # noqa: E402

_REF = {}


def _case(name):
    if name not in _REF:
        case = R.make_case(name)
        _REF[name] = (case, R.case_reference(case))
    return _REF[name]


def test_constants_match_the_header():
    assert [branching.SCORE_N_LIVE, branching.SCORE_N_OVERLAP, branching.SCORE_MIN_SEP, branching.SCORE_N_OFFROAD,
            branching.SCORE_MAX_ACCEL, branching.SCORE_MAX_YAW_RATE] == [R.N_LIVE, R.N_OVERLAP, R.MIN_SEP, R.N_OFFROAD, R.MAX_ACCEL,
                                                                         R.MAX_YAW_RATE] == list(range(6))
    assert branching.SCORE_WIDTH == 8
    from infgen_amd import _lib
    assert 'infgen_step_score' in _lib.HEADER.protos and 'infgen_token_mask_score' in _lib.HEADER.protos
    assert branching.SCORE_WEIGHTS == R.WEIGHT_DEFAULTS


@pytest.mark.parametrize('name', list(R.CASES))
def test_band_condition(name):
    """a condition, not a measurement: no pair or record decision of the case lies within BAND of zero"""
    case, ref = _case(name)
    assert ref['band'] >= R.BAND, ref['band']
    other = R.case_reference(case, sweep=1 - case['sweep'])
    assert other['band'] >= R.BAND, other['band']


@pytest.mark.parametrize('name', list(R.CASES))
def test_restatement_agrees_with_brute_force(name):
    case, ref = _case(name)
    pos, head, shape, c1 = case['pos'].astype(np.float64), case['head'].astype(np.float64), case['shape'].astype(np.float64), case['c1']
    rec = R.records_from_segments(case['segments'], case['n_segments'])
    pairs = recs = 0
    for s in range(pos.shape[0]):
        sep = ref['pair_sep'][s]
        own = 0.5 * shape[s, :, :2]
        rad = np.hypot(own[:, 0], own[:, 1])
        corners = [R.box_corners(pos[s, c1, i], head[s, c1, i], own[i]) for i in range(pos.shape[2])]
        for i, j in zip(*np.nonzero(np.isfinite(sep))):
            if j < i:
                assert (sep[i, j] < 0) == (sep[j, i] < 0)
                continue
            if np.hypot(*(pos[s, c1, i] - pos[s, c1, j])) > rad[i] + rad[j]:
                assert sep[i, j] > 0
                continue
            pairs += 1
            assert (sep[i, j] < 0) == polygons_overlap(corners[i], corners[j]), (s, i, j, sep[i, j])
        r = rec[s // case['copies']]
        for (slot, i), sb in ref['box_sep'].items():
            if slot != s:
                continue
            sp = ref['path_sep'][slot, i]
            d = pos[s, c1, i] - pos[s, c1 - 1, i]
            for e in np.flatnonzero(np.isfinite(sb)):
                mid = r[e, 0:2] + r[e, 2:4]
                oc = R.box_corners(mid, np.arctan2(r[e, 5], r[e, 4]), [r[e, 6] + case['margin'], case['margin']])
                reach = r[e, 6] + 2 * case['margin'] + rad[i]
                if np.hypot(*(mid - pos[s, c1, i])) <= reach:
                    recs += 1
                    assert (sb[e] < 0) == polygons_overlap(corners[i], oc), (s, i, e, sb[e])
                if np.isfinite(sp[e]) and np.hypot(*(mid - (pos[s, c1, i] - 0.5 * d))) <= reach + 0.5 * np.hypot(*d):
                    pc = R.box_corners(pos[s, c1, i] - 0.5 * d, np.arctan2(d[1], d[0]), [0.5 * np.hypot(*d), own[i, 1]])
                    assert (sp[e] < 0) == polygons_overlap(pc, oc), (s, i, e, sp[e])
    assert pairs > 0 and recs > 0


def polygons_overlap(pa, pb):
    return R.polygons_overlap_brute(pa, pb)


@pytest.mark.parametrize('name', list(R.CASES))
def test_cases_hold_what_they_promise(name):
    case, ref = _case(name)
    sc, row, c1 = ref['score'], ref['row'], case['c1']
    A = case['A']
    assert sc[R.FULL, R.N_LIVE] == A - 1 and row[R.FULL, 3] == 0
    assert row[R.FULL, 4] & R.OVERLAP_BIT and row[R.FULL, 5] & R.OVERLAP_BIT and sc[R.FULL, R.MIN_SEP] < 0
    assert sc[R.ONE, R.N_LIVE] == 1 and np.isinf(sc[R.ONE, R.MIN_SEP]) and sc[R.ONE, R.N_OVERLAP] == 0
    assert not sc[R.NONE, :2].any() and np.isinf(sc[R.NONE, R.MIN_SEP]) and not sc[R.NONE, 3:].any() and not row[R.NONE].any()
    assert row[R.ASTRIDE, 0] & R.OFFROAD_BIT
    swept, still = R.case_reference(case, sweep=1), R.case_reference(case, sweep=0)
    assert swept['row'][R.JUMP, 0] & R.OFFROAD_BIT and not still['row'][R.JUMP, 0] & R.OFFROAD_BIT
    if case['n_segments'][R.FULL // case['copies']] > R.ZERO_LENGTH:      # the zero-length segment is never used
        assert np.isinf(ref['box_sep'][R.FULL, 0][R.ZERO_LENGTH])
    # rows 1 and 2 of FULL take no part in the comfort terms they lack a column for
    full = dict(case, n_agents=np.where(np.arange(R.S_CASE) == R.FULL, 3, 0).astype(np.int32))
    only = R.reference(full['pos'], full['head'], full['state'], full['n_agents'], full['atype'], full['shape'], c1)
    p, h = case['pos'].astype(np.float64)[R.FULL], case['head'].astype(np.float64)[R.FULL]
    acc0 = abs(np.hypot(*(p[c1, 0] - p[c1 - 1, 0])) - np.hypot(*(p[c1 - 1, 0] - p[c1 - 2, 0]))) / 0.25
    yaw = max(abs(R._wrap(h[c1, i] - h[c1 - 1, i])) / 0.5 for i in (0, 2))
    assert only['score'][R.FULL, R.MAX_ACCEL] == pytest.approx(acc0, rel=1e-12)
    assert only['score'][R.FULL, R.MAX_YAW_RATE] == pytest.approx(yaw, rel=1e-12)
    assert (row & R.LIVE_BIT).sum(axis=1).tolist() == sc[:, R.N_LIVE].tolist()
    assert ((row & R.OVERLAP_BIT) > 0).sum(axis=1).tolist() == sc[:, R.N_OVERLAP].tolist()
    assert ((row & R.OFFROAD_BIT) > 0).sum(axis=1).tolist() == sc[:, R.N_OFFROAD].tolist()


def test_score_log_weight_against_numpy():
    rng = np.random.default_rng(5)
    S0, n, steps = 3, 4, 7
    x = np.zeros((S0 * n, steps, 8), np.float32)
    x[..., R.N_LIVE] = rng.integers(0, 9, (S0 * n, steps))
    x[..., R.N_OVERLAP] = rng.integers(0, 4, (S0 * n, steps))
    x[..., R.N_OFFROAD] = rng.integers(0, 3, (S0 * n, steps))
    x[..., R.MIN_SEP] = rng.uniform(-1.0, 3.0, (S0 * n, steps))
    x[rng.random((S0 * n, steps)) < 0.3, R.MIN_SEP] = np.inf
    x[..., R.MAX_ACCEL] = rng.uniform(0.0, 9.0, (S0 * n, steps))
    x[..., R.MAX_YAW_RATE] = rng.uniform(0.0, 2.0, (S0 * n, steps))
    t = torch.from_numpy(x)
    for weights in (None, dict(w_accel=0.5, w_yaw=2.0, w_gap=3.0), dict(w_overlap=0.0, w_gap=1.0, gap_limit=1.5, accel_limit=1.0, w_accel=1.0)):
        for t0, t1 in ((0, steps), (2, 5), (3, 3)):
            got = score_log_weight(t, t0, t1, weights, copies=n)
            assert got.shape == (S0, n) and got.dtype == torch.float32 and torch.isfinite(got).all()
            np.testing.assert_allclose(got.numpy(), R.log_weight(x, t0, t1, weights, n), rtol=1e-5, atol=1e-5)
            assert torch.equal(got, score_log_weight(t.view(S0, n, steps, 8), t0, t1, weights))
    assert (score_log_weight(t, 0, steps, copies=n) <= 0).all()
    for bad in (lambda: score_log_weight(t, 0, steps + 1, copies=n), lambda: score_log_weight(t, 3, 2, copies=n),
                lambda: score_log_weight(t, 0, 1), lambda: score_log_weight(t[..., :7], 0, 1, copies=n),
                lambda: score_log_weight(t, 0, 1, dict(w_speed=1.0), copies=n), lambda: score_log_weight(t, 0, 1, dict(w_gap=float('nan')), copies=n)):
        with pytest.raises(ValueError):
            bad()


def test_check_step_scores():
    assert check_step_scores(None) is None and check_step_scores(False) is None
    assert check_step_scores(True) == dict(road_margin=0.0, sweep=1, types=(1, 0, 1), detail=2, segments=None, dt=0.5)
    got = check_step_scores(dict(road_margin=0.25, sweep=0, types=('veh', 'ped'), detail=5, dt=0.1))
    assert got == dict(road_margin=0.25, sweep=0, types=(1, 1, 0), detail=5, segments=None, dt=0.1)
    seg = [np.zeros((2, 4), np.float32), np.ones((3, 4), np.float32)]
    got = check_step_scores(dict(segments=seg), n_scenes=2)
    assert got['segments'][0].shape == (2, 3, 4) and got['segments'][1].tolist() == [2, 3]
    for bad in (3, 'on', dict(margin=0.1), dict(road_margin=-0.1), dict(road_margin=float('inf')), dict(dt=0), dict(dt=-0.5),
                dict(dt=float('nan')), dict(dt='0.5'), dict(sweep=2), dict(detail=3), dict(types='veh'), dict(types=('car',)),
                dict(segments=np.zeros((2, 3)))):
        with pytest.raises(ValueError, match='step_scores'):
            check_step_scores(bad)
    with pytest.raises(ValueError, match='2 distinct scenes'):
        check_step_scores(dict(segments=seg[:1]), n_scenes=2)
    with pytest.raises(ValueError, match='shape'):
        check_step_scores(True, has_shape=False)
    # one road table per engine: the scores take stay_on_road's, and refuse another
    stay = constraints.check_stay_on_road(dict(detail=5, margin=0.3))
    assert check_step_scores(True, stay_on_road=stay)['detail'] == 5 and check_step_scores(True, stay_on_road=stay)['road_margin'] == 0.0
    with pytest.raises(ValueError, match='one road table'):
        check_step_scores(dict(detail=2), stay_on_road=stay)
    with pytest.raises(ValueError, match='one road table'):
        check_step_scores(dict(segments=seg), stay_on_road=stay)
    stay_seg = constraints.check_stay_on_road(dict(segments=seg))
    assert np.array_equal(check_step_scores(True, stay_on_road=stay_seg)['segments'][0], stay_seg['segments'][0])
    assert check_step_scores(dict(segments=seg), stay_on_road=stay_seg)['segments'] is not None
    assert constraints.score_key(None) is None and constraints.score_key(check_step_scores(True)) == (0.0, 1, (1, 0, 1), 2, False, 0.5)
