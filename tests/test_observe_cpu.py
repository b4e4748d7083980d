"""Observations (include/infgen_hip.h, "observations") without a GPU: the header's constants, the float32 restatement
against a brute-force float64 sort, what the shared cases hold, and the Python argument checks."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import observe_ref as R                                       # noqa: E402
from infgen_amd import _lib, observe                          # noqa: E402
from infgen_amd.closed_loop import ClosedLoopSession          # noqa: E402
from infgen_amd.engine import RolloutEngine                   # noqa: E402

SEPARATION = 1e-5            # relative: below it a float32 and a float64 ordering may differ, above it they may not


def test_constants_match_the_header():
    c = _lib.HEADER.consts
    assert (c['INFGEN_OBS_SELF'], c['INFGEN_OBS_NBR'], c['INFGEN_OBS_MAP'], c['INFGEN_OBS_MAX_K']) == (R.SELF, R.NBR, R.MAP, R.MAX_K)
    assert (observe.SELF, observe.NBR, observe.MAP, observe.MAX_K) == (8, 10, 6, 64)
    res, args = _lib.SYMBOLS['infgen_observe_rows']
    assert len(args) == 31 and args[10] is _lib._f and args[13] is _lib._p
    with open(os.path.join(os.path.dirname(_lib.HEADER_PATH), '..', 'infgen_amd', 'csrc', 'kernels.h')) as f:
        assert 'OBS_MAX_K <= 64' in f.read()                 # one lane per selected entry


def _candidates(case):
    """per observed live row: (n, kind, k, radius, candidate indices, exact float64 d2 from the float32 inputs)"""
    S, T, A = case['pos'].shape[:3]
    c = case['c']
    for n, row in enumerate(R.rows_of(case)):
        if not 0 <= row < S * A:
            continue
        s, i = divmod(int(row), A)
        if not R.live(case, s, c, i):
            continue
        px, py = case['pos'][s, c, i]
        na = min(int(case['n_agents'][s]), A)
        cand = np.array([j for j in range(na) if j != i and case['state'][s, c, j] != 0], np.int64)
        yield n, 'nbr', case['K'], case['radius'], cand, R.d2_f64(px, py, case['pos'][s, c, cand, 0], case['pos'][s, c, cand, 1])
        ms = s // case['copies']
        nm = int(case['n_map'][ms])
        yield n, 'map', case['Km'], case['map_radius'], np.arange(nm), R.d2_f64(px, py, case['map_pos'][ms, :nm, 0], case['map_pos'][ms, :nm, 1])


def _separated(d2, radius):
    """consecutive d2 values are equal (an exact tie, which the index rule decides) or differ by more than SEPARATION relative, and
    none lies within SEPARATION of radius^2 without being equal to it"""
    v = np.sort(d2)
    gap = np.diff(v)
    ok = bool(np.all((gap == 0) | (gap > SEPARATION * v[1:])))
    if np.isfinite(radius):
        r2 = float(radius) ** 2
        ok = ok and bool(np.all((v == r2) | (np.abs(v - r2) > SEPARATION * r2)))
    return ok


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_restatement_agrees_with_brute_force(name):
    """the float32 evaluation decides indices and counts; wherever the candidates are separated (every row of every case: asserted)
    a float64 sort from the same inputs gives the same, with exact ties in ascending index"""
    case = R.CASES[name]
    ref = R.evaluate(case)
    checked = 0
    for n, kind, k, radius, cand, d2 in _candidates(case):
        assert _separated(d2, radius), f'{name}: row entry {n} ({kind}) has candidates closer than the condition allows'
        r2 = float(radius) ** 2 if np.isfinite(radius) else np.inf
        keep = d2 <= r2
        order = sorted(range(int(keep.sum())), key=lambda q: (d2[keep][q], cand[keep][q]))
        want = cand[keep][order][:k]
        got = ref[kind + '_index'][n]
        assert ref[kind + '_count'][n] == keep.sum(), (name, n, kind)
        assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -1).all(), (name, n, kind)
        ties = np.flatnonzero(np.diff(d2[keep][order][:k]) == 0)
        assert (np.diff(want)[ties] > 0).all()               # exact ties: ascending index
        checked += 1
    assert checked > 0


def test_float32_values_stay_inside_the_bars_of_the_float64_values():
    """the bars the GPU test asserts (its docstring derives them), met by numpy's float32 evaluation of the same formulas"""
    for name, case in R.CASES.items():
        ref = R.evaluate(case)
        eps = 8 * 2.0 ** -23
        err = np.abs(ref['nbr_feat32'] - ref['nbr_feat'])
        assert (err[..., 0:2] <= eps * ref['nbr_scale'][..., :1]).all() and (err[..., 2:4] <= eps).all(), name
        assert (err[..., 4:6] <= eps * ref['nbr_scale'][..., 1:] / case['dt']).all(), name
        err = np.abs(ref['map_feat32'] - ref['map_feat'])
        assert (err[..., 0:2] <= eps * ref['map_scale'][..., None]).all() and (err[..., 2:4] <= eps).all(), name


def test_cases_hold_what_they_promise():
    C = R.CASES
    ev = {k: R.evaluate(v) for k, v in C.items()}
    # ragged: sizes that are no multiple of the wave, padding entries, a scene without a neighbour, one without a map, dead rows
    k, e = C['ragged'], ev['ragged']
    assert k['pos'].shape[2] == 70 and tuple(k['n_agents']) == (70, 5, 1) and tuple(k['n_map']) == (130, 3, 0)
    assert (e['nbr_index'] == -1).any() and (e['nbr_count'][:70] > k['K']).any()
    assert e['self_feat'][140, 0] == 1 and e['nbr_count'][140] == 0 and e['map_count'][140] == 0           # alone, and no map
    assert e['self_feat'][4, 0] == 0 and not (e['nbr_index'][:70] == 4).any() and (e['self_feat'][70 + 5:140, 0] == 0).all()
    assert e['self_feat'][5, 7] == 0 and e['self_feat'][5, 0] == 1 and (e['self_feat'][5, 1:4] == 0).all()
    assert e['self_feat'][7, 6] == 0 and e['self_feat'][8, 6] == 0
    assert e['map_count'][70:75].max() <= 3 and e['map_index'][70:75].max() < 3                          # a map of three tokens
    # ties and boundary, seen from row 0 at the origin
    k, e = C['ties_and_boundary'], ev['ties_and_boundary']
    assert list(e['nbr_index'][0][:9]) == [8, 11, 12, 1, 2, 3, 4, 5, 9] and e['nbr_count'][0] == 9         # d2 = 0, 2, 2, 4 x 4, 25, 25
    assert not np.isin(e['nbr_index'][0], [6, 7, 10]).any()                                              # d2 = 26, 26, 32
    assert list(e['map_index'][0][:9]) == [4, 5, 6, 7, 0, 1, 8, 9, -1] and e['map_count'][0] == 8
    assert e['nbr_index'][11][0] == 12 and e['nbr_index'][12][0] == 11                                   # two rows at one position
    # first column / a neighbour without a previous pose
    e = ev['first_column']
    assert C['first_column']['c'] == 0 and (e['self_feat'][:, 7] == 0).all() and (e['self_feat'][:, 1:4] == 0).all()
    assert (e['nbr_feat'][..., 4:6] == 0).all() and (e['nbr_feat'][..., 9] == 1).any()
    k, e = C['prev_not_live'], ev['prev_not_live']
    hit = (e['nbr_index'][:9] == 1) | (e['nbr_index'][:9] == 3)
    assert k['c'] >= 1 and hit.any() and (e['nbr_feat'][:9][hit][:, 4:6] == 0).all()
    assert (e['nbr_feat'][:9][~hit & (e['nbr_index'][:9] >= 0)][:, 4:6] != 0).any()
    assert abs(e['self_feat'][2, 3] - (2 * np.pi - 6.2) / 0.5) < 1e-5                                     # the wrapped yaw rate
    # many: several candidates per lane, more map candidates inside the radius than one list pass (512 keys) holds
    k, e = C['many'], ev['many']
    assert k['pos'].shape[2] == 200 and k['K'] == 64 and k['Km'] == 64 and k['map_pos'].shape[1] == 1030
    assert (e['nbr_count'] == 199).all() and (e['map_count'] > 512).all() and np.isfinite(k['map_radius'])
    assert (e['nbr_index'] >= 0).all() and (e['map_index'] >= 0).all()
    # copies: slots 2 and 3 read map scene 1
    k, e = C['copies'], ev['copies']
    assert k['pos'].shape[0] == 4 and k['copies'] == 2 and k['map_pos'].shape[0] == 2
    assert e['map_index'][20:40].max() < 17 and e['map_index'][:20].max() >= 17
    # far world
    k = C['far_world']
    assert np.abs(k['pos'][..., 0] - 8000).max() < 100 and np.abs(k['pos'][..., 1] + 6000).max() < 100
    # rows: a repeated entry, a row that is not live, a padding row, entries out of range; K = 0 with Km > 0 and the reverse
    k, e = C['rows'], ev['rows']
    assert (e['self_feat'][0] == e['self_feat'][1]).all() and e['self_feat'][0, 0] == 1
    assert (e['self_feat'][[3, 4, 5, 6, 7], 0] == 0).all() and (e['nbr_index'][[3, 4, 5, 6, 7]] == -1).all()
    assert e['self_feat'][2, 0] == 1 and e['self_feat'][9, 0] == 1
    assert C['rows_k0']['K'] == 0 and C['rows_k0']['Km'] > 0 and C['rows_km0']['Km'] == 0 and C['rows_km0']['K'] > 0
    assert ev['rows_k0']['nbr_count'].max() > 0 and ev['rows_km0']['map_count'].max() > 0               # counts without entries


# ---------------------------------------------------------------------------------------------- argument checks
def _tensors(S=2, T=4, A=5, M=7, S0=None):
    S0 = S if S0 is None else S0
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)
    scene = [z(S, T, A, 2), z(S, T, A), z(S, T, A, dt=torch.int32), z(S, dt=torch.int32), z(S, A, dt=torch.int32), z(S, A, 3)]
    return scene, [z(S0, M, 2), z(S0, M), z(S0, M, dt=torch.int64), z(S0, dt=torch.int32)]


def test_the_operator_checks_its_arguments():
    import infgen_amd.torch_ops  # noqa: F401
    op = torch.ops.infgen_hip.observe_rows
    scene, maps = _tensors()
    bad = [
        (scene[:1] + [scene[1][:, :3]] + scene[2:], (1, 0.5), {}, 'pos \\(S, T, A, 2\\)'),
        (scene[:4] + [scene[4][:, :2]] + scene[5:], (1, 0.5), {}, 'type \\(S, A\\)'),
        (scene, (1, 0.5), dict(copies=3), 'copies'),
        (scene, (1, 0.5, maps[0]), {}, 'come together'),
        (scene, (1, 0.5, maps[0], maps[1][:, :3], maps[2], maps[3]), {}, 'map_pos \\(S / copies, M, 2\\)'),
        (scene, (1, 0.5, *_tensors(S0=1)[1]), {}, 'map_pos \\(S / copies, M, 2\\)'),
        (scene, (4, 0.5), {}, 'column 4 outside'),
        (scene, (-1, 0.5), {}, 'column -1 outside'),
        (scene, (1, 0.0), {}, 'dt must be finite'),
        (scene, (1, float('nan')), {}, 'dt must be finite'),
        (scene, (1, 0.5), dict(neighbors=65), 'neighbors must be in 0 .. 64'),
        (scene, (1, 0.5, *maps), dict(map_tokens=-1), 'map_tokens must be in 0 .. 64'),
        (scene, (1, 0.5), dict(radius=-1.0), 'radius must be >= 0'),
        (scene, (1, 0.5, *maps), dict(map_radius=float('nan')), 'map_radius must be >= 0'),
        (scene, (1, 0.5), dict(map_tokens=4), 'needs the map arrays'),
        (scene, (1, 0.5), dict(rows=torch.zeros(3)), '1-D integer tensor'),
        (scene, (1, 0.5), dict(rows=torch.zeros(3, 1, dtype=torch.int32)), '1-D integer tensor'),
    ]
    for sc, args, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            op(*sc, *args, **kw)
    with pytest.raises(_lib.InfgenHipError, match='cuda tensors'):         # past the checks: no CPU fallback
        op(*scene, 1, 0.5, *maps, map_tokens=4, radius=float('inf'))
    m = lambda t: t.to('meta')
    out = op(*map(m, scene), 1, 0.5, *map(m, maps), 1, torch.empty(3, dtype=torch.int32, device='meta'), 3, 5.0, 4)
    assert [tuple(o.shape) for o in out] == [(3, 8), (3, 3, 10), (3, 3), (3,), (3, 4, 6), (3, 4), (3,)]
    assert [o.dtype for o in out] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.float32, torch.int32, torch.int32]


def test_the_engine_and_session_methods_check_their_arguments():
    eng = types.SimpleNamespace(T=16, S=2, A_cap=32, _shape10=torch.zeros(2, 32, 3), device=torch.device('cpu'), hc=3)
    for kw, msg in ((dict(c=16), 'column 16 outside'), (dict(c=2, neighbors=65), 'neighbors'), (dict(c=2, map_tokens=70), 'map_tokens'),
                    (dict(c=2, radius=-2.0), 'radius'), (dict(c=2, map_radius=float('nan')), 'map_radius'),
                    (dict(c=2, rows=torch.zeros(4)), '1-D integer tensor'),
                    (dict(c=2, out=dict(self_feat=torch.zeros(3, 8))), "out\\['self_feat'\\]")):
        with pytest.raises(ValueError, match=msg):
            RolloutEngine.observe_rows(eng, **kw)
    eng._shape10 = None
    with pytest.raises(ValueError, match='no shape array'):
        RolloutEngine.observe_rows(eng, 2)
    ses = types.SimpleNamespace(eng=eng, t=0, _check_open=lambda: None, _obs_rows={}, _obs_out=None, _obs_key=None)
    with pytest.raises(ValueError, match="frame must be 'world' or 'agent'"):
        ClosedLoopSession.observe(ses, frame='ego')
    with pytest.raises(ValueError, match="rows must be 'controlled', 'all' or an int tensor"):
        ClosedLoopSession._observed_rows(ses, 'ego')
    with pytest.raises(ValueError, match='1-D integer tensor'):
        ClosedLoopSession._observed_rows(ses, [1, 2])


def test_outputs_are_reused_only_where_they_fit():
    a = observe.outputs(5, 3, 2, 'cpu')
    assert observe.outputs(5, 3, 2, 'cpu', a)['nbr_feat'] is a['nbr_feat']
    assert [tuple(a[k].shape) for k in observe.KEYS] == [(5, 8), (5, 3, 10), (5, 3), (5,), (5, 2, 6), (5, 2), (5,)]
    with pytest.raises(ValueError, match="out\\['nbr_feat'\\]"):
        observe.outputs(5, 4, 2, 'cpu', a)
