"""Road-aware decoding without a GPU: the float64 restatement of tests/road_ref.py against an independent brute-force
polygon test, the host-side argument checks, the numpy record builder against a hand-computed chord, and the band conditions of
the shared operator cases."""
import functools

import numpy as np
import pytest

import collision_ref as cr
import road_ref as rr


@functools.lru_cache(maxsize=None)
def _vocab(token_size):
    from infgen_amd import synth
    full = synth.make_agent_vocab(2048)
    return full if token_size == 2048 else rr.thin_vocab(full, token_size)


@functools.lru_cache(maxsize=None)
def _case(name):
    case = rr.make_case(name, _vocab(rr.CASES[name]['token_size']))
    return case, rr.case_reference(case)


@pytest.mark.parametrize('name', ['k64_a8_c2_s1_m05', 'k2048_a8_c1_s1_m0'])
def test_axis_test_agrees_with_a_brute_force_polygon_test(name):
    case, ref = _case(name)
    centre, dth = rr.token_end_poses(case['vocab'])
    rec = rr.records_from_segments(case['segments'], case['n_segments'])
    rng = np.random.default_rng(5)
    A, c, n = case['A'], case['c'], 0
    rows = [r for r in ref['sep_end'] if np.isfinite(ref['sep_end'][r]).any()]
    for _ in range(400):
        row = rows[rng.integers(len(rows))]
        s, i = divmod(row, A)
        se, sp = ref['sep_end'][row], ref['sep_path'][row]
        k, e = rng.integers(se.shape[0]), rng.choice(np.flatnonzero(np.isfinite(se[0])))
        r = rec[s // case['copies']][e]
        p, h = case['pos'][s, c, i].astype(np.float64), float(case['head'][s, c, i])
        ty = int(case['atype'][s, i])
        ci, si = np.cos(h), np.sin(h)
        end_c = np.array([centre[ty, k, 0] * ci - centre[ty, k, 1] * si, centre[ty, k, 0] * si + centre[ty, k, 1] * ci])
        own = 0.5 * case['shape'][s, i, :2].astype(np.float64)
        obst = cr.box_corners((r[0:2] - p) + r[2:4], np.arctan2(r[5], r[4]), [r[6] + case['margin'], max(case['margin'], 1e-9)])
        if abs(se[k, e]) > 1e-6:
            assert cr.polygons_overlap_brute(cr.box_corners(end_c, h + dth[ty, k], own), obst) == (se[k, e] < 0), (row, k, e)
            n += 1
        if np.isfinite(sp[k, e]) and abs(sp[k, e]) > 1e-6:
            path = cr.box_corners(0.5 * end_c, np.arctan2(end_c[1], end_c[0]), [0.5 * np.hypot(*end_c), own[1]])
            assert cr.polygons_overlap_brute(path, obst) == (sp[k, e] < 0), (row, k, e)
            n += 1
    assert n > 400


def test_check_stay_on_road_accepts_and_refuses():
    from infgen_amd.constraints import check_stay_on_road as chk
    assert chk(False) is None and chk(None) is None
    assert chk(True) == dict(margin=0.0, sweep=1, detail=2, types=(1, 0, 1), segments=None)
    got = chk(dict(margin=0.25, sweep=0, detail=10, types=['ped', 2]))
    assert got == dict(margin=0.25, sweep=0, detail=10, types=(0, 1, 1), segments=None)
    seg = chk(dict(segments=[np.zeros((3, 4)), np.zeros((0, 4))]), n_scenes=2)['segments']
    assert seg[0].shape == (2, 3, 4) and seg[0].dtype == np.float32 and seg[1].tolist() == [3, 0]
    assert chk(dict(segments=np.zeros((2, 5, 4), np.float32)))['segments'][1].tolist() == [5, 5]
    again = chk(dict(segments=seg))['segments']                   # a checked value passes through
    assert again[0].shape == (2, 3, 4) and again[1].tolist() == [3, 0]
    for bad in (dict(margin=-0.1), dict(margin=float('nan')), dict(margin=float('inf')), dict(margin='1'), dict(margin=True),
                dict(sweep=2), dict(sweep='1'), dict(detail=3), dict(detail=0), dict(detail=True), dict(types='veh'),
                dict(types=['car']), dict(types=[3]), dict(types=5), dict(segments=np.zeros((2, 4))), dict(segments=[np.zeros((3, 3))]),
                dict(segments=[]), dict(segments=[np.array([['a'] * 4])]), dict(lanes=1), 'on', 1):
        with pytest.raises(ValueError):
            chk(bad)
    with pytest.raises(ValueError):
        chk(dict(segments=[np.zeros((1, 4))]), n_scenes=2)
    with pytest.raises(ValueError):
        chk(True, has_shape=False)


def test_road_buffers_refuse_an_unsupported_token_size():
    from infgen_amd import constraints
    conf = constraints.check_stay_on_road(True)
    assert constraints.road_buffers(None, 4, 64) is None
    b = constraints.road_buffers(conf, 4, 64)
    assert tuple(b['bits'].shape) == (4, 2) and int(b['bits'][0, 0]) == -1 and b['ident'].tolist() == [0, 1, 2, 3]
    for n in (48, 8192):
        with pytest.raises(ValueError):
            constraints.road_buffers(conf, 4, n)


def test_records_of_a_synthetic_scenes_edge_tokens_match_a_hand_computed_chord():
    from infgen_amd import synth
    cfg = synth.smart_config()
    scene = synth.make_scene(synth.scene_seed(1, 0), 8, 128, cfg)
    pt, mv = scene['pt_token'], synth.make_map_vocab()
    edge = np.flatnonzero(pt['type'] == rr.EDGE)
    assert edge.size >= 3, 'the synthetic map has road-edge tokens'
    for detail in (1, 2, 5, 10):
        rec = rr.records_from_map(pt['position'][None, :, :2], pt['orientation'][None], pt['type'][None], pt['token_idx'][None], [128], mv,
                                  detail)[0]
        assert rec.shape == (edge.size * detail, 8)
        # by hand: chord j of the second EDGE token
        m, j, hop = edge[1], detail - 1, 10 // detail
        th = float(pt['orientation'][m])
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        p0, p1 = R @ mv[pt['token_idx'][m], j * hop].astype(np.float64), R @ mv[pt['token_idx'][m], (j + 1) * hop].astype(np.float64)
        L = np.linalg.norm(p1 - p0)
        want = np.concatenate([pt['position'][m, :2], (p0 + p1) / 2, (p1 - p0) / L, [L / 2, L / 2]])
        assert np.allclose(rec[detail + j], want, rtol=0, atol=1e-12)
        assert np.array_equal(rec[detail + j][:2], pt['position'][m, :2].astype(np.float64)), 'the anchor is an exact copy'
    # fewer tokens in the map, a foreign token id, and a non-finite orientation
    ty, tok, ori = pt['type'].copy()[None], pt['token_idx'].copy()[None], pt['orientation'].copy()[None]
    tok[0, edge[0]] = 5000
    ori[0, edge[1]] = np.inf
    rec = rr.records_from_map(pt['position'][None, :, :2], ori, ty, tok, [int(edge[2]) + 1], mv, 2)[0]
    assert rec.shape == (4, 8) and (rec[:2, 7] == -1).all() and (rec[2:, 7] > 0).all()
    assert np.array_equal(rec[0], rr.NO_RECORD)
    # explicit segments: the anchor is p0, a zero-length segment is no obstacle
    sg = np.array([[[5000.0, -5000.0, 5003.0, -4996.0], [1.0, 1.0, 1.0, 1.0]]], np.float32)
    rec = rr.records_from_segments(sg, [2])[0]
    assert np.allclose(rec[0], [5000, -5000, 1.5, 2.0, 0.6, 0.8, 2.5, 2.5]) and np.array_equal(rec[1], rr.NO_RECORD)


@pytest.mark.parametrize('name', list(rr.CASES))
def test_band_conditions_and_what_the_cases_contain(name):
    """conditions on the chosen seeds, not measurements: at most 0.1 % of a case's (row, token) pairs have a smallest |sep| below
    BAND, at most one row has a straddle decision inside it - and every case holds the situations it was built for"""
    case, ref = _case(name)
    A, K, copies = case['A'], case['token_size'], case['copies']
    live = ref['live']
    in_band = (ref['min_abs_sep'] <= rr.BAND) & live[:, None]
    print(f'{name}: {int(live.sum())} ruled rows, {int(in_band.sum())} pairs in the band, {int(ref["straddle_band"].sum())} straddle rows in it')
    assert in_band.sum() <= 1e-3 * live.sum() * K
    assert ref['straddle_band'].sum() <= 1
    row0 = lambda ms: ms * copies * A
    # every count of records, the scene division, the list's capacity
    assert case['n_segments'].tolist() == [65, 0, 1, 63, 64, 150, 22]
    assert ref['kept'][row0(rr.RING)] > 128, 'more reachable records than the kernel keeps in one pass'
    assert ref['kept'][row0(rr.EMPTY)] == 0 and np.array_equal(ref['allowed'][row0(rr.EMPTY)], ref['base'][row0(rr.EMPTY)])
    if copies == 2:
        assert live[row0(rr.RING) + A] and ref['kept'][row0(rr.RING) + A] > 0, 'the second copy reads the same map scene'
    # the walled-in row: nothing left, the fallback hands back base(i)
    w = row0(rr.WALLED)
    assert ref['count'][w] == 0 and np.array_equal(ref['allowed'][w], ref['base'][w]) and ref['min_sep'][w].max() < -10 * rr.BAND
    # astride: segment 0 of MIXED is straddled by row 0 and is no obstacle of it; the zero-length segment is nobody's
    a = row0(rr.MIXED) + rr.ASTRIDE_ROW
    assert ref['straddle_sep'][a][0] < -0.5
    if a in ref['sep_end']:          # (the row has other obstacles: the straddled segment is not among them)
        assert not np.isfinite(ref['sep_end'][a][:, 0]).any() and not np.isfinite(ref['sep_path'][a][:, 0]).any()
    assert ref['straddle_sep'][a][rr.ZERO_LENGTH] == np.inf
    # the pedestrian beside a wall keeps base(i), the invalid row too; a vehicle or cyclist there would not
    p = row0(rr.MIXED) + rr.PED_ROW
    assert not live[p] and np.array_equal(ref['allowed'][p], ref['base'][p]) and not live[row0(rr.MIXED) + 3]
    assert (ref['pre'][live] != ref['base'][live]).any(axis=1).sum() >= 5, 'the rule bites on several rows'
    # the thin wall 6 m ahead: fast tokens whose end box lies beyond it - only the path rectangle sees them
    t = row0(rr.THIN_WALL)
    beyond = (ref['sep_end'][t][:, 0] > 0.1)
    if case['sweep']:
        caught = beyond & (ref['sep_path'][t][:, 0] < -0.1)
        assert caught.any() and not (ref['pre'][t] & caught).any()
    elif case['margin'] == 0.0:
        centre, _ = rr.token_end_poses(case['vocab'])
        jumped = beyond & (centre[0, :, 0] > 8.0) & ref['base'][t]
        assert jumped.any() and ref['pre'][t][jumped].all(), 'without the sweep a fast token jumps the wall'
