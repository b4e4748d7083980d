"""Operator-level tests of the two geometry kernels of the teacher-forced forward: k_radius_edges through infgen_radius_edges, in
the six combinations of filters, remaps, gap rules and buffer zones infgen_amd/forward_engine.py uses, and k_motion_features through
infgen_motion_features - against the plain float64 references of tests/graph_ref.py (radius_edges_ref, motion_features_ref).  Which
edges exist, their order, counts, totals, the index difference and the gap-rule constants are compared exactly (the generators
keep every candidate clear of the radius, and test_graph_ref_cpu.py shows that the same comparison tells the references'
deliberately wrong variants apart); distance, bearing and heading difference within graph_ref.BAR_*, the motion pair within
BAR_MOTION_FEAT_* (four times the error of an fp32 numpy evaluation).  Every array a kernel may write ends in a guard tail."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_ref as gr
from graph_ref import compare_lists
from gpu_blocks import SENT_F, SENT_I, Edges, guard_intact, guarded, guarded_copy, lib_and_check

pytestmark = pytest.mark.gpu

Q_KEYS = ('q_node', 'q_pt', 'q_c0', 'q_c1', 'q_self', 'q_pair_off')
ARRAY_KEYS = Q_KEYS + ('p_pos', 'p_head', 'p_inv', 'c_pos', 'c_head', 'c_inv', 'c_ok', 'c_src', 'pair_ok')


def call_radius_edges(g, cap, zero_total=True, **override):
    """one infgen_radius_edges call on device copies of a graph_ref case into a fresh sentinel-filled Edges (the zone above
    g['e_base']); override: fields of InfgenRadiusEdges set to other values than the case's.  The inputs must come back unchanged.
    -> (return code, the Edges)"""
    from infgen_amd import _lib
    lib, _ = lib_and_check()
    ten = {k: guarded_copy(g[k]) for k in ARRAY_KEYS if g[k] is not None}
    r = _lib.RadiusEdges()
    for k in ARRAY_KEYS:
        setattr(r, k, ten[k].data_ptr() if k in ten else None)
    r.n_q, r.radius, r.K, r.gap_rule, r.index_diff, r.e_base = len(g['q_node']), g['radius'], g['K'], g['gap_rule'], g['index_diff'], g['e_base']
    for k, v in override.items():
        setattr(r, k, v)
    e = Edges(g['n_nodes'], cap, base=g['e_base'])
    if zero_total:
        e.total[0] = 0                                   # the caller zeroes the total
    rc = lib.infgen_radius_edges(C.byref(r), C.byref(e.buf), None)
    torch.cuda.synchronize()
    for k, t in ten.items():                             # the inputs are read only
        n = g[k].size
        assert guard_intact(t, n) and np.array_equal(t[:n].cpu().numpy(), g[k].reshape(-1)), k
    return rc, e


def run_radius_edges(g, cap):
    _, check = lib_and_check()
    rc, e = call_radius_edges(g, cap)
    check(rc, 'infgen_radius_edges')
    return e.host()


def check_radius_edges(g, ref, out, cap):
    """everything but the lists themselves: the total, sentinels of the nodes without a query, the live ranges tiling the zone,
    nothing below the zone's base"""
    off, cnt, src, raw, tot = out
    base, qn = g['e_base'], g['q_node']
    total = sum(len(r[0]) for r in ref)
    assert tot == total, (tot, total)
    noq = np.setdiff1d(np.arange(g['n_nodes']), qn)
    assert all(len(ref[n][0]) == 0 for n in noq)
    assert (off[noq] == SENT_I).all() and (cnt[noq] == SENT_I).all(), 'a node without a query lost its off / cnt'
    assert ((off[qn] >= base) & (off[qn] <= base + total)).all()
    assert (src[:base] == SENT_I).all() and (raw[:base] == np.float32(SENT_F)).all(), 'written below the base of the zone'
    if total <= cap:
        # the live rows' ranges tile [base, base + total): the workgroups' ranges may come in any order
        o, c = off[qn][cnt[qn] > 0], cnt[qn][cnt[qn] > 0]
        order = np.argsort(o)
        assert np.array_equal(base + np.cumsum(c[order]) - c[order], o[order])
        assert (src[base + total:] == SENT_I).all() and (raw[base + total:] == np.float32(SENT_F)).all()


@pytest.mark.parametrize('name', list(gr.RADIUS_EDGES_CASES))
def test_radius_edges_matches_the_reference(name):
    """temporal (r * r = inf, history mask, permuted node map, index difference, empty ranges), agent (three scenes in one launch,
    self, the cap after several chunks with masked candidates counted), seed_pair (per-pair filter, offsets of -1, the upper zone of
    a shared buffer), map (gap rule 2, no candidate validity, a scene without tokens), map_graph (no validity at all); cap = exactly
    the total"""
    g = gr.gen_radius_edges(name)
    ref, _ = gr.radius_edges_ref(g)
    cap = max(sum(len(r[0]) for r in ref), 1)
    out = run_radius_edges(g, cap)
    off, cnt, src, raw, tot = out
    qn = g['q_node']
    err = compare_lists(name, off[qn], cnt[qn], src, raw, [ref[n] for n in qn], cap=g['e_base'] + cap)
    check_radius_edges(g, ref, out, cap)
    print(f'radius_edges {name}: {tot} edges, device errors dist {err[0]:.3g} bearing {err[1]:.3g} dth {err[2]:.3g} '
          f'(bars {gr.BAR_DIST:.3g} {gr.BAR_BEARING:.3g} {gr.BAR_DTH:.3g})')


@pytest.mark.parametrize('name', ['agent', 'seed_pair'])
def test_radius_edges_overflow(name):
    """cap = total - 1: the total is reported, exactly the lists whose range would pass the cap have cnt = 0, the others are complete,
    nothing is written at or beyond the cap (guard tails) - nor, for the upper zone, below its base"""
    g = gr.gen_radius_edges(name)
    ref, _ = gr.radius_edges_ref(g)
    total = sum(len(r[0]) for r in ref)
    cap = total - 1
    out = run_radius_edges(g, cap)
    off, cnt, src, raw, tot = out
    qn = g['q_node']
    assert tot == total > cap
    compare_lists(name, off[qn], cnt[qn], src, raw, [ref[n] for n in qn], cap=g['e_base'] + cap)
    check_radius_edges(g, ref, out, cap)
    lost = [n for n in qn if len(ref[n][0]) and off[n] + len(ref[n][0]) > g['e_base'] + cap]
    assert len(lost) == 1 and cnt[lost[0]] == 0
    assert all(cnt[n] == len(ref[n][0]) for n in qn if n != lost[0])


def test_radius_edges_are_strict_on_exact_coordinates():
    """gen_strict_radius's integer coordinates, exact in fp32, through infgen_radius_edges: a point at exactly r is absent, at
    nextafter(r) present"""
    for g, i, present in gr.gen_strict_radius_edges():
        ref, _ = gr.radius_edges_ref(g)
        off, cnt, src, raw, tot = run_radius_edges(g, 16)
        compare_lists('strict', off, cnt, src, raw, ref, cap=16)
        assert tot == len(ref[0][0])
        assert (i in src[off[0]:off[0] + cnt[0]]) == present, (g['radius'], i)


def test_radius_edges_refusals():
    """K <= 0 and a gap rule outside 0..2 are errors that touch no buffer (the total included: not zeroed here, it keeps its
    sentinel); no query is no error and writes nothing either"""
    g = gr.gen_radius_edges('map')
    for override, refused in ((dict(K=0), True), (dict(K=-3), True), (dict(gap_rule=3), True), (dict(gap_rule=-1), True), (dict(n_q=0), False)):
        rc, e = call_radius_edges(g, 64, zero_total=False, **override)
        assert (rc != 0) == refused, (override, rc)
        off, cnt, src, raw, tot = e.host()
        assert (off == SENT_I).all() and (cnt == SENT_I).all() and (src == SENT_I).all() and (raw == np.float32(SENT_F)).all()
        assert tot == SENT_I, override


# ------------------------------------------------------------------------------------------------ infgen_motion_features
@pytest.mark.parametrize('mask', [False, True], ids=['nomask', 'mask'])
@pytest.mark.parametrize('shape', gr.MOTION_FEATURES_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_motion_features(shape, mask):
    """(rows, T) = (7, 1), (3, 2), (37, 19) - one column, two, and 703 elements over three workgroups - with and without the gap mask:
    columns 2 and 3 exactly 0, the norms of the rule constants exact, norm and angle within the bars, nothing written past the end"""
    lib, check = lib_and_check()
    c = gr.gen_motion_features()[gr.MOTION_FEATURES_SHAPES.index(shape)]
    rows, T = shape
    assert c['state'].shape == shape
    gm = c['gap_mask'] if mask else None
    ten = {k: guarded_copy(c[k]) for k in ('pos', 'head', 'state')}
    if mask:
        ten['gap_mask'] = guarded_copy(gm)
    out = guarded(rows * T, torch.float32, 4)
    check(lib.infgen_motion_features(ten['pos'].data_ptr(), ten['head'].data_ptr(), ten['state'].data_ptr(),
                                     ten['gap_mask'].data_ptr() if mask else None, rows, T, out.data_ptr(), None), 'infgen_motion_features')
    torch.cuda.synchronize()
    assert guard_intact(out, rows * T, 4), 'written beyond the last element'
    for k, t in ten.items():
        assert guard_intact(t, c[k].size) and np.array_equal(t[:c[k].size].cpu().numpy(), c[k].reshape(-1)), k
    got = out[:rows * T * 4].cpu().numpy().reshape(rows, T, 4)
    ref, ruled = gr.motion_features_ref(c['pos'], c['head'], c['state'], gm, with_ruled=True)
    e = gr.compare_motion(got, ref, ruled)
    print(f'motion_features {shape} mask={mask}: device errors norm {e[0]:.3g} angle {e[1]:.3g} '
          f'(bars {gr.BAR_MOTION_FEAT_NORM:.3g} {gr.BAR_MOTION_FEAT_ANGLE:.3g})')
