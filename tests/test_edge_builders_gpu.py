"""Operator-level tests of the edge builders: infgen_map_graph, infgen_build_edges and infgen_point_edges called through their C
entries with hand-built state blocks, at shapes the rollout fixtures never reach, against the plain float64 reference of
tests/graph_ref.py.  Which edges exist, their order, counts, offsets and totals are compared exactly (the generators keep every
candidate clear of the radii: test_graph_ref_cpu.py); the raw features within four times the error of an fp32 numpy evaluation
(graph_ref.BAR_*).  Every buffer a kernel may write ends in a guard tail that must stay untouched."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_ref as gr
from graph_ref import compare_lists
from gpu_blocks import SENT_F, SENT_I, Edges, dev, device_block, lib_and_check

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ infgen_map_graph
def run_map_graph(g, cap):
    lib, check = lib_and_check()
    S, M_cap = g['S'], g['M_cap']
    n_map, pos, orient = (torch.from_numpy(g[k]).to(dev()) for k in ('n_map', 'pos', 'orient'))
    e = Edges(S * M_cap, cap)
    check(lib.infgen_map_graph(S, M_cap, n_map.data_ptr(), pos.data_ptr(), orient.data_ptr(), g['radius'], g['max_nbr'],
                               e.buf.off, e.buf.cnt, e.buf.src, e.buf.raw, e.buf.total, cap, None), 'infgen_map_graph')
    return e.host()


@pytest.mark.parametrize('name', list(gr.MAP_GRAPH_CASES))
def test_map_graph_matches_the_reference(name):
    """the LDS path, the global scan (a workgroup spanning two scenes, a ragged last workgroup), more than 4096 tokens (no lane
    masks), more than 128 kept neighbours (the chunk path); ragged n_map with 0 and 1; cap = exactly the total"""
    g = gr.gen_map_graph(name)
    ref, _ = gr.map_graph_ref(g['n_map'], g['pos'], g['orient'], g['radius'], g['max_nbr'])
    total = sum(len(r[0]) for r in ref)
    off, cnt, src, raw, tot = run_map_graph(g, total)
    assert tot == total
    err = compare_lists(name, off, cnt, src, raw, ref, cap=total)
    print(f'map_graph {name}: {total} edges, device errors dist {err[0]:.3g} bearing {err[1]:.3g} dth {err[2]:.3g}')
    # the rows' ranges tile [0, total): the workgroups' ranges may come in any order
    live = cnt > 0
    order = np.argsort(off[live])
    assert np.array_equal(np.cumsum(cnt[live][order]) - cnt[live][order], off[live][order])
    for s, n in enumerate(g['n_map']):
        assert (cnt[s * g['M_cap'] + n:(s + 1) * g['M_cap']] == 0).all()


@pytest.mark.parametrize('name', ['lds_1024', 'global_40', 'dense_200'])
def test_map_graph_overflow_reports_and_writes_nothing_beyond_cap(name):
    """cap = total - 1: total > cap is reported, exactly the rows whose range would pass cap have cnt = 0, the others are complete,
    and nothing is written at or beyond cap (guard tails)"""
    g = gr.gen_map_graph(name)
    ref, _ = gr.map_graph_ref(g['n_map'], g['pos'], g['orient'], g['radius'], g['max_nbr'])
    total = sum(len(r[0]) for r in ref)
    off, cnt, src, raw, tot = run_map_graph(g, total - 1)
    assert tot == total and tot > total - 1
    compare_lists(name, off, cnt, src, raw, ref, cap=total - 1)
    lost = [row for row, r in enumerate(ref) if len(r[0]) and off[row] + len(r[0]) > total - 1]
    assert len(lost) == 1 and cnt[lost[0]] == 0


def test_radius_tests_are_strict_on_exact_coordinates():
    """integer coordinates, exact in fp32 whatever the contraction: a point at exactly r is absent, at nextafter(r) present - for
    the map graph, the three sets of build_edges' column and both point searches"""
    lib, check = lib_and_check()
    pts, cases = gr.gen_strict_radius()
    n = len(pts)
    for r, i, present in cases:
        r = float(r)
        g = dict(S=1, M_cap=32, n_map=np.asarray([n], np.int32), pos=np.zeros((1, 32, 2), np.float32),
                 orient=np.zeros((1, 32), np.float32), radius=r, max_nbr=16)
        g['pos'][0, :n] = pts
        off, cnt, src, raw, tot = run_map_graph(g, 64)
        assert (i in src[off[0]:off[0] + cnt[0]]) == present, ('map_graph', r, i)
        st = gr.new_state(1, 32, 3, 32, r_map=r, r_agent=r)
        st['n_agents'][0], st['n_map'][0] = n, n
        st['pos'][0, 1, :n], st['map_pos'][0, :n] = pts, pts
        st['state'][:] = gr.VALID
        ed = {k: Edges(32, 64) for k in 'tma'}
        b, keep = device_block(st, ed)
        check(lib.infgen_build_edges(C.byref(b), 1, 0, None), 'infgen_build_edges')
        for k in 'ma':
            off, cnt, src, raw, tot = ed[k].host()
            assert (i in src[off[0]:off[0] + cnt[0]]) == present, (k, r, i)
        pa, pm = Edges(1, 64), Edges(1, 64)
        centre = torch.zeros(1, dtype=torch.int32, device=dev())
        check(lib.infgen_point_edges(C.byref(b), 1, centre.data_ptr(), None, 0, 3, r, 16, r, 16, C.byref(pa.buf), C.byref(pm.buf), None),
              'infgen_point_edges')
        for k, e in (('pa', pa), ('pm', pm)):
            off, cnt, src, raw, tot = e.host()
            assert (i in src[off[0]:off[0] + cnt[0]]) == present, (k, r, i)


# ------------------------------------------------------------------------------------------------ infgen_build_edges
def run_build_edges(st, c, caps, edgeless=0):
    lib, check = lib_and_check()
    rows = st['S'] * st['A_cap']
    ed = {k: Edges(rows, caps[k]) for k in 'tma'}
    b, keep = device_block(st, ed)
    check(lib.infgen_build_edges(C.byref(b), c, edgeless, None), 'infgen_build_edges')
    return {k: ed[k].host() for k in 'tma'}


def check_build_edges(st, c, out, ref, caps=None):
    S, A_cap = st['S'], st['A_cap']
    errs = {}
    for k in 'tma':
        off, cnt, src, raw, tot = out[k]
        total = sum(len(r[0]) for r in ref[k])
        assert tot == total, (k, tot, total)
        errs[k] = compare_lists(k, off, cnt, src, raw, ref[k], cap=caps[k] if caps else None, written=False)
        o, n = off.reshape(S, A_cap), cnt.reshape(S, A_cap)
        assert np.array_equal(o[:, 1:], o[:, :-1] + n[:, :-1]), (k, 'offsets are not an exclusive scan within a scene')
        bases = np.sort(o[:, 0])
        assert bases[0] == 0 and np.array_equal(np.sort(o[:, 0] + n.sum(1)), np.append(bases[1:], total))      # the scenes tile [0, total)
        for s, A in enumerate(st['n_agents']):
            assert (n[s, A:] == 0).all(), (k, s)
    return errs


@pytest.mark.parametrize('name,c,overrides', [('cap32', 1, True), ('cap32', 11, True), ('cap32', 12, False), ('cap32', 17, True),
                                              ('cap256', 17, True), ('cap1024', 11, True)])
def test_build_edges_matches_the_reference(name, c, overrides):
    """A in {1, 10, 11, 32 | 63, 64, 65, 200 | 700}, c in {1, W - 1, W, T - 1}; INVALID states, imask / tmask zeros, bos inside the
    window, first_new / hv_ovr set (and null in one call), map slots shared and permuted with n_map in {0, 3, 700}; the cluster of
    cap1024 has more than 301 rows in radius of 400 destinations, and its 4160 map tokens are scanned in global memory"""
    st, c = gr.gen_build_edges(name, c, overrides=overrides)
    ref = gr.build_edges_ref(st, c)
    caps = {k: max(sum(len(r[0]) for r in ref[k]), 1) for k in 'tma'}
    errs = check_build_edges(st, c, run_build_edges(st, c, caps), ref)
    for k in 'tma':
        print(f'build_edges {name} c={c} {k}: {caps[k]} edges, device errors dist {errs[k][0]:.3g} bearing {errs[k][1]:.3g} dth {errs[k][2]:.3g}')


def test_build_edges_256_and_1024_thread_instantiations_agree_bit_for_bit():
    """130 scenes at A_cap = 256 take k_build_edges<256>, two of them alone k_build_edges<1024>: both match the reference, and the
    lists and raw features of the two scenes are the same bits"""
    st, c = gr.gen_build_edges('cap256')
    pick = [6, 5]                                        # 200 and 65 agents
    assert st['S'] > 128 and [int(st['n_agents'][s]) for s in pick] == [200, 65]
    ref = gr.build_edges_ref(st, c)
    caps = {k: sum(len(r[0]) for r in ref[k]) for k in 'tma'}
    big = run_build_edges(st, c, caps)
    errs = check_build_edges(st, c, big, ref)
    for k in 'tma':
        print(f'build_edges cap256 c={c} {k}: {caps[k]} edges, device errors dist {errs[k][0]:.3g} bearing {errs[k][1]:.3g} dth {errs[k][2]:.3g}')
    st2 = gr.take_scenes(st, pick)
    ref2 = gr.build_edges_ref(st2, c)
    caps2 = {k: sum(len(r[0]) for r in ref2[k]) for k in 'tma'}
    small = run_build_edges(st2, c, caps2)
    check_build_edges(st2, c, small, ref2)
    A_cap, rows, rows2 = st['A_cap'], st['S'] * st['A_cap'], 2 * st['A_cap']
    for k in 'tma':
        off, cnt, src, raw, _ = big[k]
        off2, cnt2, src2, raw2, _ = small[k]
        for i, s in enumerate(pick):
            for a in range(A_cap):
                r1, r2 = s * A_cap + a, i * A_cap + a
                assert cnt[r1] == cnt2[r2]
                x, y = src[off[r1]:off[r1] + cnt[r1]].astype(np.int64), src2[off2[r2]:off2[r2] + cnt2[r2]].astype(np.int64)
                if k == 't':
                    x, y = x // rows, y // rows2
                elif k == 'a':
                    x, y = x - s * A_cap, y - i * A_cap
                assert np.array_equal(x, y), (k, s, a)
                assert np.array_equal(raw[off[r1]:off[r1] + cnt[r1]].view(np.int32), raw2[off2[r2]:off2[r2] + cnt2[r2]].view(np.int32)), (k, s, a)


def test_build_edges_edgeless_clears_counts_and_writes_no_edge():
    st, c = gr.gen_build_edges('cap32', 12)
    out = run_build_edges(st, c, {k: 8 for k in 'tma'}, edgeless=1)
    for k in 'tma':
        off, cnt, src, raw, tot = out[k]
        assert (off == 0).all() and (cnt == 0).all()
        assert (src == SENT_I).all() and (raw == np.float32(SENT_F)).all() and tot == SENT_I          # (edgeless leaves the totals alone)


@pytest.mark.parametrize('short', ['t', 'm', 'a'])
def test_build_edges_buffer_one_edge_too_small(short):
    """counts and offsets are still reported in full, total > cap, the edges below cap are right and nothing lands beyond it"""
    st, c = gr.gen_build_edges('cap32', 12)
    ref = gr.build_edges_ref(st, c)
    caps = {k: sum(len(r[0]) for r in ref[k]) - (1 if k == short else 0) for k in 'tma'}
    assert caps[short] > 0
    out = run_build_edges(st, c, caps)
    check_build_edges(st, c, out, ref, caps=caps)
    assert out[short][4] == caps[short] + 1 > caps[short]


# ------------------------------------------------------------------------------------------------ infgen_point_edges
def run_point_edges(g, active, exclude, which, cap_a=None, cap_m=None):
    lib, check = lib_and_check()
    st, c = g['st'], g['c']
    ref = gr.point_edges_ref(st, c, g['centre_row'], active, exclude, g['r_agent'], g['k_agent'], g['r_map'], g['k_map'])
    tot = {k: sum(len(r[0]) for r in ref[k]) for k in 'am'}
    ea = Edges(st['S'], max(tot['a'], 1) if cap_a is None else cap_a)
    em = Edges(st['S'], max(tot['m'], 1) if cap_m is None else cap_m)
    b, keep = device_block(st)
    cr = torch.from_numpy(g['centre_row']).to(dev())
    act = torch.from_numpy(np.asarray(active, np.int32)).to(dev()) if active is not None else None
    check(lib.infgen_point_edges(C.byref(b), c, cr.data_ptr(), act.data_ptr() if act is not None else None, exclude, which,
                                 g['r_agent'], g['k_agent'], g['r_map'], g['k_map'], C.byref(ea.buf), C.byref(em.buf), None),
          'infgen_point_edges')
    return ref, tot, ea, em


@pytest.mark.parametrize('name', list(gr.POINT_EDGES_CASES))
@pytest.mark.parametrize('which,exclude,act', [(3, 1, 'null'), (3, 0, 'mixed'), (1, 1, 'mixed'), (2, 0, 'null'), (3, 1, 'zero')])
def test_point_edges_matches_the_reference(name, which, exclude, act):
    """K = 24 / 128 and 300 / 2048 as production calls them, the K-th hit in a later 64-trip than the first, imask == 0 sources inside
    the first K (filtered after the cap), centre rows other than the ego, shared map slots, a scene without a hit; `which` selects the
    sets (the other buffer stays untouched), `active` null / mixed / all zero"""
    g = gr.gen_point_edges(name)
    S = g['st']['S']
    active = {'null': None, 'mixed': [s % 3 != 1 for s in range(S)], 'zero': [0] * S}[act]
    ref, tot, ea, em = run_point_edges(g, active, exclude, which)
    for k, e, bit in (('a', ea, 1), ('m', em, 2)):
        off, cnt, src, raw, total = e.host()
        if not which & bit:
            assert (off == SENT_I).all() and (cnt == SENT_I).all() and (src == SENT_I).all() and total == SENT_I
            continue
        assert total == tot[k]
        err = compare_lists(k, off, cnt, src, raw, ref[k], cap=e.cap)
        empty = [s for s in range(S) if len(ref[k][s][0]) == 0]
        assert empty and all(off[s] == 0 and cnt[s] == 0 for s in empty)            # no hit / inactive: off = cnt = 0
        if act == 'zero':
            assert total == 0
        print(f'point_edges {name} {k} which={which} active={act}: {total} edges, device errors dist {err[0]:.3g} bearing {err[1]:.3g} dth {err[2]:.3g}')


def test_point_edges_cap_reached_drops_that_scene_only():
    g = gr.gen_point_edges('heading_24_128')
    ref, tot, ea, em = run_point_edges(g, None, 1, 3)
    ref, tot, ea, em = run_point_edges(g, None, 1, 3, cap_a=tot['a'] - 1, cap_m=tot['m'] - 1)
    for k, e in (('a', ea), ('m', em)):
        off, cnt, src, raw, total = e.host()
        assert total == tot[k] > e.cap
        compare_lists(k, off, cnt, src, raw, ref[k], cap=e.cap)
        lost = [s for s in range(g['st']['S']) if len(ref[k][s][0]) and off[s] + len(ref[k][s][0]) > e.cap]
        assert len(lost) == 1 and cnt[lost[0]] == 0
