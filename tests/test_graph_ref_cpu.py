"""Anchors of tests/graph_ref.py (the plain float64 reference of the edge builders and insertion kernels) and of the input
generators the GPU tests use: the reference agrees with the oracle's helpers, with the reference project's own edge lists
(tests/golden/*_internals.npz) and with torch's softmax -> topk -> cumsum; every generator clears its ambiguity margin and reaches
the branch it is meant for; the fp32 figures the device bars are derived from still hold; the deliberately wrong variants of the
forward's two references fail the comparison the GPU tests apply."""
import math
import os

import numpy as np
import pytest
import torch

import graph_ref as gr
from conftest import GOLDEN, load_case


# ------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_first_k_within_equals_the_oracle_radius(seed):
    """k below, equal to and above the number of hits of every query"""
    from oracle.rollout_oracle import radius_first_k
    rng = np.random.default_rng(seed)
    x = rng.uniform(-50, 50, (300, 2)).astype(np.float32)
    y = rng.uniform(-50, 50, (40, 2)).astype(np.float32)
    r = 20.0
    hits = [len(gr.first_k_within(q, x, r, 10 ** 6)[0]) for q in y]
    assert min(hits) >= 2
    for k in (1, min(hits) - 1, min(hits), int(np.median(hits)), max(hits), max(hits) + 5):
        yi, xi = radius_first_k(torch.from_numpy(x).double(), torch.from_numpy(y).double(), r, k)
        for q in range(len(y)):
            mine, gap = gr.first_k_within(y[q], x, r, k)
            assert gap > 0
            assert np.array_equal(mine, xi[yi == q].numpy()), (k, q)


def test_first_k_within_is_strict():
    pts, cases = gr.gen_strict_radius()
    for r, i, present in cases:
        hits, _ = gr.first_k_within(pts[0], pts, r, 10)
        assert (i in hits) == present, (r, i)


def _fixture_state(case):
    """the block of a golden rollout at every column: the host scene setup (as test_host_scene_setup_matches_oracle_masks obtains it)
    for the history columns, then the fixture's own poses / states - recorded results, no network evaluation - for the decoded ones"""
    from infgen_amd.engine import RolloutEngine
    c = load_case(case)
    dummy = RolloutEngine.__new__(RolloutEngine)
    dummy.cfg = c['cfg']
    h = RolloutEngine._setup_scene(dummy, c['scene'])
    z, cfg = c['z'], c['cfg']
    A, M, T = h['A'], h['M'], cfg.num_columns
    st = gr.new_state(1, (A + 31) // 32 * 32, T, M, W=cfg.time_span // cfg.shift, ring=cfg.time_span // cfg.shift + 1,
                      r_map=cfg.pl2a_radius, r_agent=cfg.a2a_radius)
    st['n_agents'][0], st['n_map'][0], st['av_index'][0] = A, M, h['av']
    hc = cfg.hist_columns
    pos, head, state = z['pos_a'].astype(np.float32), z['head_a'].astype(np.float32), z['next_state_idx'].astype(np.int32)
    assert np.array_equal(pos[:, :hc], h['pos'][:, :hc]) and np.array_equal(state[:, :hc], h['state'][:, :hc])
    st['pos'][0, :, :A] = pos.transpose(1, 0, 2)
    st['head'][0, :, :A] = head.T
    st['state'][0, :, :A] = state.T
    tm, im = h['tmask'].copy(), h['imask'].copy()
    im[:, hc:] &= state[:, hc:] != gr.INVALID             # a row decoded INVALID leaves the interaction mask
    st['tmask'][0, :, :A], st['imask'][0, :, :A] = tm.T, im.T
    st['bos'][0, :A] = h['bos']
    st['map_pos'][0, :M], st['map_orient'][0, :M] = h['map_pos'], h['map_orient']
    return st, c, hc


@pytest.mark.parametrize('case', ['c1_a8_m128', 'a24_m256_edge', 'c3_a64_m1024'])
def test_build_edges_ref_reproduces_the_reference_edge_lists(case):
    """edges_t / edges_m / edges_a of the reference project's own builders, ALL decode steps: the fixtures record the poses and states
    of every column, so the block can be advanced through the whole rollout without evaluating the network"""
    st, c, hc = _fixture_state(case)
    zi = np.load(os.path.join(GOLDEN, case + '_internals.npz'))
    A_cap, rows, ring, M_cap = st['A_cap'], st['A_cap'], st['ring'], st['M_cap']
    got = {k: [] for k in 'tma'}
    steps = c['cfg'].num_decode_steps
    for t in range(steps):
        col = hc - 1 + t
        ref = gr.build_edges_ref(st, col)
        for kind in 'tma':
            for a, (src, _, _) in enumerate(ref[kind]):
                if kind == 't':
                    assert np.all(src % rows == a)
                    val = col - ((col - src // rows) % ring)
                else:
                    val = src % (M_cap if kind == 'm' else A_cap)
                got[kind] += [(t, a, int(v)) for v in val]
    for kind, key in (('t', 'edges_t'), ('m', 'edges_m'), ('a', 'edges_a')):
        mine = np.asarray(sorted(got[kind]), np.int32).reshape(-1, 3)
        want = zi[key]
        want = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
        assert np.array_equal(mine, want), (kind, len(mine), len(want))
        assert want[:, 0].max(initial=-1) in (-1, steps - 1)


def test_topk_references_agree_with_torch_softmax_topk_cumsum():
    """seeded logits with ties: torch.softmax -> topk -> cumsum in float64, the pick the first j with u * cdf[-1] < cdf[j].  torch.topk
    leaves the order of equal values open, so the picked VALUE is compared with topk and the picked INDEX with a stable descending
    sort (value descending, index ascending - the order the kernels document)"""
    for k in (1, 2, 16):
        lg, u, kinds = gr.gen_sample_topk(60, 64, k, seed=3)
        tok, _ = gr.sample_topk_ref(lg, k, u)
        p = torch.softmax(torch.from_numpy(lg).double(), -1)
        pk, _ = torch.topk(p, k, dim=-1)
        ps, idx = torch.sort(p, dim=-1, descending=True, stable=True)
        assert torch.equal(ps[:, :k], pk)
        cdf = torch.cumsum(pk, -1)
        x = torch.from_numpy(u).double() * cdf[:, -1]
        pick = (x[:, None] >= cdf).sum(-1).clamp(max=k - 1)
        exact = np.asarray([kd == 'ties' for kd in kinds])         # (their boundaries are exact in exp(v - v0), not in softmax)
        mine_pick = np.asarray([list(idx[r, :k].numpy()).index(tok[r]) for r in range(len(tok))])
        assert np.array_equal(mine_pick[~exact], pick.numpy()[~exact])
        assert np.array_equal(lg[np.arange(len(tok)), tok][~exact], lg[np.arange(len(tok)), idx[np.arange(len(tok)), pick].numpy()][~exact])
        # the exact rows: u = j / k over k equal probabilities picks the j-th of them in ascending index
        for r in np.nonzero(exact)[0]:
            j = int(round(float(u[r]) * k)) if k > 1 else 0
            assert tok[r] == np.nonzero(lg[r] == 5.0)[0][j]


def test_insert_decide_ref_cell_choice_agrees_with_torch():
    from infgen_amd import synth
    grid = synth.build_grid()
    G = grid.shape[0]
    for k in (2, 16):
        st, dec, names, max_new = gr.gen_insert_decide(G, grid, k, 0)
        rst, rdec = gr.as_ref(st), gr.as_ref(dec)
        for s, name in enumerate(names):
            gr.insert_decide_ref(rst, rdec, s, 0, 0, max_new, sample_k=k)
            if rdec['inserted'][s] != 1 or name in ('cell_tie', 'u_partial_sum'):
                continue
            p = torch.softmax(torch.from_numpy(dec['lg_pos'][s]).double(), -1)
            ps, idx = torch.sort(p, descending=True, stable=True)
            cdf = torch.cumsum(ps[:k], -1)
            pick = int((float(dec['uniform'][s]) * cdf[-1] >= cdf).sum().clamp(max=k - 1))
            assert rdec['new_cell'][s] == int(idx[pick]), name


# ------------------------------------------------------------------------------------------------ generators: margin, branch, fp32 figures
def _kth_hit_chunk(centre, cand, r, k):
    hits, _ = gr.first_k_within(centre, cand, r, k)
    return (hits[0] // 64, hits[-1] // 64, len(hits)) if len(hits) else (0, 0, 0)


@pytest.mark.parametrize('name', list(gr.MAP_GRAPH_CASES))
def test_map_graph_generator(name):
    g = gr.gen_map_graph(name)
    ref, gap = gr.map_graph_ref(g['n_map'], g['pos'], g['orient'], g['radius'], g['max_nbr'])
    assert gap > gr.MARGIN, gap
    cnt = np.asarray([len(r[0]) for r in ref]).reshape(g['S'], g['M_cap'])
    assert cnt.sum() > 0 and all(cnt[s, n:].sum() == 0 for s, n in enumerate(g['n_map']))
    if name == 'dense_200':
        # the chunk path, and the cap inside it: 200 kept where the centre is among its first 201 hits, else all 201
        assert (cnt > 128).sum() >= 10 and cnt.max() == 201 and (cnt == 200).any()
    else:
        assert (cnt == g['max_nbr']).any() and (cnt < g['max_nbr']).any()
    if name in ('global_1000', 'global_40'):
        assert g['M_cap'] % 32 and (g['S'] * g['M_cap']) % 32        # a workgroup's 32 centres span two scenes; a ragged last one
    if name == 'nomask_4160':
        assert g['n_map'].max() > 4096 and g['M_cap'] > 4096
        # the cap is reached in a later 64-chunk than the first hit
        assert any(len(r[0]) == g['max_nbr'] and r[0][-1] // 64 > r[0][0] // 64 for r in ref)
    f32 = gr.map_graph_ref(g['n_map'], g['pos'], g['orient'], g['radius'], g['max_nbr'], f=np.float32)[0]
    e = gr.raw_errors(ref, f32)
    print(f'map_graph {name}: fp32 numpy errors dist {e[0]:.4g} bearing {e[1]:.4g} dth {e[2]:.4g}')
    assert e[0] <= gr.FP32_ERR_DIST and e[1] <= gr.FP32_ERR_BEARING and e[2] <= gr.FP32_ERR_DTH


@pytest.mark.parametrize('name,c', [('cap32', 1), ('cap32', 11), ('cap32', 12), ('cap32', 17), ('cap256', None), ('cap256', 17),
                                    ('cap1024', None)])
def test_build_edges_generator(name, c):
    st, c = gr.gen_build_edges(name, c)
    assert gr.build_edges_margin(st, c) > gr.MARGIN
    ref = gr.build_edges_ref(st, c)
    S, A_cap = st['S'], st['A_cap']
    cnt = {k: np.asarray([len(r[0]) for r in ref[k]]).reshape(S, A_cap) for k in 'tma'}
    for s, A in enumerate(st['n_agents']):
        assert all(cnt[k][s, A:].sum() == 0 for k in 'tma')
        assert cnt['t'][s, max(A - 10, 0):].sum() == 0                # the A - 10 rule
        if A <= 10:
            assert cnt['t'][s].sum() == 0
    assert sorted(set(st['n_agents'].tolist())) == sorted(set(gr.BUILD_EDGES_CASES[name][0]))
    rows = np.nonzero(np.arange(A_cap)[None] < st['n_agents'][:, None])
    assert (st['imask'][:, c][rows] == 0).any() and (st['state'][:, c][rows] == gr.INVALID).any()
    if name != 'cap32' or c > 1:
        assert cnt['t'].sum() > 0
        lo = max(c - st['W'], 0)
        assert ((st['bos'] > lo) & (st['bos'] < c)).any() and (st['tmask'][:, lo:c] == 0).any()
    for k in 'tma':                                                   # every gap rule occurs
        ruled = np.concatenate([r[2] for r in ref[k]])
        both = gr.RULED_DIST | gr.RULED_DTH            # (destination INVALID only: the distance alone is a constant)
        assert set(ruled.tolist()) == ({0, both} if k == 'm' else {0, gr.RULED_DIST, both}), k
    assert st['first_new'] is not None and any(f < A for f, A in zip(st['first_new'], st['n_agents']))
    ms = st['map_scene']
    assert len(set(ms.tolist())) < S or name == 'cap1024'             # map slots are shared ...
    assert not np.array_equal(ms, np.arange(S)) or name == 'cap1024'  # ... and permuted
    assert (cnt['m'] == 5).any() and (cnt['m'][rows] < 5).any()
    if name == 'cap256':
        assert S > 128 and st['n_agents'].max() > 128                 # scans over more than one (and more than two) 64-lane trips
    if name == 'cap1024':
        # more than 301 rows in radius of several destinations: the candidate cap falls inside a ballot of a later trip
        over = 0
        for a in range(int(st['n_agents'][0])):
            n_in = len(gr.first_k_within(st['pos'][0, c, a], st['pos'][0, c, :st['n_agents'][0]], st['r_agent'], 10 ** 6)[0])
            over += n_in > gr.A2A_CANDIDATES
        assert over >= 100
        assert st['M_cap'] > 4096 and st['n_map'][st['map_scene'][0]] > 4096          # the map scan in global memory
    f32 = gr.build_edges_ref(st, c, f=np.float32)
    for k in 'tma':
        e = gr.raw_errors(ref[k], f32[k])
        print(f'build_edges {name} c={c} {k}: fp32 numpy errors dist {e[0]:.4g} bearing {e[1]:.4g} dth {e[2]:.4g}')
        assert e[0] <= gr.FP32_ERR_DIST and e[1] <= gr.FP32_ERR_BEARING and e[2] <= gr.FP32_ERR_DTH


@pytest.mark.parametrize('name', list(gr.POINT_EDGES_CASES))
def test_point_edges_generator(name):
    g = gr.gen_point_edges(name)
    st, c, cr = g['st'], g['c'], g['centre_row']
    gaps, chunks_a, chunks_m, capped_then_masked = [], [], [], False
    for s in range(st['S']):
        A, ms = int(st['n_agents'][s]), int(st['map_scene'][s])
        centre = st['pos'][s, c, cr[s]]
        others = np.delete(st['pos'][s, c, :A].astype(np.float64), cr[s], axis=0)
        gaps += [gr.first_k_within(centre, others, g['r_agent'], 1)[1],
                 gr.first_k_within(centre, st['map_pos'][ms, :st['n_map'][ms]], g['r_map'], 1)[1]]
        chunks_a.append(_kth_hit_chunk(centre, st['pos'][s, c, :A], g['r_agent'], g['k_agent']))
        chunks_m.append(_kth_hit_chunk(centre, st['map_pos'][ms, :st['n_map'][ms]], g['r_map'], g['k_map']))
        hits = gr.first_k_within(centre, st['pos'][s, c, :A], g['r_agent'], g['k_agent'])[0]
        capped_then_masked |= len(hits) == g['k_agent'] and (st['imask'][s, c, hits] == 0).any()
    assert min(gaps) > gr.MARGIN
    assert cr.min() > 0 and (st['av_index'] == 0).all()                # centre rows other than the ego
    assert capped_then_masked                                          # the imask filter comes after the cap: fewer than K emitted
    assert len(set(st['map_scene'].tolist())) < st['S']
    assert any(n == 0 for _, _, n in chunks_m) and any(n <= 1 for _, _, n in chunks_a)      # the scene without a hit
    if name == 'heading_24_128':
        assert any(n == 24 and last == 1 for _, last, n in chunks_a), chunks_a      # the 24th agent in the second 64-trip
        assert any(n == 128 and last == 3 for _, last, n in chunks_m), chunks_m     # the 128th token in the fourth
    else:
        assert any(n == 300 and last >= 4 for _, last, n in chunks_a) and any(0 < n < 300 for _, _, n in chunks_a)
        assert any(n == 2048 and last >= 32 for _, last, n in chunks_m)
    args = (st, c, cr, None, 0, g['r_agent'], g['k_agent'], g['r_map'], g['k_map'])
    ref, f32 = gr.point_edges_ref(*args), gr.point_edges_ref(*args, f=np.float32)
    for k in 'am':
        e = gr.raw_errors(ref[k], f32[k])
        print(f'point_edges {name} {k}: fp32 numpy errors dist {e[0]:.4g} bearing {e[1]:.4g} dth {e[2]:.4g}')
        assert e[0] <= gr.FP32_ERR_DIST and e[1] <= gr.FP32_ERR_BEARING and e[2] <= gr.FP32_ERR_DTH


def test_occupancy_generator_and_embedding_figure():
    from infgen_amd import synth
    G = synth.build_grid().shape[0]
    assert G == 1961
    st, c = gr.gen_occupancy(G)
    g = st['grid'][:, c]
    live = np.arange(st['A_cap'])[None] < st['n_agents'][:, None]
    assert (g[live] == -1).any() and (g[live] == 0).any() and (g[live] == G - 1).any() and (g[live] >= G).any()
    assert st['n_agents'].min() == 0 and st['n_agents'].max() == st['A_cap']
    occ = gr.occupancy_ref(st, c)
    assert occ.sum(1).min() == 0 and (occ.sum(1)[st['n_agents'] > 0] == 0).any()         # a scene with agents and no cell
    assert any(occ[s].sum() < len(set(g[s, :n].tolist())) for s, n in enumerate(st['n_agents']))
    sd, p = gr.gen_mlp_layer(G)
    w = [sd[f'{p}.{k}'] for k in ('mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias', 'mlp.3.weight', 'mlp.3.bias')]
    err = max(np.abs(gr.mlp_layer_ref(occ[s], *w) - gr.mlp_layer_ref(occ[s], *w, f=np.float32)).max() for s in range(st['S']))
    print(f'occupancy embedding: fp32 numpy error {err:.4g}')
    assert err <= gr.FP32_ERR_OCC_EMB


@pytest.mark.parametrize('rows,n,k', [(1, 17, 1), (3, 17, 16), (4, 64, 2), (5, 64, 16), (1000, 2048, 16), (1000, 2048, 2),
                                      (1000, 17, 1), (5, 2048, 1)])
def test_sample_topk_generator(rows, n, k):
    lg, u, kinds = gr.gen_sample_topk(rows, n, k)
    tok, margin = gr.sample_topk_ref(lg, k, u)
    assert ((tok >= 0) & (tok < n)).all() and np.isfinite(lg[np.arange(rows), tok]).all()
    for r, kind in enumerate(kinds):
        order = gr.topk_pick(lg[r], k, u[r])[2]
        assert np.isfinite(lg[r, order]).all() and np.isinf(lg[r]).sum() < n - k
        if kind == 'ties':
            assert (lg[r, order] == 5.0).all() and float(u[r]) * k == int(float(u[r]) * k)      # u * sum is a partial sum exactly
        else:
            assert margin[r] > gr.CDF_MARGIN, (r, kind, margin[r])
        if kind == 'tied_kth':
            assert (lg[r] == lg[r, order[-1]]).sum() > (lg[r, order] == lg[r, order[-1]]).sum()       # the tie crosses the k-th place
    if rows >= 6:
        assert set(kinds) == {'ties', 'zero', 'one', 'random', 'neg_inf', 'tied_kth'}
        assert u.min() == 0.0 and u.max() == np.float32(1.0) - np.float32(2.0 ** -24)
        if k > 1:
            assert len(set(tok[np.asarray(kinds) == 'one'].tolist())) >= 1
            one = np.nonzero(np.asarray(kinds) == 'one')[0]
            assert all(tok[r] == gr.topk_pick(lg[r], k, 0.5)[2][-1] for r in one)              # u just below 1 picks the last


@pytest.mark.parametrize('sample_k,topk_entry,t,force_enter', gr.INSERT_DECIDE_CASES)
def test_insert_decide_generator_reaches_every_branch(sample_k, topk_entry, t, force_enter):
    """exactly the calls of the GPU test (force_enter and t seed the generator: every call draws its own logits, uniforms and poses)"""
    from infgen_amd import synth
    grid = synth.build_grid()
    G = grid.shape[0]
    st, dec, names, max_new = gr.gen_insert_decide(G, grid, sample_k, t, force_enter)
    rst, rdec = gr.as_ref(st), gr.as_ref(dec)
    perr = 0.0
    for s, (name, _, _) in enumerate(gr.INSERT_DECIDE_BRANCHES):
        assert names[s] == name
        ins, act = gr.insert_decide_expect(name, sample_k, force_enter)
        A0 = int(st['n_agents'][s])
        gr.insert_decide_ref(rst, rdec, s, t, force_enter, max_new, sample_k=sample_k)
        assert (rdec['inserted'][s], rdec['active'][s]) == (ins, act), name
        if name not in ('u_zero', 'u_one', 'u_partial_sum', 'nan_logits') and sample_k > 1:
            assert gr.topk_pick(dec['lg_pos'][s], sample_k, dec['uniform'][s])[1] > gr.CDF_MARGIN, name
        if ins == 1:
            cell = rdec['new_cell'][s]
            order = gr.topk_pick(dec['lg_pos'][s], max(sample_k, 1), dec['uniform'][s])[2]
            assert rst['n_agents'][s] == A0 + 1 and rdec['new_row'][s] == s * st['A_cap'] + A0 and dec['occ'][s, cell] == 0
            if name == 'u_zero' or sample_k == 1:
                assert cell == order[0]
            if name == 'cell_tie' and sample_k == 1:
                assert cell == np.nonzero(dec['lg_pos'][s] == dec['lg_pos'][s].max())[0][0]
            if name == 'u_partial_sum' and sample_k > 1:
                assert cell == order[sample_k // 2]
            if name == 'u_one':
                assert cell == order[-1]
            if name == 'type_tie_01':
                assert rst['type'][s, A0] == 0
            if name == 'type_tie_12':
                assert rst['type'][s, A0] == 1
            av = st['av_index'][s]
            ego = (st['pos'][s, 1 + t, av, 0], st['pos'][s, 1 + t, av, 1], st['head'][s, 1 + t, av])
            p32 = gr.decode_pos(st['grid_xy'][cell], ego, f=np.float32)
            perr = max(perr, np.abs(np.asarray(p32, np.float64) - rst['pos'][s, 1 + t, A0]).max())
            assert np.abs(rst['pos'][s, 1 + t, A0]).max() < 300
        else:
            assert rst['n_agents'][s] == A0
    assert (st['av_index'] != 0).any()
    assert (rdec['inserted'][[names.index(n) for n in ('enter_below', 'enter_equal')]] == (1 if force_enter else 0)).all()
    print(f'insert_decide k={sample_k} t={t} force_enter={force_enter}: fp32 numpy position error {perr:.4g}')
    assert perr <= gr.FP32_ERR_INS_POS


def test_insert_finalize_generator():
    st, dec, c, interval, n_heading = gr.gen_insert_finalize()
    rst, rdec = gr.as_ref(st), gr.as_ref(dec)
    hv = np.full((st['S'], 2), 5.0)
    gr.insert_finalize_ref(rst, rdec, c, interval, hv)
    assert set(dec['inserted'].tolist()) == {1, 0, -1}
    herr = perr = 0.0
    wrapped = 0
    for s in range(st['S']):
        a = dec['new_row'][s] - s * st['A_cap']
        if dec['inserted'][s] <= 0:
            assert rst['head'][s, c, a] == st['head'][s, c, a] and (hv[s] == 5.0).all()
            continue
        lh = dec['lg_heading'][s]
        bi = int(np.nonzero(lh == lh.max())[0][0])
        eh = st['head'][s, c, st['av_index'][s]]
        raw = (bi * interval - 180.0) / 360.0 * 2 * math.pi + float(eh)
        wrapped += abs(raw) > math.pi
        assert gr.ang_err(rst['head'][s, c, a], raw) < 1e-12 and -math.pi <= rst['head'][s, c, a] < math.pi
        herr = max(herr, float(gr.ang_err(gr.decode_heading(bi, interval, eh, f=np.float32), rst['head'][s, c, a])))
        p32 = st['pos'][s, c, a] + np.tanh(dec['offset'][s]) * np.float32(2.0)
        perr = max(perr, np.abs(p32.astype(np.float64) - rst['pos'][s, c, a]).max())
    assert wrapped >= 2 and (dec['lg_heading'][4] == dec['lg_heading'][4].max()).sum() == 3
    assert np.abs(np.tanh(dec['offset'][6].astype(np.float64))).min() == 1.0                 # saturated
    print(f'insert_finalize: fp32 numpy errors heading {herr:.4g} position {perr:.4g}')
    assert herr <= gr.FP32_ERR_INS_HEAD and perr <= gr.FP32_ERR_INS_POS


# ------------------------------------------------------------------------------------------------ step advance: integrate, raw feature
def _butterfly_pick(d, tie_break=True, strict=True):
    """the kernel's search of one agent in fp32: 64 lanes over the cells g = lane, lane + 64, .. (strict <), then the xor butterfly
    32 .. 1 with the (distance, index) tie-break; lane 0's result.  tie_break / strict False: the two mutations the tie case catches"""
    best, bi = np.full(64, np.float32(np.inf)), np.full(64, 0x7fffffff, np.int64)
    for g, v in enumerate(d):
        ln = g % 64
        if v < best[ln] or (not strict and v == best[ln]):
            best[ln], bi[ln] = v, g
    for o in (32, 16, 8, 4, 2, 1):
        ob, oi = best[np.arange(64) ^ o], bi[np.arange(64) ^ o]
        take = (ob < best) | ((ob == best) & (oi < bi) if tie_break else False)
        best, bi = np.where(take, ob, best), np.where(take, oi, bi)
    return int(bi[0])


@pytest.mark.parametrize('name', list(gr.INTEGRATE_CASES))
def test_integrate_generator(name):
    """every case: the margin holds for every row (none is left uncompared), an fp32 evaluation in the kernel's order picks the
    same cell, its pose errors stay within the recorded figures, the cell agrees with the oracle's encode_pos on the same new
    poses, and the wrong variants of the reference differ from it where the case is meant to tell them apart"""
    from oracle.rollout_oracle import encode_pos
    st, ext, t = gr.gen_integrate(name)
    S, A_cap, nag, avs, G, step, fv, nos, teacher, _ = gr.INTEGRATE_CASES[name]
    n = 2 + t
    ref, f32 = gr.integrate_ref(st, ext, t), gr.integrate_ref(st, ext, t, f=np.float32)
    live = np.arange(A_cap)[None] < st['n_agents'][:, None]
    assert (t == 0) == (step == 'first') and (step == 'first' or (n == st['T'] - 1 and t * 5 + 5 == st['R']))
    assert (ref['search'][live] >= 0).all() and (ref['search'][~live] == -1).all()
    if name != 'ties' and G > 1:
        assert ref['gap'][live].min() > gr.GRID_MARGIN, ref['gap'][live].min()
    assert np.array_equal(ref['search'], f32['search'])                      # (the tie case too: its distances are exact)
    for k in ('state', 'token', 'grid', 'imask', 'catflag'):
        assert np.array_equal(ref[k], f32[k]), k
    e = gr.step_errors(ref, f32, st, t)
    print(f'integrate {name}: fp32 numpy errors position {e[0]:.4g} heading {e[1]:.4g}')
    assert e[0] <= gr.FP32_ERR_STEP_POS and e[1] <= gr.FP32_ERR_STEP_HEAD
    assert np.abs(ref['new_pose'][..., :2]).max() < 200 + 20
    grid = torch.from_numpy(st['grid_xy'][:G].astype(np.float64))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)            # (the oracle builds its rotation in the default type)
    try:
        for s in range(S):
            A, av = int(st['n_agents'][s]), int(st['av_index'][s])
            if A:
                p = torch.from_numpy(ref['new_pose'][s, :A])
                untied = ref['gap'][s, :A] > 0          # (the oracle's frame is turned by pi / 2 - float32(pi / 2): exact ties break)
                assert np.array_equal(encode_pos(grid, p[:, :2], p[av, :2], p[av, 2]).numpy()[untied], ref['search'][s, :A][untied]), s
    finally:
        torch.set_default_dtype(prev)
    # what the case is for
    assert gr.integrate_groups(S, A_cap) == (1 if S > 128 else A_cap // 16)
    valid_new = ref['state'][:, n][live] != gr.INVALID
    if not fv and teacher != 'all':
        assert (~valid_new).any()
    assert not (fv and (~valid_new).any())
    new_tok = ref['token'][:, n][live]
    assert set(st['type'][live].tolist()) == {0, 1, 2} or live.sum() < 20
    if live.sum() >= 20:
        assert (new_tok == 0).any() and (new_tok == gr.TOKEN_SIZE - 1).any()
    if teacher:
        forced = np.ones((S, A_cap), bool) if ext['replay_row'] is None else ext['replay_row'] != 0
        tg, tt = ext['teacher_grid'][:, n], ext['teacher_token'][:, n]
        vn = ref['state'][:, n] != gr.INVALID
        on = live & forced & vn
        assert (ref['token'][:, n][on & (tt < 0)] == -1).any()                              # the stored token stays negative
        if name != 'ties':
            assert (on & (tg == -1)).any() and (on & (tg == -2)).any() and (on & (tg >= 0)).any()
            assert (ref['grid'][:, n][on & (tg >= -1)] == tg[on & (tg >= -1)]).all()
            assert (ref['grid'][:, n][on & (tg == -2)] == ref['search'][on & (tg == -2)]).all()
            assert not np.array_equal(gr.integrate_ref(st, ext, t, mutate='grid_ge0')['grid'], ref['grid'])
        ego_flag = forced[np.arange(S), st['av_index']][st['n_agents'] > 0]
        if teacher == 'ego':
            assert ego_flag.all() and (live & ~forced).any()
            if S <= 128:                       # a flagged row in another workgroup than the flagged ego: the dup thread's flag
                grp = np.arange(A_cap)[None] // 16 != (st['av_index'] // 16)[:, None]
                assert (on & grp).any()
                mut = gr.integrate_ref(st, ext, t, mutate='dup_ignores_flag')
                assert (mut['grid'][:, n][on & grp & (tg == -2)] != ref['grid'][:, n][on & grp & (tg == -2)]).any()
        if teacher == 'noego':
            assert not ego_flag.any() and (live & forced).any()
    if G > 1 and name != 'ties' and live.sum() > 1:
        mut = gr.integrate_ref(st, ext, t, mutate='old_ego')
        assert (mut['search'][live] != ref['search'][live]).mean() > 0.2                     # the ego's NEW pose is the centre


def test_integrate_cases_cover_the_paths():
    """over all cases: the grid sizes around the 64-lane trip and the 2048-cell LDS limit, n_agents 0 / 1 / 16 / 17 / A_cap, the ego at
    row 0 / 15 / 16 / the last, in the first / the last / another workgroup, both steps, the flags singly and together, an ego that
    predicts INVALID, headings at +-pi"""
    Gs, nags, egos, where, flags, steps = set(), set(), set(), set(), set(), set()
    for name, (S, A_cap, nag, avs, G, step, fv, nos, teacher, _) in gr.INTEGRATE_CASES.items():
        st, ext, t = gr.gen_integrate(name)
        Gs.add(G)
        flags.add((fv, nos))
        steps.add(step)
        groups = gr.integrate_groups(S, A_cap)
        for s in range(S):
            A, av = int(st['n_agents'][s]), int(st['av_index'][s])
            nags.add('cap' if A == A_cap else A)
            if A:
                egos.update({av} & {0, 15, 16}, {'last'} if av == A - 1 else set())
                assert ext['next_state'][s * A_cap + av] == s % 3
                if groups > 1 and A > 16:
                    where.update({'first'} if av < 16 else set(), {'last'} if av // 16 == (A - 1) // 16 and av >= 16 else set(),
                                 {'middle'} if 16 <= av and av // 16 < (A - 1) // 16 else set())
        h = st['head'][:, 1 + t]
        assert (h == np.float32(math.pi)).any() and (h == -np.float32(math.pi)).any()
    assert Gs >= {1, 63, 64, 65, 1961, 2048, 2049}
    assert nags >= {0, 1, 16, 17, 'cap'} and egos >= {0, 15, 16, 'last'} and where >= {'first', 'last'}
    assert flags == {(0, 0), (1, 0), (0, 1), (1, 1)} and steps == {'first', 'last'}
    assert {(S, A) for S, A, *_ in gr.INTEGRATE_CASES.values()} >= {(3, 32), (1, 1024), (129, 32), (129, 96)}


def test_integrate_tie_case():
    """all values of the search are small integers: fp32 is exact, tied distances are equal bit for bit.  2- and 4-way ties occur;
    the hand-placed pairs sit 64 apart (one lane) and in different lanes with the lower index in the higher lane; the emulated
    kernel search equals the reference on every row, and differs without the `oi < bi` tie-break and with `<=` inside a lane"""
    st, ext, t = gr.gen_integrate('ties')
    n = 2 + t
    ref = gr.integrate_ref(st, ext, t)
    g = st['grid_xy'].astype(np.float64)
    assert np.array_equal(g, np.round(g)) and (g % 2 == 0).all()
    ways, same_lane, inverted, broke, loose = set(), 0, 0, 0, 0
    for s in range(st['S']):
        A, av = int(st['n_agents'][s]), int(st['av_index'][s])
        assert ext['teacher_head'][s, n, av] == np.float32(math.pi / 2)
        rel = (ext['teacher_pos'][s, n, :A] - ext['teacher_pos'][s, n, av]).astype(np.float64)
        assert np.array_equal(rel, np.round(rel)) and np.abs(rel).max() <= 9
        for a in range(A):
            d = np.sqrt(((rel[a][None] - g) ** 2).sum(1).astype(np.float32))
            tied = np.nonzero(d == d.min())[0]
            ways.add(len(tied))
            assert len(tied) == (1, 2, 2, 4)[int(rel[a, 0] % 2) + int(rel[a, 1] % 2) * 2 if (rel[a] % 2).sum() < 2 else 3]
            assert ref['search'][s, a] == tied[0] == ref['grid'][s, n, a] and (ref['gap'][s, a] == 0) == (len(tied) > 1)
            assert _butterfly_pick(d) == tied[0]
            broke += _butterfly_pick(d, tie_break=False) != tied[0]
            loose += _butterfly_pick(d, strict=False) != tied[0]
            if len(tied) == 2:
                same_lane += (tied[1] - tied[0]) % 64 == 0
                inverted += tied[0] % 64 > tied[1] % 64
    assert ways == {1, 2, 4} and same_lane >= 4 and inverted >= 4 and broke >= 4 and loose >= 4
    # the rotation of the search frame is by exactly zero in fp32
    assert -(np.float32(math.pi / 2) - np.float32(math.pi / 2)) == 0


def test_rawfeat_generator():
    """every gap rule at the columns the GPU test calls, tokens -1 / -2, grid -1, both catflags, all types; python indexing of the
    tables; the fp32 figures of the motion pair"""
    st, ext = gr.gen_rawfeat()
    G = st['grid_size']
    en = eb = 0.0
    for col in (0, 1, 2):
        ref, f32 = gr.rawfeat_prep_ref(st, ext, col), gr.rawfeat_prep_ref(st, ext, col, f=np.float32)
        sc = st['state'][:, col].reshape(-1)
        inv = sc == gr.INVALID
        if col:
            pinv = st['state'][:, col - 1].reshape(-1) == gr.INVALID
            assert (pinv & ~inv).any() and (~pinv & inv).any() and (pinv & inv).any() and (~pinv & ~inv).any()
            assert np.array_equal(ref['ruled'], np.where(pinv & inv, 2, np.where(pinv | inv, 1, 0)))
        else:
            assert (sc == gr.ENTER).any() and inv.any()
            assert np.array_equal(ref['ruled'], np.where(inv, 2, np.where(sc == gr.ENTER, 1, 0)))
            assert (ref['raw2'][ref['ruled'] == 0] == 0).all()                              # no motion into column 0
        assert np.array_equal(ref['raw2'][ref['ruled'] == 1, 0].astype(np.float32), np.full((ref['ruled'] == 1).sum(), np.float32(math.sqrt(2))))
        assert np.array_equal(ref['raw2'][ref['ruled'] == 2, 0].astype(np.float32), np.full((ref['ruled'] == 2).sum(), np.float32(2 * math.sqrt(2))))
        tok, grd, cf = (st[k][:, col].reshape(-1) for k in ('token', 'grid', 'catflag'))
        assert {-1, -2, 0, gr.TOKEN_SIZE - 1} <= set(tok.tolist()) and {-1, 0, G - 1} <= set(grd.tolist()) and set(cf.tolist()) == {0, 1}
        ty = st['type'].reshape(-1)
        assert set(ty.tolist()) == {0, 1, 2}
        r = int(np.nonzero(tok == -1)[0][0])
        assert np.array_equal(ref['tok'][r], ext['tok_tab'][ty[r], gr.TOKEN_SIZE + 1])        # no_token row; -2: the bos row
        r = int(np.nonzero(tok == -2)[0][0])
        assert np.array_equal(ref['tok'][r], ext['tok_tab'][ty[r], gr.TOKEN_SIZE])
        r = int(np.nonzero(grd == -1)[0][0])
        assert np.array_equal(ref['grid'][r], ext['grid_tab'][G])
        r = int(np.nonzero(cf == 0)[0][0])
        assert np.array_equal(ref['cat'][r], ext['cat_seed']) and np.array_equal(ref['state'][r], ext['state_emb'][sc[r]])
        en = max(en, np.abs(ref['raw2'][:, 0] - f32['raw2'][:, 0]).max())
        eb = max(eb, gr.ang_err(ref['raw2'][:, 1], f32['raw2'][:, 1]).max())
    # a row subset: compact slots, a masked-off slot reads row 0
    sub = gr.rawfeat_prep_ref(st, ext, 1, rows=[40, 7, 95], mask=[1, 0, 1])
    full = gr.rawfeat_prep_ref(st, ext, 1)
    for k in ('raw2', 'cat', 'tok', 'state', 'grid'):
        assert np.array_equal(sub[k], full[k][[40, 0, 95]]), k
    print(f'raw feature: fp32 numpy errors motion norm {en:.4g} bearing {eb:.4g}')
    assert en <= gr.FP32_ERR_MOTION_NORM and eb <= gr.FP32_ERR_MOTION_BEARING


def test_step_figures_are_the_recorded_ones():
    """GRID_MARGIN is ten times the position bar, the bars four times the figures"""
    assert gr.GRID_MARGIN == 10 * gr.BAR_STEP_POS == 40 * gr.FP32_ERR_STEP_POS
    assert (gr.BAR_STEP_HEAD, gr.BAR_MOTION_NORM, gr.BAR_MOTION_BEARING) == (4 * gr.FP32_ERR_STEP_HEAD, 4 * gr.FP32_ERR_MOTION_NORM,
                                                                           4 * gr.FP32_ERR_MOTION_BEARING)


# ------------------------------------------------------------------------------------------------ teacher-forced forward: edge builder, motion features
def _found(g, q, k=None):
    """candidate indices the radius call of query q finds (before the filters), all of them with k = a large number"""
    c0, c1 = int(g['q_c0'][q]), int(g['q_c1'][q])
    return c0 + gr.first_k_within(g['p_pos'][g['q_pt'][q]], g['c_pos'][c0:c1], g['radius'], g['K'] if k is None else k)[0]


def _passes(g, q, m):
    """the emit filters of query q on candidate indices m"""
    keep = np.ones(len(m), bool)
    if g['q_self'] is not None:
        keep &= m != g['q_self'][q]
    if g['c_ok'] is not None:
        keep &= g['c_ok'][m] != 0
    if g['pair_ok'] is not None and g['q_pair_off'][q] >= 0:
        keep &= g['pair_ok'].reshape(-1)[g['q_pair_off'][q] + m - g['q_c0'][q]] != 0
    return keep


def _validity_combinations(g, ref):
    """the (source invalid, query invalid) pairs over all emitted edges; indices recovered from a run without c_src"""
    plain = gr.radius_edges_ref(dict(g, c_src=None))[0]
    combos = set()
    for q, node in enumerate(g['q_node']):
        m = plain[node][0]
        assert len(m) == len(ref[node][0])
        d_inv = bool(g['p_inv'][g['q_pt'][q]]) if g['p_inv'] is not None else False
        s_inv = g['c_inv'][m] != 0 if g['c_inv'] is not None else np.zeros(len(m), bool)
        combos |= {(bool(s), d_inv) for s in s_inv}
    return combos


@pytest.mark.parametrize('name', list(gr.RADIUS_EDGES_CASES))
def test_radius_edges_generator(name):
    """the margin holds for every (query, candidate) pair, the case reaches what RADIUS_EDGES_CASES says it is for, coordinates stay
    within +-200 m, and the fp32 figures of the raw features stay within the recorded ones (the device bars do not move)"""
    g = gr.gen_radius_edges(name)
    ref, gap = gr.radius_edges_ref(g)
    assert gap > gr.MARGIN, gap
    assert max(np.abs(g['p_pos']).max(), np.abs(g['c_pos']).max()) <= 200.0
    nq, K = len(g['q_node']), g['K']
    assert len(set(g['q_node'].tolist())) == nq and len(ref) == g['n_nodes']
    width = g['q_c1'] - g['q_c0']
    n_in = np.asarray([len(_found(g, q, 10 ** 9)) for q in range(nq)])
    found = [_found(g, q) for q in range(nq)]
    dropped = [(~_passes(g, q, found[q])).sum() for q in range(nq)]
    combos = _validity_combinations(g, ref)
    if name == 'temporal':
        with np.errstate(over='ignore'):
            assert np.isinf(np.float32(g['radius']) * np.float32(g['radius'])) and np.isfinite(np.float32(g['radius']))
        assert (g['p_pos'].shape[0], K, g['gap_rule'], g['index_diff']) == (5 * 20, 12, 1, 1)
        assert (width == 0).any() and width.max() == 12 and (n_in == width).all()           # empty ranges at column 0; all in radius
        assert max(dropped) > 0 and (g['c_ok'] == 0).any()                                  # holes of the history mask inside a window
        assert not np.array_equal(g['c_src'], np.arange(len(g['c_src']))) and (g['q_node'] != g['q_pt']).any()
        assert combos == {(False, False), (False, True), (True, False), (True, True)}
        assert nq < g['n_nodes']                                                            # nodes without a query
        diffs = np.concatenate([r[1][:, 3] for r in ref])
        assert diffs.min() == -12 and diffs.max() == -1
    elif name == 'agent':
        assert sorted(set(width.tolist())) == [1, 70, 330] and (g['q_self'] == g['q_pt']).all() and (K, g['gap_rule']) == (301, 1)
        assert nq % 4 != 0 and nq < g['n_nodes']
        cut = [q for q in range(nq) if n_in[q] > K]
        assert len(cut) >= 100                                                              # the cap truncates ...
        assert all((found[q][-1] - g['q_c0'][q]) // 64 >= 4 for q in cut)                   # ... after several 64-candidate chunks
        assert any((g['c_ok'][found[q]] == 0).any() and g['q_self'][q] in found[q] for q in cut)     # found, counted, not emitted
        assert any(g['q_self'][q] not in found[q] for q in cut)                             # and a query beyond its own first K
        assert combos == {(False, False), (False, True), (True, False), (True, True)}
        assert any(len(ref[node][0]) == 0 for node in g['q_node'])                          # the scene of one agent: self only
    elif name == 'seed_pair':
        assert (K, g['gap_rule']) == (300, 0) and g['e_base'] > 0
        assert (g['q_pair_off'] == -1).any() and (g['q_pair_off'] >= 0).any() and (g['q_c0'] > 0).any()
        assert width.max() > 64 and max(len(f) for f in found) > 0
        for q in range(nq):                       # the pair filter alone drops candidates that pass c_ok, where it applies
            m = found[q][g['c_ok'][found[q]] != 0]
            assert (~_passes(g, q, m)).any() == (g['q_pair_off'][q] >= 0)
        assert any(np.abs(r[1][:, 0]).min(initial=1.0) == 0.0 for r in ref)                  # the ego under its seed row: d = 0
    elif name == 'map':
        assert (K, g['gap_rule']) == (5, 2) and g['c_inv'] is None and g['c_ok'] is None and g['q_self'] is None
        assert sorted(set(width.tolist())) == [0, 200]
        assert (n_in > K).any() and ((n_in < K) & (n_in > 0)).any()
        assert combos == {(False, False), (False, True)}
        assert nq < g['n_nodes']
    else:
        assert g['p_inv'] is None and g['c_inv'] is None and K == 101 and sorted(set(width.tolist())) == [1, 150]
        assert (n_in > K).sum() >= 50 and (n_in < K).any()
        assert any(g['q_self'][q] in found[q] for q in range(nq) if n_in[q] > K)
        assert any(g['q_self'][q] not in found[q] for q in range(nq) if n_in[q] > K)
    f32 = gr.radius_edges_ref(g, f=np.float32)[0]
    e = gr.raw_errors(ref, f32)
    print(f'radius_edges {name}: {sum(len(r[0]) for r in ref)} edges, fp32 numpy errors dist {e[0]:.4g} bearing {e[1]:.4g} dth {e[2]:.4g}')
    assert e[0] <= gr.FP32_ERR_DIST and e[1] <= gr.FP32_ERR_BEARING and e[2] <= gr.FP32_ERR_DTH


@pytest.mark.parametrize('name', list(gr.RADIUS_EDGES_CASES))
def test_radius_edges_ref_agrees_with_the_oracle_helpers(name):
    """the found sets against oracle.rollout_oracle.radius_first_k (filters applied here, after the call), the gap rules against
    oracle.forward_oracle._gap_rules (rule 2, two assignments in the reference, by hand)"""
    from oracle.forward_oracle import _gap_rules
    from oracle.rollout_oracle import radius_first_k, wrap_angle
    g = gr.gen_radius_edges(name)
    plain = gr.radius_edges_ref(dict(g, c_src=None))[0]
    ref = gr.radius_edges_ref(g)[0]
    t64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    for q, node in enumerate(g['q_node']):
        qp, c0, c1 = int(g['q_pt'][q]), int(g['q_c0'][q]), int(g['q_c1'][q])
        _, xi = radius_first_k(t64(g['c_pos'][c0:c1]), t64(g['p_pos'][qp][None]), g['radius'], g['K'])
        m = c0 + xi.numpy()
        m = m[_passes(g, q, m)]
        assert np.array_equal(m, plain[node][0]), (name, q)
        assert np.array_equal(g['c_src'][m] if g['c_src'] is not None else m, ref[node][0])
        if len(m) == 0:
            continue
        dp = t64(g['c_pos'][m]) - t64(g['p_pos'][qp])[None]
        dth = wrap_angle(t64(g['c_head'][m]) - float(g['p_head'][qp]))
        s_inv = torch.from_numpy(g['c_inv'][m] != 0) if g['c_inv'] is not None else torch.zeros(len(m), dtype=torch.bool)
        d_inv = torch.full((len(m),), bool(g['p_inv'][qp]) if g['p_inv'] is not None else False)
        if g['gap_rule'] == 1:
            _gap_rules(dp, dth, s_inv, d_inv)
        elif g['gap_rule'] == 2:
            dp[d_inv], dth[d_inv] = gr.MOTION_GAP, gr.HEADING_GAP
        assert np.abs(dp.norm(dim=-1).numpy() - ref[node][1][:, 0]).max() < 1e-12
        assert gr.ang_err(dth.numpy(), ref[node][1][:, 2]).max() < 1e-12


def _differs(name, lists, ref):
    """does the device comparison (compare_lists with its bars) tell `lists`, packed as fp32 device arrays, from the reference?"""
    off, cnt, src, raw, _ = gr.pack_lists(lists)
    try:
        gr.compare_lists(name, off, cnt, src, raw, ref)
    except AssertionError:
        return True
    return False


def test_radius_edges_mutants_are_told_apart():
    """every deliberate deviation of radius_edges_ref fails, on at least one case, the very comparison the GPU test applies to the
    kernel's output - and an fp32 evaluation of the unmutated reference passes it on every case"""
    cases = [(n, gr.gen_radius_edges(n)) for n in gr.RADIUS_EDGES_CASES] + [(f'strict{k}', c[0]) for k, c in enumerate(gr.gen_strict_radius_edges())]
    caught = {m: [] for m in gr.RADIUS_EDGES_MUTANTS}
    for name, g in cases:
        ref = gr.radius_edges_ref(g)[0]
        assert not _differs(name, gr.radius_edges_ref(g, f=np.float32)[0], ref), name
        for m in gr.RADIUS_EDGES_MUTANTS:
            if _differs(name, gr.radius_edges_ref(g, mutate=m)[0], ref):
                caught[m].append(name)
    print('radius_edges mutants caught by:', caught)
    assert all(caught.values()), caught
    # and by the case meant for each
    assert 'agent' in caught['filtered_not_counted'] and 'seed_pair' in caught['pair_abs_index'] and 'temporal' in caught['index_diff_sign']
    assert {'temporal', 'agent'} <= set(caught['rule1_dst_dth']) and 'map' in caught['rule2_keep_dth']
    assert {'temporal', 'agent', 'map'} <= set(caught['bearing_pre_override'])
    assert any(n.startswith('strict') for n in caught['le_radius'])


def test_strict_radius_edges_cases():
    for g, i, present in gr.gen_strict_radius_edges():
        ref, gap = gr.radius_edges_ref(g)
        assert (i in ref[0][0]) == present and 0 not in ref[0][0]
        assert present or gap == 0.0                  # (the point at exactly r: the margin does not hold here by design)


def test_motion_features_generator():
    """shapes, the far last column, every rule and every pair of rules that can coincide at t = 0 and at t > 0, EXIT at both; the
    motion vectors agree with oracle.forward_oracle.build_vector; the fp32 figures are the recorded ones"""
    from oracle.forward_oracle import build_vector
    from oracle.rollout_oracle import angle_between
    cases = gr.gen_motion_features()
    assert [c['state'].shape for c in cases] == gr.MOTION_FEATURES_SHAPES == [(7, 1), (3, 2), (37, 19)] and (37 * 19) % 256
    seen0, seen1 = set(), set()
    en = ea = 0.0
    for c in cases:
        st, gm = c['state'], c['gap_mask'] != 0
        rows, T = st.shape
        assert np.abs(c['pos']).max() <= 200 and np.abs(c['pos'][:, -1]).min() >= 120
        assert (np.abs(c['pos'][:, :-1]).max() < 200) if T > 1 else True
        inv = st == gr.INVALID
        pinv = np.concatenate([np.zeros((rows, 1), bool), inv[:, :-1]], 1)
        for t in range(T):
            for a in range(rows):
                if t == 0:
                    fired = (('invalid',) if inv[a, 0] else ()) + (('enter',) if st[a, 0] == gr.ENTER else ()) + (('mask',) if gm[a, 0] else ())
                    seen0.add(fired)
                    seen0.add(('exit',) if st[a, 0] == gr.EXIT else fired)
                else:
                    fired = (('invalid',) if inv[a, t] else ()) + (('enter',) if pinv[a, t] and not inv[a, t] else ()) + \
                            (('leave',) if not pinv[a, t] and inv[a, t] else ()) + (('mask',) if gm[a, t] else ())
                    seen1.add(fired)
                    seen1.add(('exit',) if st[a, t] == gr.EXIT else fired)
        for mask in (None, c['gap_mask']):
            ref, ruled = gr.motion_features_ref(c['pos'], c['head'], st, mask, with_ruled=True)
            f32 = gr.motion_features_ref(c['pos'], c['head'], st, mask, f=np.float32)
            en = max(en, np.abs(ref[..., 0] - f32[..., 0]).max())
            ea = max(ea, gr.ang_err(ref[..., 1], f32[..., 1]).max())
            gr.compare_motion(f32.astype(np.float32), ref, ruled)
            assert (ref[..., 2:] == 0).all()
            mv, hv = build_vector(torch.from_numpy(c['pos']).double(), torch.from_numpy(c['head']).double(), torch.from_numpy(st))
            if mask is not None:
                mv[torch.from_numpy(gm)] = gr.MOTION_GAP                                    # agent_decoder.py:1327
            assert np.abs(mv.norm(dim=-1).numpy() - ref[..., 0]).max() < 1e-12
            assert gr.ang_err(angle_between(hv, mv).numpy(), ref[..., 1]).max() < 1e-12
            want = np.where((mv == -2).all(-1).numpy(), 2, np.where((mv.abs() == 1).all(-1).numpy(), 1, 0))
            assert np.array_equal(ruled, want)
    assert seen0 >= {(), ('invalid',), ('enter',), ('mask',), ('invalid', 'mask'), ('enter', 'mask'), ('exit',)}, seen0
    assert seen1 >= {(), ('invalid',), ('enter',), ('invalid', 'leave'), ('mask',), ('invalid', 'mask'), ('enter', 'mask'),
                     ('invalid', 'leave', 'mask'), ('exit',)}, seen1
    print(f'motion features: fp32 numpy errors norm {en:.4g} angle {ea:.4g}')
    assert en <= gr.FP32_ERR_MOTION_FEAT_NORM and ea <= gr.FP32_ERR_MOTION_FEAT_ANGLE
    assert (gr.BAR_MOTION_FEAT_NORM, gr.BAR_MOTION_FEAT_ANGLE) == (4 * gr.FP32_ERR_MOTION_FEAT_NORM, 4 * gr.FP32_ERR_MOTION_FEAT_ANGLE)


def test_motion_features_mutants_are_told_apart():
    """every deliberate deviation of motion_features_ref fails, on at least one (shape, mask) input, the comparison the GPU test
    applies (compare_motion)"""
    caught = {m: [] for m in gr.MOTION_FEATURES_MUTANTS}
    for c in gr.gen_motion_features():
        for mask in (None, c['gap_mask']):
            ref, ruled = gr.motion_features_ref(c['pos'], c['head'], c['state'], mask, with_ruled=True)
            for m in gr.MOTION_FEATURES_MUTANTS:
                mut = gr.motion_features_ref(c['pos'], c['head'], c['state'], mask, mutate=m).astype(np.float32)
                try:
                    gr.compare_motion(mut, ref, ruled)
                except AssertionError:
                    caught[m].append((c['state'].shape, mask is not None))
    print('motion_features mutants caught by:', caught)
    assert all(caught.values()), caught
    assert ((7, 1), False) in caught['t0_reads_previous_row']          # a single column: every element but the first reads across
