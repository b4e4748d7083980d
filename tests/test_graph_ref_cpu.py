"""Anchors of tests/graph_ref.py (the plain float64 reference of the edge builders and insertion kernels) and of the input
generators the GPU tests use: the reference agrees with the oracle's helpers, with the reference project's own edge lists
(tests/golden/*_internals.npz) and with torch's softmax -> topk -> cumsum; every generator clears its ambiguity margin and reaches
the branch it is meant for; the fp32 figures the device bars are derived from still hold."""
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
