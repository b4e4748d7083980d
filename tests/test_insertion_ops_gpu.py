"""Operator-level tests of the insertion kernels and the top-k sampler: infgen_occupancy / _embed, infgen_insert_decide / _topk,
infgen_insert_finalize and infgen_sample_topk through their C entries on hand-built blocks, against tests/graph_ref.py.  Every
decision, index and mask is compared exactly; written poses within graph_ref.BAR_INS_*; rows the kernels must not touch bitwise.

Variants only the sequenced entries select - k_insert_decide<false> (no grid token) and the three ablated k_insert_finalize
instantiations - have no operator-level entry (insert_decide_impl's `grid` and insert_finalize_impl's flags are set by
infgen_insert_seed / infgen_insert_heading alone); they stay covered by the ablation rollouts of tests/test_ablation_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_ref as gr
from gpu_blocks import SENT_F, SENT_I, dev, device_block, guard_intact, guarded, lib_and_check

pytestmark = pytest.mark.gpu

STATE_KEYS = ('pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag', 'type', 'bos', 'n_agents',
              'pred_traj', 'pred_head', 'pred_state')


def grid_xy():
    from infgen_amd import synth
    return synth.build_grid()


# ------------------------------------------------------------------------------------------------ occupancy
def test_occupancy_and_its_embedding():
    """G = 1961, 64 scenes of 0 .. 64 agents, grid tokens -1, duplicated, 0, G - 1 and (ignored by both kernels) >= G: occ exact
    and identical between infgen_occupancy and infgen_occupancy_embed; emb against the float64 MLPLayer of the unpacked weights, every
    scene embedded (the public entry passes no active mask), a scene without an occupied cell giving the bias' embedding"""
    from infgen_amd import packing
    lib, check = lib_and_check()
    G = grid_xy().shape[0]
    st, c = gr.gen_occupancy(G)
    S = st['S']
    want = gr.occupancy_ref(st, c)
    b, keep = device_block(st)
    occ1, occ2, emb = guarded(S * G, torch.float32), guarded(S * G, torch.float32), guarded(S * 128, torch.float32)
    sd, p = gr.gen_mlp_layer(G)
    pack = torch.from_numpy(packing.pack_mlp_layer(sd, p)).to(dev())
    check(lib.infgen_occupancy(C.byref(b), c, occ1.data_ptr(), None), 'infgen_occupancy')
    check(lib.infgen_occupancy_embed(C.byref(b), c, occ2.data_ptr(), pack.data_ptr(), emb.data_ptr(), None), 'infgen_occupancy_embed')
    torch.cuda.synchronize()
    assert guard_intact(occ1, S * G) and guard_intact(occ2, S * G) and guard_intact(emb, S * 128)
    o1, o2 = occ1[:S * G].cpu().numpy().reshape(S, G), occ2[:S * G].cpu().numpy().reshape(S, G)
    assert np.array_equal(o1, want) and np.array_equal(o2, want)
    w = [sd[f'{p}.{k}'] for k in ('mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias', 'mlp.3.weight', 'mlp.3.bias')]
    ref = np.stack([gr.mlp_layer_ref(want[s], *w) for s in range(S)])
    got = emb[:S * 128].cpu().numpy().reshape(S, 128).astype(np.float64)
    err = np.abs(got - ref).max()
    print(f'occupancy embedding: device error {err:.3g} (bar {gr.BAR_OCC_EMB:.3g})')
    assert err <= gr.BAR_OCC_EMB
    bias_only = gr.mlp_layer_ref(np.zeros(G), *w)
    for s in np.nonzero(want.sum(1) == 0)[0]:
        assert np.abs(got[s] - bias_only).max() <= gr.BAR_OCC_EMB


# ------------------------------------------------------------------------------------------------ insert_decide
def run_decide(st, dec, t, force_enter, max_new, sample_k, topk_entry):
    lib, check = lib_and_check()
    b, ten = device_block(st)
    d = {k: torch.from_numpy(v.copy()).to(dev()) for k, v in dec.items()}
    P = lambda k: d[k].data_ptr()
    args = (C.byref(b), t, force_enter, max_new, P('lg_state'), P('lg_type'), P('shape'), P('lg_pos'), P('occ'), P('active'), P('n_new'),
            P('inserted'), P('new_row'), P('new_shape'), P('new_cell'))
    if topk_entry:
        check(lib.infgen_insert_decide_topk(*args, sample_k, P('uniform'), None), 'infgen_insert_decide_topk')
    else:
        check(lib.infgen_insert_decide(*args, None), 'infgen_insert_decide')
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in ten.items()}, {k: v.cpu().numpy() for k, v in d.items()}


@pytest.mark.parametrize('sample_k,topk_entry,t,force_enter', gr.INSERT_DECIDE_CASES)
def test_insert_decide_branch_table(sample_k, topk_entry, t, force_enter):
    """one scene per named branch (graph_ref.INSERT_DECIDE_BRANCHES): inactive; enter logit below / equal / above; force_enter; type
    ties; the chosen cell occupied (greedy: the scene stops; sampled: inserted = 0 and the scene stays active); n_new == max_new;
    A == A_cap (-1, nothing touched); cell ties; u = 0, u * sum on a partial sum exactly, u = 1 - 2^-24; every cell logit NaN (no cell:
    the scene stops, occ is not indexed); an ego that is not row 0.  t = 0 writes no pred_*, t > 0 the five slots (t-1)*5.. of the
    new row.  Everything but the decoded position is compared exactly, so rows of other scenes and other rows of the same scene are
    bitwise unchanged and all T columns of the new row are reset."""
    gxy = grid_xy()
    G = gxy.shape[0]
    st, dec, names, max_new = gr.gen_insert_decide(G, gxy, sample_k, t, force_enter)
    rst, rdec = gr.as_ref(st), gr.as_ref(dec)
    for s in range(st['S']):
        gr.insert_decide_ref(rst, rdec, s, t, force_enter, max_new, sample_k=sample_k)
    got, gdec = run_decide(st, dec, t, force_enter, max_new, sample_k, topk_entry)
    c, A_cap = 1 + t, st['A_cap']
    for k in ('inserted', 'active', 'n_new'):
        assert np.array_equal(gdec[k], rdec[k]), (k, dict(zip(names, zip(gdec[k], rdec[k]))))
    for s, name in enumerate(names):                           # the table's literal expectations, not through the reference
        assert (gdec['inserted'][s], gdec['active'][s]) == gr.insert_decide_expect(name, sample_k, force_enter), name
    ins = rdec['inserted'] == 1
    assert ins.sum() >= 8 and (rdec['inserted'] == -1).sum() == 1 and (rdec['inserted'] == 0).sum() >= 3
    for k in ('new_row', 'new_cell', 'new_shape'):
        assert np.array_equal(gdec[k], rdec[k]), k                 # (scenes that did not insert keep their old values)
    for k in ('lg_state', 'lg_type', 'shape', 'occ', 'uniform'):
        assert np.array_equal(gdec[k], dec[k]), k
    for k in STATE_KEYS:
        if k in ('pos', 'pred_traj'):
            continue
        assert np.array_equal(got[k].astype(np.float64), np.asarray(rst[k], np.float64)), k
    # positions: the decoded one within the bar of float64, every other entry exactly the reference's (zeros of the reset, or untouched)
    tol = np.zeros(st['pos'].shape[:3], bool)
    ptol = np.zeros(st['pred_traj'].shape[:2], bool)
    for s in np.nonzero(ins)[0]:
        a = rdec['new_row'][s] - s * A_cap
        tol[s, c, a] = True
        if t > 0:
            ptol[rdec['new_row'][s], (t - 1) * 5:(t - 1) * 5 + 5] = True
    assert t == 0 or ptol.sum() == 5 * ins.sum()
    for k, m in (('pos', tol), ('pred_traj', ptol)):
        g64 = got[k].astype(np.float64)
        assert np.array_equal(g64[~m], rst[k][~m]), k
        if m.any():
            err = np.abs(g64[m] - rst[k][m]).max()
            print(f'insert_decide k={sample_k} t={t} {k}: device error {err:.3g} m (bar {gr.BAR_INS_POS:.3g})')
            assert err <= gr.BAR_INS_POS
    if t == 0:
        for k in ('pred_traj', 'pred_head', 'pred_state'):
            assert np.array_equal(got[k], st[k]), k
    # spot checks of the table against literal expectations (not through the reference)
    by = dict(zip(names, range(len(names))))
    s = by['rows_full']
    assert gdec['inserted'][s] == -1 and gdec['active'][s] == 0 and got['n_agents'][s] == A_cap
    s = by['occupied']
    assert gdec['inserted'][s] == 0 and gdec['active'][s] == (1 if sample_k > 1 else 0) and gdec['n_new'][s] == dec['n_new'][s]
    s = by['nan_logits']
    assert gdec['inserted'][s] == 0 and gdec['active'][s] == 0 and got['n_agents'][s] == st['n_agents'][s]
    s = by['enter_equal']
    assert gdec['inserted'][s] == (1 if force_enter else 0)
    s = by['enter_above']
    a = st['n_agents'][s]
    assert np.array_equal(got['imask'][s, :, a], np.arange(st['T']) >= c) and np.array_equal(got['catflag'][s, :, a], np.arange(st['T']) >= c)
    assert (got['tmask'][s, :, a] == 1).all() and got['state'][s, c, a] == gr.ENTER and got['token'][s, c, a] == -2
    assert (np.delete(got['state'][s, :, a], c) == gr.INVALID).all() and (np.delete(got['token'][s, :, a], c) == -1).all()
    assert got['grid'][s, c, a] == gdec['new_cell'][s] and got['bos'][s, a] == c and got['head'][s, c, a] == st['head'][s, c, 0]
    if sample_k == 1:
        s = by['cell_tie']
        assert gdec['new_cell'][s] == np.nonzero(dec['lg_pos'][s] == 9.0)[0][0]
    s = by['type_tie_01']
    assert got['type'][s, st['n_agents'][s]] == 0
    s = by['type_tie_12']
    assert got['type'][s, st['n_agents'][s]] == 1


# ------------------------------------------------------------------------------------------------ insert_finalize
def test_insert_finalize():
    """heading arg-max with ties (first index), decoded headings that cross +-pi with the ego's (wrap_angle), saturating offsets,
    hv_ovr = (cos, sin) of the new heading; inserted = 0 and inserted = -1 (no row was appended: new_row is an older iteration's)
    leave every array of the scene alone, as k_insert_cat and the engine treat -1"""
    lib, check = lib_and_check()
    st, dec, c, interval, n_heading = gr.gen_insert_finalize()
    S = st['S']
    rst, rdec = gr.as_ref(st), gr.as_ref(dec)
    hv_ref = np.full((S, 2), np.float64(np.float32(SENT_F)))
    gr.insert_finalize_ref(rst, rdec, c, interval, hv_ref)
    b, ten = device_block(st)
    d = {k: torch.from_numpy(dec[k].copy()).to(dev()) for k in ('inserted', 'new_row', 'lg_heading', 'offset')}
    hv = guarded(S, torch.float32, 2)
    check(lib.infgen_insert_finalize(C.byref(b), c, interval, d['inserted'].data_ptr(), d['new_row'].data_ptr(), d['lg_heading'].data_ptr(),
                                     n_heading, d['offset'].data_ptr(), hv.data_ptr(), None), 'infgen_insert_finalize')
    torch.cuda.synchronize()
    assert guard_intact(hv, S, 2)
    got = {k: v.cpu().numpy() for k, v in ten.items()}
    hv = hv[:2 * S].cpu().numpy().reshape(S, 2).astype(np.float64)
    m = np.zeros(st['head'].shape, bool)
    for s in np.nonzero(dec['inserted'] > 0)[0]:
        m[s, c, dec['new_row'][s] - s * st['A_cap']] = True
    assert m.sum() == (dec['inserted'] > 0).sum() == 8
    for k in STATE_KEYS:
        if k not in ('pos', 'head'):
            assert np.array_equal(got[k], st[k]), k
    assert np.array_equal(got['pos'][~m], st['pos'][~m]) and np.array_equal(got['head'][~m], st['head'][~m])     # 0 / -1: bitwise
    herr = gr.ang_err(got['head'][m], rst['head'][m]).max()
    perr = np.abs(got['pos'][m].astype(np.float64) - rst['pos'][m]).max()
    on = dec['inserted'] > 0
    verr = np.abs(hv[on] - hv_ref[on]).max()
    print(f'insert_finalize: device errors heading {herr:.3g} rad (bar {gr.BAR_INS_HEAD:.3g}) position {perr:.3g} m (bar {gr.BAR_INS_POS:.3g}) '
          f'hv_ovr {verr:.3g}')
    assert herr <= gr.BAR_INS_HEAD and perr <= gr.BAR_INS_POS and verr <= gr.BAR_INS_HEAD
    assert np.array_equal(hv[~on], hv_ref[~on])                                      # untouched
    assert ((got['head'][m] >= -np.float32(np.pi)) & (got['head'][m] <= np.float32(np.pi))).all()


# ------------------------------------------------------------------------------------------------ sample_topk
@pytest.mark.parametrize('rows,n,k', [(1, 17, 1), (3, 17, 16), (4, 64, 2), (5, 64, 16), (1000, 2048, 16), (1000, 2048, 2),
                                      (1000, 17, 1), (5, 2048, 1)])
def test_sample_topk_tokens_are_exact(rows, n, k):
    """rows in {1, 3, 4, 5, 1000}, n in {17, 64, 2048}, k in {1, 2, 16}: ties inside and across the k-th place, -inf entries,
    u = 0, u * sum on a partial sum exactly, u = 1 - 2^-24"""
    lib, check = lib_and_check()
    lg, u, kinds = gr.gen_sample_topk(rows, n, k)
    want, _ = gr.sample_topk_ref(lg, k, u)
    tok = guarded(rows, torch.int32)
    dl, du = torch.from_numpy(lg).to(dev()), torch.from_numpy(u).to(dev())
    check(lib.infgen_sample_topk(dl.data_ptr(), rows, n, k, du.data_ptr(), tok.data_ptr(), None), 'infgen_sample_topk')
    torch.cuda.synchronize()
    assert guard_intact(tok, rows)
    got = tok[:rows].cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, [(int(r), kinds[r], int(got[r]), int(want[r])) for r in bad[:8]]


def test_sample_topk_refuses_k_beyond_n_and_16():
    """the refusal and its text, not a launch: the k-th pick of fewer than k logits would be no token"""
    from infgen_amd import _lib
    lib = _lib.load()
    lg, u = torch.zeros(4, 8, device=dev()), torch.zeros(4, device=dev())
    tok = guarded(4, torch.int32)
    for k, text in ((9, 'k must not exceed n'), (17, 'k must be in 1..16'), (0, 'k must be in 1..16')):
        assert lib.infgen_sample_topk(lg.data_ptr(), 4, 8, k, u.data_ptr(), tok.data_ptr(), None) != 0
        assert text in lib.infgen_last_error().decode()
    torch.cuda.synchronize()
    assert (tok.cpu().numpy() == SENT_I).all()
    assert lib.infgen_sample_topk(lg.data_ptr(), 4, 8, 8, u.data_ptr(), tok.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (tok[:4].cpu().numpy() == 0).all() and guard_intact(tok, 4)
