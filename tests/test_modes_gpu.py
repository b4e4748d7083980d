"""GPU: the mode selection (infgen_amd/modes.py over k_select_modes; "modes" of include/infgen_hip.h) against the fixtures the
reference's batch_nms / new_batch_nms produced and against tests/modes_ref.py on random inputs - indices and scores exactly,
trajectories bit-equal to the gathered input -, RolloutEngine.select_modes / InfGenDecoder.predict_modes on small synthetic
scenes, and minMultiADE / minMultiFDE (k_multi_traj_error): counters exactly, float sums within 4 x the reference's own float32
error against its float64 value (one float32 ulp of the value where that error is zero)."""
import os

import numpy as np
import pytest
import torch

import modes_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DEV = torch.device('cuda:0')
SENT = 0x5A


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(got, want, what=''):
    (gt, gs, gi), (wt, ws, wi) = got, want
    assert gi.dtype == torch.int32 and gs.dtype == torch.float32
    assert np.array_equal(gi.cpu().numpy(), wi), what
    assert np.array_equal(gs.cpu().numpy(), ws), what
    if gt is not None:
        assert np.array_equal(gt.cpu().numpy(), wt), what


def _random_case(B, N, T, F, seed, spread=3.0):
    rng = np.random.default_rng(seed)
    traj = rng.normal(0, spread, (B, N, T, F)).astype(np.float32)
    scores = rng.uniform(0.01, 1.0, (B, N)).astype(np.float32)
    return traj, scores


# ------------------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize('name', ['b5_n33', 'b3_n64', 'b4_n6', 'b2_n2', 'b1_n1', 'b257_n16'])
def test_batch_nms_equals_the_reference(name):
    from infgen_amd import modes
    f = _load('modes_nms.npz')
    trajs, scores, thr, k = f[name + '_trajs'], f[name + '_scores'], float(f[name + '_thresh']), int(f[name + '_k'])
    t, s, i = modes.batch_nms(_t(trajs), _t(scores), thr, num_ret_modes=k)
    assert i.dtype == torch.int64
    assert np.array_equal(i.cpu().numpy(), f[name + '_ret_idxs'])
    assert np.array_equal(s.cpu().numpy(), f[name + '_ret_scores'])
    assert np.array_equal(t.cpu().numpy(), f[name + '_ret_trajs'])
    a = modes.select_modes(_t(trajs), k=k, dist_thresh=thr, scores=_t(scores))
    b = modes.select_modes(_t(trajs), k=k, dist_thresh=thr, scores=_t(scores))
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                             # two identical calls: bitwise


@pytest.mark.parametrize('name', ['n33', 'n64', 'n33_k8'])
def test_new_batch_nms_equals_the_reference_up_to_the_cluster_member(name):
    from infgen_amd import modes
    f = _load('modes_density.npz')
    trajs, label, thr, k = f[name + '_trajs'], f[name + '_label'], float(f[name + '_thresh']), int(f[name + '_k'])
    t, s, i = modes.new_batch_nms(_t(trajs), thr, num_ret_modes=k)
    i = i.cpu().numpy()
    assert np.array_equal(s.cpu().numpy(), f[name + '_ret_scores'])          # exactly
    rows = np.arange(len(label))[:, None]
    assert np.array_equal(label[rows, i], label[rows, f[name + '_ret_idxs']])
    wt, ws, wi = R.select_modes(trajs, k, thr)
    assert np.array_equal(i, wi) and np.array_equal(t.cpu().numpy(), wt)     # the member: the restatement's, exactly


# ------------------------------------------------------------------------------------------------------- random inputs, shapes
SHAPES = [(1, 1, 1, 2, (1,)), (5, 2, 7, 2, (1, 2)), (1, 64, 1, 7, (1, 6, 16)), (5, 1, 1, 7, (1,)), (5, 2, 1, 7, (1, 2)), (5, 33, 7, 7, (1, 6, 16)), (257, 16, 1, 2, (6, 16)),
          (257, 64, 7, 2, (6,)), (5, 6, 1, 2, (6,))]


@pytest.mark.parametrize('B, N, T, F, ks', SHAPES)
def test_given_scores_and_density_equal_the_restatement(B, N, T, F, ks):
    from infgen_amd import modes
    # (seeds chosen on the CPU so that no pair of goals sits on the threshold: a million pairs at the largest shape)
    traj, scores = _random_case(B, N, T, F, 1004 if (B, N) == (257, 64) else 100 + B + N + T + F)
    thr = 2.5
    assert len(R.near_threshold(traj, thr)) == 0
    for k in ks:
        _check(modes.select_modes(_t(traj), k=k, dist_thresh=thr, scores=_t(scores)), R.select_modes(traj, k, thr, scores=scores), (k, 'scores'))
        _check(modes.select_modes(_t(traj), k=k, dist_thresh=thr), R.select_modes(traj, k, thr), (k, 'density'))
    _, s, i = modes.select_modes(_t(traj), k=ks[0], dist_thresh=thr, with_traj=False)
    assert _ is None and np.array_equal(i.cpu().numpy(), R.select_modes(traj, ks[0], thr)[2])


@pytest.mark.parametrize('T, t_goal', [(7, 0), (7, 3), (7, 6), (7, -1), (7, -7)])
def test_goal_step(T, t_goal):
    from infgen_amd import modes
    traj, scores = _random_case(5, 33, T, 2, 77)
    assert len(R.near_threshold(traj, 2.5, t_goal)) == 0
    _check(modes.select_modes(_t(traj), k=6, scores=_t(scores), t_goal=t_goal), R.select_modes(traj, 6, 2.5, scores=scores, t_goal=t_goal))
    _check(modes.select_modes(_t(traj), k=6, t_goal=t_goal), R.select_modes(traj, 6, 2.5, t_goal=t_goal))


def test_special_rows_validity_and_the_words_behind_the_outputs():
    """row 0: every candidate within the threshold of the first pick (picks 2..K: the covered candidates in order); row 1: all
    scores 0; rows 2, 3, 4: 0, 1 and K - 1 valid candidates; row 5: half of the candidates invalid; sentinels behind the outputs"""
    from infgen_amd import _lib
    B, N, T, F, K, thr = 6, 33, 7, 2, 6, 2.5
    traj, scores = _random_case(B, N, T, F, 5)
    rng = np.random.default_rng(6)
    traj[0, :, -1] = rng.uniform(-0.5, 0.5, (N, 2)).astype(np.float32)
    scores[1] = 0
    valid = np.ones((B, N), bool)
    valid[2] = False
    valid[3] = False; valid[3, 17] = True
    valid[4] = False; valid[4, [3, 9, 20, 21, 32]] = True
    valid[5, ::2] = False
    assert len(R.near_threshold(traj, thr, valid=valid)) == 0
    for sc in (scores, None):
        wt, ws, wi = R.select_modes(traj, K, thr, scores=sc, valid=valid)
        if sc is not None:
            assert wi[0].tolist() == np.argsort(-scores[0], kind='stable')[:K].tolist()
            assert np.array_equal(wi[1], np.arange(K))
        assert (wi[2] == -1).all() and wi[3].tolist() == [17, -1, -1, -1, -1, -1] and (wi[4] >= 0).sum() == K - 1 and wi[4, -1] == -1
        # ctypes entry on buffers with guard words behind [B][K] / [B][K][T][F]
        x, s_dev, v_dev = _t(traj), (None if sc is None else _t(sc)), _t(valid).view(torch.uint8)
        gi = torch.full((B * K + 64,), -7, dtype=torch.int32, device=DEV)
        gs = torch.full((B * K + 64,), -7.0, device=DEV)
        gt = torch.full((B * K * T * F + 64,), -7.0, device=DEV)
        _lib.check(_lib.load().infgen_select_modes(x.data_ptr(), N * T * F, 0, T * F, F, 1, B, N, T, F, T - 1, K, thr,
                                                   None if s_dev is None else s_dev.data_ptr(), 0, v_dev.data_ptr(), None, 0, 0, 0,
                                                   0.0, 0.0, None, 0, gi.data_ptr(), gs.data_ptr(), gt.data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream), 'infgen_select_modes')
        assert np.array_equal(gi[:B * K].cpu().numpy().reshape(B, K), wi) and bool((gi[B * K:] == -7).all())
        assert np.array_equal(gs[:B * K].cpu().numpy().reshape(B, K), ws) and bool((gs[B * K:] == -7).all())
        assert np.array_equal(gt[:B * K * T * F].cpu().numpy().reshape(B, K, T, F), wt) and bool((gt[B * K * T * F:] == -7).all())
        assert not wt[2].any() and not ws[2].any()


def test_strided_views_are_read_in_place_and_the_torch_op():
    import infgen_amd.torch_ops  # noqa: F401
    from infgen_amd import modes
    S0, n, A_cap, Rr, k = 3, 5, 32, 7, 4
    rng = np.random.default_rng(8)
    eng_layout = rng.normal(0, 3.0, (S0, n, A_cap, Rr, 2)).astype(np.float32)          # a rollout's pred_traj
    scores = rng.uniform(0.01, 1, (S0, A_cap, n)).astype(np.float32)
    view = _t(eng_layout).permute(0, 2, 1, 3, 4)                                       # [S0, A_cap, copies, R, 2], strided
    assert not view.is_contiguous()
    flat = np.ascontiguousarray(eng_layout.transpose(0, 2, 1, 3, 4)).reshape(S0 * A_cap, n, Rr, 2)
    assert len(R.near_threshold(flat, 2.5)) == 0
    want = R.select_modes(flat, k, 2.5, scores=scores.reshape(-1, n))
    got5 = modes.select_modes(view, k=k, scores=_t(scores))
    got4 = modes.select_modes(_t(flat), k=k, scores=_t(scores.reshape(-1, n)))
    _check(got4, want)
    for a, b in zip(got5, got4):
        assert torch.equal(a.reshape(b.shape), b)
    # a wider feature dimension seen through a slice (step stride 7, F = 2), and an odd offset (no 16-byte alignment)
    wide = _t(rng.normal(0, 3.0, (4, 9, 5, 7)).astype(np.float32))
    for sl in (wide[..., :2], wide[..., 1:4], wide[1:, 1:, 1:, :]):
        ref = R.select_modes(sl.cpu().numpy(), 3, 2.5)
        assert len(R.near_threshold(sl.cpu().numpy(), 2.5)) == 0
        _check(modes.select_modes(sl, k=3), ref)
    op = torch.ops.infgen_hip.select_modes(_t(flat), k, 2.5, _t(scores.reshape(-1, n)), None, -1)
    for a, b in zip(op, got4):
        assert torch.equal(a, b)
    op = torch.ops.infgen_hip.select_modes(_t(flat), k)
    for a, b in zip(op, modes.select_modes(_t(flat), k=k)):
        assert torch.equal(a, b)


def test_c_entry_refuses_bad_arguments():
    from infgen_amd import _lib
    lib = _lib.load()
    x = torch.zeros(2 * 65 * 2 * 2, device=DEV)
    i, s = torch.zeros(64, dtype=torch.int32, device=DEV), torch.zeros(64, device=DEV)

    def call(N=4, K=2, T=2, F=2, t_goal=1, step=2, traj=x, idx=i):
        return lib.infgen_select_modes(traj.data_ptr() if traj is not None else None, N * T * F, 0, T * F, step, 1, 2, N, T, F, t_goal, K,
                                       2.5, None, 0, None, None, 0, 0, 0, 0.0, 0.0, None, 0,
                                       idx.data_ptr() if idx is not None else None, s.data_ptr(), None, None)
    assert call() == 0
    for kw, word in ((dict(N=65), '1..64'), (dict(N=0), '1..64'), (dict(K=17, N=32), 'min(N, 16)'), (dict(K=5), 'min(N, 16)'),
                     (dict(K=0), 'min(N, 16)'), (dict(t_goal=2), 't_goal'), (dict(F=1, step=1), 'F at least 2'),
                     (dict(step=1), 'step_stride'), (dict(traj=None), 'traj is NULL'), (dict(idx=None), 'mode_idx')):
        assert call(**kw) < 0
        assert word in lib.infgen_last_error().decode(), kw
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ engine level
def _uniforms(c, S, seed=11):
    return np.random.default_rng(seed).random((c['cfg'].num_decode_steps, S, 8), dtype=np.float32)


def _stacked(eng):
    """[S0, A_cap, copies, R, 2] / [S0, A_cap, copies, R] from outputs_device()'s per-scene dicts, padded with the engine's rows"""
    H = eng.cfg.num_historical_steps
    traj = eng.pred_traj.view(eng.S0, eng.copies, eng.A_cap, eng.R, 2).clone()
    state = eng.pred_state.view(eng.S0, eng.copies, eng.A_cap, eng.R).clone()
    for s, o in enumerate(eng.outputs_device()):
        A = o['pred_traj'].shape[0]
        assert torch.equal(o['pred_traj'][:, H:], traj[s // eng.copies, s % eng.copies, :A])
        assert torch.equal(o['pred_state'][:, H:], state[s // eng.copies, s % eng.copies, :A])
    return traj.permute(0, 2, 1, 3, 4).contiguous(), state.permute(0, 2, 1, 3).contiguous()


def test_engine_select_modes_equals_the_function_on_the_stacked_outputs():
    from infgen_amd import modes, synth
    from test_replay_gpu import _case, _eng, _snap, _same
    c = _case('c1_a8_m128')
    scenes = [c['scene'], synth.make_scene(9301, 8, 128, c['cfg'], vocab=c['vocab'], grid=c['grid'])]
    u = _uniforms(c, 8)
    kw = dict(copies=4, sample_k=5, sample_uniforms=u, token_logprob=True)
    eng, plain = _eng(c, scenes, **kw), _eng(c, scenes, **kw)
    S0, n, A_cap, Rr = eng.S0, eng.copies, eng.A_cap, eng.R
    traj, state = _stacked(eng)
    n0 = torch.tensor([h['A'] for h in eng.hosts[::n]], device=DEV)
    assert not torch.equal(traj[:, :, 0], traj[:, :, 1])                               # the copies were sampled apart
    for t_goal, k, thr in ((None, 4, 2.5), (0, 2, 0.5), (Rr // 2, 4, 1.0)):
        t = Rr - 1 if t_goal is None else t_goal
        # the validity rule, restated: the state at the goal step is neither INVALID nor ENTER, and the row is an initial agent
        valid = (state[..., t] != synth.INVALID) & (state[..., t] != synth.ENTER) & (torch.arange(A_cap, device=DEV)[None, :, None] < n0[:, None, None])
        got = eng.select_modes(k=k, dist_thresh=thr, t_goal=t_goal)
        wt, ws, wi = modes.select_modes(traj, k=k, dist_thresh=thr, valid=valid, t_goal=t)
        assert torch.equal(got['mode_idx'], wi) and torch.equal(got['mode_score'], ws) and torch.equal(got['mode_traj'], wt)
        assert got['mode_idx'].shape == (S0, A_cap, k) and got['mode_traj'].shape == (S0, A_cap, k, Rr, 2)
        assert bool((got['mode_idx'][:, 8:] == -1).all()) and bool((got['mode_idx'][:, :8, 0] >= 0).any())
        assert torch.equal(got['mode_prob'], modes.mode_prob(ws, wi))
        filled = got['mode_idx'][:, :8, 0] >= 0
        assert torch.allclose(got['mode_prob'][:, :8].sum(-1)[filled], torch.ones((), device=DEV))
        # the host-side restatement agrees where no pair sits on the threshold
        flat, v = traj.reshape(-1, n, Rr, 2).cpu().numpy(), valid.reshape(-1, n).cpu().numpy()
        if len(R.near_threshold(flat, thr, t, valid=v)) == 0:
            assert np.array_equal(wi.reshape(-1, k).cpu().numpy(), R.select_modes(flat, k, thr, valid=v, t_goal=t)[2])
    # given scores [S0, copies] serve every row of a scene; 'logprob' is their softmax of rollout_logprob()
    sc = torch.softmax(eng.rollout_logprob().view(S0, n), dim=1).float()
    a, b = eng.select_modes(k=3, scores='logprob'), eng.select_modes(k=3, scores=sc)
    valid = (state[..., -1] != synth.INVALID) & (state[..., -1] != synth.ENTER) & (torch.arange(A_cap, device=DEV)[None, :, None] < n0[:, None, None])
    wt, ws, wi = modes.select_modes(traj, k=3, scores=sc[:, None, :].expand(S0, A_cap, n).contiguous(), valid=valid)
    for x in (a, b):
        assert torch.equal(x['mode_idx'], wi) and torch.equal(x['mode_score'], ws) and torch.equal(x['mode_traj'], wt)
    with pytest.raises(ValueError, match='scenes, copies'):
        eng.select_modes(k=3, scores=torch.zeros(S0, n + 1, device=DEV))
    with pytest.raises(ValueError, match='t_goal'):
        eng.select_modes(k=3, t_goal=Rr)
    # tokens, poses and logits are those of an engine on which select_modes was never called
    _same(_snap(eng), _snap(plain), 'select_modes left the rollout alone')
    for key in ('pred_traj', 'pred_head', 'pred_state', 'token_logprob'):
        assert torch.equal(getattr(eng, key), getattr(plain, key)), key


def test_greedy_copies_return_copy_0_first_with_density_1():
    from test_replay_gpu import _case, _eng
    c = _case('c1_a8_m128')
    eng = _eng(c, copies=4)
    m = eng.select_modes(k=4)
    live = m['mode_idx'][0, :8, 0] >= 0
    assert bool(live.any())
    assert torch.equal(m['mode_idx'][0, :8][live], torch.arange(4, device=DEV, dtype=torch.int32).expand(int(live.sum()), 4))
    assert bool((m['mode_score'][0, :8][live] == 1.0).all())
    assert bool((m['mode_idx'][0, :8][~live] == -1).all()) and bool((m['mode_idx'][0, 8:] == -1).all())
    assert torch.equal(m['mode_traj'][0, :8][live][:, 0], eng.pred_traj[0, :8][live])
    one = _eng(c, run=False)
    with pytest.raises(ValueError, match='copies = 1'):
        one.select_modes()
    cold = _eng(c, run=False, copies=4)                                               # nothing has run on its batch yet
    with pytest.raises(RuntimeError, match='nothing has run'):
        cold.select_modes(k=4)
    eng.reload([c['scene']])                                                          # a reload outdates the rollout
    with pytest.raises(RuntimeError, match='nothing has run'):
        eng.select_modes(k=4)
    eng.rollout()
    assert torch.equal(eng.select_modes(k=4)['mode_idx'], m['mode_idx'])


def test_insertion_engine_rows_beyond_the_initial_count_return_minus_1():
    from test_replay_gpu import _case, _eng
    c = _case('ins_forced_a16_m256', insertion=True)
    eng = _eng(c, copies=2, force_enter=True)
    A0 = eng.hosts[0]['A']
    assert int(eng.n_agents.max()) > A0                                               # agents were inserted
    m = eng.select_modes(k=2)
    assert bool((m['mode_idx'][0, A0:] == -1).all()) and not m['mode_traj'][0, A0:].any() and not m['mode_score'][0, A0:].any()
    assert bool((m['mode_idx'][0, :A0, 0] >= 0).any())


def test_predict_modes_on_a_batch_equals_single_graph_calls():
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_modules_gpu import _to_data
    from test_token_logprob_gpu import _decoder_and_scenes
    c, dec, scenes = _decoder_and_scenes()
    dec.agent_encoder.motion_beam_size = 5
    n, k = 3, 2
    u = _uniforms(c, 2 * n, seed=12)
    both = dec.predict_modes(batch_datas([_to_data(sc, DEV) for sc in scenes[:2]]), n, k=k, sample_uniforms=u)
    assert isinstance(both, list) and len(both) == 2
    for g, sc in enumerate(scenes[:2]):
        one = dec.predict_modes(_to_data(sc, DEV), n, k=k, sample_uniforms=u[:, g * n:(g + 1) * n])
        assert set(one) == {'agent_id', 'pred_traj_modes', 'pred_prob_modes', 'mode_idx'}
        A = one['agent_id'].shape[0]
        assert one['pred_traj_modes'].shape == (A, k, c['cfg'].num_recurrent_steps_val, 2) and one['pred_prob_modes'].shape == (A, k)
        for key in one:
            assert torch.equal(one[key], both[g][key]), (g, key)
        assert bool((one['mode_idx'][:, 0] >= 0).any())
    with pytest.raises(ValueError, match='copies = 1'):
        dec.predict_modes(_to_data(scenes[0], DEV), 1)


# ------------------------------------------------------------------------------------------------------------------ the metrics
def _bar(ref32, ref64):
    """4 x the float32 evaluation's error, or one float32 ulp of the value where that error is zero"""
    err = abs(float(ref32) - float(ref64))
    return (4.0 * err if err > 0 else float(np.spacing(np.float32(abs(ref64))))), err


@pytest.mark.parametrize('name', ['n1_m1_t1', 'n3_m6_t5', 'n300_m8_t5', 'n3_m8_t1', 'n300_m1_t5'])
def test_multi_errors_counters_exact_sums_inside_the_float_bar(name):
    from infgen_amd.utils.metrics import minMultiADE, minMultiFDE, update_multi_traj_metrics
    f = _load('modes_multi.npz')
    pn, qn, wn, vn = (f[f'{name}_{k}'] for k in ('pred', 'target', 'prob', 'valid'))
    p, q, w, v = _t(pn), _t(qn), _t(wn), _t(vn)
    G = int(f['max_guesses'])
    for with_prob in (0, 1):
        for keep in (0, 1):
            key = f'{name}_p{with_prob}_k{keep}'
            kw = dict(pred=p, target=q, prob=w if with_prob else None, valid_mask=v, keep_invalid_final_step=bool(keep))
            runs = []
            for _ in range(2):
                fde, a_f, a_a = minMultiFDE(max_guesses=G), minMultiADE(max_guesses=G), minMultiADE(max_guesses=G)
                fde.update(**kw)
                a_f.update(min_criterion='FDE', **kw)
                a_a.update(min_criterion='ADE', **kw)
                both = (minMultiADE(max_guesses=G), minMultiFDE(max_guesses=G))
                update_multi_traj_metrics(both[0], both[1], p, q, kw['prob'], v, bool(keep), 'FDE')      # one pass feeds both
                runs.append(torch.cat([m.state()['buf'] for m in (fde, a_f, a_a, both[1], both[0])]))
            assert torch.equal(runs[0], runs[1])                                   # bitwise
            assert torch.equal(runs[0][0:4], runs[0][6:10])
            buf = runs[0].cpu()
            for j, tag in enumerate(('fde', 'ade_fde', 'ade_ade')):
                got, cnt = float(buf.view(torch.float64)[2 * j]), int(buf[2 * j + 1])
                assert cnt == int(f[f'{key}_{tag}_count']), (key, tag)
                ref64, ref32 = float(f[f'{key}_{tag}_sum64']), float(f[f'{key}_{tag}_sum32'])
                bar, err32 = _bar(ref32, ref64)
                err = abs(got - ref64)
                print(f'{key} {tag}: device error {err:.3e}, float32 reference error {err32:.3e}, bar {bar:.3e}')
                assert err <= bar, (key, tag, err, bar)
            a, fd, cnt = R.multi_traj_error(pn, qn, wn if with_prob else None, vn, G, bool(keep), 'ADE')
            assert abs(float(buf.view(torch.float64)[4]) - a) <= 1e-12 * max(a, 1e-300) and int(buf[5]) == cnt
            if cnt:
                assert float(fde.compute()) == pytest.approx(float(f[f'{key}_fde_sum64']) / cnt, rel=1e-12)
                assert float(fde.sum) == float(buf.view(torch.float64)[0]) and int(fde.count) == cnt


def test_multi_errors_merge_of_two_halves_and_valid_mask_none():
    from infgen_amd.utils.metrics import minMultiADE, minMultiFDE
    f = _load('modes_multi.npz')
    name = 'n300_m8_t5'
    p, q, w, v = (_t(f[f'{name}_{k}']) for k in ('pred', 'target', 'prob', 'valid'))
    for cls in (minMultiFDE, minMultiADE):
        full, lo, hi = cls(), cls(), cls()
        full.update(pred=p, target=q, prob=w, valid_mask=v)
        lo.update(pred=p[:150], target=q[:150], prob=w[:150], valid_mask=v[:150])
        hi.update(pred=p[150:], target=q[150:], prob=w[150:], valid_mask=v[150:])
        lo.merge(hi.state())
        a, b = full.state()['buf'].cpu(), lo.state()['buf'].cpu()
        assert int(a[1]) == int(b[1]) == int(f[f'{name}_p1_k1_fde_count'])
        sa, sb = float(a.view(torch.float64)[0]), float(b.view(torch.float64)[0])
        # two fixed summation orders of positive float64 terms: a lane holds at most two rows, then a 256-lane tree (8 levels), the
        # workgroups' partials and k_vm_finish's tree (8 levels), one more addition for the merge - fewer than 20 roundings along
        # any path, each at most 2^-53 of the total, in either order
        assert abs(sa - sb) <= 40 * 2.0 ** -53 * sa
        full.update(pred=p, target=q, prob=w, valid_mask=v)
        assert int(full.state()['buf'][1]) == 2 * int(a[1])
        full.reset()
        assert not full.state()['buf'].cpu().numpy().any()
    # no mask: every step valid
    m, m2 = minMultiFDE(), minMultiFDE()
    m.update(pred=p, target=q, prob=w)
    m2.update(pred=p, target=q, prob=w, valid_mask=torch.ones_like(v))
    assert torch.equal(m.state()['buf'], m2.state()['buf']) and int(m.state()['buf'][1]) == 300
    want = R.multi_traj_error(p.cpu().numpy(), q.cpu().numpy(), w.cpu().numpy(), None, 6)[1]
    assert abs(float(m.sum) - want) <= 1e-12 * want
    # the C entry refuses what it cannot do, before anything is launched
    from infgen_amd import _lib
    lib = _lib.load()
    sc = torch.zeros(_lib.VM_SCRATCH_DOUBLES, dtype=torch.float64, device=DEV)
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    args = (p.data_ptr(), q.data_ptr(), None, v.view(torch.uint8).data_ptr(), 300)
    assert lib.infgen_multi_traj_error(*args, 65, 5, 6, 1, 0, acc.data_ptr(), None, sc.data_ptr(), None) < 0
    assert 'M must be' in lib.infgen_last_error().decode()
    assert lib.infgen_multi_traj_error(*args, 8, 5, 6, 1, 2, acc.data_ptr(), None, sc.data_ptr(), None) < 0
    assert lib.infgen_multi_traj_error(*args, 8, 5, 0, 1, 0, acc.data_ptr(), None, sc.data_ptr(), None) < 0
    assert lib.infgen_multi_traj_error(*args, 8, 5, 6, 1, 0, None, None, sc.data_ptr(), None) < 0
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()
