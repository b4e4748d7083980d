"""GPU: the validation-step metrics and the open-loop loss on the device (infgen_amd/utils/metrics.py over
infgen_amd/csrc/val_metrics.hip) against the fixtures the reference's own infgen/utils/metrics.py produced
(tests/golden/valmetrics_*.npz): integer counters exactly, float sums within 4 x the error of the reference's own float32
evaluation of the same inputs (4 float32 ulps where that error is zero) - the margin is 4 because the summation orders differ -,
accumulation / merge / reset, bitwise determinism, the argument checks of the C entries, and the caller
(InfGen.validation_step, check_inputs) against tests/val_metrics_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import val_metrics_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ST = R.STATE_TOKEN


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def _dev():
    return torch.device('cuda:0')


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(_dev())
    return t if dtype is None else t.to(dtype)


def _bar(ref32, ref64):
    """4 x the float32 evaluation's error, or 4 float32 ulps of the result where that error is zero"""
    err = abs(float(ref32) - float(ref64))
    return (4.0 * err if err > 0 else 4.0 * float(np.spacing(np.float32(abs(ref64))))), err


def _ints(metric):
    return metric.state()['buf'].cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ integers
@pytest.mark.parametrize('dtype', [torch.int64, torch.int32])
@pytest.mark.parametrize('T', [18, 162])
def test_state_accuracy_counters_exact(T, dtype):
    from infgen_amd.utils.metrics import NumInsertAccuracy, StateAccuracy
    f = _load('valmetrics_state.npz')
    state, mask = _t(f[f't{T}_state'], dtype), _t(f[f't{T}_mask'])
    for n in ('n65', 'n7', 'n1'):
        lo, hi = (int(x) for x in f[f't{T}_{n}_rows'])
        for cls in (StateAccuracy, NumInsertAccuracy):
            m = cls(state_token=ST)
            m.update(state_idx=state[lo:hi])
            assert np.array_equal(_ints(m), f[f't{T}_{n}_nomask']), (T, n)
            m.reset()
            m.update(state_idx=state[lo:hi], valid_mask=mask[lo:hi])
            assert np.array_equal(_ints(m), f[f't{T}_{n}_mask']), (T, n)
    # a view with a row stride (the columns of a wider array) is read in place; a uint8 mask equals the bool mask
    wide = torch.full((65, T + 5), 3, dtype=dtype, device=_dev())
    wide[:, 2:T + 2] = state
    m = StateAccuracy(state_token=ST)
    m.update(state_idx=wide[:, 2:T + 2], valid_mask=mask.to(torch.uint8))
    assert np.array_equal(_ints(m), f[f't{T}_n65_mask'])
    res = m.compute()
    assert res['valid'].is_cuda and float(res['valid']) == pytest.approx(f[f't{T}_n65_mask'][0] / f[f't{T}_n65_mask'][1], rel=1e-6)
    # the reference's text: a 0-dim tensor formats as its number
    assert repr(m) == 'Results of StateAccuracy\n    valid: {}\n    invalid: {}'.format(res['valid'].cpu(), res['invalid'].cpu())


@pytest.mark.parametrize('sdtype, gdtype', [(torch.int64, torch.int64), (torch.int32, torch.int64), (torch.int64, torch.int32),
                                            (torch.int32, torch.int32)])
def test_grid_overlap_counters_exact(sdtype, gdtype):
    from infgen_amd.utils.metrics import GridOverlapRate
    g = _load('valmetrics_grid.npz')
    state, grid = _t(g['state'], sdtype), _t(g['grid'], gdtype)
    kw = dict(num_step=18, state_token=ST, seed_size=int(g['seed_size']), grid_size=int(g['grid_size']))
    m = GridOverlapRate(**kw)
    m.update(state_token=state, grid_index=grid)
    assert np.array_equal(_ints(m).reshape(4, 18), g['out_one'])
    res = m.compute()
    assert set(res) == {'num_overlap_t', 'num_insert_agent_t', 'num_total_agent_t', 'overlap_rate_t', 'num_exceed_seed_t'}
    want = np.nan_to_num(g['out_one'][0] / np.where(g['out_one'][1] == 0, np.nan, g['out_one'][1]))
    assert np.allclose(res['overlap_rate_t'].cpu().numpy(), want, rtol=1e-6) and float(res['overlap_rate_t'][4]) == 0.0
    assert 'num_overlap_t: %s' % g['out_one'][0].tolist() in repr(m)
    m = GridOverlapRate(**kw)
    m.update(state_token=state, grid_index=grid, ptr=_t(g['ptr3']))
    assert np.array_equal(_ints(m).reshape(4, 18), g['out_groups'])
    m = GridOverlapRate(num_step=18, state_token=ST, seed_size=int(g['seed_size']))          # default grid_size: the kernel's limit
    m.update(state_token=state, grid_index=grid)
    assert np.array_equal(_ints(m).reshape(4, 18), g['out_one'])


def test_token_cls_and_average_meter():
    from infgen_amd.utils.metrics import AverageMeter, TokenCls
    rng = np.random.default_rng(5)
    R_ = 1031
    pred = torch.from_numpy(rng.integers(0, 6, (R_, 10)))
    target = torch.from_numpy(rng.integers(0, 6, R_))
    mask = torch.from_numpy(rng.random(R_) > 0.4)
    for guesses, pdt, tdt in ((1, torch.int64, torch.int64), (3, torch.int32, torch.int64), (6, torch.int64, torch.int32), (20, torch.int32, torch.int32)):
        m = TokenCls(max_guesses=guesses)
        m.update(pred=pred.to(_dev(), pdt), target=target.to(_dev(), tdt), valid_mask=mask.to(_dev()))
        acc = (pred[:, :guesses] == target[:, None]).any(1) * mask
        assert _ints(m).tolist() == [int(acc.sum()), int(mask.sum())]
        assert float(m.compute()) == pytest.approx(float(acc.sum()) / float(mask.sum()), rel=1e-6)
    m = TokenCls(max_guesses=1)                                   # [R, 1] argmax column, the state head's layout
    m.update(pred=pred[:, :1].to(_dev()), target=target.to(_dev()), valid_mask=mask.to(_dev()))
    assert _ints(m)[0] == int(((pred[:, 0] == target) & mask).sum())
    val = torch.from_numpy(rng.normal(0, 3, (700, 9)).astype(np.float32))
    a = AverageMeter()
    a.update(val.to(_dev()))
    a.update(val[:3].to(_dev()))
    want = (val.double().sum() + val[:3].double().sum()) / (val.numel() + val[:3].numel())
    assert abs(float(a.compute()) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))


# -------------------------------------------------------------------------------------------------- accumulation, merge, reset
def test_accumulation_merge_reset():
    from infgen_amd.utils.metrics import GridOverlapRate, StateAccuracy, minADE
    f, g, t = _load('valmetrics_state.npz'), _load('valmetrics_grid.npz'), _load('valmetrics_traj.npz')
    state, mask = _t(f['t18_state']), _t(f['t18_mask'])
    a = StateAccuracy(state_token=ST)
    a.update(state_idx=state, valid_mask=mask)
    a.update(state_idx=state[3:10])
    assert np.array_equal(_ints(a), f['t18_n65_mask'] + f['t18_n7_nomask'])
    b, c = StateAccuracy(state_token=ST), StateAccuracy(state_token=ST)
    b.update(state_idx=state, valid_mask=mask)
    c.update(state_idx=state[3:10])
    b.merge(c.state())
    assert np.array_equal(_ints(b), _ints(a))
    a.reset()
    assert not _ints(a).any()
    kw = dict(num_step=18, state_token=ST, seed_size=int(g['seed_size']), grid_size=int(g['grid_size']))
    go, go2 = GridOverlapRate(**kw), GridOverlapRate(**kw)
    for _ in range(2):
        go.update(state_token=_t(g['state']), grid_index=_t(g['grid']))
    assert np.array_equal(_ints(go).reshape(4, 18), 2 * g['out_one'])
    go2.update(state_token=_t(g['state']), grid_index=_t(g['grid']))
    go2.merge(go2.state())
    assert np.array_equal(_ints(go2), _ints(go))
    go.reset()
    assert not _ints(go).any()
    # a float state: two updates = the sum, merge adds the float64 slot as a float
    p, q, v = (_t(t[f't5_{k}']) for k in ('pred', 'target', 'valid'))
    m1, m2 = minADE(max_guesses=1), minADE(max_guesses=1)
    m1.update(pred=p, target=q, valid_mask=v)
    m1.update(pred=p, target=q, valid_mask=v)
    m2.update(pred=p, target=q, valid_mask=v)
    one = float(m2.state()['buf'].view(torch.float64)[0])
    m2.merge(m2.state())
    for m in (m1, m2):
        buf = m.state()['buf']
        assert float(buf.view(torch.float64)[0]) == one + one and int(buf[1]) == 2 * int(t['t5_ade_count'])
    m1.reset()
    assert not _ints(m1).any()


# ---------------------------------------------------------------------------------------------------- float bar and determinism
def _traj_f32(p, q, v):
    """the reference's minADE / minFDE arithmetic (:462-464, :384-387) in float32 on the CPU"""
    T = p.shape[1]
    E = min(70, T)
    ade = ((torch.norm(p[:, :E] - q[:, :E], p=2, dim=-1) * v[:, :E]).sum(dim=-1) / T).sum()
    F = E - 1
    fde = ((torch.norm(p[:, F - 1:F] - q[:, F - 1:F], p=2, dim=-1) * v[:, F - 1].unsqueeze(1)).sum(dim=-1)).sum()
    return float(ade), float(fde)


@pytest.mark.parametrize('T', [5, 91])
def test_traj_error_float_bar_and_determinism(T):
    from infgen_amd.utils.metrics import minADE, minFDE, update_traj_metrics
    t = _load('valmetrics_traj.npz')
    pn, qn, vn = (t[f't{T}_{k}'] for k in ('pred', 'target', 'valid'))
    p, q, v = _t(pn), _t(qn), _t(vn)
    runs = []
    for _ in range(2):
        ade, fde = minADE(max_guesses=1), minFDE(max_guesses=1)
        ade.update(pred=p, target=q, valid_mask=v)
        fde.update(pred=p, target=q, valid_mask=v)
        both = (minADE(max_guesses=1), minFDE(max_guesses=1))
        update_traj_metrics(both[0], both[1], p, q, v)                     # the one-pass form feeds both
        runs.append(torch.cat([ade.state()['buf'], fde.state()['buf'], both[0].state()['buf'], both[1].state()['buf']]))
    assert torch.equal(runs[0], runs[1])                                   # bitwise
    assert torch.equal(runs[0][:4], runs[0][4:])
    buf = runs[0].cpu()
    got = dict(ade=float(buf.view(torch.float64)[0]), fde=float(buf.view(torch.float64)[2]))
    assert int(buf[1]) == int(t[f't{T}_ade_count']) and int(buf[3]) == int(t[f't{T}_fde_count'])
    a32, f32 = _traj_f32(torch.from_numpy(pn), torch.from_numpy(qn), torch.from_numpy(vn))
    for k, ref32 in (('ade', a32), ('fde', f32)):
        ref64 = float(t[f't{T}_{k}_sum'])
        bar, err32 = _bar(ref32, ref64)
        err = abs(got[k] - ref64)
        print(f'traj T={T} {k}: device error {err:.3e}, float32 reference error {err32:.3e}, bar {bar:.3e}')
        assert err <= bar, (k, err, bar)
    assert float(ade.compute()) == pytest.approx(float(t[f't{T}_ade_sum']) / int(t[f't{T}_ade_count']), rel=1e-12)


@pytest.mark.parametrize('name', ['c4_r300', 'c4_r1', 'c2048_r300', 'c2048_r1', 'c4_allmasked'])
def test_masked_cross_entropy_float_bar_and_determinism(name):
    from infgen_amd.utils.metrics import masked_cross_entropy, masked_cross_entropy_sums
    c = _load('valmetrics_ce.npz')
    xn = R.expand_logits(c[name + '_a'], c[name + '_u'], c[name + '_b'], c[name + '_v'])
    wn = c[name + '_weight'] if name + '_weight' in c.files else None
    eps = float(c[name + '_eps'])
    x, y, m = _t(xn), _t(c[name + '_target']), _t(c[name + '_mask'])
    w = _t(wn) if wn is not None else None
    s1 = masked_cross_entropy_sums(x, y, m, w, eps)
    s2 = masked_cross_entropy_sums(x, y.to(torch.int32), m.to(torch.uint8), w, eps)
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))         # bitwise, and int32 targets / uint8 masks are the same
    loss = masked_cross_entropy(x, y, m, weight=w, label_smoothing=eps)
    assert loss.is_cuda and loss.dim() == 0
    if name == 'c4_allmasked':
        assert bool(torch.isnan(loss)) and not s1.cpu().numpy().any()
        return
    mt = torch.from_numpy(c[name + '_mask'])
    ref32 = torch.nn.CrossEntropyLoss(weight=None if wn is None else torch.from_numpy(wn), label_smoothing=eps)(
        torch.from_numpy(xn)[mt], torch.from_numpy(c[name + '_target'])[mt])
    ref64 = float(c[name + '_loss'])
    bar, err32 = _bar(ref32, ref64)
    err = abs(float(loss) - ref64)
    print(f'cross-entropy {name}: device error {err:.3e}, float32 reference error {err32:.3e}, bar {bar:.3e}')
    assert err <= bar, (err, bar)
    want = c[name + '_sums'] if eps else np.array([c[name + '_sums'][0], 0.0, c[name + '_sums'][2]])
    assert np.allclose(s1.cpu().numpy(), want, rtol=1e-12, atol=0)
    # rows of a wider array are read in place (row stride > C)
    wide = torch.zeros(x.shape[0], x.shape[1] + 3, device=_dev())
    wide[:, :x.shape[1]] = x
    assert torch.equal(masked_cross_entropy_sums(wide[:, :x.shape[1]], y, m, w, eps), s1)


# -------------------------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_launch_nothing():
    from infgen_amd import _lib
    lib = _lib.load()
    dev = _dev()
    acc = torch.zeros(4 * 18, dtype=torch.int64, device=dev)
    z = torch.zeros(4, 18, dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.infgen_grid_overlap(z.data_ptr(), 1, 18, z.data_ptr(), 1, 18, 4, 18, None, 1, _lib.GRID_OVERLAP_MAX_CELLS + 1, 2, 4,
                                 acc.data_ptr(), stream)
    assert rc < 0 and b'grid_size' in lib.infgen_last_error()
    rc = lib.infgen_state_accuracy(z.data_ptr(), 1, 4, 0, 18, None, 0, 0, 1, 2, 3, acc.data_ptr(), stream)
    assert rc < 0 and b'T must be' in lib.infgen_last_error()
    assert lib.infgen_state_accuracy(None, 1, 4, 18, 18, None, 0, 0, 1, 2, 3, acc.data_ptr(), stream) < 0
    assert lib.infgen_state_accuracy(z.data_ptr(), 1, -1, 18, 18, None, 0, 0, 1, 2, 3, acc.data_ptr(), stream) < 0
    sc = torch.zeros(_lib.VM_SCRATCH_DOUBLES, dtype=torch.float64, device=dev)
    x = torch.zeros(4, 8, device=dev)
    assert lib.infgen_masked_cross_entropy(x.data_ptr(), 8, z.data_ptr(), 1, z.data_ptr(), None, 4, 0, 0.0, acc.data_ptr(),
                                           sc.data_ptr(), stream) < 0
    assert b'C must be' in lib.infgen_last_error()
    assert lib.infgen_traj_error(x.data_ptr(), x.data_ptr(), z.data_ptr(), 2, 0, acc.data_ptr(), None, sc.data_ptr(), stream) < 0
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()
    with pytest.raises(_lib.InfgenHipError):
        from infgen_amd.utils.metrics import GridOverlapRate
        GridOverlapRate(num_step=18, state_token=ST, seed_size=4, grid_size=10 ** 6).update(state_token=z, grid_index=z)


# -------------------------------------------------------------------------------------------------------------------- the caller
@pytest.fixture(scope='module')
def world():
    from conftest import make_weights
    from infgen_amd import synth
    cfg = synth.standard_config()
    return dict(cfg=cfg, vocab=synth.make_agent_vocab(cfg.token_size), map_vocab=synth.make_map_vocab(),
                sd=make_weights(seed=1, head_gain=64.0))


def _model(world, path, **over):
    from test_model_gpu import _model_config
    from infgen_amd.model import InfGen
    mc = _model_config(world['cfg'])
    for k, v in over.items():
        setattr(mc, k, v)
    m = InfGen(mc, save_path=str(path), map_token_traj=world['map_vocab'], agent_tokens=world['vocab'])
    sd = world['sd']
    full = {k: torch.from_numpy(sd[k[len('encoder.'):]]) if k.startswith('encoder.') and k[len('encoder.'):] in sd else v
            for k, v in m.state_dict().items()}
    m.load_state_dict(full, strict=True)
    m = m.to(_dev()).eval()
    m.noise = False
    m.on_validation_start()
    return m


def _ratio(c):
    with np.errstate(invalid='ignore', divide='ignore'):            # (0 / 0 = nan, like the device division)
        return np.float64(c[0]) / np.float64(c[1]), np.float64(c[2]) / np.float64(c[3])


def _approx(x, rel):
    return pytest.approx(float(x), rel=rel, nan_ok=True)


def test_validation_step_logs_state_accuracy(world, tmp_path):
    """closed loop: the scene of tests/test_model_gpu.py, then a 3-graph Batch (its rows in one call, accumulated on top)"""
    from test_batch_inference_gpu import _raw_batch
    from test_model_gpu import _raw_scene
    dev = _dev()
    model = _model(world, tmp_path)
    model.log_traj_metrics = True
    data = _raw_scene(4242, 12, 160, dev)
    out = model.validation_step(data, 0)
    one = R.state_accuracy(out['next_state_idx'].cpu().numpy())
    assert np.array_equal(_ints(model.StateAccuracy), one)
    va, ia = _ratio(one)
    assert model.logged['valid_accuracy'].is_cuda
    assert one[1] > 0 and float(model.logged['valid_accuracy']) == _approx(va, 1e-6)
    assert float(model.logged['invalid_accuracy']) == _approx(ia, 1e-6)
    # minADE / minFDE of the rollout against the logged tracks (ids 1..11 are rows 1..11 of the scene)
    ids = out['agent_id'].cpu().numpy()
    vm = data['agent']['valid_mask'].cpu().numpy().astype(bool)
    valid = vm[ids] & vm[ids, 10][:, None]
    a, ca, f, cf = R.traj_error(out['pred_traj'].cpu().numpy()[..., :2], data['agent']['position'].cpu().numpy()[ids][..., :2], valid)
    assert ca > 0 and cf > 0
    assert float(model.logged['val_minADE']) == _approx(a / ca, 1e-9)
    assert float(model.logged['val_minFDE']) == _approx(f / cf, 1e-9)
    model.log_traj_metrics = False
    batch = _raw_batch([_raw_scene(s, a_, p, dev) for s, a_, p in ((4243, 9, 96), (4244, 17, 200), (4245, 6, 64))], dev)
    outb = model.validation_step(batch, 1)
    both = one + R.state_accuracy(outb['next_state_idx'].cpu().numpy())
    assert np.array_equal(_ints(model.StateAccuracy), both)
    assert float(model.logged['valid_accuracy']) == _approx(_ratio(both)[0], 1e-6)
    end = model.on_validation_epoch_end()
    assert float(end['invalid_accuracy']) == _approx(_ratio(both)[1], 1e-6)
    assert not _ints(model.StateAccuracy).any() and not _ints(model.minADE).any()


def test_check_inputs_counters(world, tmp_path, capsys):
    from test_model_gpu import _raw_scene
    model = _model(world, tmp_path)
    data = _raw_scene(4242, 12, 160, _dev())
    data = model._fetch_enterings(model.sample_pt_pred(model.match_token_map(model.token_processer(data))))
    model.check_inputs(data)
    inputs = model.get_agent_inputs(data)
    want = R.state_accuracy(inputs['next_state_idx_gt'].cpu().numpy(), inputs['raw_agent_valid_mask'].cpu().numpy())
    assert np.array_equal(_ints(model.StateAccuracy), want)
    assert torch.equal(inputs['next_state_idx_gt'], data['agent']['token_idx'].roll(-1, 1))           # as written (:947)
    grid = R.grid_overlap(inputs['state_token'].cpu().numpy(), inputs['grid_index'].cpu().numpy(), 18, ST['enter'],
                          model.GridOverlapRate.seed_size)
    assert np.array_equal(_ints(model.GridOverlapRate).reshape(4, 18), grid) and grid[2].sum() > 0
    printed = capsys.readouterr().out
    assert 'Results of StateAccuracy' in printed and 'Results of GridOverlapRate' in printed


def test_open_loop_val_loss_within_the_bar(world, tmp_path):
    """val_loss of the open-loop branch against torch.nn.functional.cross_entropy on the gathered rows (the expression the
    branch used before) in float64; yardstick: the same expression in float32 on the CPU"""
    from test_model_gpu import _raw_scene
    weights = [0.5, 1.0, 2.0]                 # the state head has three classes (the agent decoder's valid_state_type)
    model = _model(world, tmp_path, val_open_loop=True, val_close_loop=False, loss_weight={'state_weight': weights})
    torch.manual_seed(0)
    loss = model.validation_step(_raw_scene(4242, 12, 160, _dev()), 0)
    assert loss is model.val_loss and loss.is_cuda and loss.dim() == 0
    pred = {k: v.cpu() for k, v in model.open_loop_pred.items() if torch.is_tensor(v)}
    mt, ms = pred['next_token_eval_mask'], pred['next_state_eval_mask']
    assert int(mt.sum()) > 0 and int(ms.sum()) > 0

    def expression(dt):
        w = torch.tensor(weights, dtype=dt)
        return (torch.nn.functional.cross_entropy(pred['next_token_prob'].to(dt)[mt], pred['next_token_idx_gt'][mt], label_smoothing=0.1)
                + torch.nn.functional.cross_entropy(pred['next_state_prob'].to(dt)[ms], pred['next_state_idx_gt'][ms], weight=w))
    ref64, ref32 = float(expression(torch.float64)), float(expression(torch.float32))
    bar, err32 = _bar(ref32, ref64)
    err = abs(float(loss) - ref64)
    print(f'open-loop val_loss: device error {err:.3e}, float32 reference error {err32:.3e}, bar {bar:.3e}')
    assert err <= bar, (err, bar)
    top = pred['next_token_idx'].reshape(-1, pred['next_token_idx'].shape[-1])[:, 0]
    hits = ((top == pred['next_token_idx_gt'].reshape(-1)) & mt.reshape(-1)).sum()
    assert _ints(model.TokenCls).tolist() == [int(hits), int(mt.sum())]
    assert float(model.logged['val_token_cls_acc']) == pytest.approx(int(hits) / int(mt.sum()), rel=1e-6)
