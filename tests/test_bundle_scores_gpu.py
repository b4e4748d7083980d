"""The batched rollout sink on the GPU: every rollout of every scenario of a rollouts dict from the features to the scores in a
fixed number of library calls (compute_metric_features_batch, infgen_bundle_scores, LongMetric.update_rollouts,
InfGen.score_all_rollouts) against the reference's bundle fixture (tests/golden/make_golden_scores_bundle.py) and against the
per-rollout path applied to the concatenated rollouts."""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 2e-3          # tests/test_metrics_gpu.py::test_scenario_scores_golden: a last-bit feature difference can change a bin


def _fixture(dev):
    from test_bundle_scores_cpu import bundle_fixture
    z, scen, fields, cfg, logp = bundle_fixture()
    config = {f: dict(histogram=dict(min_val=c[0], max_val=c[1], num_bins=int(c[2])), metametric_weight=c[4]) for f, c in cfg.items()}
    return z, _to_dev(scen, dev), fields, config, logp


def _to_dev(scen, dev):
    """the dict as `format_rollouts` leaves it: arrays on the device, scenario_id on the host; plus the host-side row counts"""
    out = {k: v.to(dev) if torch.is_tensor(v) and k != 'scenario_id' else v for k, v in scen.items()}
    out['agent_count'] = torch.bincount(scen['agent_batch'].cpu(), minlength=scen['scenario_id'].shape[0]).tolist()
    return out


def _bits(a, b):
    """equal, NaN positions and payloads included"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.is_floating_point:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _per_rollout_features(scen, road=None):
    from infgen_amd.metrics import compute_metric_features, output_to_rollouts
    return [[compute_metric_features(sc, road_edge_polylines=None if road is None else road[s]) for sc in sr.joint_scenes]
            for s, sr in enumerate(output_to_rollouts({k: v for k, v in scen.items() if k != 'agent_count'}))]


def _concat(per):
    """the reference's bundle (compute_metrics.py:911-916): every field of the rollouts' MetricFeatures concatenated on dim 0"""
    from infgen_amd.metrics import MetricFeatures
    cat = lambda k: None if getattr(per[0], k) is None else torch.cat([getattr(p, k) for p in per], 0)
    return MetricFeatures(**{f.name: cat(f.name) for f in dataclasses.fields(MetricFeatures)})


def _tile(scen, n_scen, n_roll):
    """the same dict repeated to n_scen x the scenarios and n_roll x the rollouts"""
    out = {}
    S = scen['scenario_id'].shape[0]
    n = scen['agent_batch'].shape[0]
    for k, v in scen.items():
        if k == 'scenario_id':
            out[k] = v.repeat(n_scen, 1)
        elif k == 'agent_batch':
            out[k] = torch.cat([v + S * i for i in range(n_scen)])
        elif k == 'agent_count':
            out[k] = list(v) * n_scen
        elif torch.is_tensor(v) and v.dim() >= 2 and v.shape[0] == n:
            out[k] = v.repeat((n_scen, n_roll) + (1,) * (v.dim() - 2))
        else:
            out[k] = v
    return out


def _road(dev):
    from infgen_amd.metrics import tensorize_polylines
    g = np.random.default_rng(5)
    roads = []
    for s in range(2):
        lines = []
        for k in range(3 + s):
            n = (15, 12, 9, 9)[k]                  # the same padded length in both scenarios: identical segment indexing
            t = np.linspace(0, 250, n)
            off = (k - 1.5) * 6.0
            lines.append(np.stack([t * np.cos(0.3) - off * np.sin(0.3) + g.normal(0, 0.2, n),
                                   t * np.sin(0.3) + off * np.cos(0.3) + g.normal(0, 0.2, n), np.zeros(n)], -1).astype(np.float32))
        roads.append(tensorize_polylines(lines, device=dev))
    return roads


def test_batched_features_equal_the_per_rollout_features():
    """(a) `.rollout(b)` against `compute_metric_features` of the same rollout from `output_to_rollouts`: the same kernels on the
    same rows, bitwise on every field (the padding changes only which thread of a launch computes a row, not its arithmetic:
    no feature needs a looser bar), road edges included"""
    from infgen_amd.metrics import compute_metric_features_batch
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    road = _road(dev)
    fb = compute_metric_features_batch(scen, road_edge_polylines=road)
    per = _per_rollout_features(scen, road)
    R = scen['pred_traj'].shape[1]
    assert fb.valid.shape[0] == 2 * R and fb.n_rows.tolist() == [12] * R + [7] * R and fb.bundle.tolist() == [0] * R + [1] * R
    assert not bool(fb.valid[R:, 7:].any()) and bool((fb.object_id[R:, 7:] == -1).all())          # padding rows: invalid
    for s in range(2):
        for r in range(R):
            got, want = fb.rollout(s * R + r), per[s][r]
            for f in dataclasses.fields(want):
                assert _bits(getattr(got, f.name), getattr(want, f.name)), (s, r, f.name)
    assert fb.distance_to_road_edge is not None and fb.offroad_per_step.dtype == torch.bool
    assert compute_metric_features_batch(scen).distance_to_road_edge is None


def test_bundle_scores_match_the_reference_fixture():
    """(b) dict -> batched features -> infgen_bundle_scores against the REFERENCE's compute_scenario_metrics_for_bundle"""
    from infgen_amd.metrics import compute_metric_features_batch, compute_scenario_metrics_batch
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    res = compute_scenario_metrics_batch(config, logp, compute_metric_features_batch(scen), as_dicts=True)
    assert len(res) == 2
    for s, (out, long) in enumerate(res):
        for f in fields:
            got, want = out[f + '_likelihood'], float(z[f's{s}_m_{f}_likelihood'])
            print(f'scenario {s} {f}: {got:.7f} reference {want:.7f}')
            assert abs(got - want) <= BAR, (s, f)
            wl = z[f's{s}_l_{f}_likelihood']
            assert tuple(long[f + '_likelihood'].shape) == wl.shape, (s, f)
            assert np.abs(long[f + '_likelihood'].numpy() - wl).max() <= BAR, (s, f)
        assert abs(out['metametric'] - float(z[f's{s}_metametric'])) <= 1e-3
        assert np.abs(long['metametric'].numpy() - z[f's{s}_l_metametric']).max() <= BAR
        assert abs(out['simulated_collision_rate'] - float(z[f's{s}_simulated_collision_rate'])) <= 1e-6


def _compare(res, per, config, logp):
    """-> the largest difference between the fused scoring's per-scenario dicts and `compute_scenario_metrics` on the
    concatenated per-rollout features ``per[s]``; NaN positions and zeros must be the same"""
    from infgen_amd.metrics import compute_scenario_metrics
    worst = 0.0
    for s, (out, long) in enumerate(res):
        want, want_long = compute_scenario_metrics(config, logp, _concat(per[s]))
        for k in want:
            a, b = out[k], want[k]
            assert (a == 0) == (b == 0) and np.isnan(a) == np.isnan(b), (s, k, a, b)
            if not np.isnan(a):
                worst = max(worst, abs(a - b))
        for k in want_long:
            a, b = long[k], want_long[k].cpu()
            assert a.shape == b.shape, (s, k, a.shape, b.shape)
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a == 0, b == 0), (s, k)
            worst = max(worst, float(torch.nan_to_num(a - b).abs().max()))
    return worst


def _compare_with_existing_path(scen, config, logp, fields):
    """the fused scoring of a dict against the per-rollout path on the concatenated rollouts -> (largest difference, result)"""
    from infgen_amd.metrics import compute_metric_features_batch, compute_scenario_metrics_batch
    res = compute_scenario_metrics_batch(config, logp, compute_metric_features_batch(scen), as_dicts=True)
    return _compare(res, _per_rollout_features(scen), config, logp), res


def test_bundle_scores_match_the_per_rollout_path_on_concatenated_rollouts():
    """(c) same features, same per-(object, window) sums: what differs is the order of the reductions over objects and windows
    (and libm's exp against torch's).  The bar stays the 2e-3 of the device-vs-reference test; the measured maximum is printed"""
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    worst, _ = _compare_with_existing_path(scen, config, logp, fields)
    print(f'max |fused - per-rollout path| = {worst:.3e}')
    assert worst <= BAR


def test_nan_and_zero_rules():
    """(d) a scenario without any placement (two fields empty everywhere: likelihood 0, meta-metric per window 0), agents that
    are invalid over whole windows (NaN per (object, window), left out of the means), and a scenario none of whose agents is
    ever valid (every windowed field empty): NaN positions and zeros equal the existing path's"""
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    scen = dict(scen)
    st = scen['pred_state'].clone()
    st[scen['agent_batch'] == 0] = 1                                   # scenario 0: nobody enters or leaves
    valid = scen['pred_valid'].clone()
    rows1 = torch.nonzero(scen['agent_batch'] == 1)[:, 0]
    valid[rows1[:3], :, 11:131] = False                                # windows 0..8 of three agents of scenario 1: no valid step
    scen.update(pred_state=st, pred_valid=valid)
    worst, res = _compare_with_existing_path(scen, config, logp, fields)
    assert worst <= BAR
    out0, long0 = res[0]
    assert out0['distance_placement_likelihood'] == 0 and out0['distance_removement_likelihood'] == 0
    assert float(long0['distance_placement_likelihood'].abs().max()) == 0 and float(long0['metametric'].abs().max()) == 0
    assert res[1][0]['distance_placement_likelihood'] > 0
    dead = dict(scen)
    v2 = valid.clone()
    v2[rows1] = False
    dead['pred_valid'] = v2
    worst, res = _compare_with_existing_path(dead, config, logp, fields)
    assert worst <= BAR
    assert all(res[1][0][f + '_likelihood'] == 0 for f in fields if f not in ('collision_indication', 'num_placement', 'num_removement'))


class _Counting:
    """stands in for the ctypes handle `_lib.load()` returns: counts the calls of every entry"""

    def __init__(self, lib):
        self._lib_, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib_, name)
        if not name.startswith('infgen_'):
            return fn

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return counted


def test_launch_and_copy_counts_do_not_grow_with_the_batch(monkeypatch):
    """(e) library calls for the fixture's 2 x 3 dict and for the same dict tiled to 8 x 6: equal; one device -> host copy per
    update_rollouts"""
    from infgen_amd import _lib
    from infgen_amd.metrics import LongMetric, compute_metrics as cm
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    big = _tile(scen, 4, 2)
    assert big['scenario_id'].shape[0] == 8 and big['pred_traj'].shape[1] == 6
    proxy = _Counting(_lib.load())
    monkeypatch.setattr(_lib, '_lib', proxy)
    copies = []
    real = cm.to_host
    monkeypatch.setattr(cm, 'to_host', lambda t: (copies.append(tuple(t.shape)), real(t))[1])
    counts = []
    for d in (scen, big):
        proxy.calls = {}
        copies.clear()
        lm = LongMetric(metrics_config=config, log_distributions=logp)
        fb = lm.update_rollouts(d)
        assert len(copies) <= 1, copies
        assert lm.scenario_counter == d['scenario_id'].shape[0]
        counts.append(dict(proxy.calls))
        assert fb.valid.shape[0] == d['scenario_id'].shape[0] * d['pred_traj'].shape[1]
    print('library calls:', counts[0])
    assert counts[0] == counts[1]
    assert counts[0].get('infgen_bundle_scores') == 1 and 'infgen_window_log_likelihood' not in counts[0]
    assert sum(v for k, v in counts[0].items() if k != 'infgen_last_error') <= 6


def test_update_rollouts_leaves_the_state_of_per_scenario_updates():
    """(f) LongMetric.update_rollouts == update(metrics=...) per scenario fed from the batch result; compute() works; the
    device counters agree with the accumulated ones"""
    from infgen_amd.metrics import LongMetric, compute_metric_features_batch, compute_scenario_metrics_batch
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    a = LongMetric(prefix='val', metrics_config=config, log_distributions=logp)
    a.update_rollouts(scen)
    res = compute_scenario_metrics_batch(config, logp, compute_metric_features_batch(scen))
    b = LongMetric(prefix='val', metrics_config=config, log_distributions=logp)
    for m in res.to_dicts():
        b.update(metrics=m)
    sa, sb = a.state(), b.state()
    assert sa['sums'] == sb['sums'] and sa['counters'] == sb['counters']
    assert tuple(int(c) for c in sa['counters']) == tuple(res.counters.tolist()) == (2, 2, 2)
    for k in a.field_names:
        assert len(sa['longs'][k]) == len(sb['longs'][k])
        assert all(_bits(p, q) for p, q in zip(sa['longs'][k], sb['longs'][k])), k
    assert [tuple(t.shape) for t in sa['longs']['num_placement_likelihood']] == [(3, 25)] * 2
    out = a.compute()
    assert out['val/wosac/scenario_counter'] == 2
    want = np.mean([float(z[f's{s}_metametric']) for s in range(2)])
    assert abs(out['val/wosac/realism_meta_metric'] - want) <= 1e-3
    assert len(out['val/wosac_long/realism_meta_metric']) == 25


def test_validation_step_scores_all_rollouts(tmp_path):
    """(g) a 3-graph Batch with n_rollout_close_val = 3: score_all_rollouts fills scenario_features_batch with 9 bundles and
    feeds the LongMetric; with the flag off the step does what it does today"""
    from conftest import make_weights
    from test_batch_inference_gpu import _raw_batch
    from test_model_gpu import _model_config, _raw_scene
    from infgen_amd import synth
    from infgen_amd.metrics import LongMetric
    from infgen_amd.model import InfGen
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    cfg = synth.standard_config()
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    sd = make_weights(seed=1, head_gain=64.0)

    def model(path, flag):
        m = InfGen(_model_config(cfg), save_path=str(path), map_token_traj=map_vocab, agent_tokens=vocab)
        assert m.score_all_rollouts is False
        full = {k: torch.from_numpy(sd[k[len('encoder.'):]]) if k.startswith('encoder.') and k[len('encoder.'):] in sd else v
                for k, v in m.state_dict().items()}
        m.load_state_dict(full, strict=True)
        m = m.to(dev).eval()
        m.set('validation')
        m.noise = False
        m.n_rollout_close_val = 3
        m.score_all_rollouts = flag
        m._long_metrics = LongMetric(metrics_config=config, log_distributions=logp)
        m.on_validation_start()
        return m
    spec = [(4242, 12, 160), (4243, 9, 96), (4244, 17, 200)]
    for name in ('on', 'off'):
        (tmp_path / name).mkdir()
    on, off = model(tmp_path / 'on', True), model(tmp_path / 'off', False)
    torch.manual_seed(0)
    r_on = on.validation_step(_raw_batch([_raw_scene(s, a, p, dev) for s, a, p in spec], dev), 0)
    torch.manual_seed(0)
    r_off = off.validation_step(_raw_batch([_raw_scene(s, a, p, dev) for s, a, p in spec], dev), 0)
    fb = on.scenario_features_batch
    assert fb is not None and fb.valid.shape[0] == 9 and fb.n_scenario == 3 and fb.n_rollout == 3
    assert on._long_metrics.scenario_counter == 3
    assert [tuple(t.shape)[0] for t in on._long_metrics.longs['num_placement_likelihood']] == [3, 3, 3]
    assert on.scenario_features == []
    # flag off: the last rollout alone, per scenario, as before
    assert off.scenario_features_batch is None and len(off.scenario_features) == 3 and len(off.scenario_rollouts) == 3
    assert off._long_metrics.scenario_counter == 3
    assert [tuple(t.shape)[0] for t in off._long_metrics.longs['num_placement_likelihood']] == [1, 1, 1]
    assert torch.equal(r_on['next_token_idx'], r_off['next_token_idx'])
    # bundle 2 of graph 0 is the rollout the flag-off path scored
    want = off.scenario_features[0].linear_speed
    assert _bits(fb.rollout(2).linear_speed[:want.shape[0]], want)
    assert on._long_metrics.compute()['/wosac/scenario_counter'] == 3


def test_scoring_is_bitwise_reproducible():
    """(h) two runs of the fused scoring: identical bits"""
    from infgen_amd.metrics import compute_metric_features_batch, compute_scenario_metrics_batch
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    fb = compute_metric_features_batch(scen)
    a = compute_scenario_metrics_batch(config, logp, fb).flat.clone()
    b = compute_scenario_metrics_batch(config, logp, compute_metric_features_batch(scen)).flat
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_bundle_scores_torch_op_and_error_returns():
    """the torch.library operator gives the wrapper's numbers; impossible sizes are refused by the C ABI"""
    import infgen_amd.torch_ops  # noqa: F401
    from infgen_amd import _lib
    from infgen_amd.metrics import compute_metric_features_batch, compute_scenario_metrics_batch, pack_score_table
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    fb = compute_metric_features_batch(scen)
    res = compute_scenario_metrics_batch(config, logp, fb)
    scal, lng, per, counters = torch.ops.infgen_hip.bundle_scores(
        fb.valid, fb.collision_per_step, fb.linear_speed, fb.linear_acceleration, fb.angular_speed, fb.angular_acceleration,
        fb.distance_to_nearest_object, fb.time_to_collision, fb.distance_placement, fb.distance_removement, fb.num_placement,
        fb.num_removement, fb.n_rows, pack_score_table(config, logp, dev), 2)
    assert _bits(scal, res.scalars) and _bits(lng, res.long) and _bits(per.view(2, 3, 2, 25), res.long_rollout)
    assert counters.tolist() == res.counters.tolist()
    lib = _lib.load()
    p = fb.n_rows.data_ptr()
    args = lambda T, T2, size: [p] * 14 + [2, 3, 12, T, T, T2, T2, T2, size, 5, 5] + [p] * 4 + [None]
    assert lib.infgen_bundle_scores(*args(200, 40, 300)) != 0              # window longer than the series
    assert lib.infgen_bundle_scores(*args(200, 45, 80)) != 0               # token columns beyond the steps
    assert lib.infgen_bundle_scores(*args(200, 40, 82)) != 0               # size not a multiple of shift


def test_single_windows_without_a_valid_step():
    """(d), sharper: in scenario 1 nobody is valid during the first 100 steps, so windows 0..4 (steps 5 w .. 5 w + 79) are empty
    for EVERY object of every rollout while the later windows hold values: the per-window value of every windowed field is 0
    there and only there, and the per-window meta-metric is 0 exactly where some field is (the zero rule), as in the existing
    path"""
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    scen = dict(scen)
    valid = scen['pred_valid'].clone()
    valid[scen['agent_batch'] == 1, :, 11:111] = False
    scen['pred_valid'] = valid
    worst, res = _compare_with_existing_path(scen, config, logp, fields)
    assert worst <= BAR
    out, long = res[1]
    windowed = [f for f in fields if f not in ('collision_indication', 'num_placement', 'num_removement')]
    for f in windowed:
        assert float(long[f + '_likelihood'][0, :5].abs().max()) == 0, f
    assert bool((long['linear_speed_likelihood'][0, 5:] > 0).all()) and out['linear_speed_likelihood'] > 0
    meta = long['metametric'][0]
    some_zero = torch.stack([long[f + '_likelihood'][0] == 0 for f in fields]).any(0)      # (the counts' fields: rollout 0's row)
    assert torch.equal(meta == 0, some_zero) and bool((meta[:5] == 0).all())
    assert bool((res[0][1]['linear_speed_likelihood'][0] > 0).all())          # scenario 0 is untouched


def _long_dict(steps, dev, agents=(5, 3), R=2, seed=3):
    """a small seeded dict over many steps (vehicles on three lanes, the ego = last row of a scenario, id 999); agent 0 is
    invalid over a long stretch, so some of its windows are empty"""
    rng = np.random.default_rng(seed)
    T10, T2 = 11 + steps, (11 + steps) // 5
    n = sum(agents)
    t = np.arange(T10)[None, None] * 0.1
    s = rng.uniform(0, 60, (n, 1, 1)) + rng.uniform(2, 12, (n, R, 1)) * t
    off = (rng.integers(0, 3, (n, 1, 1)) - 1) * 3.5 + rng.normal(0, 0.3, (n, R, 1))
    heading = 0.3 + rng.normal(0, 0.01, (n, R, T10))
    traj = np.stack([s * np.cos(0.3) - off * np.sin(0.3), s * np.sin(0.3) + off * np.cos(0.3)], -1)
    valid = rng.random((n, R, T10)) > 0.05
    valid[0, :, 200:400] = False
    ids, last = [], -1
    for N in agents:
        last += N
        valid[last] = True
        ids += list(range(100, 100 + N - 1)) + [999]
    shape = np.concatenate([rng.uniform(4.0, 5.5, (n, 1, 1)), rng.uniform(1.8, 2.2, (n, 1, 1)), np.full((n, 1, 1), 1.6)], -1)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    from infgen_amd.metrics import get_scenario_id_int_tensor
    return dict(scenario_id=get_scenario_id_int_tensor(['w%d' % i for i in range(len(agents))]), av_id=999,
                agent_id=torch.tensor(ids)[:, None].repeat(1, R).to(dev),
                agent_batch=torch.repeat_interleave(torch.arange(len(agents)), torch.tensor(agents)).to(dev),
                agent_count=list(agents), pred_traj=f32(traj), pred_z=torch.zeros(n, R, T10, device=dev), pred_head=f32(heading),
                pred_shape=f32(np.broadcast_to(shape, (n, R, 3))), pred_type=torch.zeros(n, R, dtype=torch.long, device=dev),
                pred_state=torch.from_numpy(rng.choice([0, 1, 1, 1, 1, 1, 2, 3], size=(n, R, T2)).astype(np.int64)).to(dev),
                pred_valid=torch.from_numpy(valid).to(dev), token_pos=f32(traj[:, :, ::5][:, :, :T2]),
                token_head=f32(heading[:, :, ::5][:, :, :T2]))


@pytest.mark.parametrize('steps,windows', [(800, 145), (1400, 265)])
def test_window_counts_beyond_a_wave_and_beyond_a_workgroup(steps, windows):
    """the lane layout of k_bundle_field at 145 windows (an 800-step rollout: 256 window lanes, one row lane) and at 265 (more
    windows than the workgroup has threads: the chunked window loop), against the per-rollout path on the concatenated
    rollouts, to the same 2e-3 bar"""
    dev = torch.device('cuda:0')
    z, _, fields, config, logp = _fixture(dev)
    scen = _long_dict(steps, dev)
    worst, res = _compare_with_existing_path(scen, config, logp, fields)
    print(f'{windows} windows: max |fused - per-rollout path| = {worst:.3e}')
    assert worst <= BAR
    for out, long in res:
        assert all(tuple(long[f + '_likelihood'].shape) == ((2 if f.startswith('num_') else 1), windows) for f in fields)
        assert long['metametric'].shape == (1, windows) and out['linear_speed_likelihood'] > 0


def _split_copies(scen, drop):
    """the fixture's dict taken apart into the per-copy dicts `InfGenDecoder.inference_rollouts` returns for a 2-graph Batch:
    copy j = rollout j without the rows ``drop[j]`` (as if only the other copies had inserted those agents)"""
    back = dict(pred_valid='pred_valid', pos_a='token_pos', head_a='token_head', pred_traj='pred_traj', pred_head='pred_head',
                pred_z='pred_z', eval_shape='pred_shape', pred_type='pred_type', next_state_idx='pred_state', agent_id='agent_id')
    n = scen['agent_batch'].shape[0]
    dev = scen['pred_traj'].device
    copies = []
    for j, gone in enumerate(drop):
        keep = torch.tensor([i for i in range(n) if i not in gone], device=dev)
        d = {dst: scen[src][keep, j].contiguous() for dst, src in back.items()}
        batch = scen['agent_batch'][keep]
        ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.bincount(batch, minlength=2).cumsum(0)])
        d.update(agent_batch=batch, agent_ptr=ptr, ego_index=torch.nonzero(d['agent_id'] == 999)[:, 0])
        copies.append(d)
    return copies


def test_copies_of_different_row_counts_through_the_batched_sink(monkeypatch):
    """a 2-graph Batch with insertion: every copy has its own rows (10 / 12 / 12 of graph 0, 7 / 6 / 5 of graph 1).
    align_rollouts -> format_rollouts -> compute_metric_features_batch -> the fused scoring: the rows a copy lacks are padding
    (invalid, state `invalid`, id -1, outside `n_rows`), `rollout(b)` equals `compute_metric_features` of that copy's OWN rows
    bit for bit, and the scores equal the per-rollout path's on the concatenation of the copies' own features.  Host copies of
    this path: the `agent_ptr`s and the result, two whatever the batch"""
    from infgen_amd.metrics import (LongMetric, align_rollouts, compute_metric_features, compute_metrics as cm,
                                    compute_scenario_metrics_batch, format_rollouts, output_to_rollouts)
    dev = torch.device('cuda:0')
    z, scen, fields, config, logp = _fixture(dev)
    copies = _split_copies(scen, [{3, 7}, {12 + 2}, {12 + 0, 12 + 4}])
    data = {'scenario_id': ['b0', 'b1']}
    host = []
    real = cm.to_host
    monkeypatch.setattr(cm, 'to_host', lambda t: (host.append(tuple(t.shape)), real(t))[1])
    aligned, counts, per_copy = align_rollouts(copies, return_counts=True)
    assert counts == [12, 7] and per_copy == [[10, 12, 12], [7, 6, 5]]
    every = format_rollouts(data, aligned)
    every['agent_count'], every['rollout_rows'] = counts, per_copy
    assert every['pred_traj'].shape[:2] == (19, 3) and every['av_id'].tolist() == [999, 999]
    lm = LongMetric(metrics_config=config, log_distributions=logp)
    fb = lm.update_rollouts(every)
    assert len(host) == 2 and host[0] == (3, 3)
    assert fb.n_rows.tolist() == [10, 12, 12, 7, 6, 5] and fb.valid.shape[:2] == (6, 12)
    state = every['pred_state']
    per = [[None] * 3 for _ in range(2)]
    for j, c in enumerate(copies):
        own = output_to_rollouts(format_rollouts(data, [c]))
        for s in range(2):
            b, n = s * 3 + j, per_copy[s][j]
            want = compute_metric_features(own[s].joint_scenes[0])
            per[s][j] = want
            assert want.valid.shape[0] == n
            got = fb.rollout(b)
            for f in dataclasses.fields(want):
                assert _bits(getattr(got, f.name), getattr(want, f.name)), (s, j, f.name)
            assert not bool(fb.valid[b, n:].any()) and bool((fb.object_id[b, n:] == -1).all())
            rows = torch.nonzero(every['agent_batch'] == s)[:, 0][n:]
            assert bool((state[rows, j] == cm.AGENT_STATE.index('invalid')).all()) and not bool(every['pred_valid'][rows, j].any())
    res = compute_scenario_metrics_batch(config, logp, fb, as_dicts=True)
    worst = _compare(res, per, config, logp)
    print(f'copies of different row counts: max |fused - per-rollout path| = {worst:.3e}')
    assert worst <= BAR
    assert lm.scenario_counter == 2 and lm.compute()['/wosac/scenario_counter'] == 2
