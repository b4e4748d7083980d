"""GPU: multi-graph (Batch) closed-loop inference - a ragged PyG-style Batch set up on the device by the ingest kernel
(infgen_ingest_batch), decoded in lockstep, returned concatenated through the ragged row pack (infgen_pack_rows).  Every
graph's rows must be what the single-scene / per-scene-list entries return for it."""
import numpy as np
import pytest
import torch

from conftest import load_case
from test_boundary_cpu import _decoder
from test_modules_gpu import _load, _to_data

pytestmark = pytest.mark.gpu

# ('valid_mask' is one of InfGenDecoder.data_keys: the caller's own array passes through, in both entries)
_PER_AGENT = ('agent_id', 'pos_a', 'head_a', 'gt_traj', 'pred_traj', 'pred_head', 'pred_state', 'pred_valid',
              'pred_type', 'pred_shape', 'eval_shape', 'pred_z', 'next_token_idx', 'next_state_idx')


def _dec(c, insertion=False):
    dec = _decoder(c['cfg'])
    dec.agent_encoder.disable_insertion = not insertion
    _load(dec, c['sd'])
    return dec.to(torch.device('cuda:0')).eval()


def _rows(out, key, s):
    """graph s's rows of a batched dict (gt_traj: initial agents; the same rows without insertion)"""
    ptr = out['agent_ptr'].tolist()
    return out[key][ptr[s]:ptr[s + 1]]


def _ragged3(c):
    from infgen_amd import synth
    cfg = c['cfg']
    # (A, M) = (24, 256) with a row filtered before its ego (ego last), (9, 100) with its ego at row 0, (40, 300): the
    # unfiltered maximum 40 and the filtered one round to the same A_cap, so both engines have one shape
    spec = [(24, 256, True, True), (9, 100, False, False), (40, 300, True, False)]
    scenes = [synth.make_scene(7100 + i, a, m, cfg, ego_last=e, edge_cases=ec, vocab=c['vocab'], grid=c['grid'])
              for i, (a, m, e, ec) in enumerate(spec)]
    assert (scenes[0]['agent']['state_idx'][:, cfg.hist_columns - 1] == 0).any()        # a filtered row
    return scenes


def test_ragged_batch_equals_single_scenes():
    from infgen_amd.modules.infgen_decoder import batch_datas
    c = load_case('a24_m256_edge')
    dev = torch.device('cuda:0')
    dec = _dec(c)
    scenes = _ragged3(c)
    datas = [_to_data(sc, dev) for sc in scenes]
    b = batch_datas(datas)
    bs0 = b['batch_size_a'].clone()
    out = dec.inference(b)
    assert out['agent_batch'].dtype == torch.long and out['agent_ptr'].numel() == 4 and out['ego_index'].shape == (3,)
    lst = dec.inference_batch([_to_data(sc, dev) for sc in scenes])             # the per-scene host path
    ptr = out['agent_ptr'].tolist()
    assert torch.equal(out['agent_batch'], torch.repeat_interleave(torch.arange(3, device=dev), torch.tensor(np.diff(ptr), device=dev)))
    mptr = b['pt_token']['ptr'].tolist()
    assert out['valid_mask'] is b['valid_mask'] and out['scenario_id'] == b['scenario_id']
    for s, ref in enumerate(lst):
        for k in _PER_AGENT:
            mine = _rows(out, k, s)
            assert mine.dtype == ref[k].dtype and mine.shape == ref[k].shape and torch.equal(mine, ref[k]), (s, k)
        assert int(out['ego_index'][s]) - ptr[s] == ref['ego_index']
        assert torch.equal(out['x_pt'][mptr[s]:mptr[s + 1]], ref['x_pt'])
    # three single-scene calls: tokens exact, poses to round-off (the bar of test_batched_scenes_equal_single_scene_runs)
    for s, sc in enumerate(scenes):
        d = _to_data(sc, dev)
        bsa = int(d['batch_size_a'][0])
        one = dec.inference(d)
        assert torch.equal(_rows(out, 'next_token_idx', s), one['next_token_idx'])
        assert torch.equal(_rows(out, 'next_state_idx', s), one['next_state_idx'])
        assert float((_rows(out, 'pos_a', s) - one['pos_a']).abs().max()) <= 1e-5
        assert torch.equal(_rows(out, 'agent_id', s), one['agent_id'])
        assert int(out['agent_id'][int(out['ego_index'][s])]) == int(one['agent_id'][one['ego_index']])
        # batch_size_a decreased per graph like the single call's
        assert int(b['batch_size_a'][s]) - int(bs0[s]) == int(d['batch_size_a'][0]) - bsa
    assert int((bs0 - b['batch_size_a']).sum()) >= 1


@pytest.mark.parametrize('copies', [1, 3])
def test_ingest_equals_host_setup(copies):
    """after the ingest kernel every scene buffer and every epilogue input equals what the host setup
    (_setup_scenes -> _scene_arrays -> upload, _epi_from_hosts) leaves, bit for bit - padding included"""
    from infgen_amd import engine, synth
    from infgen_amd.modules.infgen_decoder import batch_datas
    c = load_case('a24_m256_edge')
    cfg = c['cfg']
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(5)
    scenes = [synth.make_scene(8200 + i, int(rng.integers(9, 41)), int(rng.integers(60, 300)), cfg, ego_last=bool(i % 3),
                               edge_cases=bool(i % 2), vocab=c['vocab'], grid=c['grid'], slip=0.1) for i in range(16)]
    nfilt = sum(int((sc['agent']['state_idx'][:, cfg.hist_columns - 1] == 0).sum()) for sc in scenes)
    assert nfilt >= 3
    w = engine.PackedWeights(c['sd'], cfg, dev)
    b = batch_datas([_to_data(sc, dev) for sc in scenes])
    eb = engine.RolloutEngine(w, None, c['vocab'], c['map_vocab'], c['grid'], batch=b, copies=copies)
    eh = engine.RolloutEngine(w, scenes, c['vocab'], c['map_vocab'], c['grid'], copies=copies, a_cap=eb.A_cap, m_cap=eb.M_cap)
    assert (eb.S, eb.S0) == (16 * copies, 16)
    for k in eb._SCENE_ARRAYS:
        x, y = getattr(eb, k), getattr(eh, k)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k
    for k, x, y in zip(('map_tok', 'map_type', 'map_pl', 'map_light'), eb._map_cat, eh._map_cat):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k
    Eh = eh._epi_from_hosts()
    for k in ('htok', 'hst', 'p0', 'h0', 'shp', 'gt', 'val', 'ids', 'n0', 'eval_shape'):
        x, y = eb._epi[k], Eh[k]
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), k
    n_fin, counts = eb.batch_counts()
    assert counts[:, 0].tolist() == [h['A'] for h in eh.hosts] and counts[:, 1].tolist() == [h['av'] for h in eh.hosts]
    removed = [int((~h['filt'][:int(sc['agent']['av_index'][0])]).sum()) for h, sc in zip(eh.hosts, [x for x in scenes for _ in range(copies)])]
    assert counts[:, 2].tolist() == removed


def test_insertion_batch_equals_per_scene_list(monkeypatch):
    """scenario insertion (DEBUG=1 forces 'enter'): agent counts, inserted rows, ids and tokens of a ragged 4-graph batch equal
    the per-scene inference_batch results"""
    from infgen_amd import synth
    from infgen_amd.modules.infgen_decoder import batch_datas
    c = load_case('ins_forced_a16_m256')
    monkeypatch.setenv('DEBUG', '1')
    dev = torch.device('cuda:0')
    dec = _dec(c, insertion=True)
    cfg = c['cfg']
    scenes = [c['scene']] + [synth.make_scene(9300 + i, a, m, cfg, ego_last=False, vocab=c['vocab'], grid=c['grid'])
                             for i, (a, m) in enumerate([(11, 200), (16, 256), (7, 120)])]
    out = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
    lst = dec.inference_batch([_to_data(sc, dev) for sc in scenes], seed_outputs=True)
    assert out['num_inserted'].tolist() == [int(o['num_inserted']) for o in lst] and int(out['num_inserted'].sum()) > 0
    ptr = out['agent_ptr'].tolist()
    assert np.diff(ptr).tolist() == [o['pos_a'].shape[0] for o in lst]
    labels = out['agent_labels']
    for s, ref in enumerate(lst):
        for k in ('agent_id', 'next_token_idx', 'next_state_idx', 'pred_type', 'pred_shape', 'pred_valid'):
            assert torch.equal(_rows(out, k, s), ref[k]), (s, k)
        assert float((_rows(out, 'pos_a', s) - ref['pos_a']).abs().max()) <= 1e-5
        assert labels[ptr[s]:ptr[s + 1]] == ref['agent_labels']
        n = ref['next_state_prob_seed'].shape[0]
        assert torch.allclose(out['next_state_prob_seed'][s * n:(s + 1) * n], ref['next_state_prob_seed'], atol=1e-5)
    assert out['log_message'].count('\n') == 3


def test_sampling_uniforms_per_graph():
    """motion_beam_size = 5 with supplied uniforms [steps][B][cols]: graph s's slice reproduces a single-scene call"""
    from infgen_amd.modules.infgen_decoder import batch_datas
    c = load_case('a24_m256_edge')
    dev = torch.device('cuda:0')
    dec = _dec(c)
    dec.agent_encoder.motion_beam_size = 5
    scenes = _ragged3(c)
    steps = c['cfg'].num_decode_steps
    u = np.random.default_rng(3).random((steps, 3, 40)).astype(np.float32)
    out = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]), sample_uniforms=u)
    greedy = _dec(c).inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
    assert not torch.equal(out['next_token_idx'], greedy['next_token_idx'])           # the uniforms were used
    for s, sc in enumerate(scenes):
        one = dec.inference(_to_data(sc, dev), sample_uniforms=u[:, s:s + 1])
        assert torch.equal(_rows(out, 'next_token_idx', s), one['next_token_idx'])
        assert float((_rows(out, 'pos_a', s) - one['pos_a']).abs().max()) <= 1e-5


def test_pack_rows_equals_cat_of_slices():
    from infgen_amd.engine import pack_rows
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(11)
    S, A_cap = 7, 32
    cnt = torch.tensor([5, 0, 32, 1, 17, 0, 9], dtype=torch.int32)          # a zero-row scene, a full A_cap scene
    srcs = [torch.randn(S, A_cap, 18, 2, generator=g).to(dev),                # 144 B rows: 16-byte copies
            torch.randint(0, 9, (S, A_cap, 18), generator=g).to(dev).bool(),  # 18 B rows: byte copies
            torch.randn(S, A_cap, 3, generator=g).to(dev),                    # 12 B rows: 4-byte copies
            torch.randint(-5, 5, (S, A_cap, 2), generator=g).to(dev)]         # 16 B rows of int64
    counts = torch.stack([cnt, cnt.flip(0), cnt]).T.contiguous().to(dev)      # [S][3]: columns with stride 3
    cols = [counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 0]]
    for scene0, step, n in ((0, 1, S), (1, 2, 3)):
        idx = [scene0 + i * step for i in range(n)]
        tot = [int(sum(int(c_[s].item()) for s in idx)) for c_ in cols]
        got = pack_rows(srcs, cols, tot, n, scene0, step)
        for t_, c_, o in zip(srcs, cols, got):
            ref = torch.cat([t_[s, :int(c_[s].item())] for s in idx])
            assert o.dtype == ref.dtype and o.shape == ref.shape and torch.equal(o, ref)


def test_bad_batch_raises_before_any_launch():
    from infgen_amd.modules.infgen_decoder import batch_datas
    c = load_case('a24_m256_edge')
    dev = torch.device('cuda:0')
    dec = _dec(c)
    scenes = _ragged3(c)
    b = batch_datas([_to_data(sc, dev) for sc in scenes])
    bad = dict(b, agent=dict(b['agent'], ptr=torch.tensor([0, 24, 20, 73], device=dev)))
    with pytest.raises(ValueError):
        dec.inference(bad)
    av = b['agent']['av_index'].clone()
    av[2] = int(b['agent']['ptr'][2]) - 1                                      # the last row of graph 1
    with pytest.raises(ValueError):
        dec.inference(dict(b, agent=dict(b['agent'], av_index=av)))
    assert not dec._engines                                                    # nothing was built


def _raw_batch(raws, dev):
    """raw (pre-tokenisation) scenes of the `_raw_scene` kind -> one Batch of them: rows concatenated, ptr / batch vectors,
    av_idx per graph (inside it, as PyG leaves it), the polygon indices of map_save offset to the batch's polygon rows"""
    B = len(raws)
    cat = lambda vals: torch.cat([v.to(dev) for v in vals])
    A = [r['agent']['num_nodes'] for r in raws]
    P = [r['pt_token']['num_nodes'] for r in raws]
    L = [r['map_polygon']['num_nodes'] for r in raws]
    ptr = lambda n: torch.tensor(np.concatenate([[0], np.cumsum(n)]), device=dev)
    bvec = lambda n: torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(n, device=dev))
    agent = {k: cat([r['agent'][k] for r in raws]) for k in ('id', 'type', 'category', 'valid_mask', 'position', 'heading',
                                                            'velocity', 'shape')}
    agent.update(num_nodes=sum(A), av_idx=torch.tensor([r['agent']['av_idx'] for r in raws], device=dev), ptr=ptr(A), batch=bvec(A))
    pt = {k: cat([r['pt_token'][k] for r in raws]) for k in ('side', 'type', 'pl_type')}
    pt.update(num_nodes=sum(P), ptr=ptr(P), batch=bvec(P))
    loff = np.concatenate([[0], np.cumsum(L)])
    ms = dict(traj_pos=cat([r['map_save']['traj_pos'] for r in raws]), traj_theta=cat([r['map_save']['traj_theta'] for r in raws]),
              pl_idx_list=cat([r['map_save']['pl_idx_list'] + int(loff[i]) for i, r in enumerate(raws)]))
    return {'agent': agent, 'pt_token': pt, 'city': 'synthetic', 'num_graphs': B,
            'scenario_id': [x for r in raws for x in r['scenario_id']], 'tfrecord_path': [x for r in raws for x in r['tfrecord_path']],
            'map_save': ms, 'map_polygon': dict(num_nodes=sum(L), light_type=cat([r['map_polygon']['light_type'] for r in raws]))}


@pytest.mark.parametrize('n_roll', [1, 2])
def test_validation_step_on_a_batch(tmp_path, n_roll):
    """InfGen.validation_step on a 4-graph Batch of raw scenes (pre-processing, rollout, pickle, metric split) writes ONE
    rollouts pickle whose per-scene rows equal four single-graph validation_step pickles; output_to_rollouts yields one
    ScenarioRollouts per scene with that scene's own av_id"""
    import pickle
    from conftest import make_weights
    from test_model_gpu import _model_config, _raw_scene
    from infgen_amd import synth
    from infgen_amd.metrics import compute_metrics as cm
    from infgen_amd.model import InfGen
    dev = torch.device('cuda:0')
    cfg = synth.standard_config()
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    sd = make_weights(seed=1, head_gain=64.0)

    def model(path):
        m = InfGen(_model_config(cfg), save_path=str(path), map_token_traj=map_vocab, agent_tokens=vocab)
        full = {k: torch.from_numpy(sd[k[len('encoder.'):]]) if k.startswith('encoder.') and k[len('encoder.'):] in sd else v
                for k, v in m.state_dict().items()}
        m.load_state_dict(full, strict=True)
        m = m.to(dev).eval()
        m.set('validation')
        m.noise = False
        m.n_rollout_close_val = n_roll
        m.on_validation_start()
        return m
    spec = [(4242, 12, 160), (4243, 9, 96), (4244, 17, 200), (4245, 6, 64)]
    (tmp_path / 'b').mkdir()
    (tmp_path / 's').mkdir()
    mb = model(tmp_path / 'b')
    mb.validation_step(_raw_batch([_raw_scene(s, a, p, dev) for s, a, p in spec], dev), 3)
    assert sorted(x.name for x in (tmp_path / 'b').iterdir()) == ['idx_0_3_rollouts.pkl']
    with open(tmp_path / 'b' / 'idx_0_3_rollouts.pkl', 'rb') as f:
        roll = pickle.load(f)
    assert roll['scenario_id'].shape == (4, 16) and roll['av_id'].dtype == torch.long and roll['av_id'].shape == (4,)
    assert len(mb.scenario_rollouts) == 4 and len(mb.scenario_features) == 4
    ms = model(tmp_path / 's')
    for i, (s, a, p) in enumerate(spec):
        ms.validation_step(_raw_scene(s, a, p, dev), i)
        with open(tmp_path / 's' / f'idx_0_{i}_rollouts.pkl', 'rb') as f:
            one = pickle.load(f)
        rows = torch.nonzero(roll['agent_batch'] == i)[:, 0]
        assert int(roll['av_id'][i]) == one['av_id']
        for k in ('agent_id', 'pred_type', 'pred_state', 'pred_valid', 'pred_shape', 'pred_z'):
            assert torch.equal(roll[k][rows], one[k]), (i, k)
        for k in ('pred_traj', 'pred_head', 'token_pos', 'token_head'):
            assert roll[k][rows].shape == one[k].shape and float((roll[k][rows] - one[k]).abs().max()) <= 1e-4, (i, k)
        assert torch.equal(roll['scenario_id'][i], one['scenario_id'][0])
    sims = cm.output_to_rollouts(roll)
    assert len(sims) == 4 and [x.scenario_id for x in sims] == ['raw_%d' % s for s, _, _ in spec]
    assert [x.joint_scenes[0].av_id for x in sims] == roll['av_id'].tolist()
    assert [x.scenario_id for x in mb.scenario_rollouts] == ['raw_%d' % s for s, _, _ in spec]
    assert [x.joint_scenes[0].av_id for x in mb.scenario_rollouts] == [x.joint_scenes[0].av_id for x in ms.scenario_rollouts]


@pytest.mark.parametrize('path', ['single', 'batch'])
def test_headroom_retry_inside_the_driver(path, monkeypatch):
    """ins_forced_a16_m256 inserts 20 agents into its 16 (DEBUG=1 forces 'enter').  An engine built with 8 rows of head-room has
    A_cap = 32: the rollout raises InsertionHeadroomError (a Python exception from a count the kernel reports) inside the driver,
    which builds an engine of twice the rows, keeps it under the same key, and returns what a decoder that never ran out returns"""
    import infgen_amd.modules.infgen_decoder as idec
    from infgen_amd import synth
    c = load_case('ins_forced_a16_m256')
    monkeypatch.setenv('DEBUG', '1')
    dev = torch.device('cuda:0')
    scenes = [c['scene'], synth.make_scene(9300, 11, 200, c['cfg'], ego_last=False, vocab=c['vocab'], grid=c['grid'])]
    data = ((lambda: idec.batch_datas([_to_data(sc, dev) for sc in scenes])) if path == 'batch' else
            (lambda: _to_data(c['scene'], dev)))
    want = _dec(c, insertion=True).inference(data())
    assert int(torch.as_tensor(want['num_inserted']).reshape(-1)[0]) == 20
    real, built = idec.RolloutEngine, []

    def small_first(*a, **kw):
        if kw.get('insert_headroom') is None:
            kw['insert_headroom'] = 8
        built.append(real(*a, **kw))
        return built[-1]
    monkeypatch.setattr(idec, 'RolloutEngine', small_first)
    dec = _dec(c, insertion=True)
    out = dec.inference(data())
    assert [e.A_cap for e in built] == [32, 64]
    assert len(dec._engines) == 1 and next(iter(dec._engines.values())) is built[1]
    assert set(out) == set(want)
    for k in want:
        a, b = out[k], want[k]
        if isinstance(b, torch.Tensor):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
        else:
            assert a == b, k
