"""GPU: the reference's token-ablation models (use_grid_token / use_head_token / use_state_token = False) roll out through the
HIP library and reproduce the reference's own rollouts (tests/golden/make_golden_ablation.py): tokens, states, ids, types and
labels exact, logits within 1e-3, poses within 1e-3, headings within 1e-4, the seed node's state probability within 1e-4 and
the grid's seed outputs None where the reference returns None.  Every fixture is free-running with a margin above the bar."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ('abl_grid_c1_a8_m128', 'abl_grid_ins_forced_a16_m256', 'abl_grid_ins_natural_a20_m256', 'abl_head_ins_forced_a16_m256',
         'abl_gridhead_ins_natural_a20_m256', 'abl_state_live_a16_m128')
SEED_KEYS = ('next_pos_rel_prob_seed', 'grid_agent_occ_seed', 'grid_pt_occ_seed', 'grid_agent_occ_gt_seed')


def _shapes(variant):
    from infgen_amd import synth
    with open(os.path.join(GOLDEN, 'state_dict_shapes.json')) as f, open(os.path.join(GOLDEN, 'state_dict_shapes_ablation.json')) as g:
        return synth.ablation_shapes(json.load(f), json.load(g)[variant])


def _load(name):
    from infgen_amd import synth
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(str(z['meta']))
    cfg = synth.smart_config() if meta['cfg'] == 'smart' else synth.standard_config()
    for k, v in meta['flags'].items():
        setattr(cfg, k, v)
    cfg.disable_insertion = not meta['insertion']
    vocab = synth.make_agent_vocab(cfg.token_size)
    map_vocab = synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scene = synth.make_scene(meta['seed'], meta['A'], meta['M'], cfg, ego_last=meta['ego_last'], edge_cases=meta['edge_cases'],
                             vocab=vocab, grid=grid)
    sd = synth.fill_state_dict(_shapes(meta['variant']), seed=meta['weight_seed'], rich=True, head_gain=meta['head_gain'])
    return dict(z=z, meta=meta, cfg=cfg, vocab=vocab, map_vocab=map_vocab, grid=grid, scene=scene, sd=sd)


@pytest.fixture(params=[(2, 1), (1, 1), (0, 1), (2, 2), (1, 2), (0, 0)],
                ids=['by-size', 'split16', 'fp32mfma', 'by-size+edge-tile', 'split16+edge-tile', 'fp32mfma+unfused'])
def attn_mode(request):
    """the node-side / edge-side kernel choices of test_rollout_gpu.py's fixture of the same name"""
    from infgen_amd import _lib
    lib = _lib.load()
    _lib.check(lib.infgen_set_attn_mode(request.param[0]))
    _lib.check(lib.infgen_set_edge_fuse(request.param[1]))
    yield request.param
    _lib.check(lib.infgen_set_attn_mode(2))
    _lib.check(lib.infgen_set_edge_fuse(1))


def _check(o, z, meta, ins, logits_tol=1e-3):
    n_lg = z['logits'].shape[0]
    assert z['margin'].min() > 1e-3
    assert o['pos_a'].shape[0] == z['pos_a'].shape[0], (o['pos_a'].shape, z['pos_a'].shape)
    for k in ('next_token_idx', 'next_state_idx', 'agent_id', 'pred_type', 'pred_state', 'pred_valid'):
        assert np.array_equal(np.asarray(o[k]), z[k]), k
    assert np.abs(o['pos_a'] - z['pos_a']).max() <= 1e-3
    assert np.abs(o['head_a'] - z['head_a']).max() <= 1e-4
    assert np.abs(o['pred_traj'] - z['pred_traj']).max() <= 1e-3
    assert np.abs(o['pred_head'] - z['pred_head']).max() <= 1e-4
    assert np.abs(o['pred_shape'] - z['pred_shape']).max() <= 1e-4
    assert np.abs(o['x_pt'] - z['x_pt']).max() <= 1e-4
    if 'logits' in o:
        lg = o['logits']
        for i in range(n_lg):
            n = int(z['n_agents_step'][i])
            assert np.abs(lg[i, :n] - z['logits'][i, :n]).max() <= logits_tol, i
        for i, n in enumerate(z['n_agents_step']):
            assert np.abs(lg[i, :n].max(-1) - z['logit_max'][i, :n]).max() <= logits_tol, i
            assert np.array_equal(lg[i, :n].argmax(-1), z['logit_argmax'][i, :n]), i
    if ins:
        assert np.array_equal(o['next_state_prob_seed'] > 0, z['seed_state_prob'] > 0)
        assert np.abs(o['next_state_prob_seed'] - z['seed_state_prob']).max() <= 1e-4
        for k, none in zip(SEED_KEYS, z['seed_none']):
            assert (o[k] is None) == bool(none), k
        if 'seed_pos_prob' in z.files:
            assert np.abs(o['next_pos_rel_prob_seed'] - z['seed_pos_prob']).max() <= 1e-4
        lab = np.asarray([[int(l[1:]) if l else 0 for l in row] for row in o['agent_labels']], np.int16)
        assert np.array_equal(lab, z['agent_label_k'])


def _np_out(o):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}


@pytest.mark.parametrize('name', CASES)
def test_ablation_rollout_matches_reference_fixture(name, attn_mode):
    from infgen_amd import engine
    c = _load(name)
    z, m = c['z'], c['meta']
    w = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    ins = bool(m['insertion'])
    eng = engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], store_logits=True,
                               live_state=m['live_state'], force_enter=m['insertion'] == 'forced', seed_outputs=ins)
    eng.rollout()
    o = eng.outputs()[0]
    # the fp32-input MFMA kernels (attn_mode 0) sum in another order than the split kernels: on abl_grid_ins_natural_a20_m256
    # their logits differ from the reference's by 1.5e-3 at head gain 64 (2.4e-5 of the gain-1 scale, fp32 noise); tokens stay exact
    _check(o, z, m, ins, logits_tol=1e-3 if attn_mode[0] != 0 else 2e-3)
    if not c['cfg'].use_grid_token and ins:
        assert eng.A_cap >= z['pos_a'].shape[0]         # the default head-room of a grid-off model holds 10 rows per step
    # a second rollout of the same engine is bitwise the first
    eng.rollout()
    o2 = eng.outputs()[0]
    for k in ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'logits'):
        assert np.array_equal(o2[k], o[k]), k
    if ins:
        assert np.array_equal(o2['next_state_prob_seed'], o['next_state_prob_seed'])


def test_state_ablation_changes_the_rollout():
    """the live-state fixture predicts exits: with use_state_token = True the same weights give other states"""
    from infgen_amd import engine
    c = _load('abl_state_live_a16_m128')
    assert c['meta']['exits_predicted'] > 0
    c['cfg'].use_state_token = True
    w = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    eng = engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], live_state=True)
    eng.rollout()
    assert not np.array_equal(eng.outputs()[0]['next_state_idx'], c['z']['next_state_idx'])


def _decoder(c):
    from infgen_amd.modules import Attr_Tokenizer, InfGenDecoder
    from infgen_amd import synth
    cfg = c['cfg']
    tok = Attr_Tokenizer(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius, cfg.angle_interval)
    dec = InfGenDecoder(
        decoder_type='agent_decoder', dataset='waymo', input_dim=2, hidden_dim=128, num_historical_steps=11,
        pl2pl_radius=cfg.pl2pl_radius, time_span=cfg.time_span, pl2a_radius=cfg.pl2a_radius,
        pl2seed_radius=cfg.pl2seed_radius, a2a_radius=cfg.a2a_radius, a2sa_radius=cfg.a2sa_radius,
        pl2sa_radius=cfg.pl2sa_radius, num_freq_bands=64, num_map_layers=3, num_agent_layers=6, num_heads=8,
        head_dim=16, dropout=0.1, map_token={'traj_src': torch.from_numpy(synth.make_map_vocab())}, token_size=2048,
        attr_tokenizer=tok, predict_motion=True, predict_state=True, predict_map=False, predict_occ=cfg.use_grid_token,
        disable_insertion=cfg.disable_insertion, state_token=cfg.state_token, seed_size=1, buffer_size=128,
        num_recurrent_steps_val=cfg.num_recurrent_steps_val, use_grid_token=cfg.use_grid_token,
        use_head_token=cfg.use_head_token, use_state_token=cfg.use_state_token)
    full = {k: torch.from_numpy(c['sd'][k]) if k in c['sd'] else v for k, v in dec.state_dict().items()}
    dec.load_state_dict(full, strict=True)
    return dec.to(torch.device('cuda:0')).eval()


@pytest.mark.parametrize('name', [n for n in CASES if 'live' not in n])
def test_ablation_inference_through_the_module(name, monkeypatch):
    from test_modules_gpu import _to_data
    c = _load(name)
    monkeypatch.setenv('DEBUG', '1' if c['meta']['insertion'] == 'forced' else '0')
    dec = _decoder(c)
    if not c['cfg'].use_grid_token:
        dec.agent_encoder.insert_beam_size = 10      # accepted and ignored without the grid (no cell is drawn)
    out = dec.inference(_to_data(c['scene'], torch.device('cuda:0')))
    _check(_np_out(out), c['z'], c['meta'], bool(c['meta']['insertion']))
    if not c['cfg'].use_grid_token:
        for k in SEED_KEYS:
            assert out[k] is None, k


def test_forward_on_an_ablated_model_names_the_flag():
    c = _load('abl_grid_c1_a8_m128')
    dec = _decoder(c)
    with pytest.raises(NotImplementedError, match='use_grid_token'):
        dec({})


def test_batch_of_three_graphs_and_copies_equal_per_scene_runs(monkeypatch):
    """grid and heading off, natural insertion: a 3-graph Batch (inference) and 3 copies of one scene (inference_rollouts) equal
    the per-scene runs"""
    from infgen_amd import synth
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_modules_gpu import _to_data
    c = _load('abl_gridhead_ins_natural_a20_m256')
    monkeypatch.setenv('DEBUG', '0')
    dev = torch.device('cuda:0')
    dec = _decoder(c)
    scenes = [c['scene']] + [synth.make_scene(7300 + i, a, 256, c['cfg'], ego_last=i == 0, vocab=c['vocab'], grid=c['grid'])
                             for i, a in enumerate((12, 28))]
    out = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
    ptr = out['agent_ptr'].tolist()
    assert out['next_pos_rel_prob_seed'] is None and out['grid_agent_occ_seed'] is None
    for s, sc in enumerate(scenes):
        one = dec.inference(_to_data(sc, dev))
        for k in ('next_token_idx', 'next_state_idx', 'agent_id', 'pred_type'):
            assert torch.equal(out[k][ptr[s]:ptr[s + 1]], one[k]), (s, k)
        assert float((out['pos_a'][ptr[s]:ptr[s + 1]] - one['pos_a']).abs().max()) <= 1e-5
        assert float((out['head_a'][ptr[s]:ptr[s + 1]] - one['head_a']).abs().max()) <= 1e-5
    single = dec.inference(_to_data(c['scene'], dev))
    rolls = dec.inference_rollouts(_to_data(c['scene'], dev), 3)
    assert len(rolls) == 3
    for r in rolls:
        for k in ('next_token_idx', 'next_state_idx', 'agent_id'):
            assert torch.equal(r[k], single[k]), k
        assert float((r['pos_a'] - single['pos_a']).abs().max()) <= 1e-5
        assert torch.allclose(r['next_state_prob_seed'], single['next_state_prob_seed'], atol=1e-6)
        assert r['next_pos_rel_prob_seed'] is None


def test_bf16_mode_on_a_grid_off_model():
    """rollout_precision 'bf16' on a grid-off model (unsharpened head, C2's scene shape), teacher-forced on the fp32 rollout's own
    tokens: within test_bf16_mode_gpu.py's bar - error <= 2e-2, mean <= 3e-3, arg-max agreement >= 95 %"""
    from infgen_amd import engine, synth
    cfg = synth.standard_config()
    cfg.use_grid_token = False
    sd = synth.fill_state_dict(_shapes('grid'), seed=1, rich=True, head_gain=1.0)
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scene = synth.make_scene(synth.scene_seed(2, 0), 32, 512, cfg, vocab=vocab, grid=grid)
    dev = torch.device('cuda:0')
    ref_eng = engine.RolloutEngine(engine.PackedWeights(sd, cfg, dev), [scene], vocab, map_vocab, grid, store_logits=True)
    ref_eng.rollout()
    ref = ref_eng.outputs()[0]
    teacher = [(ref['next_token_idx'], ref['next_state_idx'])]
    w8 = engine.PackedWeights(sd, cfg, dev, operand_bits=8)
    eng = engine.RolloutEngine(w8, [scene], vocab, map_vocab, grid, store_logits=True, teacher=teacher,
                               options=dict(attn_mode=1, fourier_mode=1, layers_p=0, gemm_terms=2))
    eng.rollout()
    lg = eng.outputs()[0]['logits']
    d = np.abs(lg - ref['logits'])
    agree = float((lg.argmax(-1) == ref['logits'].argmax(-1)).mean())
    print(f'grid-off bf16 vs fp32 logits: max {d.max():.2e} mean {d.mean():.2e} agreement {agree:.4f}')
    assert d.max() <= 2e-2 and d.mean() <= 3e-3 and agree >= 0.95
    assert d.mean() > 0                      # (the mode is on)
