"""GPU: the map encoder's token-prediction head (reference infgen/modules/map_decoder.py:119-129) - infgen_map_token_head through
the operator entry, the torch op and every drop-in entry.  The reference's head is restated here in fp64 (MLPLayer, layers.py:195-215,
then topk of the softmax) and evaluated on the map encoding the module returns (whose own parity with the reference, 1e-4, is
checked by test_modules_gpu.py); pt_pred_mask / pt_target_mask are seeded masks over about a third of the tokens, the share
InfGen.sample_pt_pred draws."""
import numpy as np
import pytest
import torch

from conftest import load_case
from test_batch_inference_gpu import _dec
from test_modules_gpu import _to_data

pytestmark = pytest.mark.gpu

HEAD = 'map_encoder.token_predict_head'


def _head64(sd, x, bf16=False):
    """MLPLayer 128 -> 128 (LayerNorm, ReLU) -> 1024 in fp64; bf16: every GEMM operand rounded to bf16 first (the arithmetic of
    rollout_precision 'bf16': bf16 products, wide accumulation)"""
    g = lambda k: torch.from_numpy(np.asarray(sd[f'{HEAD}.mlp.{k}'], np.float32))
    r = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t.double())
    h = r(x.float().cpu()) @ r(g('0.weight')).T + g('0.bias').double()
    h = torch.nn.functional.layer_norm(h, (128,), g('1.weight').double(), g('1.bias').double(), 1e-5).relu()
    return (r(h.float()) @ r(g('3.weight')).T + g('3.bias').double()).numpy()


def _check_top10(top, ref):
    """indices equal the reference's (softmax -> topk: descending, ties lower index first), except where the reference's logits
    of the two indices differ by at most 1e-4; such mismatches at most 2 % of the (row, position) pairs"""
    top = np.asarray(top)
    want = np.argsort(-ref, axis=1, kind='stable')[:, :10]
    assert top.shape == want.shape
    bad = np.nonzero(top != want)
    for r, p in zip(*bad):
        assert abs(ref[r, top[r, p]] - ref[r, want[r, p]]) <= 1e-4, (r, p)
    assert bad[0].size <= 0.02 * top.size


def _masks(M, seed):
    rng = np.random.default_rng(seed)
    pred = rng.random(M) < 1 / 3
    return pred, np.roll(pred, 1)


def _with_masks(data, pred, target, dev):
    data['pt_token']['pt_pred_mask'] = torch.from_numpy(pred).to(dev)
    data['pt_token']['pt_target_mask'] = torch.from_numpy(target).to(dev)
    return data


def _check_keys(out, sd, pred, target, token_idx):
    n = int(pred.sum())
    assert n > 0
    assert out['map_next_token_prob'].shape == (n, 1024) and out['map_next_token_prob'].dtype == torch.float32
    assert out['map_next_token_idx'].shape == (n, 10) and out['map_next_token_idx'].dtype == torch.long
    assert out['map_next_token_eval_mask'].shape == (n,) and bool(out['map_next_token_eval_mask'].all())
    assert torch.equal(out['map_next_token_idx_gt'].cpu(), torch.as_tensor(token_idx)[torch.from_numpy(target)])
    ref = _head64(sd, out['x_pt'][torch.from_numpy(pred).to(out['x_pt'].device)])
    err = float(np.abs(out['map_next_token_prob'].cpu().numpy() - ref).max())
    print(f'n_pred={n} max logit error {err:.3e}')
    assert err <= 1e-3
    _check_top10(out['map_next_token_idx'].cpu().numpy(), ref)


@pytest.mark.parametrize('name', ['c1_a8_m128', 'c2_a32_m512'])
def test_inference_fills_the_map_head(name):
    """fails on the parent: the keys were (0, 10) / (0, 1024) / (0,) whatever the masks"""
    c = load_case(name)
    dev = torch.device('cuda:0')
    dec = _dec(c)
    M = c['meta']['M']
    pred, target = _masks(M, 11)
    data = _with_masks(_to_data(c['scene'], dev), pred, target, dev)
    out = dec.inference(data)
    _check_keys(out, c['sd'], pred, target, c['scene']['pt_token']['token_idx'])
    # the map encoder alone returns the same keys, bit for bit; a second call too
    enc = dec.map_encoder(data)
    for k in ('map_next_token_prob', 'map_next_token_idx', 'map_next_token_idx_gt', 'map_next_token_eval_mask'):
        assert torch.equal(enc[k], out[k]), k
    again = dec.inference(data)
    assert torch.equal(again['map_next_token_prob'], out['map_next_token_prob'])
    assert torch.equal(again['map_next_token_idx'], out['map_next_token_idx'])
    # inference_no_map passes the caller's map_enc through
    nm = dec.inference_no_map(data, enc)
    assert nm['map_next_token_prob'] is enc['map_next_token_prob']


def test_empty_masks_keep_the_empty_keys():
    c = load_case('c1_a8_m128')
    dev = torch.device('cuda:0')
    dec = _dec(c)
    out = dec.inference(_to_data(c['scene'], dev))          # synth scenes: all-False masks
    for k, shape, dt in (('map_next_token_idx', (0, 10), torch.long), ('map_next_token_prob', (0, 1024), torch.float32),
                         ('map_next_token_idx_gt', (0,), torch.long), ('map_next_token_eval_mask', (0,), torch.bool)):
        assert out[k].shape == shape and out[k].dtype == dt and out[k].device == dev, k


def test_batch_and_copies_equal_single_calls():
    from infgen_amd import synth
    from infgen_amd.modules.infgen_decoder import batch_datas
    c = load_case('a24_m256_edge')
    dev = torch.device('cuda:0')
    dec = _dec(c)
    cfg = c['cfg']
    spec = [(24, 256), (9, 100), (40, 300)]
    scenes = [synth.make_scene(7300 + i, a, m, cfg, ego_last=True, edge_cases=False, vocab=c['vocab'], grid=c['grid'])
              for i, (a, m) in enumerate(spec)]
    masks = [_masks(m, 20 + i) for i, (_, m) in enumerate(spec)]
    datas = [_with_masks(_to_data(sc, dev), p, t, dev) for sc, (p, t) in zip(scenes, masks)]
    singles = [dec.inference(d) for d in datas]
    for s, (sc, (p, t)) in enumerate(zip(scenes, masks)):
        _check_keys(singles[s], c['sd'], p, t, sc['pt_token']['token_idx'])
    b = batch_datas(datas)
    for k in ('pt_pred_mask', 'pt_target_mask'):
        b['pt_token'][k] = torch.cat([d['pt_token'][k] for d in datas])
    out = dec.inference(b)
    for k in ('map_next_token_prob', 'map_next_token_idx', 'map_next_token_idx_gt', 'map_next_token_eval_mask'):
        assert torch.equal(out[k], torch.cat([r[k] for r in singles])), k
    # n rollouts of one scene / n copies per scene: every copy carries the single call's tensors
    for r in dec.inference_rollouts(datas[0], 3):
        for k in ('map_next_token_prob', 'map_next_token_idx', 'map_next_token_idx_gt'):
            assert torch.equal(r[k], singles[0][k]), k
    lst = dec.inference_batch(datas[:2], copies=2)
    assert len(lst) == 4
    for i, r in enumerate(lst):
        assert torch.equal(r['map_next_token_prob'], singles[i // 2]['map_next_token_prob'])
        assert torch.equal(r['map_next_token_idx'], singles[i // 2]['map_next_token_idx'])
    for rr in dec.inference_rollouts(b, 2):
        assert torch.equal(rr['map_next_token_prob'], out['map_next_token_prob'])


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_operator_entry_and_torch_op(mode):
    """both arithmetic paths (mode 0: fp32 MFMA; 1: the split kernel; 2: by size - 12,000 rows take the split kernel) through
    torch.ops.infgen_hip.map_token_head, gathered rows of a wider matrix"""
    import infgen_amd.torch_ops  # noqa: F401
    from infgen_amd import _lib, packing
    c = load_case('c1_a8_m128')
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(mode)
    X = torch.randn(20000, 128, generator=g) * 2.0
    rows = torch.randperm(20000, generator=g)[:12000 if mode == 2 else 700]
    pack = torch.from_numpy(packing.pack_mlp_layer(c['sd'], HEAD)).to(dev)
    lib = _lib.load()
    _lib.check(lib.infgen_set_attn_mode(mode))
    try:
        lg, top = torch.ops.infgen_hip.map_token_head(X.to(dev), rows.to(dev), pack)
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
    ref = _head64(c['sd'], X[rows])
    err = float(np.abs(lg.cpu().numpy() - ref).max())
    print(f'mode {mode}: rows={rows.numel()} max logit error {err:.3e}')
    assert err <= 1e-3
    assert top.dtype == torch.long
    _check_top10(top.cpu().numpy(), ref)


def test_bf16_precision_matches_the_bf16_emulation():
    """rollout_precision 'bf16': the head's max / rms logit error against fp64 within 1.25 x that of a bf16-operand emulation of
    the reference MLPLayer on the same rows (the bar of tests/test_precision_gpu.py)"""
    c = load_case('c2_a32_m512')
    dev = torch.device('cuda:0')
    dec = _dec(c)
    dec.rollout_precision = 'bf16'
    pred, target = _masks(c['meta']['M'], 5)
    out = dec.inference(_with_masks(_to_data(c['scene'], dev), pred, target, dev))
    x = out['x_pt'][torch.from_numpy(pred).to(dev)]
    ref = _head64(c['sd'], x)
    emu = _head64(c['sd'], x, bf16=True)
    mine = out['map_next_token_prob'].cpu().numpy().astype(np.float64)
    e_m, e_e = np.abs(mine - ref), np.abs(emu - ref)
    print(f'bf16: max {e_m.max():.3e} vs {e_e.max():.3e}, rms {np.sqrt((e_m ** 2).mean()):.3e} vs {np.sqrt((e_e ** 2).mean()):.3e}')
    assert e_m.max() <= 1.25 * e_e.max()
    assert np.sqrt((e_m ** 2).mean()) <= 1.25 * np.sqrt((e_e ** 2).mean())


# ---------------------------------------------------------------- against the reference's own outputs (make_golden_maphead.py)
_KEYS = ('map_next_token_prob', 'map_next_token_idx', 'map_next_token_idx_gt', 'map_next_token_eval_mask')


def _fixture(name):
    import json
    import os
    from conftest import GOLDEN, make_weights
    from infgen_amd import synth
    z = np.load(os.path.join(GOLDEN, name + '.npz'))
    meta = json.loads(str(z['meta']))
    cfg = synth.standard_config()
    vocab = synth.make_agent_vocab(cfg.token_size)
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scenes = [synth.make_scene(g['seed'], g['A'], g['M'], cfg, ego_last=g['ego_last'], edge_cases=False, vocab=vocab, grid=grid)
              for g in meta['graphs']]
    return dict(z=z, meta=meta, cfg=cfg, vocab=vocab, grid=grid, scenes=scenes,
                sd=make_weights(seed=meta['weight_seed'], head_gain=meta['head_gain']))


def _fixture_data(f, dev):
    """the fixture's scene (one graph) or Batch (several) with the reference's sampled masks"""
    from infgen_amd.modules.infgen_decoder import batch_datas
    datas = [_to_data(sc, dev) for sc in f['scenes']]
    o = np.concatenate([[0], np.cumsum([g['M'] for g in f['meta']['graphs']])])
    for i, d in enumerate(datas):
        for k in ('pt_pred_mask', 'pt_target_mask', 'pt_valid_mask'):
            d['pt_token'][k] = torch.from_numpy(f['z'][k][o[i]:o[i + 1]]).to(dev)
    if len(datas) == 1:
        return datas[0]
    b = batch_datas(datas)
    for k in ('pt_pred_mask', 'pt_target_mask', 'pt_valid_mask'):
        b['pt_token'][k] = torch.from_numpy(f['z'][k]).to(dev)
    return b


def _check_reference(out, z, where):
    """logits within 1e-3 of the reference's (its stored rows), top-10 equal to the reference's under the rule of
    _check_top10_ref, token_idx[pt_target_mask] and the evaluation mask exact"""
    n = int(z['pt_pred_mask'].sum())
    assert out['map_next_token_prob'].shape == (n, 1024) and out['map_next_token_idx'].shape == (n, 10), where
    lg = out['map_next_token_prob'].cpu().numpy()[z['logit_rows']]
    err = float(np.abs(lg - z['logits']).max())
    print(f'{where}: n_pred={n} max logit error vs the reference {err:.3e}')
    assert err <= 1e-3, where
    _check_top10_ref(out['map_next_token_idx'].cpu().numpy()[z['logit_rows']], z['top_idx'][z['logit_rows']], z['logits'])
    assert np.array_equal(out['map_next_token_idx_gt'].cpu().numpy(), z['idx_gt']), where
    assert out['map_next_token_eval_mask'].dtype == torch.bool and out['map_next_token_eval_mask'].shape == (n,)
    assert bool(out['map_next_token_eval_mask'].all())


def _check_top10_ref(top, want, ref):
    """a mismatch at (row, position) only where the reference's logits of the two indices differ by <= 1e-4; at most 2 % of the
    (row, position) pairs"""
    bad = np.nonzero(top != want)
    for r, p in zip(*bad):
        assert abs(ref[r, top[r, p]] - ref[r, want[r, p]]) <= 1e-4, (r, p)
    assert bad[0].size <= 0.02 * top.size


@pytest.mark.parametrize('name', ['maphead_a8_m128', 'maphead_a32_m512', 'maphead_batch3'])
def test_full_model_matches_the_reference_fixture(name):
    import infgen_amd.torch_ops  # noqa: F401
    f = _fixture(name)
    z = f['z']
    dev = torch.device('cuda:0')
    dec = _dec(f)
    data = _fixture_data(f, dev)
    out = dec.inference(data)
    _check_reference(out, z, f'{name} inference')
    if 'x_pt' in z.files:
        assert float(np.abs(out['x_pt'].cpu().numpy() - z['x_pt']).max()) <= 1e-4
        enc = dec.map_encoder(data)
        _check_reference(enc, z, f'{name} map_encoder')
        rows = torch.from_numpy(np.nonzero(z['pt_pred_mask'])[0]).to(dev)
        lg, top = torch.ops.infgen_hip.map_token_head(enc['x_pt'], rows, dec._weights().map_head)
        _check_reference(dict(enc, map_next_token_prob=lg, map_next_token_idx=top), z, f'{name} torch op')


def _map_only_decoder(f):
    from infgen_amd.modules import Attr_Tokenizer, InfGenDecoder
    from infgen_amd import synth
    cfg = f['cfg']
    tok = Attr_Tokenizer(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius, cfg.angle_interval)
    dec = InfGenDecoder(
        decoder_type='agent_decoder', dataset='waymo', input_dim=2, hidden_dim=128, num_historical_steps=11,
        pl2pl_radius=cfg.pl2pl_radius, time_span=cfg.time_span, pl2a_radius=cfg.pl2a_radius,
        pl2seed_radius=cfg.pl2seed_radius, a2a_radius=cfg.a2a_radius, a2sa_radius=cfg.a2sa_radius,
        pl2sa_radius=cfg.pl2sa_radius, num_freq_bands=64, num_map_layers=3, num_agent_layers=6, num_heads=8,
        head_dim=16, dropout=0.1, map_token={'traj_src': torch.from_numpy(synth.make_map_vocab())}, token_size=2048,
        attr_tokenizer=tok, predict_motion=False, predict_state=False, predict_map=True, predict_occ=False,
        disable_insertion=True, state_token=cfg.state_token, seed_size=1, buffer_size=32,
        num_recurrent_steps_val=cfg.num_recurrent_steps_val)
    dec.load_state_dict({k: torch.from_numpy(f['sd'][k]) if k in f['sd'] else v for k, v in dec.state_dict().items()}, strict=True)
    return dec.to(torch.device('cuda:0')).eval()


@pytest.mark.parametrize('name', ['maphead_a8_m128', 'maphead_a32_m512', 'maphead_batch3'])
def test_map_only_model_matches_the_reference_fixture(name, monkeypatch):
    """configs/pretrain_scalable_map.yaml's model: forward and inference return the reference's key set and values; no
    RolloutEngine is built; with empty masks the head's keys are the empty tensors"""
    import infgen_amd.modules.infgen_decoder as idec
    f = _fixture(name)
    z = f['z']
    dev = torch.device('cuda:0')
    dec = _map_only_decoder(f)

    def refuse(*a, **k):
        raise AssertionError('the map-only model built a RolloutEngine')
    monkeypatch.setattr(idec, 'RolloutEngine', refuse)
    data = _fixture_data(f, dev)
    for entry in (dec.forward, dec.inference):
        out = entry(data)
        assert sorted(out) == f['meta']['map_only_keys'], entry.__name__
        _check_reference(out, z, f'{name} map-only {entry.__name__}')
        if 'x_pt' in z.files:
            assert float(np.abs(out['x_pt'].cpu().numpy() - z['x_pt']).max()) <= 1e-4
    for k in ('pt_pred_mask', 'pt_target_mask'):
        data['pt_token'][k] = torch.zeros_like(data['pt_token'][k])
    out = dec.inference(data)
    for k, shape, dt in (('map_next_token_idx', (0, 10), torch.long), ('map_next_token_prob', (0, 1024), torch.float32),
                         ('map_next_token_idx_gt', (0,), torch.long), ('map_next_token_eval_mask', (0,), torch.bool)):
        assert out[k].shape == shape and out[k].dtype == dt and out[k].device == dev, k
