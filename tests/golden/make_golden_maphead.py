#!/usr/bin/env python
"""Golden vectors of the map encoder's token-prediction head (reference infgen/modules/map_decoder.py:119-129), produced by the
REFERENCE's own modules on CPU like make_golden.py (whose scene / weight recipe and stand-ins this reuses):

    tests/golden/maphead_<case>.npz

For every case the reference's ``InfGen.sample_pt_pred`` (infgen/model/infgen.py:986-1006) draws pt_valid / pt_pred / pt_target
masks under torch.manual_seed(seed) over a ``traj_mask`` of 16 points per polyline (side 0), so the M = 16 n_pl map tokens of
synth.make_scene are the True entries in order.  Then:

  * the full model's map encoder (``InfGenDecoder.map_encoder``) -> x_pt, map_next_token_* ;
  * the map-pretraining model (configs/pretrain_scalable_map.yaml: predict_motion / predict_state / predict_occ False, predict_map
    True), with the full model's weights for every key it has (load_state_dict strict), through ``forward`` and ``inference`` -
    both return exactly the map encoder's tensors plus the data keys (checked here, stored once, with the key set).

Stored: masks, logits (the rows ``logit_rows``: every predicted row unless a case sets ``row_stride``; ``meta`` says which), top-10
indices, token_idx[pt_target_mask], x_pt (single scenes), the map-only model's key set.  The batch case is one stand-in
``Batch`` of three ragged graphs (the reference's radius_graph keeps edges inside a graph through pt_token.batch).

Usage:  python tests/golden/make_golden_maphead.py [--cases maphead_a8_m128 ...] [--out DIR]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from infgen_amd import synth  # noqa: E402
import make_golden as mg  # noqa: E402

N_PT = 16

CASES = {
    'maphead_a8_m128': dict(graphs=[dict(A=8, M=128, seed=synth.scene_seed(1, 0), ego_last=True)], mask_seed=0),
    'maphead_a32_m512': dict(graphs=[dict(A=32, M=512, seed=synth.scene_seed(2, 0), ego_last=True)], mask_seed=1),
    'maphead_batch3': dict(graphs=[dict(A=24, M=256, seed=synth.scene_seed(9, 21), ego_last=True),
                                   dict(A=9, M=96, seed=synth.scene_seed(9, 22), ego_last=False),
                                   dict(A=40, M=304, seed=synth.scene_seed(9, 23), ego_last=True)], mask_seed=2),
}
HEAD_GAIN, WEIGHT_SEED = 64.0, 1


def build_map_only(cfg, map_vocab):
    import _standins
    _standins.install()
    from infgen.modules.attr_tokenizer import Attr_Tokenizer
    from infgen.modules.infgen_decoder import InfGenDecoder
    _standins.assert_reference(InfGenDecoder)
    tok = Attr_Tokenizer(grid_range=cfg.grid_range, grid_interval=cfg.grid_interval, radius=cfg.pl2seed_radius,
                         angle_interval=cfg.angle_interval)
    dec = InfGenDecoder(
        decoder_type='agent_decoder', dataset='waymo', input_dim=cfg.input_dim, hidden_dim=cfg.hidden_dim,
        num_historical_steps=cfg.num_historical_steps, pl2pl_radius=cfg.pl2pl_radius, time_span=cfg.time_span,
        pl2a_radius=cfg.pl2a_radius, pl2seed_radius=cfg.pl2seed_radius, a2a_radius=cfg.a2a_radius,
        a2sa_radius=cfg.a2sa_radius, pl2sa_radius=cfg.pl2sa_radius, num_freq_bands=cfg.num_freq_bands,
        num_map_layers=cfg.num_map_layers, num_agent_layers=cfg.num_agent_layers, num_heads=cfg.num_heads,
        head_dim=cfg.head_dim, dropout=0.1, map_token={'traj_src': torch.from_numpy(map_vocab)},
        token_size=cfg.token_size, attr_tokenizer=tok, predict_motion=False, predict_state=False, predict_map=True,
        predict_occ=False, disable_insertion=cfg.disable_insertion, state_token=cfg.state_token, seed_size=cfg.seed_size,
        buffer_size=cfg.buffer_size, num_recurrent_steps_val=cfg.num_recurrent_steps_val, loss_weight=mg.LOSS_WEIGHT, logger=None)
    dec.eval()
    return dec


def sample_masks(data, n_pl, seed):
    """the reference's own InfGen.sample_pt_pred under torch.manual_seed(seed)"""
    # (the module imports the metrics' generated protobuf files, which the installed protobuf only loads in its pure-python mode)
    os.environ.setdefault('PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION', 'python')
    from infgen.model.infgen import InfGen
    import _standins
    _standins.assert_reference(InfGen)
    tm = torch.zeros(n_pl, 3, N_PT, dtype=torch.bool)
    tm[:, 0, :] = True
    data['pt_token']['traj_mask'] = tm
    torch.manual_seed(seed)
    InfGen.sample_pt_pred(None, data)
    del data['pt_token']['traj_mask']
    return data


def make_batch(datas):
    """stand-in Batch of HeteroData graphs laid out like Batch.from_data_list: rows concatenated, ptr / batch, edges offset"""
    from _standins import Batch
    b = Batch()
    M = [int(d['pt_token']['position'].shape[0]) for d in datas]
    L = [int(d['map_polygon']['light_type'].shape[0]) for d in datas]
    mo, lo = np.concatenate([[0], np.cumsum(M)]), np.concatenate([[0], np.cumsum(L)])
    pt = {k: torch.cat([d['pt_token'][k] for d in datas]) for k in datas[0]['pt_token'] if isinstance(datas[0]['pt_token'][k], torch.Tensor)}
    pt['ptr'] = torch.from_numpy(mo)
    pt['batch'] = torch.repeat_interleave(torch.arange(len(datas)), torch.tensor(M))
    b['pt_token'] = pt
    b['map_polygon'] = {'light_type': torch.cat([d['map_polygon']['light_type'] for d in datas])}
    key = ('pt_token', 'to', 'map_polygon')
    b[key] = {'edge_index': torch.cat([d[key]['edge_index'] + torch.tensor([[int(mo[i])], [int(lo[i])]])
                                       for i, d in enumerate(datas)], dim=1)}
    return b


def run_case(name, spec, out_dir):
    cfg = synth.standard_config()
    vocab = synth.make_agent_vocab(cfg.token_size)
    map_vocab = synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    full, _ = mg.build_reference(cfg, map_vocab)
    mg.load_weights(full, seed=WEIGHT_SEED, head_gain=HEAD_GAIN)
    mo = build_map_only(cfg, map_vocab)
    fsd = full.state_dict()
    mo.load_state_dict({k: fsd[k] for k in mo.state_dict()}, strict=True)
    datas = []
    for g in spec['graphs']:
        assert g['M'] % N_PT == 0
        sc = synth.make_scene(g['seed'], g['A'], g['M'], cfg, ego_last=g['ego_last'], edge_cases=False, vocab=vocab, grid=grid)
        datas.append(mg.to_hetero(sc))
    if len(datas) == 1:
        data = sample_masks(datas[0], spec['graphs'][0]['M'] // N_PT, spec['mask_seed'])
    else:
        data = make_batch(datas)
        sample_masks(data, sum(g['M'] for g in spec['graphs']) // N_PT, spec['mask_seed'])
        for k in ('agent_valid_mask', 'category', 'valid_mask', 'av_index', 'shape'):
            data[k] = torch.cat([d[k].reshape(-1) if k == 'av_index' else d[k] for d in datas])
        data['scenario_id'] = [x for d in datas for x in d['scenario_id']]
    with torch.no_grad():
        enc = full.map_encoder(data)
        f_out = mo(data)
        i_out = mo.inference(data)
    keys = sorted(enc) + sorted(k for k in full.data_keys)
    for o in (f_out, i_out):
        assert sorted(o) == sorted(set(keys)), sorted(o)
        for k in enc:
            assert torch.equal(o[k], enc[k]), k
    pm = data['pt_token']['pt_pred_mask'].numpy()
    lg = enc['map_next_token_prob'].numpy().astype(np.float32)
    stride = int(spec.get('row_stride', 1))
    rows = np.arange(0, lg.shape[0], stride)
    top11 = -np.sort(-lg, axis=1)[:, :11]
    gaps = np.diff(-top11, axis=1)
    meta = dict(case=name, cfg='standard', weight_seed=WEIGHT_SEED, head_gain=HEAD_GAIN, mask_seed=spec['mask_seed'], n_pt=N_PT,
                graphs=spec['graphs'], n_pred=int(pm.sum()), logit_rows=f'every {stride} predicted row(s) from row 0',
                map_only_keys=sorted(f_out), small_gap_share=float((gaps < 1e-4).mean()))
    if len(datas) == 1:
        g = spec['graphs'][0]
        meta.update(seed=g['seed'], A=g['A'], M=g['M'], ego_last=g['ego_last'], edge_cases=False)
    extra = dict(x_pt=enc['x_pt'].numpy().astype(np.float32)) if len(datas) == 1 else {}
    np.savez_compressed(os.path.join(out_dir, name + '.npz'), meta=json.dumps(meta),
                        pt_pred_mask=pm, pt_target_mask=data['pt_token']['pt_target_mask'].numpy(),
                        pt_valid_mask=data['pt_token']['pt_valid_mask'].numpy(), logits=lg[rows], logit_rows=rows,
                        top_idx=enc['map_next_token_idx'].numpy(), idx_gt=enc['map_next_token_idx_gt'].numpy(), **extra)
    print(f'{name}: M={pm.size} n_pred={int(pm.sum())} top-11 gaps < 1e-4: {100 * meta["small_gap_share"]:.2f} %')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='*', default=list(CASES))
    ap.add_argument('--out', default=HERE)
    args = ap.parse_args()
    torch.set_num_threads(8)
    for c in args.cases:
        run_case(c, CASES[c], args.out)


if __name__ == '__main__':
    main()
