"""Batched closed-loop rollout engine on one MI355X.

S independent scenes are decoded in lockstep; every per-step kernel works on the
``S * A_cap`` agent rows of the current token column only (windowed K/V ring instead of the
reference's all-columns recompute).  Host code here only allocates device
memory (torch), packs weights and sequences C-ABI calls; all arithmetic of the path runs in
libinfgen_hip.so.

Reference path: ``InfGenDecoder.inference`` -> ``InfGenMapDecoder.forward`` +
``InfGenAgentDecoder.inference`` (infgen/modules/infgen_decoder.py:123-130,
map_decoder.py:70-130, agent_decoder.py:1605-2389), greedy decoding, insertion disabled.
"""
from __future__ import annotations

from collections import namedtuple
import ctypes as C
import hashlib
from dataclasses import replace as dataclasses_replace
import os
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib, constraints, controllers, insertion_rules, logprob, modes, observe, packing, scene_setup
from .scene_setup import EVAL_SHAPE, INVALID_SHAPE
from .synth import INVALID, VALID, ENTER, EXIT, AGENT_SHAPE, RolloutConfig

D = 128
SEED_TYPE = 3


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class LazyOut(dict):
    """One scene's slice of a batch result: a ``dict`` whose values are created on first access.  ``outputs_device`` of a
    512-scene batch used to spend ~30 ms cutting 17 views per scene (and ``InfGenDecoder._run`` another ~60 ms copying and
    completing the dicts) before anything was read; a consumer such as ``validation_step`` reads a handful of keys of one
    scene.  Pending values are thunks in ``_lazy``; every dict operation that could observe a value resolves it first, so
    the object behaves like the plain dict it replaces (same keys, same tensors - views of the batch arrays)."""
    __slots__ = ('_lazy',)

    def __init__(self, eager=None, lazy=None):
        super().__init__(eager or {})
        self._lazy = dict(lazy or {})

    def _force(self, k):
        f = self._lazy.pop(k, None)
        if f is not None:
            super().__setitem__(k, f())

    def _force_all(self):
        for k in list(self._lazy):
            self._force(k)

    def __missing__(self, k):
        if k in self._lazy:
            self._force(k)
            return super().__getitem__(k)
        raise KeyError(k)

    def __contains__(self, k):
        return super().__contains__(k) or k in self._lazy

    def __setitem__(self, k, v):
        self._lazy.pop(k, None)
        super().__setitem__(k, v)

    def __delitem__(self, k):
        if self._lazy.pop(k, None) is None:
            super().__delitem__(k)

    def __len__(self):
        return super().__len__() + len(self._lazy)

    def __iter__(self):
        yield from super().__iter__()
        yield from list(self._lazy)

    def keys(self):
        # a real view (set operations such as ``d.keys() & other`` work); the pending keys are resolved first - every caller that
        # only wants the names uses ``in`` / iteration, which stay lazy
        self._force_all()
        return super().keys()

    def update(self, *args, **kw):
        for k, v in dict(*args, **kw).items():
            self[k] = v

    def __ior__(self, other):
        self.update(other)
        return self

    def __or__(self, other):
        out = self.copy()
        out.update(other)
        return out

    def clear(self):
        self._lazy.clear()
        super().clear()

    def popitem(self):
        self._force_all()
        return super().popitem()

    def values(self):
        self._force_all()
        return super().values()

    def items(self):
        self._force_all()
        return super().items()

    def get(self, k, default=None):
        return self[k] if k in self else default

    def pop(self, k, *default):
        if k in self._lazy:
            self._force(k)
        return super().pop(k, *default)

    def setdefault(self, k, default=None):
        if k in self:
            return self[k]
        self[k] = default
        return default

    def set_lazy(self, k, thunk):
        super().pop(k, None)
        self._lazy[k] = thunk

    def merged(self, first=None, last=None) -> 'LazyOut':
        """{**first, **self, **last} without resolving this dict's pending values"""
        eager = dict(first or {})
        eager.update({k: super(LazyOut, self).__getitem__(k) for k in super().__iter__()})
        out = LazyOut(eager, self._lazy)
        for k, v in (last or {}).items():
            out[k] = v
        return out

    def copy(self):
        return LazyOut({k: super(LazyOut, self).__getitem__(k) for k in super().__iter__()}, self._lazy)

    def __eq__(self, other):
        self._force_all()
        return super().__eq__(other)

    def __repr__(self):
        return f'LazyOut(resolved={list(super().__iter__())}, pending={list(self._lazy)})'


class InsertionHeadroomError(RuntimeError):
    """scenario insertion ran out of agent rows in some scene: results would differ from the reference's, so the rollout
    stops instead of dropping the insertion; the caller re-runs with more ``insert_headroom``"""

    def __init__(self, msg, needed=0):
        super().__init__(msg)
        self.needed = needed


class PackedWeights:
    """Device-resident packed weights of one checkpoint (shared by every engine on the GPU)."""

    def __init__(self, sd: Mapping[str, np.ndarray], cfg: RolloutConfig, device: torch.device,
                 agent_prefix: str = 'agent_encoder', map_prefix: str = 'map_encoder', operand_bits: int = 11):
        """``operand_bits`` = 8: the fp16 planes of every pack hold bf16-precision weights (packing.operand_bits) - the packs
        of the reduced bf16 mode, which only engines running ``gemm_terms = 2`` accept (and which accept no other)"""
        self.operand_bits = int(operand_bits)
        with packing.operand_bits(self.operand_bits):
            self._pack(sd, cfg, device, agent_prefix, map_prefix)

    def _pack(self, sd, cfg, device, agent_prefix, map_prefix):
        self.cfg = cfg
        self.device = device
        ap, mp = agent_prefix, map_prefix
        self.sd = sd
        self.ap, self.mp = ap, mp
        L = cfg.num_agent_layers

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)

        self.attn_t = [dev(packing.pack_attention_layer(sd, f'{ap}.t_attn_layers.{i}')) for i in range(L)]
        self.attn_m = [dev(packing.pack_attention_layer(sd, f'{ap}.pt2a_attn_layers.{i}')) for i in range(L)]
        self.attn_a = [dev(packing.pack_attention_layer(sd, f'{ap}.a2a_attn_layers.{i}')) for i in range(L)]
        self.attn_pt = [dev(packing.pack_attention_layer(sd, f'{mp}.pt2pt_layers.{i}'))
                        for i in range(cfg.num_map_layers)]
        self.four_t = dev(packing.pack_fourier(sd, f'{ap}.r_t_emb', 4))
        self._time_gap_tables = {}
        self.four_m = dev(packing.pack_fourier(sd, f'{ap}.r_pt2a_emb', 3))
        self.four_a = dev(packing.pack_fourier(sd, f'{ap}.r_a2a_emb', 3))
        self.four_xa = dev(packing.pack_fourier(sd, f'{ap}.x_a_emb', 2))
        self.four_pt = dev(packing.pack_fourier(sd, f'{mp}.r_pt2pt_emb', 3))
        # fusion_emb: [token | x_a | state | grid] -> 128, K0 = 384 without the grid embedding (use_grid_token = False)
        self.fusion_k0 = D * (4 if cfg.use_grid_token else 3)
        k0 = packing._get(sd, f'{ap}.fusion_emb.mlp.0.weight').shape[1]
        if k0 != self.fusion_k0:
            raise ValueError(f'fusion_emb takes {k0} inputs, use_grid_token = {cfg.use_grid_token} needs {self.fusion_k0}')
        self.fusion = dev(packing.pack_mlp_embedding(sd, f'{ap}.fusion_emb'))
        self.shape_emb = dev(packing.pack_mlp_embedding(sd, f'{ap}.shape_emb'))
        self.tok_emb = [dev(packing.pack_mlp_embedding(sd, f'{ap}.token_emb_{k}')) for k in ('veh', 'ped', 'cyc')]
        self.grid_emb = dev(packing.pack_mlp_embedding(sd, f'{ap}.token_emb_grid'))
        self.map_tok_emb = dev(packing.pack_mlp_embedding(sd, f'{mp}.token_emb'))
        # the map-token prediction head (map_decoder.py:59-60, 119-121; infgen_map_token_head)
        self.map_head = dev(packing.pack_mlp_layer(sd, f'{mp}.token_predict_head'))
        self.tok_head = dev(packing.pack_mlp_layer(sd, f'{ap}.token_predict_head'))
        self.st_head = dev(packing.pack_mlp_layer(sd, f'{ap}.state_predict_head', row_major_out=True))
        g = lambda k: dev(packing._get(sd, k))
        self.type_a_emb = g(f'{ap}.type_a_emb.weight')
        self.state_a_emb = g(f'{ap}.state_a_emb.weight')
        self.no_token = g(f'{ap}.no_token_emb.weight')
        self.bos_token = g(f'{ap}.bos_token_emb.weight')
        self.invalid_offset = g(f'{ap}.invalid_offset_token_emb.weight')
        self.type_pt_emb = g(f'{mp}.type_pt_emb.weight')
        self.polygon_type_emb = g(f'{mp}.polygon_type_emb.weight')
        self.light_pl_emb = g(f'{mp}.light_pl_emb.weight')
        # scenario insertion (agent_decoder.py:236-290)
        self.attn_pt2sa = [dev(packing.pack_attention_layer(sd, f'{ap}.pt2sa_attn_layers.{i}')) for i in range(3)]
        self.attn_a2sa = [dev(packing.pack_attention_layer(sd, f'{ap}.a2sa_attn_layers.{i}')) for i in range(3)]
        self.attn_occ2sa = [dev(packing.pack_attention_layer(sd, f'{ap}.occ2sa_attn_layers.{i}', has_pos_emb=False))
                            for i in range(3)]
        self.four_pt2sa = dev(packing.pack_fourier(sd, f'{ap}.r_pt2sa_emb', 3))
        self.four_a2sa = dev(packing.pack_fourier(sd, f'{ap}.r_a2sa_emb', 3))
        # the heads of the variant's state_dict: use_grid_token = False replaces the cell / offset heads and the occupancy embedding
        # by seed_pos_rel_xy_predict_head, use_head_token = False the heading-token head by seed_heading_rel_theta_predict_head
        # (agent_decoder.py:267-283)
        heads = ['seed_state_predict_head', 'seed_type_predict_head', 'seed_shape_predict_head']
        heads += (['seed_pos_rel_token_predict_head', 'seed_offset_xy_predict_head', 'seed_agent_occ_embed'] if cfg.use_grid_token
                  else ['seed_pos_rel_xy_predict_head'])
        heads += ['seed_heading_rel_token_predict_head' if cfg.use_head_token else 'seed_heading_rel_theta_predict_head']
        self.heads = {k: dev(packing.pack_mlp_layer(sd, f'{ap}.{k}')) for k in heads}
        self._tables = None
        self._tables_key = None
        self._tables_by_key = {}

    def time_gap_table(self, lib, terms: int, stream):
        """[32][128] table of r_t_emb's fourth branch (the time gap of a temporal edge is one of -1 .. -16, agent_decoder.py:586-600)
        under the arithmetic ``terms`` (infgen_fourier_last_dim_table), cached per pack"""
        tab = self._time_gap_tables.get(terms)
        if tab is None:
            # (the arithmetic is chosen through the calling thread's option block, not by editing the process-wide default)
            o = _lib.Options()
            _lib.check(lib.infgen_get_effective_options(C.byref(o)), 'infgen_get_effective_options')
            tab = torch.zeros(32, D, device=self.four_t.device)
            o.gemm_terms, o.use = terms, 0
            with _lib.thread_options(o):
                _lib.check(lib.infgen_fourier_last_dim_table(_lib.ptr(self.four_t), 4, _lib.ptr(tab), stream),
                           'infgen_fourier_last_dim_table')
            torch.cuda.synchronize(tab.device)
            self._time_gap_tables[terms] = tab
        return tab

    def tables(self, ops: 'Ops', vocab_dev: torch.Tensor, grid_dev: torch.Tensor, map_vocab_dev: torch.Tensor, key: bytes):
        """Per-checkpoint constants (the reference recomputes them in every inference call,
        agent_decoder.py:347-373, map_decoder.py:77-78): token-embedding tables with the bos /
        no_token rows appended, the grid-embedding table with the invalid row, the seed
        categorical embedding and the map-token embedding table.  ``key``: a content hash of the vocabularies / grid the
        caller computed on the host before the upload (``tables_key``) - device addresses say nothing about contents, the
        caching allocator hands a freed engine's addresses to the next one."""
        # one entry PER key, never evicted: engines of different vocabularies share a pack and keep raw pointers to their
        # tables in their contexts / captured graphs (a single-entry cache freed tables a live engine still addressed)
        hit = self._tables_by_key.get(key)
        if hit is not None:
            self._tables, self._tables_key = hit, key
            return hit
        dev, ts, G = self.device, self.cfg.token_size, grid_dev.shape[0]
        tok_tab = torch.empty(3, ts + 2, D, device=dev)
        for k in range(3):
            ops.mlp_embedding(vocab_dev[k][:, -1].reshape(ts, 8).contiguous(), self.tok_emb[k], 8, out=tok_tab[k, :ts])
            tok_tab[k, ts] = self.bos_token[0]
            tok_tab[k, ts + 1] = self.no_token[0]
        grid_tab = torch.empty(G + 1, D, device=dev)
        ops.mlp_embedding(grid_dev, self.grid_emb, 2, out=grid_tab[:G])
        grid_tab[G] = self.invalid_offset[0]
        seed_shape = ops.mlp_embedding(torch.full((1, 3), INVALID_SHAPE, device=dev), self.shape_emb, 3)
        cat_seed = (self.type_a_emb[SEED_TYPE] + seed_shape[0]).contiguous()
        map_tab = ops.mlp_embedding(map_vocab_dev, self.map_tok_emb, map_vocab_dev.shape[1])
        # the all-invalid seed query row (agent_decoder.py:1814-1818): a constant of the weights
        raw = torch.tensor([[2.0 * 2.0 ** 0.5, -2.356194490192345, 0.0, 0.0]], device=dev)   # |(-2,-2)|, atan2(-2,-2)
        fus = torch.zeros(1, self.fusion_k0, device=dev)
        fus[0, :D] = self.no_token[0]
        fus[0, 2 * D:3 * D] = self.state_a_emb[0]
        if self.cfg.use_grid_token:
            fus[0, 3 * D:] = grid_tab[G // 2]
        ops.fourier(raw, 2, self.four_xa, fus[:, D:2 * D], cat=cat_seed[None].contiguous())
        f_seed = ops.mlp_embedding(fus, self.fusion, self.fusion_k0)
        self._tables = dict(tok_tab=tok_tab, grid_tab=grid_tab, cat_seed=cat_seed, map_tab=map_tab, f_seed=f_seed)
        self._tables_key = key
        self._tables_by_key[key] = self._tables
        return self._tables

    @staticmethod
    def tables_key(*arrays: np.ndarray) -> bytes:
        h = hashlib.blake2b(digest_size=16)
        for a in arrays:
            a = np.ascontiguousarray(a)
            h.update(str((a.shape, a.dtype.str)).encode())
            h.update(a.tobytes())
        return h.digest()


class Ops:
    """Thin typed wrappers over the C ABI (torch tensors in, device pointers out)."""

    def __init__(self, device: torch.device):
        self.lib = _lib.load()
        self.device = device

    @property
    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def linear(self, x, w_pack, w_off, n, k, bias_off=None, post_ln_off=None, relu=False, pre_ln=None,
               out=None, ldx=None, gather=None, rows=None):
        """y = [LN relu]( x @ W^T + b ); weight/bias/LN live inside ``w_pack`` at float offsets."""
        rows = x.shape[0] if rows is None else rows
        npad = _round_up(n, 32)
        if out is None:
            out = torch.empty(rows, n, device=self.device, dtype=torch.float32)
        base = w_pack.data_ptr()
        bias = base + 4 * bias_off if bias_off is not None else None
        pg = base + 4 * post_ln_off if post_ln_off is not None else None
        pb = base + 4 * (post_ln_off + 128) if post_ln_off is not None else None
        prg, prb = (pre_ln if pre_ln is not None else (None, None))
        _lib.check(self.lib.infgen_linear(_lib.ptr(x), ldx or x.stride(0), _lib.ptr(gather), rows, k,
                                          base + 4 * w_off, npad, bias, n, prg, prb, pg, pb, int(relu),
                                          _lib.ptr(out), out.stride(0), self.stream), 'infgen_linear')
        return out

    def map_token_head(self, x, rows, pack, token_size=1024):
        """the map encoder's token_predict_head on rows ``rows`` (int32, device) of ``x`` [..][128] (map_decoder.py:119-121) ->
        logits [n][token_size], the indices of the 10 largest [n][10] (int64, descending)"""
        n = int(rows.numel())
        logits = torch.empty(n, token_size, device=self.device)
        top = torch.empty(n, 10, device=self.device, dtype=torch.long)
        if n:
            # the fp32 path's scratch only where that path runs (the entry's rule: split kernel under gemm_terms 1 / 2, with
            # attn_mode 1, or from 10,241 rows under the by-size modes)
            o = _lib.Options()
            _lib.check(self.lib.infgen_get_effective_options(C.byref(o)), 'infgen_get_effective_options')
            split = o.gemm_terms != 3 or o.attn_mode == 1 or (o.attn_mode >= 2 and n > 10240)
            hidden = None if split else torch.empty(n, D, device=self.device)
            _lib.check(self.lib.infgen_map_token_head(_lib.ptr(x), x.stride(0), _lib.ptr(rows), n, _lib.ptr(pack), int(token_size),
                                                      _lib.ptr(hidden), _lib.ptr(logits), _lib.ptr(top), self.stream),
                       'infgen_map_token_head')
        return logits, top

    def mlp_embedding(self, x, pack, k0, out=None):
        """MLPEmbedding.forward (reference infgen/modules/layers.py:180-192)"""
        k0p, o1, o2, o3 = packing.mlp_embedding_offsets(k0)
        h = self.linear(x, pack, o1, 128, k0, bias_off=o1 + k0p * 128, post_ln_off=o1 + k0p * 128 + 128, relu=True)
        h = self.linear(h, pack, o2, 128, 128, bias_off=o2 + 16384, post_ln_off=o2 + 16384 + 128, relu=True)
        return self.linear(h, pack, o3, 128, 128, bias_off=o3 + 16384, out=out)

    def mlp_layer(self, x, pack, k0, n_out, out=None):
        """MLPLayer.forward (reference infgen/modules/layers.py:214): pack = packing.pack_mlp_layer"""
        k0p = _round_up(k0, 8)
        o_b0 = k0p * 128
        h = self.linear(x, pack, 0, 128, k0, bias_off=o_b0, post_ln_off=o_b0 + 128, relu=True)
        o_w3 = o_b0 + 3 * 128
        return self.linear(h, pack, o_w3, n_out, 128, bias_off=o_w3 + 128 * _round_up(n_out, 32), out=out)

    def mlp_layers(self, x, packs_nout):
        """several MLPLayers (``mlp_layer``) on the same input in two launches: all first Linears (+ LayerNorm, ReLU), then
        all output Linears.  packs_nout: [(pack, n_out), ...] -> list of outputs"""
        rows, n = x.shape[0], len(packs_nout)
        hid = torch.empty(n, rows, 128, device=self.device, dtype=torch.float32)
        outs = [torch.empty(rows, no, device=self.device, dtype=torch.float32) for _, no in packs_nout]
        d1, d2 = (_lib.LinearDesc * n)(), (_lib.LinearDesc * n)()
        o_b0, o_w3 = 128 * 128, 128 * 128 + 3 * 128
        for i, (pack, no) in enumerate(packs_nout):
            base = pack.data_ptr()
            a = d1[i]
            a.X, a.ldx, a.gather, a.rows, a.K = x.data_ptr(), x.stride(0), None, rows, 128
            a.Wp, a.Np, a.bias, a.N = base, 128, base + 4 * o_b0, 128
            a.pre_g = a.pre_b = None
            a.post_g, a.post_b, a.relu = base + 4 * (o_b0 + 128), base + 4 * (o_b0 + 256), 1
            a.Y, a.ldy = hid[i].data_ptr(), 128
            b = d2[i]
            npad = _round_up(no, 32)
            b.X, b.ldx, b.gather, b.rows, b.K = hid[i].data_ptr(), 128, None, rows, 128
            b.Wp, b.Np, b.bias, b.N = base + 4 * o_w3, npad, base + 4 * (o_w3 + 128 * npad), no
            b.pre_g = b.pre_b = b.post_g = b.post_b = None
            b.relu = 0
            b.Y, b.ldy = outs[i].data_ptr(), outs[i].stride(0)
        _lib.check(self.lib.infgen_linear_multi(d1, n, self.stream), 'infgen_linear_multi')
        _lib.check(self.lib.infgen_linear_multi(d2, n, self.stream), 'infgen_linear_multi')
        return outs

    def fourier(self, raw, n, pack, out, count_dev=None, rows=None, cat=None, normalize=False):
        rows = raw.shape[0] if rows is None else rows
        _lib.check(self.lib.infgen_fourier_embed(_lib.ptr(raw), n, _lib.ptr(count_dev), rows, _lib.ptr(pack),
                                                 _lib.ptr(cat), cat.stride(0) if cat is not None else 0,
                                                 out.data_ptr(), out.stride(0), int(normalize), self.stream),
                   'infgen_fourier_embed')
        return out

    def attn_pre(self, x, pack, use_src_ln=False, q=None, u=None, k=None, v=None, rows=None):
        rows = x.shape[0] if rows is None else rows
        _lib.check(self.lib.infgen_attn_pre(_lib.ptr(x), rows, _lib.ptr(pack), int(use_src_ln), _lib.ptr(q),
                                            _lib.ptr(u), _lib.ptr(k), _lib.ptr(v), self.stream), 'infgen_attn_pre')

    def edge_attn(self, rows, q, u, ksrc, vsrc, off, cnt, src, rhat, agg, z, sig, wide=None):
        args = (rows, _lib.ptr(q), _lib.ptr(u), _lib.ptr(ksrc), _lib.ptr(vsrc), _lib.ptr(off), _lib.ptr(cnt),
                _lib.ptr(src), _lib.ptr(rhat), _lib.ptr(agg), _lib.ptr(z), _lib.ptr(sig))
        if wide == 'fused':         # u is the layer pack: U / Z / SIG stay on chip, agg already holds the positional part
            _lib.check(self.lib.infgen_edge_attn_fused(rows, _lib.ptr(q), _lib.ptr(u), *args[3:10], self.stream),
                       'infgen_edge_attn_fused')
        elif wide is None:
            _lib.check(self.lib.infgen_edge_attn(*args, self.stream), 'infgen_edge_attn')
        else:
            _lib.check(self.lib.infgen_edge_attn_mode(*args, int(wide), self.stream), 'infgen_edge_attn_mode')

    def attn_post(self, x, pack, agg, z, sig, has_pos=True, rows=None):
        rows = x.shape[0] if rows is None else rows
        _lib.check(self.lib.infgen_attn_post(_lib.ptr(x), rows, _lib.ptr(pack), _lib.ptr(agg), _lib.ptr(z),
                                             _lib.ptr(sig), int(has_pos), self.stream), 'infgen_attn_post')

    def attn_post_pre(self, x, pack, agg, z, sig, next_pack, has_pos=True, q=None, u=None, k=None, v=None):
        """the post part of one layer and the pre part (q / absorbed query / K / V) of the next in one launch"""
        _lib.check(self.lib.infgen_attn_post_pre(_lib.ptr(x), x.shape[0], _lib.ptr(pack), _lib.ptr(agg), _lib.ptr(z),
                                                 _lib.ptr(sig), int(has_pos), _lib.ptr(next_pack), _lib.ptr(q), _lib.ptr(u),
                                                 _lib.ptr(k), _lib.ptr(v), self.stream), 'infgen_attn_post_pre')

    def attention_layer(self, x, pack, off, cnt, src, rhat, x_src=None, scratch=None, wide=None):
        """AttentionLayer.forward (layers.py:61-76) on CSR edges; in place on ``x``."""
        rows = x.shape[0]
        dev = self.device
        sc = scratch if scratch is not None else {}
        q = sc.get('Q', torch.empty(rows, D, device=dev))
        u = sc.get('U', torch.empty(rows, 8 * D, device=dev))
        agg = sc.get('AGG', torch.empty(rows, D, device=dev))
        z = sc.get('Z', torch.empty(rows, 8 * D, device=dev))
        sig = sc.get('SIG', torch.empty(rows, 8, device=dev))
        fused = wide == 'fused'
        if x_src is None:
            k = torch.empty(rows, D, device=dev)
            v = torch.empty(rows, D, device=dev)
            self.attn_pre(x, pack, q=q, u=None if fused else u, k=k, v=v)
        else:
            k = torch.empty(x_src.shape[0], D, device=dev)
            v = torch.empty(x_src.shape[0], D, device=dev)
            self.attn_pre(x_src, pack, use_src_ln=True, k=k, v=v)
            self.attn_pre(x, pack, q=q, u=None if fused else u)
        self.edge_attn(rows, q, pack if fused else u, k, v, off, cnt, src, rhat, agg, z, sig, wide=wide)
        self.attn_post(x, pack, agg, z, sig, has_pos=rhat is not None and not fused)
        return x


def _edge_index(data):
    try:
        return data[('pt_token', 'to', 'map_polygon')]['edge_index']
    except (KeyError, TypeError):
        return data['pt_token__to__map_polygon']['edge_index']


def read_batch_layout(data, T: int, hc: int, max_rows: int, extra: Sequence[torch.Tensor] = ()) -> Dict:
    """the offsets of a ragged PyG-style ``Batch`` (rows of every graph concatenated, ``agent.ptr`` / ``pt_token.ptr`` [B + 1],
    ``agent.av_index`` [B] as GLOBAL rows, i.e. ``av_index + ptr[:-1]``) with ONE device -> host copy: the two ``ptr`` and
    ``av_index`` concatenated (plus the raw bytes of the ``extra`` device tensors, returned as host arrays of their dtype and
    shape).  Raises ValueError on a malformed batch - before anything is launched."""
    ag, pt = data['agent'], data['pt_token']
    if 'ptr' not in ag or 'ptr' not in pt:
        raise ValueError('a Batch needs agent.ptr and pt_token.ptr')
    aptr, mptr = torch.as_tensor(ag['ptr']), torch.as_tensor(pt['ptr'])
    av = torch.as_tensor(ag['av_index']).reshape(-1)
    B = int(aptr.numel()) - 1
    if B < 1 or int(mptr.numel()) != B + 1 or int(av.numel()) != B:
        raise ValueError(f'agent.ptr {tuple(aptr.shape)}, pt_token.ptr {tuple(mptr.shape)} and av_index {tuple(av.shape)} '
                         'do not describe one batch of B graphs ([B + 1], [B + 1], [B])')
    dev = aptr.device
    parts = [aptr.to(dev, torch.int64), mptr.to(dev, torch.int64), av.to(dev, torch.int64)]
    ex = [e for e in extra if isinstance(e, torch.Tensor) and e.device == dev]
    flat = [p_.contiguous().view(torch.uint8) for p_ in parts] + [e.detach().contiguous().reshape(-1).view(torch.uint8) for e in ex]
    host = torch.cat(flat).cpu().numpy() if len(flat) > 1 else flat[0].cpu().numpy()
    head = host[:(3 * B + 2) * 8].view(np.int64)
    a, m, v = head[:B + 1], head[B + 1:2 * B + 2], head[2 * B + 2:]
    extra_host, o = [], (3 * B + 2) * 8
    for e in extra:
        if isinstance(e, torch.Tensor) and e.device == dev:
            nb = e.numel() * e.element_size()
            extra_host.append(host[o:o + nb].view(_lib_np_dtype(e.dtype)).reshape(tuple(e.shape)))
            o += nb
        else:
            extra_host.append(e.detach().cpu().numpy() if isinstance(e, torch.Tensor) else np.asarray(e))
    A, M = np.diff(a), np.diff(m)
    if a[0] != 0 or m[0] != 0 or (A < 0).any() or (M < 0).any():
        raise ValueError('agent.ptr / pt_token.ptr must start at 0 and be non-decreasing')
    st = ag['state_idx']
    if int(st.shape[0]) != int(a[-1]) or int(pt['position'].shape[0]) != int(m[-1]):
        raise ValueError(f'ptr ends ({int(a[-1])} agents, {int(m[-1])} map tokens) do not match the arrays '
                         f'({int(st.shape[0])}, {int(pt["position"].shape[0])})')
    if int(_edge_index(data).shape[1]) != int(m[-1]):
        raise ValueError('pt_token -> map_polygon edge_index must hold one edge per map token')
    T0 = int(st.shape[1])
    if not hc <= T0 <= T:
        raise ValueError(f'token columns {T0} outside [{hc}, {T}]')
    if int(A.max()) > max_rows:
        raise ValueError(f'a graph holds {int(A.max())} agents, more than the {max_rows} rows a scene can have')
    if (A < 1).any():
        raise ValueError('every graph needs at least one agent (its ego)')
    if not ((v >= a[:-1]) & (v < a[1:])).all():
        bad = int(np.nonzero(~((v >= a[:-1]) & (v < a[1:])))[0][0])
        raise ValueError(f'av_index[{bad}] = {int(v[bad])} lies outside graph {bad} (rows {int(a[bad])} .. {int(a[bad + 1]) - 1}); '
                         'a Batch carries global ego rows (av_index + ptr[:-1])')
    return dict(B=B, agent_ptr=a.copy(), pt_ptr=m.copy(), av=v.copy(), A=A, M=M, amax=int(A.max()), mmax=int(max(M.max(), 1)),
                T0=T0, P=int(ag['position'].shape[1]), device=dev, extra=extra_host)


def pack_rows(srcs: Sequence[torch.Tensor], counts: Sequence[torch.Tensor], totals: Sequence[int], n_scenes: int,
              scene0: int = 0, scene_step: int = 1) -> List[torch.Tensor]:
    """infgen_pack_rows: per key k, the first counts[k][s] rows of every scene s = scene0 + i scene_step (i < n_scenes) of
    srcs[k] ([scenes][rows][...], contiguous, on one device) concatenated into a new [totals[k]][...] tensor.  counts[k]: an
    int32 device vector or a column of an int32 matrix (its stride is used); totals[k] must be the sum of those counts."""
    n = len(srcs)
    dev = srcs[0].device
    for t_, c_ in zip(srcs, counts):
        if not (t_.is_contiguous() and c_.dtype == torch.int32 and t_.device == c_.device == dev and t_.dim() >= 2):
            raise ValueError('pack_rows takes contiguous [scenes][rows][...] sources and int32 counts on one device')
    outs = [torch.empty((int(tot),) + tuple(t_.shape[2:]), dtype=t_.dtype, device=dev) for t_, tot in zip(srcs, totals)]
    P_ = C.c_void_p * n
    src = P_(*[t_.data_ptr() for t_ in srcs])
    dst = P_(*[o.data_ptr() if o.numel() else t_.data_ptr() for o, t_ in zip(outs, srcs)])     # (an empty output gets no row)
    stride = (C.c_longlong * n)(*[t_.stride(0) * t_.element_size() for t_ in srcs])
    rb = (C.c_int * n)(*[int(np.prod(t_.shape[2:], dtype=np.int64)) * t_.element_size() for t_ in srcs])
    cnt = P_(*[c_.data_ptr() for c_ in counts])
    cst = (C.c_int * n)(*[c_.stride(0) for c_ in counts])
    lib = _lib.load()
    _lib.check(lib.infgen_pack_rows(n, src, stride, rb, cnt, cst, dst, n_scenes, scene0, scene_step,
                                    torch.cuda.current_stream(dev).cuda_stream), 'infgen_pack_rows')
    return outs


def _lib_np_dtype(dt):
    return {torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32, torch.uint8: np.uint8,
            torch.bool: np.bool_, torch.float64: np.float64}[dt]


_FLT_MIN = float(np.finfo(np.float32).tiny)      # the smallest normal float32: below it 1 / T overflows

# The step riders in the order the engine resolves them.  ``name``: the keyword, and the engine attribute that holds the
# checked configuration while the rider is on; ``buffers`` / ``reg``: the attributes of its buffer dict and of what the handle has
# registered; ``check(engine, value)`` / ``key(conf)``: the constraints.py check and the part of its result that decides launches;
# ``entry`` / ``off``: the library's attach entry and the arguments that detach; ``public``: the buffer attributes the engine exposes.
_Rider = namedtuple('_Rider', 'name buffers reg check key entry off public')
RIDERS = (
    _Rider('avoid_collisions', '_coll', '_coll_reg',
           lambda e, v: constraints.check_avoid_collisions(v, has_shape=e._has_shape), constraints.collision_key,
           'infgen_token_mask_collision', (None, None, None, None, 1, 0.0, None), ('collision_bits', 'collision_allowed')),
    _Rider('stay_on_road', '_road', '_road_reg',
           lambda e, v: constraints.check_stay_on_road(v, has_shape=e._has_shape, n_scenes=e.S0), constraints.road_key,
           'infgen_token_mask_road', (None, None, None, None, None, None, None, 0, 1, 1, 0.0, None, None), ('road_bits', 'road_allowed')),
    _Rider('step_scores', None, '_score_reg',
           lambda e, v: constraints.check_step_scores(v, has_shape=e._has_shape, n_scenes=e.S0, stay_on_road=e.stay_on_road),
           constraints.score_key, 'infgen_token_mask_score', (None, 0, None, None, None, None, 0, 1, 1, 0.0, None, 0.5),
           ('step_score', 'score_row')),
    _Rider('follow_routes', '_route', '_route_reg',
           lambda e, v: constraints.check_follow_routes(v, n_scenes=e.S0, a_cap=e.A_cap), constraints.route_key,
           'infgen_token_mask_route', (None, None, None, None, None, None, 2, 1, 0.0, 0.0, 0.0, 0.0, None, None, None),
           ('route_bits', 'route_allowed', 'route_progress')),
    _Rider('obey_signals', '_signal', '_signal_reg',
           lambda e, v: constraints.check_obey_signals(v, has_shape=e._has_shape, n_scenes=e.S0), constraints.signal_key,
           'infgen_token_mask_signal', (None, None, None, None, None, None, 1, 1, 1, 0.0, 0.0, None, None, None),
           ('signal_bits', 'signal_allowed', 'signal_info')))
_SCORES = RIDERS[2]
STEP_KEYWORDS = ('token_masks', 'token_mask_type', 'token_mask_row') + tuple(r.name for r in RIDERS)


def _step_keywords(args: Mapping) -> Dict:
    """what rides on the decode step, out of the ``locals()`` of the constructor or a reload entry: gathered once per entry"""
    return {k: args[k] for k in STEP_KEYWORDS}


class RolloutEngine:
    """Device state + launch sequence for a batch of scenes."""
    copies = 1          # rollouts per scene over one map encoding (instance attribute when given; see __init__)

    def __init__(self, weights: PackedWeights, scenes: Sequence[Mapping], vocab: Mapping[str, np.ndarray],
                 map_vocab: np.ndarray, grid: np.ndarray, a_cap: Optional[int] = None, m_cap: Optional[int] = None,
                 store_logits: bool = False, live_state: bool = False,
                 teacher: Optional[Sequence] = None, x_pt_override: Optional[Sequence] = None,
                 force_enter: bool = False, insert_headroom: Optional[int] = None,
                 sample_k: int = 1, sample_uniforms: Optional[np.ndarray] = None, options: Optional[Mapping[str, int]] = None,
                 insert_k: int = 1, insert_uniforms: Optional[np.ndarray] = None, seed_outputs: bool = False,
                 use_graph: Optional[bool] = None, copies: int = 1, flags: Optional[Mapping[str, bool]] = None,
                 tap_layers: bool = False, batch=None, batch_layout: Optional[Dict] = None, replay=None,
                 token_logprob: bool = False, sample_logprob: bool = False,
                 sample_temperature=1.0, sample_top_p: float = 1.0, insert_temperature: float = 1.0, insert_top_p: float = 1.0,
                 token_masks=None, token_mask_type=None, token_mask_row=None, avoid_collisions=False, stay_on_road=False,
                 step_scores=False, follow_routes=False, insert_rules=None, obey_signals=False):
        """``insert_rules``: insertion rules ("INSERTION RULES" of include/infgen_hip.h) - None or dict(clearance=,
        ego_keepout=(back, front, half_width), edge_clearance=, near_lane=dict(dist=, types=), zones=, types=, max_agents=,
        per_step=): a cell mask computed on the device in front of every insertion decision (``infgen_amd.insertion_rules``).
        ``insert_allowed`` [S, W] holds the bits of the last iteration, ``insert_allowed_count`` [S, steps] the iteration-0 count of
        every step; ``set_insert_zones`` rewrites the zone table.  Engines without scenario insertion or without the grid token
        refuse it.
        ``batch``: a ragged PyG-style Batch of device tensors instead of host ``scenes`` (pass ``scenes=None``): the engine
        is sized from its offsets (``read_batch_layout``; A_cap from the unfiltered per-graph maxima, which the filtered counts
        never exceed) and set up on the device by the ingest kernel (``reload_batch``).
        ``replay``: log replay - the flagged rows follow a plan (their logged future, or a planner's), every other row is
        generated around them.  Host scenes: one entry per scene, None, a bool mask over the scene's rows (the plan is the
        scene's own token_idx / state_idx / token_pos / token_heading from column hist_columns on) or (mask, tokens, states[,
        pos, head]) with (A, T) / (A, T, 2) arrays.  A Batch: a bool mask over its N concatenated rows on the device, or (mask,
        dict of token_idx / state_idx[, token_pos, token_heading] [N][T0]).  Flags refer to initial rows (rows scenario insertion
        appends are always generated); a flagged row's logged enter / exit / invalid states are forced like ``teacher``'s.
        ``reload`` / ``reload_device`` / ``reload_batch`` take a new mask and plan.  ``teacher`` (all rows, test hook) excludes it.
        ``token_logprob``: every decode step also records the full-softmax log-probability of the motion token each row emitted
        (``next_token_logprob`` / ``next_token_logprob_mask`` of the outputs; infgen_amd/logprob.py).  Large greedy batches compute
        it inside the heads kernel; small or sampled ones read the step's logits (a [rows][token_size] scratch is allocated when
        neither ``store_logits`` nor sampling keeps them).
        ``sample_logprob``: every decode step also records the log-probability of the sampled motion token under the sampler's OWN
        distribution, the softmax re-normalised over the ``sample_k`` best logits (``next_token_sample_logprob``, masked by
        ``next_token_logprob_mask``; ``rollout_sample_logprob()``).  Independent of ``token_logprob``; 0 where masked when
        ``sample_k <= 1`` (a point mass).  Sampled rollouts whose every step samples inside the heads kernel
        (``infgen_heads_sample_fused``) keep no logits in memory: ``logits_scratch`` is None.
        ``sample_temperature`` / ``sample_top_p``: temperature and nucleus (top-p) truncation of the motion-token draw (DESIGN 5.10;
        read where ``sample_k > 1``): the softmax over the ``sample_k`` best logits at temperature T, cut to the smallest prefix that
        holds ``sample_top_p`` of its mass.  ``sample_temperature`` is a float, an array [S] (one entry per agent-side scene: with
        ``copies = n`` one per copy - a batch of copies is a temperature sweep) or [S][rows]; 0 makes those rows greedy - also as a
        float, which then means every row (unlike the C struct's scalar, where 0 reads "unset")
        (``next_token_sample_logprob`` 0 there).  Arrays live in one static device buffer that ``reload*(sample_temperature=...)``
        rewrites, so captured graphs replay the new values; rows scenario insertion appends take their scene's value.
        ``next_token_logprob`` stays the model's own full softmax at temperature 1.  ``insert_temperature`` / ``insert_top_p``: the
        same for the cell draw of scenario insertion (scalars; ``insert_k > 1``; a temperature of 0 is refused: the arg-max cell is
        ``insert_k = 1``).  ``reload*(sample_top_p=...)`` changes the nucleus mass of an engine that exists.  The defaults are the plain samplers bit for bit.
        ``step_scores``: step scores ("step scores" of include/infgen_hip.h) - False, True or ``dict(road_margin=,
        sweep=, types=, detail=, segments=, dt=)``.  Every decode step then also reduces the column it produced per scene slot:
        ``step_score`` [S, steps, 8] = n_live, n_overlap, min_sep, n_offroad, max_accel, max_yaw_rate, 0, 0 of step t at [:, t], and
        ``score_row`` [S, A_cap] uint8 (bit 0 live, 1 overlap, 2 off-road) of the newest step - static device buffers, what
        ``branching.score_log_weight`` and ``rollout_guided`` read.  The record table is the engine's one road table: shared with
        ``stay_on_road`` when that is on (a different ``detail`` / ``segments`` raises ValueError), otherwise built the same way.
        Tokens, poses and logits are those of the engine without it.  ``reload*(step_scores=...)`` turns it on or off (None:
        keep).  Engines with scenario insertion refuse it.

        ``token_masks`` / ``token_mask_type`` / ``token_mask_row``: constrained decoding (infgen_amd/constraints.py).
        ``token_masks`` is a ``TokenMasks`` table of allowed-token sets; a generated row takes the set ``token_mask_row`` names
        ([S][rows] host integers, range-checked here, or an int32 device tensor [S][A_cap] taken as it is; -1 = no choice of its own)
        and otherwise the set of its type, ``token_mask_type`` (three set indices, -1 = unconstrained; default: the table's own
        per-type selection, ``TokenMasks.type_sets``).  Rows scenario insertion appends follow their type.  Replayed, commanded and
        teacher-forced rows, the state head and the insertion cell draw are left alone; logits and ``next_token_logprob`` stay the
        model's own.  Table and per-row selectors live in static device buffers that ``reload*(token_masks=..., token_mask_row=...)``
        rewrite, so captured graphs replay the new values.  None (the default): today's kernels, bit for bit.
        ``avoid_collisions``: collision-aware decoding ("collision masks" of include/infgen_hip.h) - False, True or
        ``dict(margin=metres, predict=0 | 1)``.  Every decode step first computes, from the agents' boxes, which motion tokens would
        end the step inside another agent's (constant-velocity extrapolated, ``predict``) box and bans them on top of the row's static
        set (all tokens without ``token_masks``); a row whose every token collides keeps its static set.  ``collision_bits``
        [S * A_cap][token_size / 32] and ``collision_allowed`` [S * A_cap] (the sets' sizes before that fallback) are static device
        buffers that hold the sets of the step that just ran.  ``reload*(avoid_collisions=...)`` turns it on or off (None: keep).
        ``follow_routes``: route-following decoding ("route masks" of include/infgen_hip.h) - False or
        ``dict(routes=, n_points=, corridor=2.0, back=0.5, pace=0.0, finish=1.0, types=('veh', 'cyc'))``: ``routes`` [S0][A][P][2]
        world-coordinate waypoints per distinct scene and initial row (2 <= P <= 32, A <= A_cap), ``n_points`` [S0][A].  Every
        decode step bans, for the generated rows of those types that have a route and have not finished it, the motion tokens
        whose end box's centre leaves the corridor around the route (unless it ends nearer to it than the row is), falls more
        than ``back`` metres behind the row's arc position or - ``pace`` > 0 - gains less than ``pace`` times the best gain; on top
        of the static, collision or road set, and a row with no token left keeps that set.  ``route_bits`` / ``route_allowed`` /
        ``route_progress`` ([rows, 4] = s0, d0, total, flag) are static device buffers of the step that just ran;
        ``set_routes(routes, n_points)`` replaces the routes between two steps.  ``reload*(follow_routes=...)`` turns it on or
        off (None: keep).  Rows scenario insertion appends have no route.
        ``obey_signals``: signal-aware decoding ("signal masks" of include/infgen_hip.h) - False or
        ``dict(lines=, n_lines=, phase=, setback=0.5, align=0.5, types=('veh', 'cyc'))``: ``lines`` [S0][K][4] = (ax, ay, bx, by)
        world-coordinate stop lines per distinct scene (K <= 64; a the left, b the right end as the stopped traffic sees them),
        ``n_lines`` [S0] (default: all K), ``phase`` [S0][n_phase][K] bytes, non-zero = closed at the decode steps t with
        t mod n_phase == that row (``constraints.signal_phase`` / ``stop_lines_from_map`` make them).  Every decode step bans,
        for the generated rows of those types, the motion tokens that carry the row's front bumper across a closed line it faces
        and has not passed; on top of the static, collision or road set and underneath the route set, and a row with no token
        left keeps the set it had.  ``signal_bits`` / ``signal_allowed`` / ``signal_info`` ([rows, 4] = gap, line, flag, 0) are
        static device buffers of the step that just ran; ``set_signals(phase=, lines=, n_lines=)`` rewrites the tables between two
        steps.  ``reload*(obey_signals=...)`` turns it on or off (None: keep).  A signal's state is a function of the step and the
        map scene alone, so branching and snapshots copy nothing for it: a branched or restored slot sees the phase row of its
        step.  Engines with scenario insertion are allowed: appended rows keep their base in the step that appends them and are
        ruled from the next.
        ``stay_on_road``: road-aware decoding ("road masks" of include/infgen_hip.h) - False, True or
        ``dict(margin=metres, sweep=0 | 1, detail=1 | 2 | 5 | 10, types=('veh', 'cyc'), segments=None)``.  Every decode step bans the
        motion tokens whose end box or (``sweep``) path rectangle overlaps a road-edge segment the row does not already straddle, on
        top of the static set - or of the collision set with ``avoid_collisions`` -; a row with no token left keeps that set.  The
        segments are ``detail`` chords of every EDGE (type 12) map token's polyline, or the explicit world-coordinate ``segments``
        ([S0][E][4] or one [E][4] array per distinct scene: the data set's real road edges).  ``road_bits`` / ``road_allowed`` (per
        row, like the collision pair) and ``road_records`` [S0][capacity][8] / ``road_n_records`` [S0] are static device buffers;
        the records are rebuilt after every reload.  ``reload*(stay_on_road=...)`` turns it on or off (None: keep; explicit segments
        belong to the scenes they came with - pass new ones with new scenes)."""
        self.w = weights
        self.options = dict(options) if options else None      # per-engine kernel switches (fields of InfgenOptions)
        # per-engine launch-sequence switches (none changes what is computed beyond fp32 summation order): read from the environment
        # ONCE, here, as defaults (diagnostic A/B runs), overridden by ``flags`` - two engines of one process may differ
        env = os.environ.get
        self.flags = dict(dt_table=env('INFGEN_NO_DT_TAB', '0') != '1',        # the temporal edges' time-gap branch as a lookup
                          map_fuse=env('INFGEN_MAP_FUSE', '1') != '0',        # map encoder's edge side through k_edge_fused
                          row_groups=env('INFGEN_ROW_GROUPS', '1') != '0',    # insertion: visit only the 16-row groups that hold agents
                          row_groups_tight=env('INFGEN_ROW_GROUPS_TIGHT', '1') != '0',
                          graph=env('INFGEN_GRAPH', '0'))                     # '1': replay decode steps from a HIP graph, '2': whole rollout
        self.flags.update(flags or {})
        # test hook (InfgenRollout.tap_x): the residual stream after every (temporal, map, agent) triple of the last decode step
        self._tap_layers = bool(tap_layers)
        self.tap_x = None
        self.cfg = cfg = weights.cfg
        self.device = dev = weights.device
        self.ops = Ops(dev)
        self.lib = self.ops.lib
        # copies = n: every scene is decoded n times in lockstep (the reference's n_rollout_close_val loop, infgen/model/infgen.py:
        # 704-706, whose inference_no_map(data, map_enc), infgen_decoder.py:132-134, exists so that the map is encoded once): the
        # batch has S = len(scenes) * n agent-side scenes (scene i's copies are rows i n .. i n + n - 1: own state, own uniforms)
        # over S0 = len(scenes) map-side scenes - ONE map-token graph, map encoding and set of map K / V rows per scene, found
        # through InfgenRollout.map_scene
        self.copies = int(copies)
        assert self.copies >= 1
        self.scenes = scenes
        self._batch_lay = None
        self._bc_host = None
        if batch is not None:
            assert scenes is None and teacher is None and x_pt_override is None, 'a Batch engine takes no host scenes / teacher'
            batch_layout = batch_layout or read_batch_layout(batch, cfg.num_columns, cfg.hist_columns,
                                                             self.lib.infgen_layout_query(_lib.Q_MAX_AGENTS))
            self._batch_lay = batch_layout
        self.S0 = len(scenes) if batch is None else batch_layout['B']
        self.S = S = self.S0 * self.copies
        self.T = T = cfg.num_columns
        self.R = R = cfg.num_recurrent_steps_val
        self.hc = hc = cfg.hist_columns
        assert hc == 2, 'the kernels assume num_historical_steps=11, shift=5'
        self.W = cfg.window
        self.ring = self.W + 1
        self.store_logits = store_logits
        self.sample_k = int(sample_k)
        self._sample_uniforms = sample_uniforms      # [steps][S][A] float32 in [0,1) (top-k inverse-CDF sampling)
        self.sample_top_p = self._check_top_p(sample_top_p, 'sample_top_p')
        self.insert_temperature = self._check_temperature(insert_temperature, 'insert_temperature')
        self.insert_top_p = self._check_top_p(insert_top_p, 'insert_top_p')
        self.sample_temperature, self.sample_temp_row = 1.0, None     # (set below, once the row layout is known)
        # scenario insertion: the cell of a new agent from the insert_k most probable ones (reference insert_beam_size = 10,
        # agent_decoder.py:1900-1904) with insert_uniforms [steps][10][S]; 1: arg-max
        # (use_grid_token = False: no cell is drawn - the position is regressed - and insert_k is accepted and ignored, as in the reference)
        self.insert_k = int(insert_k) if cfg.use_grid_token else 1
        self._insert_u = None
        # record the seed node's per-insertion outputs of the reference's return dict (agent_decoder.py:2099-2113, :2364-2386:
        # next_state_prob_seed, next_pos_rel_prob_seed, grid_*_occ_seed - plot inputs of the reference; two more heads per iteration)
        self.seed_outputs = bool(seed_outputs)
        self.seed_out = None
        # capture the decode steps of a rollout (no insertion: ~47 launches per step, all shapes static) in a HIP graph at the
        # first run and replay it afterwards
        # use_graph = 'all': the WHOLE rollout (reset, map encoder, column-0 chain, every decode step) as one graph, replayed on a
        # stream of the engine's own - what lets one host thread keep several engines on several streams busy (rollout_many): a
        # rollout is ~1,000 launches, and issuing four engines' launches one after the other takes longer than the GPU needs
        self._graph_all = use_graph == 'all' or (use_graph is None and str(self.flags['graph']) == '2')
        if self._graph_all:
            use_graph = False
        self._wgraph = None
        self._wgraph_opts = None
        self._use_graph_arg = use_graph              # None: by size (set below, once the row count is known)
        self.use_graph = bool(use_graph)
        self._graph = None
        self._graph_opts = None
        if self.insert_k > 1:
            assert insert_uniforms is not None, 'cell sampling needs caller-supplied uniforms [steps][10][S]'
            self._insert_u = torch.from_numpy(np.ascontiguousarray(insert_uniforms, dtype=np.float32)).to(weights.device)
        self._x_pt_override = x_pt_override
        self.force_valid = bool(cfg.disable_insertion) and not live_state
        self.insertion = not cfg.disable_insertion
        self.force_enter = force_enter
        # insertion rules: checked here, the device tables are allocated with the insertion buffers
        self.insert_rules = insertion_rules.InsertRules.from_config(insert_rules, n_scenes=self.S0, n_slots=self.S)
        self._ins_rules, self._ins_map_dirty = None, True
        if self.insert_rules is not None and not self.insertion:
            raise ValueError('insert_rules: engines with disable_insertion insert nothing: there is no decision to rule')
        if self.insert_rules is not None and not cfg.use_grid_token:
            raise ValueError('insert_rules: a model with use_grid_token = False draws no cell (the position is regressed): there is '
                             'no cell to mask')

        # ------------------------------------------------ host-side scene setup
        self._hosts_light = False
        if batch is None:
            hosts, staged = self._setup_scenes(scenes)
            self.hosts = self._replicate(hosts)
            amax, mmax = int(staged['A'].max()), int(staged['M'].max())
        else:                                  # (the padded fill arrays below; the ingest kernel writes the scenes)
            self.hosts, staged = None, None
            amax, mmax = batch_layout['amax'], batch_layout['mmax']
        self._amax0 = amax
        head = 0
        if self.insertion:
            # rows kept free for inserted agents.  The full model's grid rejects occupied cells, so 96 rows have been plenty; without the
            # grid nothing is rejected and forced / eager seed heads append the maximum 10 rows at every step: room for all of them
            # (up to the layout's row limit - a scene that still runs out raises InsertionHeadroomError, nothing is dropped)
            default = min(10 * cfg.num_decode_steps, 96) if cfg.use_grid_token else 10 * cfg.num_decode_steps
            head = insert_headroom if insert_headroom is not None else default
        self.A_cap = A_cap = a_cap or min(_round_up(max(amax + head, 1), 32), self.lib.infgen_layout_query(_lib.Q_MAX_AGENTS))
        self.M_cap = M_cap = m_cap or _round_up(max(mmax, 1), 32)
        assert amax <= A_cap <= self.lib.infgen_layout_query(_lib.Q_MAX_AGENTS) and A_cap % 32 == 0
        assert mmax <= M_cap
        self.rows = rows = S * A_cap
        if self._use_graph_arg is None:
            # replaying the decode steps from a captured HIP graph: opt-in (use_graph=True or INFGEN_GRAPH=1).  Measured in round 3:
            # 64 scenes 25.9 ms with and without it (the step is its kernels' dependency chains, not launch overhead)
            self.use_graph = str(self.flags['graph']) == '1' and not self.insertion

        arr = self._scene_arrays(staged)
        t = lambda a: torch.from_numpy(a).to(dev)
        for k in self._SCENE_ARRAYS:
            setattr(self, k, t(arr[k]))
        self._map_cat = tuple(t(arr[k]) for k in ('map_tok', 'map_type', 'map_pl', 'map_light'))
        self.map_scene = (torch.arange(S, device=dev, dtype=torch.int32) // self.copies).contiguous() if self.copies > 1 else None
        vocab_np = np.stack([vocab[k] for k in ('veh', 'ped', 'cyc')]).astype(np.float32)
        map_vocab_np = np.asarray(map_vocab, dtype=np.float32).reshape(map_vocab.shape[0], -1)
        grid_np = np.asarray(grid, dtype=np.float32)
        # (the token ablations select the fusion input of the fused seed row: part of the tables' content)
        flags = (cfg.use_grid_token, cfg.use_head_token, cfg.use_state_token)
        extra = () if all(flags) else (np.asarray(flags, np.int8),)
        self._tables_key = PackedWeights.tables_key(vocab_np, grid_np, map_vocab_np, *extra)
        self.vocab, self._map_vocab, self.grid_xy = t(vocab_np), t(map_vocab_np), t(grid_np)
        self.G = int(grid.shape[0])
        self.teacher_token = self.teacher_state = None
        self.teacher_grid = self.teacher_pos = self.teacher_head = None
        if teacher is not None:
            tt = np.full((S, T, A_cap), -1, np.int32); ts = np.zeros((S, T, A_cap), np.int32)
            tg = np.full((S, T, A_cap), -2, np.int32)
            tp, th = None, None
            for s, tch in enumerate(teacher):
                tok_s, st_s = tch[0], tch[1]
                A = min(np.asarray(tok_s).shape[0], A_cap)        # rows beyond the initial agents: inserted ones (insertion on)
                tt[s, :, :A] = np.asarray(tok_s)[:A].T; ts[s, :, :A] = np.asarray(st_s)[:A].T
                if len(tch) > 2 and tch[2] is not None:           # optional third entry: grid cells (A, T) of the teacher state
                    tg[s, :, :A] = np.asarray(tch[2])[:A].T
                if len(tch) > 4 and tch[3] is not None:           # optional fourth / fifth: poses (A, T, 2) / (A, T) of the teacher state
                    if tp is None:
                        tp, th = np.zeros((S, T, A_cap, 2), np.float32), np.zeros((S, T, A_cap), np.float32)
                    tp[s, :, :A] = np.asarray(tch[3], np.float32)[:A].transpose(1, 0, 2); th[s, :, :A] = np.asarray(tch[4], np.float32)[:A].T
            self.teacher_token, self.teacher_state = t(tt), t(ts)
            if (tg > -2).any():
                self.teacher_grid = t(tg)
            if tp is not None:
                self.teacher_pos, self.teacher_head = t(tp), t(th)
        self.replay_row = None                 # [S][A_cap] uint8 once a replay was asked for (InfgenRollout.replay_row)
        self._session = None                   # the closed-loop session stepping this engine (``session()``; ``reset`` ends it)
        self._replay_pose = None               # the pose buffers of a replay engine (teacher_pos / teacher_head point at them or are None)
        if replay is not None and teacher is not None:
            raise ValueError('teacher= forces every row; replay= forces the flagged rows: give one of them')

        # ------------------------------------------------ scratch / caches
        f = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float32)
        i32 = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.int32)
        L = cfg.num_agent_layers
        self.X, self.Q, self.U = f(rows, D), f(rows, D), f(rows, 8 * D)
        if self._tap_layers:
            self.tap_x = f(cfg.num_agent_layers, rows, D)
        self.Ka, self.Va, self.AGG, self.Z, self.SIG = f(rows, D), f(rows, D), f(rows, D), f(rows, 8 * D), f(rows, 8)
        self.ringK = [f(self.ring, rows, D) for _ in range(L)]
        self.ringV = [f(self.ring, rows, D) for _ in range(L)]
        self.mapK = [f(self.S0 * M_cap, D) for _ in range(L)]
        self.mapV = [f(self.S0 * M_cap, D) for _ in range(L)]
        self.edges = {}
        totals = i32(3)        # the three edge totals back to back: infgen_build_edges clears them with one memset
        for k, (name, cap) in enumerate((('t', rows * self.W), ('m', rows * 5), ('a', rows * (A_cap - 1)))):
            cap = max(cap, 32)
            self.edges[name] = dict(off=i32(rows), cnt=i32(rows), src=i32(cap), raw=f(cap, 4), rhat=f(cap, D),
                                    total=totals[k:k + 1], cap=cap)
        self.raw2, self.cat, self.fus_in = f(rows, 4), f(rows, D), f(rows, 4 * D)
        self.tmp1, self.tmp2 = f(rows, D), f(rows, D)
        self.next_token, self.next_state = i32(rows), i32(rows)
        steps = cfg.num_decode_steps
        self.logits = f(steps, rows, cfg.token_size) if store_logits else None
        self.pred_traj, self.pred_head, self.pred_state = f(S, A_cap, R, 2), f(S, A_cap, R), f(S, A_cap, R)
        self.sample_u = self.logits_scratch = None
        if self.sample_k > 1:
            assert sample_uniforms is not None, 'top-k sampling needs caller-supplied uniforms'
            self.sample_u = torch.from_numpy(self._uniform_rows(sample_uniforms, amax)).to(dev)
        self._ctx = None
        self._load_temperature(sample_temperature, amax)
        self.token_masks, self.token_mask_type = None, [-1, -1, -1]
        self.mask_bits = self.mask_row = None             # static device buffers: [n_sets][token_size / 32] words, [S * A_cap] int32
        self._mask_handle = 0                             # infgen_token_mask_create's handle of (mask_bits, mask_row, token_mask_type)
        for r in RIDERS:      # per rider: the checked configuration while it is on, its buffers, what the handle has registered
            for attr in filter(None, (r.name, r.buffers, r.reg) + r.public):
                setattr(self, attr, None)
        self.road_records = self.road_n_records = self._road_paths = self._road_seg = None      # the engine's one road table
        self._road_cap, self._road_dirty = 0, False
        self._coll_end = self._score_arg = self._score_shape = None
        self._load_riders(_step_keywords(locals()))
        # (the sampler's logits scratch, where the context needs one, is allocated once the kernel switches are known: _refresh_opts)
        # [steps][rows] log-probability of the emitted token (InfgenRollout.token_logprob); its logits scratch, where the context
        # needs one, is allocated once the kernel switches are known (_refresh_opts)
        self.token_logprob = f(steps, rows) if token_logprob else None
        # [steps][rows] log-probability of the sampled token under the re-normalised top-k (InfgenRollout.sample_logprob)
        self.sample_logprob = f(steps, rows) if sample_logprob else None
        self._rollout_lp = self._rollout_slp = None
        # [1] int32: the entries of the last ``branch`` call's parent vector that broke the contract and were read as the identity
        self._branch_bad = torch.zeros(1, device=dev, dtype=torch.int32)      # (read through the ``branch_bad`` property)
        # snapshots: the same counters for ``snapshot`` (slots out of range) and ``restore`` (entries read as "keep"), this engine's
        # mark in a snapshot's layout signature, and the number of batches loaded so far (a reload outdates the snapshots before it)
        self.snapshot_bad = torch.zeros(1, device=dev, dtype=torch.int32)
        self.restore_bad = torch.zeros(1, device=dev, dtype=torch.int32)
        self._snap_token, self._reload_gen = object(), 0
        self.tok_tab = self.grid_tab = self.cat_agent = self.cat_seed = None
        self.x_pt = None
        self._ctx = None
        self._init = None
        self.ins = None
        self._mg = None
        self._mg_checked = False
        self._map_nbr_cap = 40          # compacted pt<->pt edges per map token (grown on overflow)
        self._prologue_done = False
        self._decoded_rows = torch.zeros((), device=dev, dtype=torch.int64)
        self._ing = None
        if batch is not None:
            self._ingest(batch, batch_layout, replay=replay)
        elif replay is not None:
            self._replay_from_hosts(replay)

    # ------------------------------------------------------------------ scene arrays (host -> device)
    _SCENE_ARRAYS = ('pos', 'head', 'state', 'token', 'gridtok', 'tmask', 'imask', 'catflag', 'atype', 'bos', 'n_agents', 'n_map',
                     'av', 'map_pos', 'map_orient', '_shape10')

    _MAP_SIDE = ('n_map', 'map_pos', 'map_orient', 'map_tok', 'map_type', 'map_pl', 'map_light')

    def _replicate(self, hosts0):
        """the per-scene host dicts of the agent-side batch: scene i's copies are adjacent (the dicts are shared, read-only)"""
        return hosts0 if self.copies == 1 else [h for h in hosts0 for _ in range(self.copies)]

    def _setup_scenes(self, scenes):
        """host scenes -> (the per-scene host dicts: A / M / av / filt and numpy views of the batch arrays cut to the scene's
        agents and map tokens; the batch arrays themselves, [S0, max A, T, ...] / [S0, max M, ...] / A, M, av [S0], the rows
        beyond a scene's count holding the padding values): ``scene_setup`` for all scenes at once"""
        ag, av, A, filts = scene_setup.stage_agents(scenes, self.cfg, self.cfg.num_columns)
        a = {k: v.numpy() for k, v in scene_setup.setup_agents(ag, av, self.cfg, self.cfg.num_columns, A).items()}
        m, M = scene_setup.stage_map(scenes)
        hosts = [dict({k: v[s, :A[s]] for k, v in a.items()}, **{k: v[s, :M[s]] for k, v in m.items()},
                      A=int(A[s]), M=int(M[s]), av=int(av[s]), filt=filts[s]) for s in range(len(scenes))]
        return hosts, dict(a, **m, A=A, M=M, av=av.numpy())

    def _setup_scene(self, scene) -> Dict[str, np.ndarray]:
        """the host dict of one scene (a batch of one through ``_setup_scenes``)"""
        return self._setup_scenes([scene])[0][0]

    def _scene_arrays(self, k) -> Dict[str, np.ndarray]:
        """the padded [S][T][A_cap] / [S0][M_cap] arrays of a batch (section 4 of DESIGN.md) from the batch arrays of
        ``_setup_scenes`` (None: the padding alone); with copies, every scene's agent side is repeated, its map side is not"""
        S, S0, T, A_cap, M_cap = self.S, self.S // self.copies, self.T, self.A_cap, self.M_cap

        def zeros(shape, dtype):
            return np.zeros(shape, dtype=dtype)
        a = dict(pos=zeros((S, T, A_cap, 2), np.float32), head=zeros((S, T, A_cap), np.float32),
                 state=zeros((S, T, A_cap), np.int32), token=np.full((S, T, A_cap), -1, np.int32),
                 gridtok=np.full((S, T, A_cap), -1, np.int32), tmask=zeros((S, T, A_cap), np.uint8),
                 imask=zeros((S, T, A_cap), np.uint8), catflag=zeros((S, T, A_cap), np.uint8),
                 atype=zeros((S, A_cap), np.int32), bos=zeros((S, A_cap), np.int32),
                 _shape10=np.full((S, A_cap, 3), INVALID_SHAPE, np.float32),
                 n_agents=zeros((S,), np.int32), n_map=zeros((S0,), np.int32), av=zeros((S,), np.int32),
                 map_pos=zeros((S0, M_cap, 2), np.float32), map_orient=zeros((S0, M_cap), np.float32),
                 map_tok=zeros((S0, M_cap), np.int64), map_type=zeros((S0, M_cap), np.int64),
                 map_pl=zeros((S0, M_cap), np.int64), map_light=zeros((S0, M_cap), np.int64))
        if k is None:
            return a
        rep = (lambda x: x) if self.copies == 1 else (lambda x: np.repeat(x, self.copies, axis=0))
        A, M = k['pos'].shape[1], k['map_pos'].shape[1]
        a['n_agents'][:], a['n_map'][:], a['av'][:] = rep(k['A']), k['M'], rep(k['av'])
        a['pos'][:, :, :A] = rep(k['pos']).transpose(0, 2, 1, 3)
        for dst, src in (('head', 'head'), ('state', 'state'), ('token', 'token'), ('gridtok', 'grid'), ('tmask', 'tmask'),
                         ('imask', 'imask'), ('catflag', 'catflag')):
            a[dst][:, :, :A] = rep(k[src]).transpose(0, 2, 1)
        a['atype'][:, :A] = rep(k['type']); a['bos'][:, :A] = rep(k['bos']); a['_shape10'][:, :A] = rep(k['shape10'])
        for key in self._MAP_SIDE[1:]:
            a[key][:, :M] = k[key]
        return a

    def _fits(self, n_scenes: int, amax: int, mmax: int, T0: int = 0) -> bool:
        """same scene count, agents + insertion head-room and map tokens inside the rows this engine allocated, token columns
        inside T"""
        if n_scenes != self.S // self.copies or (self.teacher_token is not None and getattr(self, 'replay_row', None) is None):
            return False                       # (an all-row teacher belongs to its scenes; a replay engine takes a new plan)
        head = (self.A_cap - self._amax0) if self.insertion else 0
        return amax + head <= self.A_cap and mmax <= self.M_cap and T0 <= self.T

    def fits(self, scenes: Sequence[Mapping]) -> bool:
        """can ``reload`` take this batch? (the agents counted after the row filter)"""
        amax = max(int((np.asarray(sc['agent']['state_idx'])[:, self.hc - 1] != INVALID).sum()) for sc in scenes)
        mmax = max(int(np.asarray(sc['pt_token']['position']).shape[0]) for sc in scenes)
        return self._fits(len(scenes), amax, mmax)

    @staticmethod
    def _check_temperature(t, name: str) -> float:
        """a scalar temperature of the cell draw: finite and a normal float32 above 0 (1 / T must stay finite).  0 is refused here:
        the C struct reads it as "unset", i.e. 1, and the cell draw has no per-row form where it could mean greedy - a greedy
        cell is ``insert_k = 1``"""
        t = float(t)
        if not (np.isfinite(t) and t >= _FLT_MIN):
            raise ValueError(f'{name} must be finite and > 0, no denormal (got {t}; the arg-max cell is insert_k = 1)')
        return t

    @staticmethod
    def _check_top_p(p, name: str) -> float:
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f'{name} must be in (0, 1] (got {p})')
        return p

    def _load_temperature(self, temperature, amax):
        """``sample_temperature`` into the engine (None: keep what is there).  A float is the context's scalar - unless a per-row
        buffer exists already, which it then fills; an array [S] or [S][rows] is checked here, on the host, once per load (finite,
        >= 0: the library cannot look into device memory) and written into the static [S * A_cap] buffer the context points at."""
        if temperature is None:
            return
        S, A_cap = self.S, self.A_cap
        t = np.asarray(temperature, dtype=np.float32)
        if not (np.isfinite(t).all() and ((t == 0) | (t >= _FLT_MIN)).all()):
            raise ValueError('sample_temperature must be finite and 0 (greedy) or a normal float32 above 0 (1 / T must stay finite)')
        if t.ndim == 0 and self.sample_temp_row is None and float(t) > 0.0:      # (a scalar 0 is "every row greedy": the array's 0)
            if float(t) != self.sample_temperature:
                self._drop_graphs()      # (a captured graph holds the old kernel argument)
            self.sample_temperature = float(t)
        else:
            if t.ndim == 0:
                rows = np.full((S, A_cap), float(t), np.float32)
            elif t.ndim == 1:
                assert t.shape == (S,), f'sample_temperature {t.shape}: one entry per agent-side scene [S={S}]'
                rows = np.repeat(t[:, None], A_cap, axis=1)      # (rows insertion appends: their scene's value)
            else:
                need = A_cap if self.insertion else amax
                assert t.ndim == 2 and t.shape[0] == S and t.shape[1] >= need, \
                    f'sample_temperature {t.shape} does not cover [S={S}][rows={need}]'
                rows = np.ones((S, A_cap), np.float32)
                rows[:, :min(A_cap, t.shape[1])] = t[:, :A_cap]
            rows = torch.from_numpy(np.ascontiguousarray(rows.reshape(S * A_cap)))
            if self.sample_temp_row is None:
                self.sample_temp_row = rows.to(self.device)
                self._drop_graphs()
            else:
                self.sample_temp_row.copy_(rows)
        self._apply_sampling()

    def _load_token_masks(self, token_masks=None, token_mask_type=None, token_mask_row=None):
        """constrained decoding into the engine (None: keep what is there).  Everything on the host is checked here, before any
        launch; a device tensor of per-row selectors is taken as it is (the kernels read an index beyond the table as
        unconstrained).  The table and the per-row selectors are written into static buffers (allocated once per table shape)."""
        if token_masks is None and token_mask_type is None and token_mask_row is None:
            return
        S, A_cap = self.S, self.A_cap
        if token_masks is not None:
            if not isinstance(token_masks, constraints.TokenMasks):
                raise ValueError('token_masks takes an infgen_amd.constraints.TokenMasks')
            if token_masks.token_size != self.cfg.token_size:
                raise ValueError(f'token_masks are {token_masks.token_size} tokens wide, the model\'s vocabulary holds {self.cfg.token_size}')
            words = torch.from_numpy(token_masks.words.view(np.int32).copy())
            if self.mask_bits is None or self.mask_bits.shape != words.shape:
                self.mask_bits = words.to(self.device)
                self._drop_graphs()      # (a captured graph holds the old table's address and size)
            else:
                self.mask_bits.copy_(words)
            if token_mask_type is None and (self.token_masks is None or token_masks.n_sets != self.token_masks.n_sets):
                token_mask_type = token_masks.type_sets
            self.token_masks = token_masks
        if self.token_masks is None:
            raise ValueError('token_mask_type / token_mask_row need token_masks (a table of allowed-token sets)')
        n_sets = self.token_masks.n_sets
        if token_mask_type is not None:
            sel = constraints.check_type_selectors(token_mask_type, n_sets)
            if sel != self.token_mask_type:
                self._drop_graphs()      # (a captured graph holds the old kernel arguments)
            self.token_mask_type = sel
        elif any(v >= n_sets for v in self.token_mask_type):
            raise ValueError('the new token_masks hold fewer sets than token_mask_type selects')
        if self.mask_row is None:
            self.mask_row = torch.full((S * A_cap,), -1, dtype=torch.int32, device=self.device)
            self._drop_graphs()
        if token_mask_row is not None:
            if isinstance(token_mask_row, torch.Tensor) and token_mask_row.is_cuda:
                if tuple(token_mask_row.shape) != (S, A_cap) or token_mask_row.dtype != torch.int32:
                    raise ValueError(f'a device token_mask_row is int32 [S={S}][A_cap={A_cap}]')
                self.mask_row.copy_(token_mask_row.reshape(-1))
            else:
                r = constraints.check_row_selectors(np.asarray(token_mask_row), n_sets)
                if r.ndim != 2 or r.shape[0] != S or r.shape[1] > A_cap:
                    raise ValueError(f'token_mask_row {r.shape} does not fit [S={S}][rows <= {A_cap}]')
                rows = np.full((S, A_cap), -1, np.int32)
                rows[:, :r.shape[1]] = r
                self.mask_row.copy_(torch.from_numpy(rows.reshape(-1)))
        self._apply_token_masks()

    def _drop_graphs(self):
        """a captured graph holds the launches, kernel arguments and addresses of its capture: whatever changes one drops both"""
        self._graph = self._wgraph = None

    @property
    def _has_shape(self) -> bool:
        return getattr(self, '_shape10', None) is not None

    def _load_rider(self, rider, value):
        """one rider's keyword into the engine (None: keep what is there), checked on the host before anything is allocated or
        launched.  ``_settle_<name>`` does what is the rider's own around ``store()``: a new key drops the graphs, ``conf`` is kept"""
        if value is None:
            return
        conf, old = rider.check(self, value), getattr(self, rider.name)
        if conf is None and old is None:
            return

        def store():
            if rider.key(conf) != rider.key(old):
                self._drop_graphs()
            setattr(self, rider.name, conf)
        getattr(self, '_settle_' + rider.name)(conf, value, store)
        self._apply_token_masks()

    def _settle_avoid_collisions(self, conf, value, store):
        """the buffers are allocated once and stay, also while the rider is off (static addresses for captured graphs)"""
        if conf is not None and self._coll is None:
            self._coll = constraints.collision_buffers(conf, self.S * self.A_cap, self.cfg.token_size, self.device)
            self.collision_bits, self.collision_allowed = self._coll['bits'], self._coll['allowed']
            self._coll['shape'].copy_(self._shape10.reshape(-1, 3))
            self._end_pose_table()
        store()

    def _end_pose_table(self):
        """the per-token end poses of the vocabulary, once per engine (collision and road masks read the same table)"""
        if self._coll_end is None:
            self._coll_cols = torch.arange(self.A_cap, device=self.device, dtype=torch.int32)[None]
            self._coll_end = torch.zeros(12 * self.cfg.token_size + 4, device=self.device)
            _lib.check(self.lib.infgen_collision_end_poses(_lib.ptr(self.vocab), self.cfg.token_size, _lib.ptr(self._coll_end),
                                                           self.ops.stream), 'infgen_collision_end_poses')

    def _settle_stay_on_road(self, conf, value, store):
        """the record table is built by the next prologue (``_road_build``): the map may not be in the buffers yet"""
        if conf is not None and self._road is None:
            self._road = constraints.road_buffers(conf, self.S * self.A_cap, self.cfg.token_size, self.device)
            self.road_bits, self.road_allowed = self._road['bits'], self._road['allowed']
            self._road['shape'].copy_(self._shape10.reshape(-1, 3))
            self.road_n_records = torch.zeros(self.S0, device=self.device, dtype=torch.int32)
            self._end_pose_table()
            self._road_paths = torch.zeros(12 * self.cfg.token_size, device=self.device)
            _lib.check(self.lib.infgen_road_paths(_lib.ptr(self._coll_end), self.cfg.token_size, _lib.ptr(self._road_paths),
                                                  self.ops.stream), 'infgen_road_paths')
        store()
        if conf is not None:
            self._road_source(conf)
        if self.step_scores is not None:               # the scores read the engine's one road table: checked against the new one
            self._load_rider(_SCORES, self._score_arg)

    def _settle_follow_routes(self, conf, value, store):
        """the routes are uploaded and their records built at once (they do not depend on the scene in the buffers)"""
        store()
        if conf is not None:
            self._upload_routes(conf.pop('routes'), conf.pop('n_points'))
        else:      # off: nothing of the last routed step stays readable
            self._route = self.route_bits = self.route_allowed = self.route_progress = None

    def set_routes(self, routes, n_points):
        """new routes for an engine with ``follow_routes`` on - allowed between two steps of a rollout or session: uploaded into
        the static buffers (new ones when P changes), the records rebuilt by k_route_records on the engine's stream.  A captured
        graph is dropped, as after every change of a pointer"""
        if self.follow_routes is None:
            raise ValueError('set_routes: the engine was built without follow_routes')
        self._upload_routes(*constraints.route_arrays(routes, n_points, n_scenes=self.S0, a_cap=self.A_cap))
        self._drop_graphs()
        self._apply_token_masks()

    def _upload_routes(self, routes: np.ndarray, n_points: np.ndarray):
        P = int(routes.shape[2])
        if self._route is None or self._route['P'] != P:
            self._route = constraints.route_buffers(self.S0, self.S * self.A_cap, self.A_cap, P, self.cfg.token_size, self.device)
            self.route_bits, self.route_allowed, self.route_progress = (self._route[k] for k in ('bits', 'allowed', 'progress'))
            self._end_pose_table()
            self._drop_graphs()          # (a captured graph holds the old buffers' addresses)
        k, A = self._route, int(routes.shape[1])
        full, n = np.zeros((self.S0, self.A_cap, P, 2), np.float32), np.zeros((self.S0, self.A_cap), np.int32)
        full[:, :A], n[:, :A] = routes, n_points
        k['routes'].copy_(torch.from_numpy(full))
        k['n_points'].copy_(torch.from_numpy(n))
        _lib.check(self.lib.infgen_route_records(_lib.ptr(k['routes']), _lib.ptr(k['n_points']), self.S0, self.A_cap, P,
                                                 _lib.ptr(k['records']), _lib.ptr(k['total']), self.ops.stream), 'infgen_route_records')

    def _settle_obey_signals(self, conf, value, store):
        """uploaded at once like the routes; every upload drops the graphs, not only a new key (``_upload_signals``)"""
        if conf is not None:
            self._upload_signals(conf.pop('phase'), conf.pop('lines'), conf.pop('n_lines'))
            conf.update(K=self._signal['K'], n_phase=self._signal['n_phase'])
        else:      # off: nothing of the last ruled step stays readable
            self._signal = self.signal_bits = self.signal_allowed = self.signal_info = None
        store()

    def set_signals(self, phase=None, lines=None, n_lines=None):
        """new signal tables for an engine with ``obey_signals`` on - allowed between two steps of a rollout or session, and between
        two rollouts: ``phase`` [S0][n_phase][K] (or [S0][K]) and / or ``lines`` [S0][K][4] with ``n_lines`` [S0] (default: all K) are
        uploaded into the static buffers (new ones when K or n_phase changes), and new lines' records rebuilt by k_signal_records
        on the engine's stream.  A captured graph is dropped by every upload (``_upload_signals``), as ``set_routes`` drops it: the
        next rollout captures again."""
        if self.obey_signals is None:
            raise ValueError('set_signals: the engine was built without obey_signals')
        if phase is None and lines is None:
            if n_lines is not None:
                raise ValueError('set_signals: n_lines comes with lines')
            return
        k = self._signal
        if lines is not None:
            lines, n_lines = constraints.signal_lines(lines, n_lines, n_scenes=self.S0, what='set_signals')
            if phase is None and lines.shape[1] != k['K']:
                raise ValueError(f'set_signals: lines for K = {lines.shape[1]} need a phase table of that K (the engine holds K = {k["K"]})')
        elif n_lines is not None:
            raise ValueError('set_signals: n_lines comes with lines')
        if phase is not None:
            phase = constraints.signal_phase_table(phase, self.S0, k['K'] if lines is None else lines.shape[1], 'set_signals')
        self._upload_signals(phase, lines, n_lines)
        conf = self.obey_signals
        if (conf['K'], conf['n_phase']) != (self._signal['K'], self._signal['n_phase']):
            conf.update(K=self._signal['K'], n_phase=self._signal['n_phase'])
        self._apply_token_masks()

    def _upload_signals(self, phase, lines, n_lines):
        """phase and / or lines (checked host arrays, None: keep) into the static buffers; new extents take new buffers"""
        k = self._signal
        K = int(lines.shape[1]) if lines is not None else k['K']
        n_phase = int(phase.shape[1]) if phase is not None else k['n_phase']
        if k is None or (k['K'], k['n_phase']) != (K, n_phase):
            if lines is None or phase is None:
                if k is None or k['K'] != K:
                    raise ValueError('set_signals: a new K needs both lines and phase')
                # a phase table of another length over the lines that are there
                lines, n_lines = k['lines'].cpu().numpy(), k['n_lines'].cpu().numpy()
            self._signal = k = constraints.signal_buffers(self.S0, self.S * self.A_cap, K, n_phase, self.cfg.token_size, self.device)
            self.signal_bits, self.signal_allowed, self.signal_info = k['bits'], k['allowed'], k['info']
            k['shape'].copy_(self._shape10.reshape(-1, 3))
            self._end_pose_table()
        # every upload drops a captured graph - through set_signals and through reload*(obey_signals=...) alike -, also where the
        # buffers keep their addresses: the next rollout captures again and no graph is replayed over tables rewritten under it
        self._drop_graphs()
        if phase is not None:
            k['phase'].copy_(torch.from_numpy(phase))
        if lines is not None:
            k['lines'].copy_(torch.from_numpy(lines))
            k['n_lines'].copy_(torch.from_numpy(n_lines))
            _lib.check(self.lib.infgen_signal_records(_lib.ptr(k['lines']), _lib.ptr(k['n_lines']), self.S0, K, _lib.ptr(k['records']),
                                                      self.ops.stream), 'infgen_signal_records')

    def _settle_step_scores(self, conf, value, store):
        """the scores share road's record table and drive it where road is off; ``value`` is kept for road's re-check"""
        if conf is not None and self.insertion:
            raise ValueError('step_scores: engines with scenario insertion are left out (rows appended inside a step), as branching is')
        if conf is not None and self.step_score is None:
            self.step_score = torch.zeros(self.S, self.cfg.num_decode_steps, 8, device=self.device)
            self.score_row = torch.zeros(self.S, self.A_cap, device=self.device, dtype=torch.uint8)
            if self._road is None:                     # (with road buffers in the engine the scores read their shape array)
                self._score_shape = self._shape10.reshape(-1, 3).clone()
        if self.road_n_records is None and conf is not None:
            self.road_n_records = torch.zeros(self.S0, device=self.device, dtype=torch.int32)
        store()
        self._score_arg = value if conf is not None else None
        if conf is not None and self.stay_on_road is None:      # the scores alone drive the road table
            self._road_source(conf)

    def _road_source(self, conf):
        """``conf`` (road or scores) drives the engine's one road table: built again by the next prologue, from conf's explicit
        segments where it has some, else from the map"""
        self._road_dirty = True
        self._road_seg = None
        if conf['segments'] is not None:
            self._road_seg = tuple(torch.from_numpy(a).to(self.device) for a in conf['segments'])
        self._road_room(64)

    def _score_boxes(self) -> torch.Tensor:
        """the [rows, 3] shape array the score kernel reads: the road buffers' where the engine has them, else the scores' own"""
        if self._road is not None:
            self._score_shape = None
            return self._road['shape']
        return self._score_shape

    def _road_room(self, need: int):
        """a record table of at least ``need`` records per distinct scene: grown (a new buffer, so captured graphs go and the
        configuration is attached again), never shrunk"""
        if self.road_records is None or need > self._road_cap:
            self._road_cap = _round_up(max(need, 1), 64)
            self.road_records = torch.zeros(self.S0, self._road_cap, 8, device=self.device)
            self._drop_graphs()

    def _road_build(self):
        """the record table from the map in the buffers (or the explicit segments), once per reload: one count of EDGE tokens per
        scene sizes it (the only host synchronisation), k_road_records_map / _seg fills it"""
        conf, P = (self.stay_on_road if self.stay_on_road is not None else self.step_scores), _lib.ptr
        if self._road_seg is not None:
            seg, nseg = self._road_seg
            self._road_room(int(seg.shape[1]))
            self._apply_token_masks(validate=False)
            _lib.check(self.lib.infgen_road_records_from_segments(P(seg), P(nseg), self.S0, int(seg.shape[1]), P(self.road_records),
                                                                  self._road_cap, P(self.road_n_records), self.ops.stream),
                       'infgen_road_records_from_segments')
        else:
            mtok, mtype = self._map_cat[0], self._map_cat[1]
            inmap = torch.arange(self.M_cap, device=self.device)[None] < self.n_map[:, None]
            edges = int(((mtype == 12) & inmap).sum(dim=1).max().item())
            self._road_room(edges * conf['detail'])
            self._apply_token_masks(validate=False)
            _lib.check(self.lib.infgen_road_records_from_map(P(self.map_pos), P(self.map_orient), P(mtype), P(mtok), P(self.n_map),
                                                             self.S0, self.M_cap, P(self._map_vocab), int(self._map_vocab.shape[0]),
                                                             conf['detail'], P(self.road_records), self._road_cap,
                                                             P(self.road_n_records), self.ops.stream), 'infgen_road_records_from_map')
        self._road_dirty = False

    def _apply_token_masks(self, validate: bool = True):
        """the library's handle of (table, per-row selectors, per-type sets) into the context: registered again when one of the
        three changed as a VALUE of the registration (a new buffer, other per-type indices) - new contents need nothing.  The
        riders' configurations ride on the handle (one without a table when the engine has no ``token_masks``)"""
        if self._ctx is None or (self.token_masks is None and all(getattr(self, r.name) is None for r in RIDERS)
                                 and not self._mask_handle):
            return
        if self.token_masks is not None:
            reg = (self.mask_bits.data_ptr(), self.token_masks.n_sets, self.mask_row.data_ptr(), tuple(self.token_mask_type))
        else:
            reg = (None, 0, None, (-1, -1, -1))
        if reg != getattr(self, '_mask_reg', None):
            self._drop_mask_handle()
            h = self.lib.infgen_token_mask_create(reg[0], reg[1], reg[2], (C.c_int * 3)(*reg[3]), None)
            if h < 1:
                _lib.check(-1, 'infgen_token_mask_create')
            self._mask_handle, self._mask_reg = h, reg
        h = self._mask_handle
        # every rider onto the handle where its registration changed: ``_attach_<name>``'s arguments, the table's "off" ones without
        for r in RIDERS:
            conf = getattr(self, r.name)
            reg, args = (None, r.off) if conf is None else getattr(self, '_attach_' + r.name)(conf)
            reg = None if conf is None else (h,) + reg
            if reg != getattr(self, r.reg):
                _lib.check(getattr(self.lib, r.entry)(h, *args), r.entry)
                setattr(self, r.reg, reg)
        self._ctx.token_mask = h
        if validate:
            _lib.check(self.lib.infgen_rollout_validate(C.byref(self._ctx)), 'infgen_rollout_validate')

    # per rider -> (what the registration depends on besides the handle, the attach entry's arguments behind the handle)
    def _attach_avoid_collisions(self, conf):
        k, P = self._coll, _lib.ptr
        return ((conf['predict'], conf['margin']),
                (P(k['bits']), P(k['ident']), P(k['shape']), P(self._coll_end), conf['predict'], conf['margin'], P(k['allowed'])))

    def _attach_stay_on_road(self, conf):      # (the table's address is part of the registration)
        k, P = self._road, _lib.ptr
        return ((conf['margin'], conf['sweep'], conf['types'], self.road_records.data_ptr(), self._road_cap),
                (P(k['bits']), P(k['ident']), P(k['shape']), P(self._coll_end), P(self._road_paths), P(self.road_records),
                 P(self.road_n_records), self._road_cap, self.copies, conf['sweep'], conf['margin'], (C.c_int * 3)(*conf['types']),
                 P(k['allowed'])))

    def _attach_step_scores(self, conf):
        P, boxes = _lib.ptr, self._score_boxes()
        return ((constraints.score_key(conf), self.road_records.data_ptr(), self._road_cap, boxes.data_ptr()),
                (P(self.step_score), int(self.step_score.shape[1]), P(self.score_row), P(boxes), P(self.road_records),
                 P(self.road_n_records), self._road_cap, self.copies, conf['sweep'], conf['road_margin'],
                 (C.c_int * 3)(*conf['types']), conf['dt']))

    def _attach_follow_routes(self, conf):
        k, P = self._route, _lib.ptr
        return ((constraints.route_key(conf), k['records'].data_ptr()),
                (P(k['bits']), P(k['ident']), P(k['shape']), P(self._coll_end), P(k['records']), P(k['total']), k['P'], self.copies,
                 conf['corridor'], conf['back'], conf['pace'], conf['finish'], (C.c_int * 3)(*conf['types']), P(k['allowed']),
                 P(k['progress'])))

    def _attach_obey_signals(self, conf):
        k, P = self._signal, _lib.ptr
        return ((constraints.signal_key(conf), k['records'].data_ptr(), k['phase'].data_ptr()),
                (P(k['bits']), P(k['ident']), P(k['shape']), P(self._coll_end), P(k['records']), P(k['phase']), k['n_phase'], k['K'],
                 self.copies, conf['setback'], conf['align'], (C.c_int * 3)(*conf['types']), P(k['allowed']), P(k['info'])))

    def _drop_mask_handle(self):
        if getattr(self, '_mask_handle', 0):
            self.lib.infgen_token_mask_destroy(self._mask_handle)
            self._mask_handle, self._mask_reg = 0, None
            for r in RIDERS:
                setattr(self, r.reg, None)
            if getattr(self, '_ctx', None) is not None:
                self._ctx.token_mask = 0

    def __del__(self):
        try:
            self._drop_mask_handle()
        except Exception:      # (interpreter shutdown: the library may be gone)
            pass

    def _apply_sampling(self):
        if self._ctx is not None:
            c = self._ctx
            c.sample_temperature, c.sample_top_p = self.sample_temperature, self.sample_top_p
            c.sample_temp_row = _lib.ptr(self.sample_temp_row)

    def _load_riders(self, step: Mapping):
        """what rides on the decode step (``STEP_KEYWORDS``; each None: keep what is there) into the engine, in the one order it is
        resolved in: masks, collisions, road, scores, routes, signals.  Road and scores are checked against each other once both
        are resolved: the scores' argument is recorded - and scores that go are gone - before road's ``_settle_stay_on_road``
        checks the scores that are on against the new road"""
        self._load_token_masks(*(step[k] for k in STEP_KEYWORDS[:3]))
        for r in RIDERS:
            if r.name == 'stay_on_road' and step['step_scores'] is not None:
                self._score_arg = step['step_scores'] if step['step_scores'] is not False else None
                if step['step_scores'] is False:
                    self._load_rider(_SCORES, False)
            self._load_rider(r, step[r.name])

    def _load_uniforms(self, sample_uniforms, insert_uniforms, amax, sample_temperature, sample_top_p, step: Mapping):
        self._load_riders(step)
        if sample_top_p is not None:
            p = self._check_top_p(sample_top_p, 'sample_top_p')
            if p != self.sample_top_p:
                self._drop_graphs()      # (a captured graph holds the old kernel argument)
            self.sample_top_p = p
            self._apply_sampling()
        self._load_temperature(sample_temperature, amax)
        if self.sample_k > 1:
            assert sample_uniforms is not None, 'top-k sampling needs caller-supplied uniforms'
            self.sample_u.copy_(torch.from_numpy(self._uniform_rows(sample_uniforms, amax)))
        if self.insert_k > 1:
            assert insert_uniforms is not None, 'cell sampling needs caller-supplied uniforms [steps][10][S]'
            self._insert_u.copy_(torch.from_numpy(np.ascontiguousarray(insert_uniforms, dtype=np.float32)))

    def _end_session(self):
        """a closed-loop session ends before a new batch (and its plan) is loaded: its end restores the plan pointers it found"""
        if self._session is not None:
            self._session._end()

    def _invalidate(self):
        """what a new batch in the buffers outdates"""
        self._init = None                  # reset() snapshots the new initial state
        self._wgraph = None                # (the whole-rollout graph restores the state from the old snapshot's buffers)
        self._mg_checked = False           # the new map may hold more pt <-> pt edges than the buffers
        self._prologue_done = False
        self._road_dirty = True            # the road records belong to the old map
        self._ins_map_dirty = True         # ... and so do the insertion rules'
        self._reload_gen += 1              # snapshots of the old batch are refused (``restore``)

    # ------------------------------------------------------------------ log replay
    def _alloc_replay(self, with_pose: bool):
        """the plan buffers of a replay engine (once) and which of them the context points at: a plan without poses leaves
        teacher_pos / teacher_head NULL (the stored pose is the forced token's integration).  The pointers are static like every
        other of the context - a new plan changes contents only; a captured graph is dropped when a pointer does change"""
        S, T, A_cap, dev = self.S, self.T, self.A_cap, self.device
        changed = False
        if self.replay_row is None:
            self.teacher_token = torch.full((S, T, A_cap), -1, dtype=torch.int32, device=dev)
            self.teacher_state = torch.zeros((S, T, A_cap), dtype=torch.int32, device=dev)
            self.replay_row = torch.zeros((S, A_cap), dtype=torch.uint8, device=dev)
            changed = True
        if with_pose and self._replay_pose is None:
            self._replay_pose = (torch.zeros((S, T, A_cap, 2), device=dev), torch.zeros((S, T, A_cap), device=dev))
        if with_pose != (self.teacher_pos is not None):
            self.teacher_pos, self.teacher_head = self._replay_pose if with_pose else (None, None)
            changed = True
        if changed and self._ctx is not None:
            c, P = self._ctx, _lib.ptr
            c.teacher_token, c.teacher_state, c.replay_row = P(self.teacher_token), P(self.teacher_state), P(self.replay_row)
            c.teacher_pos, c.teacher_head = P(self.teacher_pos), P(self.teacher_head)
            self._drop_graphs()
            _lib.check(self.lib.infgen_rollout_validate(C.byref(c)), 'infgen_rollout_validate')

    def _load_replay(self, mask: Optional[torch.Tensor], plan: Optional[Mapping[str, torch.Tensor]]):
        """row mask [S0, A] + plan ([S0, A, T0, ...], ``scene_setup.replay_arrays``) on any device -> this engine's plan buffers;
        None: nothing is replayed (an engine that has the buffers clears its flags)"""
        if mask is None:
            if self.replay_row is not None:
                self.replay_row.zero_()
            return
        arrs = scene_setup.replay_arrays(mask, plan, self.hc, self.T, self.A_cap, self.copies)
        self._alloc_replay('teacher_pos' in arrs)
        for k, v in arrs.items():
            getattr(self, k).copy_(v)

    def _replay_from_hosts(self, replay):
        if replay is None:
            return self._load_replay(None, None)
        self._load_replay(*scene_setup.stage_replay(self.scenes, [h['filt'] for h in self.hosts[::self.copies]], replay, self.T))

    def reload(self, scenes: Sequence[Mapping], sample_uniforms: Optional[np.ndarray] = None,
               insert_uniforms: Optional[np.ndarray] = None, x_pt_override: Optional[Sequence] = None, replay=None,
               sample_temperature=None, sample_top_p=None, token_masks=None, token_mask_type=None, token_mask_row=None,
               avoid_collisions=None, stay_on_road=None, step_scores=None, follow_routes=None, obey_signals=None):
        """a new batch of scenes of the same layout into this engine's device buffers: one upload per array, no allocation, the
        context block / captured graph / scratch stay (the drop-in entry keeps one engine per layout across calls)"""
        assert self.fits(scenes), 'batch does not fit this engine (RolloutEngine.fits)'
        self._end_session()
        self.scenes = scenes
        self._hosts_light = False
        hosts, staged = self._setup_scenes(scenes)
        self.hosts = self._replicate(hosts)
        arr = self._scene_arrays(staged)
        for k in self._SCENE_ARRAYS:
            getattr(self, k).copy_(torch.from_numpy(arr[k]), non_blocking=False)
        for dst, k in zip(self._map_cat, ('map_tok', 'map_type', 'map_pl', 'map_light')):
            dst.copy_(torch.from_numpy(arr[k]))
        self._load_uniforms(sample_uniforms, insert_uniforms, int(staged['A'].max()), sample_temperature, sample_top_p,
                            _step_keywords(locals()))
        self._x_pt_override = x_pt_override
        self._epi = None
        self._replay_from_hosts(replay)
        self._invalidate()

    # ------------------------------------------------------------------ a batch that is already on the device
    def fits_device(self, k: Mapping) -> bool:
        """``fits`` for a stacked device batch (``_setup_device``): shapes only, no host copy"""
        S, A, T0 = (int(n) for n in k['agent']['state_idx'].shape)
        if self.copies > 1 or A < 1:
            return False                        # (batches with copies take the host path: reload)
        return self._fits(S, A, int(k['pt_token']['position'].shape[1]), T0)

    def reload_device(self, k: Mapping, scenes, sample_uniforms: Optional[np.ndarray] = None,
                      insert_uniforms: Optional[np.ndarray] = None, x_pt_override: Optional[Sequence] = None, replay=None,
                      sample_temperature=None, sample_top_p=None, token_masks=None, token_mask_type=None,
                      token_mask_row=None, avoid_collisions=None, stay_on_road=None, step_scores=None, follow_routes=None,
                      obey_signals=None) -> bool:
        """``reload`` for a batch whose scenes arrive as DEVICE tensors of one shape, stacked per key (``k``: what
        ``modules.infgen_decoder.stack_datas`` returns): the setup statements (``scene_setup.setup_agents``) and the epilogue's
        input arrays run as torch ops on the device and write this engine's buffers - no device -> host -> device
        round trip of the scene arrays (~70 ms of a 512-scene call before the first launch).  ``scenes`` is the (lazy) host form
        of the same batch, only read if somebody asks for the host-side ``outputs()``.  Returns False, having changed nothing,
        when a row would be filtered (the host path handles that: ``reload``).  ``replay``: a bool mask [S, A] on the device (the
        plan is the stacked logged future) or (mask, dict of stacked token_idx / state_idx[, token_pos, token_heading]) - copied
        into the plan buffers on the device before the future columns are zeroed."""
        assert self.fits_device(k), 'batch does not fit this engine (RolloutEngine.fits_device)'
        self._end_session()
        if not self._setup_device(k, replay):
            return False
        self.scenes = scenes
        self._load_uniforms(sample_uniforms, insert_uniforms, self.hosts[0]['A'], sample_temperature, sample_top_p,
                            _step_keywords(locals()))
        self._x_pt_override = x_pt_override
        self._invalidate()
        return True

    def _setup_device(self, k: Mapping, replay=None) -> bool:
        """``scene_setup`` for a one-shape batch on the device, written into this engine's buffers"""
        cfg = self.cfg
        T, hc, H, S = cfg.num_columns, cfg.hist_columns, cfg.num_historical_steps, self.S
        ag, pt = k['agent'], k['pt_token']
        A, M = int(ag['state_idx'].shape[1]), int(pt['position'].shape[1])
        av = ag['av_index'].reshape(S, -1)[:, 0].long()
        # the one host copy of the way in: the ego rows + "is any row filtered?" (then the host path takes the batch)
        chk = torch.cat([av, (ag['state_idx'][:, :, hc - 1] == INVALID).any().long()[None]]).cpu().numpy()
        if chk[-1]:
            return False
        av_host = chk[:-1]
        if replay is not None:                # (the logged future of the flagged rows, before setup_agents zeroes it)
            mask, plan = replay if isinstance(replay, (tuple, list)) else (replay, None)
            self._load_replay(mask, {k_: ag[k_] for k_ in scene_setup.PLAN_KEYS} if plan is None else plan)
        elif getattr(self, 'replay_row', None) is not None:
            self.replay_row.zero_()
        a = scene_setup.setup_agents(dict(ag, eval_mask=ag['valid_mask'][:, :, H - 1], shape10=ag['shape'][:, :, H - 1]), av, cfg, T)

        def put(dst, src, fill=0):          # [S, A, T, ...] -> the engine's [S, T, A_cap, ...]
            dst.fill_(fill)
            dst[:, :, :A] = src.transpose(1, 2)
        put(self.pos, a['pos']); put(self.head, a['head']); put(self.state, a['state']); put(self.token, a['token'], -1)
        put(self.gridtok, a['grid'], -1); put(self.tmask, a['tmask']); put(self.imask, a['imask']); put(self.catflag, a['catflag'])
        self.atype.zero_(); self.atype[:, :A] = a['type']
        self.bos.zero_(); self.bos[:, :A] = a['bos']
        self._shape10.fill_(INVALID_SHAPE); self._shape10[:, :A] = a['shape10']
        self.n_agents.fill_(A); self.n_map.fill_(M); self.av.copy_(av)
        self.map_pos.zero_(); self.map_pos[:, :M] = pt['position'][:, :, :2]
        self.map_orient.zero_(); self.map_orient[:, :M] = pt['orientation']
        light = torch.gather(k['light_type'].long(), 1, k['edge_index'][:, 1].long())
        for dst, src in zip(self._map_cat, (pt['token_idx'], pt['type'], pt['pl_type'], light)):
            dst.zero_()
            dst[:, :M] = src
        self._gt_len = [int(ag['position'].shape[2]) - H] * S
        self._epi = dict(scene_setup.epilogue_inputs(ag, a['valid'], self.A_cap, cfg), n0_host=np.full(S, A, np.int64))
        filt = np.ones(A, bool)
        self.hosts = [dict(A=A, M=M, av=int(av_host[s]), filt=filt) for s in range(S)]
        self._hosts_light = True             # (the host-side ``outputs()`` rebuilds the full per-scene dicts when asked)
        return True

    def _full_hosts(self):
        """the per-scene host dicts with every array of ``_setup_scenes`` (a device-side reload keeps only A / M / av / filt)"""
        if getattr(self, '_hosts_light', False):
            self.scenes = list(self.scenes)
            self.hosts = self._replicate(self._setup_scenes(self.scenes)[0])
            self._hosts_light = False
        return self.hosts

    # ------------------------------------------------------------------ a ragged Batch on the device
    def fits_batch(self, layout: Mapping) -> bool:
        """``fits`` for a ragged Batch (``read_batch_layout``): the unfiltered rows counted"""
        return self._batch_lay is not None and self._fits(layout['B'], layout['amax'], layout['mmax'], layout['T0'])

    def reload_batch(self, batch, src_graph: Optional[torch.Tensor] = None, sample_uniforms: Optional[np.ndarray] = None,
                     insert_uniforms: Optional[np.ndarray] = None, layout: Optional[Mapping] = None, replay=None,
                     sample_temperature=None, sample_top_p=None, token_masks=None, token_mask_type=None, token_mask_row=None,
                     avoid_collisions=None, stay_on_road=None, step_scores=None, follow_routes=None, obey_signals=None):
        """``reload`` for a ragged PyG-style Batch of device tensors: the ingest kernel (infgen_ingest_batch) filters, pads and
        writes every scene buffer and the epilogue inputs from the concatenated arrays - no host copy of the scene data; the
        only device -> host copy before the first launch is the offsets' (``read_batch_layout``, skipped when ``layout`` is
        given).  ``src_graph`` [S] (int32, device): the graph of every agent-side scene; default: graph i's copies adjacent."""
        if layout is None:
            layout = read_batch_layout(batch, self.T, self.hc, self.lib.infgen_layout_query(_lib.Q_MAX_AGENTS))
        assert self.fits_batch(layout), 'batch does not fit this engine (RolloutEngine.fits_batch)'
        self._end_session()
        self._load_uniforms(sample_uniforms, insert_uniforms, layout['amax'], sample_temperature, sample_top_p,
                            _step_keywords(locals()))
        self._ingest(batch, layout, src_graph, replay=replay)
        self._invalidate()

    def _ingest(self, batch, layout, src_graph=None, replay=None):
        cfg, dev, lib = self.cfg, self.device, self.lib
        S, A_cap, M_cap, T, hc, H = self.S, self.A_cap, self.M_cap, self.T, self.hc, cfg.num_historical_steps
        ag, pt = batch['agent'], batch['pt_token']
        keep = []                                   # converted inputs stay referenced until the launch is enqueued

        def arr(x, dtype):
            t_ = torch.as_tensor(x, device=dev)
            if t_.dtype != dtype:
                t_ = t_.view(torch.uint8) if (t_.dtype == torch.bool and dtype == torch.uint8) else t_.to(dtype)
            t_ = t_.contiguous()
            keep.append(t_)
            return t_.data_ptr()
        P = layout['P']
        Rg = P - H
        i64, f32, u8 = torch.int64, torch.float32, torch.uint8
        if self._ing is None or self._ing['gt'].shape[2] != Rg:
            z = lambda *shape, dt=f32: torch.zeros(*shape, dtype=dt, device=dev)
            self._ing = dict(htok=z(S, A_cap, hc, dt=i64), hst=z(S, A_cap, hc, dt=i64), p0=z(S, A_cap, 2), h0=z(S, A_cap),
                             ids=z(S, A_cap, dt=i64), shp=z(S, A_cap, 3), gt=z(S, A_cap, Rg, 2), val=z(S, A_cap, T, dt=torch.bool),
                             counts=z(S, 3, dt=torch.int32))
        E = self._ing
        if src_graph is None:
            src_graph = (torch.arange(S, device=dev, dtype=torch.int32) // self.copies)
        src_graph = src_graph.to(dev, torch.int32).contiguous()
        a = _lib.BatchIngest()
        a.S, a.copies, a.A_cap, a.M_cap, a.T, a.T0, a.P = S, self.copies, A_cap, M_cap, T, layout['T0'], P
        a.hc, a.H, a.motion_cols = hc, H, H // cfg.shift
        pos_t, ppos_t = torch.as_tensor(ag['position']), torch.as_tensor(pt['position'])
        a.pos_dim, a.pt_pos_dim = int(pos_t.shape[2]), int(ppos_t.shape[1])
        light = torch.as_tensor(batch['map_polygon']['light_type'])
        a.n_polygons = int(light.shape[0])
        a.agent_ptr, a.pt_ptr, a.av_index = arr(ag['ptr'], i64), arr(pt['ptr'], i64), arr(torch.as_tensor(ag['av_index']).reshape(-1), i64)
        a.src_graph = src_graph.data_ptr()
        a.state_idx, a.token_idx, a.grid_token_idx = arr(ag['state_idx'], i64), arr(ag['token_idx'], i64), arr(ag['grid_token_idx'], i64)
        a.token_pos, a.token_heading = arr(ag['token_pos'], f32), arr(ag['token_heading'], f32)
        a.raw_valid, a.valid_mask = arr(ag['raw_agent_valid_mask'], u8), arr(ag['valid_mask'], u8)
        a.shape, a.position, a.heading = arr(ag['shape'], f32), arr(pos_t, f32), arr(ag['heading'], f32)
        a.type, a.id = arr(ag['type'], u8), arr(ag['id'], i64)
        a.pt_position, a.pt_orientation = arr(ppos_t, f32), arr(pt['orientation'], f32)
        a.pt_token_idx, a.pt_type, a.pt_pl_type = arr(pt['token_idx'], i64), arr(pt['type'], u8), arr(pt['pl_type'], u8)
        a.pt_polygon = arr(torch.as_tensor(_edge_index(batch))[1], i64)
        a.light_type = arr(light, u8)
        for k_ in ('pos', 'head', 'state', 'token', 'gridtok', 'tmask', 'imask', 'catflag', 'atype', 'bos', 'n_agents', 'av', 'n_map',
                   'map_pos', 'map_orient'):
            setattr(a, k_, getattr(self, k_).data_ptr())
        a.shape10 = self._shape10.data_ptr()
        a.map_tok, a.map_type, a.map_pl, a.map_light = (t_.data_ptr() for t_ in self._map_cat)
        for k_ in ('htok', 'hst', 'p0', 'h0', 'shp', 'gt', 'val', 'ids', 'counts'):
            setattr(a, k_, E[k_].data_ptr())
        if replay is not None:
            # log replay: the kernel keeps the flagged rows' future columns (or the caller's plan) as the plan buffers' contents
            mask, plan = replay if isinstance(replay, (tuple, list)) else (replay, None)
            N = int(torch.as_tensor(ag['state_idx']).shape[0])
            if int(torch.as_tensor(mask).numel()) != N:
                raise ValueError(f'replay mask of {int(torch.as_tensor(mask).numel())} rows for a Batch of {N} agent rows')
            if layout['T0'] < T:
                raise ValueError(f"the plan covers {layout['T0']} token columns, the rollout has {T}")
            with_pose = True if plan is None else scene_setup.check_plan(plan)
            self._alloc_replay(with_pose)
            a.replay_in = arr(torch.as_tensor(mask).reshape(-1), u8)
            if plan is not None:
                for dst, key, dt, shape in (('plan_token', 'token_idx', i64, (N, layout['T0'])), ('plan_state', 'state_idx', i64, (N, layout['T0'])),
                                            ('plan_pos', 'token_pos', f32, (N, layout['T0'], 2)), ('plan_head', 'token_heading', f32, (N, layout['T0']))):
                    if plan.get(key) is not None:
                        if tuple(torch.as_tensor(plan[key]).shape) != shape:
                            raise ValueError(f'replay plan: {key} has shape {tuple(torch.as_tensor(plan[key]).shape)}, need {shape}')
                        setattr(a, dst, arr(plan[key], dt))
            a.teacher_token, a.teacher_state, a.replay_row = (x.data_ptr() for x in (self.teacher_token, self.teacher_state, self.replay_row))
            if with_pose:
                a.teacher_pos, a.teacher_head = self.teacher_pos.data_ptr(), self.teacher_head.data_ptr()
        elif self.replay_row is not None:
            self.replay_row.zero_()
        _lib.check(lib.infgen_ingest_batch(C.byref(a), self.ops.stream), 'infgen_ingest_batch')
        del keep
        self._batch_lay = layout
        self._bc_host = None
        self.scenes, self.hosts, self._hosts_light = None, None, False
        self._gt_len = [Rg] * S
        self._epi = dict(htok=E['htok'], hst=E['hst'], p0=E['p0'], h0=E['h0'], ids=E['ids'], shp=E['shp'], gt=E['gt'], val=E['val'],
                         n0=E['counts'][:, 0].long(), n0_host=None, eval_shape=torch.tensor(EVAL_SHAPE, device=dev))

    def batch_counts(self):
        """(final agent counts [S], ingest counts [S][3]: kept rows, ego row after filtering, rows removed before the ego) of an
        ingested Batch - the one device -> host copy after its rollout; also rebuilds the light per-scene host dicts"""
        if self._bc_host is None:
            S = self.S
            h = torch.cat([self.n_agents, self._ing['counts'].reshape(-1)]).cpu().numpy().astype(np.int64)
            n_fin, c = h[:S], h[S:].reshape(S, 3)
            self._bc_host = (n_fin, c)
            M = self._batch_lay['M']
            self.hosts = [dict(A=int(c[s, 0]), M=int(M[s // self.copies]), av=int(c[s, 1]), removed=int(c[s, 2])) for s in range(S)]
            self._epi['n0_host'] = c[:, 0].copy()
        return self._bc_host

    def _uniform_rows(self, sample_uniforms, amax) -> np.ndarray:
        steps, S, A_cap = self.cfg.num_decode_steps, self.S, self.A_cap
        su = np.asarray(sample_uniforms, dtype=np.float32)
        # a missing column would sample with u = 0, i.e. greedily - never fill in silently
        need = A_cap if self.insertion else amax
        assert su.ndim == 3 and su.shape[0] >= steps and su.shape[1] >= S and su.shape[2] >= need, \
            f'sample_uniforms {su.shape} does not cover [steps={steps}][S={S}][rows={need}]'
        u = np.zeros((steps, S, A_cap), np.float32)
        u[:, :, :min(A_cap, su.shape[2])] = su[:steps, :S, :A_cap]
        return u.reshape(steps, S * A_cap)

    def _fourier_split(self) -> bool:
        """is the Fourier embedding of the operator-level entries the split kernel (infgen_set_fourier_mode != 0)?  (they read
        the process-wide switches, like every call of the map encoder)"""
        o = _lib.Options()
        _lib.check(self.lib.infgen_get_effective_options(C.byref(o)), 'infgen_get_effective_options')
        return o.fourier_mode != 0

    # ------------------------------------------------------------------ prologue (once per rollout)
    def reset(self):
        """restore the scene state to the rollout's initial condition (device-to-device copies); ends a closed-loop session"""
        self._end_session()
        if self._init is None:
            self._init = {k: getattr(self, k).clone() for k in self._STATE}
        else:
            for k in self._STATE:
                getattr(self, k).copy_(self._init[k])
        for buf in (self.pred_traj, self.pred_head, self.pred_state):
            buf.zero_()
        if self.token_logprob is not None:
            self.token_logprob.zero_()
        if self.sample_logprob is not None:
            self.sample_logprob.zero_()

    _STATE = ('pos', 'head', 'state', 'token', 'gridtok', 'imask', 'catflag', 'tmask', 'atype', 'bos', 'n_agents')

    def prologue(self, map_only: bool = False):
        """per-scene constants and the first columns: agent categorical embeddings, map encoder
        (map_decoder.py:70-130), map K/V of the six map->agent layers, the edgeless column-0 chain
        (SURVEY a-Q3) and column 1's raw feature."""
        # the operator-level calls below (map encoder, tables) run under THIS engine's switches: installed as the calling thread's
        # option block for the duration of the prologue (re-entrant across host threads; include/infgen_hip.h)
        with _lib.thread_options(self._effective_options()):
            return self._prologue(map_only)

    def _effective_options(self):
        o = _lib.Options()
        _lib.check(self.lib.infgen_get_options(C.byref(o)), 'infgen_get_options')
        for k, v in (self.options or {}).items():
            setattr(o, k, int(v))
        o.use, o.row_groups, o.n_row_groups = 0, None, None
        return o

    def _prologue(self, map_only: bool = False):
        ops, w, cfg, dev = self.ops, self.w, self.cfg, self.device
        S, A_cap, M_cap, rows = self.S, self.A_cap, self.M_cap, self.rows
        tabs = w.tables(ops, self.vocab, self.grid_xy, self._map_vocab, self._tables_key)
        self.tok_tab, self.grid_tab, self.cat_seed = tabs['tok_tab'], tabs['grid_tab'], tabs['cat_seed']
        self.f_seed = tabs['f_seed']                 # (this engine's entry, not whatever the pack built last)
        self.reset()
        if self._coll is not None:                   # the rows' boxes for k_collision_mask (rows insertion appends: _step_gen)
            self._coll['shape'].copy_(self._shape10.reshape(rows, 3))
        if self.stay_on_road is not None:            # road-aware decoding: the rows' boxes, and the record table of a new map
            self._road['shape'].copy_(self._shape10.reshape(rows, 3))
            if self._road_dirty:
                self._road_build()
        if self._signal is not None:                 # signal-aware decoding: the rows' boxes (the lines are the caller's)
            self._signal['shape'].copy_(self._shape10.reshape(rows, 3))
        if self.step_scores is not None:             # step scores: the rows' boxes, and the record table where the scores alone drive it
            if self.stay_on_road is None:            # (otherwise the one shape array was refreshed just above)
                self._score_boxes().copy_(self._shape10.reshape(rows, 3))
            if self._road_dirty:
                self._road_build()
        # categorical embedding rows (agent_decoder.py:376-380,492)
        if self.cat_agent is None:
            self.cat_agent = torch.empty(rows, D, device=dev)
        shp = ops.mlp_embedding(self._shape10.reshape(rows, 3), w.shape_emb, 3)
        torch.add(w.type_a_emb[self.atype.reshape(-1).long()], shp, out=self.cat_agent)

        if self._x_pt_override is not None:
            return self._prologue_with_given_map()
        # ---- map encoder (once per DISTINCT scene)
        S0 = self.S0
        mrows = S0 * M_cap
        mtok, mtype, mpl, mlight = self._map_cat
        if self.x_pt is None:
            self.x_pt = torch.empty(mrows, D, device=dev)
        # token-table row + (type + polygon type) + light embedding (map_decoder.py:87-89) in one pass over the rows
        mt = tabs['map_tab']
        _lib.check(self.lib.infgen_embedding_sum4(_lib.ptr(mt), _lib.ptr(mtok), mt.shape[0], _lib.ptr(w.type_pt_emb), _lib.ptr(mtype),
                                                  w.type_pt_emb.shape[0], _lib.ptr(w.polygon_type_emb), _lib.ptr(mpl),
                                                  w.polygon_type_emb.shape[0], _lib.ptr(w.light_pl_emb), _lib.ptr(mlight),
                                                  w.light_pl_emb.shape[0], mrows, _lib.ptr(self.x_pt), ops.stream),
                   'infgen_embedding_sum4')
        x_pt = self.x_pt
        K = 100
        if self._mg is None:
            cap = mrows * self._map_nbr_cap
            self._mg = dict(off=torch.zeros(mrows, device=dev, dtype=torch.int32),
                            cnt=torch.zeros(mrows, device=dev, dtype=torch.int32),
                            src=torch.zeros(cap, device=dev, dtype=torch.int32), raw=torch.zeros(cap, 4, device=dev),
                            rhat=torch.empty(cap, D, device=dev), total=torch.zeros(1, device=dev, dtype=torch.int32),
                            cap=cap, K=torch.empty(mrows, D, device=dev), V=torch.empty(mrows, D, device=dev),
                            Q=torch.empty(mrows, D, device=dev), AGG=torch.empty(mrows, D, device=dev))
        g = self._mg
        _lib.check(self.lib.infgen_map_graph(S0, M_cap, _lib.ptr(self.n_map), _lib.ptr(self.map_pos),
                                             _lib.ptr(self.map_orient), float(cfg.pl2pl_radius), K, _lib.ptr(g['off']),
                                             _lib.ptr(g['cnt']), _lib.ptr(g['src']), _lib.ptr(g['raw']),
                                             _lib.ptr(g['total']), g['cap'], ops.stream), 'infgen_map_graph')
        if not self._mg_checked:
            tot = int(g['total'].item())           # one host sync, first prologue only
            if tot > g['cap']:
                self._map_nbr_cap = (tot + mrows - 1) // mrows + 4
                self._mg = None
                return self._prologue(map_only=map_only)
            self._mg_checked = True
        fused = bool(self.flags['map_fuse'])
        # rhat rows of the pt <-> pt edges: fp32 by default; options['rhat_format'] = 1: the packed 24-bit form when both ends know
        # it (split Fourier kernel -> k_edge_fused), like the rollout's own edge sets (include/infgen_hip.h: InfgenOptions.rhat_format)
        eo = self._effective_options()
        r24 = fused and eo.rhat_format == 1 and eo.fourier_mode != 0
        if r24:
            _lib.check(self.lib.infgen_fourier_embed_r24(_lib.ptr(g['raw']), 3, _lib.ptr(g['total']), g['cap'], _lib.ptr(w.four_pt),
                                                         g['rhat'].data_ptr(), ops.stream), 'infgen_fourier_embed_r24')
        else:
            ops.fourier(g['raw'], 3, w.four_pt, g['rhat'], count_dev=g['total'], rows=g['cap'], normalize=True)
        for i in range(cfg.num_map_layers):
            if not fused:                                           # the unfused sequence (comparison)
                if 'U' not in g:
                    g.update(U=torch.empty(mrows, 8 * D, device=dev), Z=torch.empty(mrows, 8 * D, device=dev),
                             SIG=torch.empty(mrows, 8, device=dev))
                ops.attn_pre(x_pt, w.attn_pt[i], q=g['Q'], u=g['U'], k=g['K'], v=g['V'])
                ops.edge_attn(mrows, g['Q'], g['U'], g['K'], g['V'], g['off'], g['cnt'], g['src'], g['rhat'],
                              g['AGG'], g['Z'], g['SIG'])
                ops.attn_post(x_pt, w.attn_pt[i], g['AGG'], g['Z'], g['SIG'])
                continue
            # edge side with k_edge_fused: the absorbed query and the positional aggregate stay on chip (no U / Z arrays); the pre
            # part of layer i + 1 rides in the post launch of layer i (as in the agent layers)
            if i == 0:
                ops.attn_pre(x_pt, w.attn_pt[0], q=g['Q'], k=g['K'], v=g['V'])
            if r24:
                _lib.check(self.lib.infgen_edge_attn_fused_r24(mrows, _lib.ptr(g['Q']), _lib.ptr(w.attn_pt[i]), _lib.ptr(g['K']),
                                                               _lib.ptr(g['V']), _lib.ptr(g['off']), _lib.ptr(g['cnt']),
                                                               _lib.ptr(g['src']), g['rhat'].data_ptr(), _lib.ptr(g['AGG']),
                                                               ops.stream), 'infgen_edge_attn_fused_r24')
            else:
                ops.edge_attn(mrows, g['Q'], w.attn_pt[i], g['K'], g['V'], g['off'], g['cnt'], g['src'], g['rhat'],
                              g['AGG'], None, None, wide='fused')
            if i + 1 < cfg.num_map_layers:
                ops.attn_post_pre(x_pt, w.attn_pt[i], g['AGG'], None, None, w.attn_pt[i + 1], has_pos=False,
                                  q=g['Q'], k=g['K'], v=g['V'])
            else:
                ops.attn_post(x_pt, w.attn_pt[i], g['AGG'], None, None, has_pos=False)
        if map_only:
            return
        self._finish_prologue()

    def map_token_head(self, rows: torch.Tensor):
        """the map encoder's token_predict_head (map_decoder.py:119-121) on rows ``rows`` (int32, device) of this engine's map
        encoding ``x_pt`` [S0 * M_cap][128] - map scene ms's token m is row ms * M_cap + m - under this engine's arithmetic (the
        prologue's option block).  Runs after the prologue: x_pt is final once the map layers ran and nothing later writes it.
        -> logits [n][1024], top-10 indices [n][10] (int64, descending)"""
        with _lib.thread_options(self._effective_options()):
            return self.ops.map_token_head(self.x_pt, rows.to(self.device, torch.int32).contiguous(), self.w.map_head)

    def _prologue_with_given_map(self):
        """inference_no_map: x_pt comes from the caller (reference infgen_decoder.py:132-134)"""
        S0, M_cap, dev = self.S0, self.M_cap, self.device
        if self.x_pt is None:
            self.x_pt = torch.zeros(S0 * M_cap, D, device=dev)
        assert len(self._x_pt_override) == S0, 'one x_pt per distinct scene'
        for s, xp in enumerate(self._x_pt_override):
            M = self.hosts[s * self.copies]['M']
            self.x_pt[s * M_cap:s * M_cap + M] = xp.detach().to(dev, torch.float32)
        self._finish_prologue()

    def _finish_prologue(self):
        ops, w, cfg = self.ops, self.w, self.cfg
        x_pt = self.x_pt
        # map K/V of the six pt2a layers (bipartite source LayerNorm)
        for i in range(cfg.num_agent_layers):
            ops.attn_pre(x_pt, w.attn_m[i], use_src_ln=True, k=self.mapK[i], v=self.mapV[i])

        if self.insertion:
            self._alloc_insertion()
            for i in range(3):
                ops.attn_pre(x_pt, w.attn_pt2sa[i], use_src_ln=True, k=self.ins['mapK'][i], v=self.ins['mapV'][i])
        if self._ctx is None:
            self._build_ctx()
        self._refresh_opts()
        self._decoded_rows.zero_()
        st = ops.stream
        # column 0: edgeless chain, its K/V land in ring slot 0 (SURVEY a-Q3); then column 1's raw feature
        _lib.check(self.lib.infgen_raw_feature(C.byref(self._ctx), 0, st), 'raw_feature(0)')
        _lib.check(self.lib.infgen_decode_layers(C.byref(self._ctx), 0, 1, st), 'decode_layers(0)')
        _lib.check(self.lib.infgen_raw_feature(C.byref(self._ctx), 1, st), 'raw_feature(1)')
        self._prologue_done = True

    def rollout(self):
        """one full pass of the hot path over the batch: prologue + every decode step"""
        self._bc_host = None
        self._end_session()
        if (self._graph_all and not self.insertion and self._x_pt_override is None and self._mg_checked and self._init is not None
                and self._ctx is not None and not _lib.prof_active()):
            self._rollout_graph()                # (the first rollout of a batch runs eagerly: buffers, tables, edge capacities)
            return
        self.prologue()
        self.run()

    def _rollout_graph(self):
        """prologue + decode steps as ONE HIP-graph replay on the engine's own stream, fenced against the caller's stream on both
        sides (see _run_graph for why not on the caller's stream).  Nothing in a rollout without insertion depends on the host
        after the first one: the scene state is restored from device copies, every launch has static shapes."""
        cur = torch.cuda.current_stream(self.device)
        if getattr(self, '_gstream', None) is None:
            self._gstream = torch.cuda.Stream(device=self.device)
        gs = self._gstream
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            self._refresh_opts(groups=True)
            snap = bytes(self._ctx.opts)[:_lib.OPTIONS_VALUE_BYTES] + bytes([self._ctx.four_t_dt is not None])
            if self._wgraph is not None and snap != self._wgraph_opts:
                self._wgraph = None
            if self._wgraph is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=gs):
                    self.prologue()
                    self.run()
                self._wgraph, self._wgraph_opts = g, snap
            self._wgraph.replay()
            self._prologue_done = True
        cur.wait_stream(gs)

    # ------------------------------------------------------------------ scenario insertion (host-sequenced)
    def _alloc_insertion(self):
        if self.ins is not None:
            for k in ('n_new', 'active', 'inserted'):
                self.ins[k].zero_()
            self.ins['shape_all'].fill_(INVALID_SHAPE)
            self.ins['first_new'].fill_(self.A_cap)
            self.ins['inserted_rows'] = [[] for _ in range(self.S)]
            if self.seed_out is not None:
                for v in self.seed_out.values():
                    v.zero_()
            self._reset_insert_rules()
            return
        dev, S, rows, A_cap, M_cap, G = self.device, self.S, self.rows, self.A_cap, self.M_cap, self.G
        f = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.float32)
        i32 = lambda *shape: torch.zeros(*shape, device=dev, dtype=torch.int32)

        def ebuf(cap):
            cap = max(cap, 32)
            return dict(off=i32(S), cnt=i32(S), src=i32(cap), raw=f(cap, 4), rhat=f(cap, D), total=i32(1), cap=cap)
        ar = torch.arange(S, device=dev, dtype=torch.int32)
        self.ins = dict(
            occ=f(S, G), occ_emb=f(S, D), Kocc=[f(S, D) for _ in range(3)], Vocc=[f(S, D) for _ in range(3)],
            mapK=[f(self.S0 * M_cap, D) for _ in range(3)], mapV=[f(self.S0 * M_cap, D) for _ in range(3)],
            Ksa=[f(rows, D) for _ in range(3)], Vsa=[f(rows, D) for _ in range(3)],
            Kh=[f(rows, D) for _ in range(3)], Vh=[f(rows, D) for _ in range(3)],
            Xc=f(rows, D), AGG0=f(rows, D), Z0=f(rows, 8 * D), SIG0=f(rows, 8),
            XS=f(2 * S, D), QS=f(2 * S, D), US=f(2 * S, 8 * D), AGGS=f(2 * S, D), ZS=f(2 * S, 8 * D), SIGS=f(2 * S, 8),
            KN=f(2 * S, D), VN=f(2 * S, D),
            ea_s=ebuf(S * A_cap), em_s=ebuf(S * min(M_cap, 2048)), ea_h=ebuf(S * 24), em_h=ebuf(S * 128),
            occ_off=ar.clone(), occ_cnt=torch.ones(S, device=dev, dtype=torch.int32), occ_src=ar.clone(),
            dec3=i32(3 * S), n_new=i32(S), new_cell=i32(S), new_shape=f(S, 3),
            first_new=torch.full((S,), A_cap, device=dev, dtype=torch.int32), hv_ovr=f(S, 2), shape_all=torch.full((rows, 3), INVALID_SHAPE, device=dev),
            scene_base=(ar * A_cap).contiguous(), inserted_rows=[[] for _ in range(S)],
            groups=i32((rows + 15) // 16), n_groups=i32(1),
            host_dec=torch.zeros(3, S, dtype=torch.int32).pin_memory(),
            new_local=i32(S), prev_row=i32(S), prev_mask=i32(S), pend_row=i32(S), pend_mask=i32(S),
            hid=f(6, S, D), lg_state=f(S, 2), lg_type=f(S, 3), shape=f(S, 3), lg_pos=f(S, G), lg_heading=f(S, int(360.0 / self.cfg.angle_interval)),
            offset=f(S, 2), t1=f(S, D), t2=f(S, D), shp=f(S, D), struct=None,
            host_ev=torch.cuda.Event())
        # inserted | new_row | active back to back: one device-to-host copy per iteration hands all three over
        d3 = self.ins['dec3']
        self.ins['inserted'], self.ins['new_row'], self.ins['active'] = d3[:S], d3[S:2 * S], d3[2 * S:]
        self._reset_insert_rules()
        if self.seed_outputs and not self.cfg.use_grid_token:
            # use_grid_token = False: next_pos_rel_prob_seed and grid_*_occ_seed are None in the reference (agent_decoder.py:2376-2386)
            self.seed_out = dict(state=f(S, 11, self.cfg.num_decode_steps))
        elif self.seed_outputs:
            steps = self.cfg.num_decode_steps
            self.seed_out = dict(state=f(S, 11, steps), pos=f(S, 11, steps, G), occ_a=f(S, 11, steps, G), occ_p=f(S, 11, steps, G),
                                 occ_gt=f(S, 11, steps, G))
            sd, ap, dv = self.w.sd, self.w.ap, self.device
            if not hasattr(self.w, 'fwd_heads'):
                self.w.fwd_heads = {k: torch.from_numpy(np.ascontiguousarray(packing.pack_mlp_layer(sd, f'{ap}.{k}'), dtype=np.float32)).to(dv)
                                    for k in ('grid_index_head', 'grid_agent_occ_head', 'grid_pt_occ_head')}

    def _reset_insert_rules(self):
        """the device tables of the insertion rules, allocated once and brought back to the start of a rollout: the boxes of the
        rows that exist (the masked decision adds the appended rows'), an empty count log, and - with ``edge_clearance`` - the
        road-record table of the map in the buffers (two chords per EDGE token, the road masks' default; its size takes one count)"""
        rules = self.insert_rules
        if rules is None:
            return
        P = _lib.ptr
        if self._ins_rules is None:
            self._ins_rules = insertion_rules.device_tables(rules, self.S, self.S0, self.A_cap, self.G, self.cfg.num_decode_steps,
                                                            self.device)
            self.ins['struct'] = None
        k = self._ins_rules
        k['shape'].copy_(self._shape10.reshape(self.rows, 3))
        k['count_log'].zero_()
        if rules.edge_clearance is not None and self._ins_map_dirty:
            self._ins_map_dirty = False
            mtok, mtype = self._map_cat[0], self._map_cat[1]
            inmap = torch.arange(self.M_cap, device=self.device)[None] < self.n_map[:, None]
            cap = _round_up(max(2 * int(((mtype == 12) & inmap).sum(dim=1).max().item()), 1), 64)
            if k.get('records') is None or k['records'].shape[1] < cap:
                k['records'], k['n_records'] = torch.zeros(self.S0, cap, 8, device=self.device), torch.zeros(self.S0, device=self.device, dtype=torch.int32)
                self.ins['struct'] = None
            _lib.check(self.lib.infgen_road_records_from_map(P(self.map_pos), P(self.map_orient), P(mtype), P(mtok), P(self.n_map),
                                                             self.S0, self.M_cap, P(self._map_vocab), int(self._map_vocab.shape[0]), 2,
                                                             P(k['records']), int(k['records'].shape[1]), P(k['n_records']),
                                                             self.ops.stream), 'infgen_road_records_from_map')

    def _insert_rule_args(self):
        """the rule arguments of infgen_insert_seed_rules (None without insert_rules); the ctypes arrays are kept alive with them"""
        rules, k = self.insert_rules, self._ins_rules
        if rules is None:
            return None
        P = _lib.ptr
        ko = (C.c_float * 3)(*rules.ego_keepout) if rules.ego_keepout is not None else None
        edges, lanes, zones = rules.edge_clearance is not None, rules.near_lane is not None, rules.zones is not None
        return (rules.rule_bits, ko, rules.clearance or 0.0, rules.edge_clearance or 0.0, rules.near_lane[0] if lanes else 0.0,
                rules.lane_type_mask, P(k['records']) if edges else None, P(k['n_records']) if edges else None,
                int(k['records'].shape[1]) if edges else 0, P(self._map_cat[1]) if lanes else None,
                P(k['zones']) if zones else None, P(k['n_zones']) if zones else None, int(k['zones'].shape[1]) if zones else 0,
                self.copies, (C.c_int * 3)(*rules.types), P(k['max_agents']), P(k['shape']), P(k['static']), P(k['allowed']), k['W'],
                P(k['count']), P(k['live']), P(k['count_log']), int(k['count_log'].shape[1]))

    @property
    def insert_allowed(self):
        """[S, W] int32 words: the allowed cells of the last insertion iteration (``insertion_rules.cells_allowed_to_indices``)"""
        return None if self._ins_rules is None else self._ins_rules['allowed']

    @property
    def insert_allowed_count(self):
        """[S, steps] int32: the allowed cells at iteration 0 of every decode step (0 where no insertion ran: step 0)"""
        return None if self._ins_rules is None else self._ins_rules['count_log']

    def set_insert_zones(self, zones, n_zones=None):
        """rewrites the zone table of the insertion rules between rollouts or steps (the library keeps the pointers, not the
        contents): the same capacity Z, other circles or counts"""
        if self.insert_rules is None or self.insert_rules.zones is None:
            raise ValueError('set_insert_zones: the engine has no insert_rules with zones')
        z, n = insertion_rules.check_zones(zones, n_zones, n_scenes=self.S0)
        if z.shape != self.insert_rules.zones[0].shape:
            raise ValueError(f'set_insert_zones: the zone table is {self.insert_rules.zones[0].shape}, got {z.shape}')
        self.insert_rules = dataclasses_replace(self.insert_rules, zones=(z, n))
        if self._ins_rules is not None:
            self._ins_rules['zones'].copy_(torch.from_numpy(z))
            self._ins_rules['n_zones'].copy_(torch.from_numpy(n))

    def _ebuf_struct(self, e):
        b = _lib.EdgeBuf()
        P = _lib.ptr
        b.off, b.cnt, b.src, b.raw, b.rhat, b.total, b.cap = P(e['off']), P(e['cnt']), P(e['src']), P(e['raw']), P(e['rhat']), P(e['total']), e['cap']
        return b

    def _insertion_struct(self):
        """InfgenInsertion: the device arrays / weights of the sub-loop for the library's sequencing (include/infgen_hip.h)"""
        I, w, cfg, P = self.ins, self.w, self.cfg, _lib.ptr
        b = _lib.Insertion()
        for i in range(3):
            b.attn_occ2sa[i], b.attn_pt2sa[i], b.attn_a2sa[i] = P(w.attn_occ2sa[i]), P(w.attn_pt2sa[i]), P(w.attn_a2sa[i])
            b.Kocc[i], b.Vocc[i], b.mapK[i], b.mapV[i] = P(I['Kocc'][i]), P(I['Vocc'][i]), P(I['mapK'][i]), P(I['mapV'][i])
            b.Ksa[i], b.Vsa[i], b.Kh[i], b.Vh[i] = P(I['Ksa'][i]), P(I['Vsa'][i]), P(I['Kh'][i]), P(I['Vh'][i])
        H = w.heads
        Pn = lambda k: P(H[k]) if k in H else None         # (the heads of the other variants: NULL)
        b.four_a2sa, b.four_pt2sa = P(w.four_a2sa), P(w.four_pt2sa)
        b.head_state, b.head_type, b.head_shape = P(H['seed_state_predict_head']), P(H['seed_type_predict_head']), P(H['seed_shape_predict_head'])
        b.head_pos, b.head_heading = Pn('seed_pos_rel_token_predict_head'), Pn('seed_heading_rel_token_predict_head')
        b.head_offset, b.occ_embed = Pn('seed_offset_xy_predict_head'), Pn('seed_agent_occ_embed')
        b.head_pos_xy, b.head_heading_theta = Pn('seed_pos_rel_xy_predict_head'), Pn('seed_heading_rel_theta_predict_head')
        b.no_grid_token, b.no_head_token = int(not cfg.use_grid_token), int(not cfg.use_head_token)
        b.shape_emb, b.type_a_emb, b.f_seed = P(w.shape_emb), P(w.type_a_emb), P(self.f_seed)
        b.occ, b.occ_emb, b.Xc = P(I['occ']), P(I['occ_emb']), P(I['Xc'])
        b.zero_agg, b.zero_z, b.zero_sig = P(I['AGG0']), P(I['Z0']), P(I['SIG0'])
        for k in ('XS', 'QS', 'US', 'AGGS', 'ZS', 'SIGS', 'KN', 'VN'):
            setattr(b, k, P(I[k]))
        b.ea_s, b.em_s, b.ea_h, b.em_h = (self._ebuf_struct(I[k]) for k in ('ea_s', 'em_s', 'ea_h', 'em_h'))
        b.occ_off, b.occ_cnt, b.occ_src = P(I['occ_off']), P(I['occ_cnt']), P(I['occ_src'])
        for k in ('active', 'n_new', 'inserted', 'new_row', 'new_cell', 'new_local', 'new_shape', 'prev_row', 'prev_mask', 'pend_row',
                  'pend_mask', 'hv_ovr', 'shape_all', 'hid', 'lg_state', 'lg_type', 'shape', 'lg_pos', 'lg_heading', 'offset', 't1', 't2', 'shp'):
            setattr(b, k, P(I[k]))
        b.host_dec = I['host_dec'].data_ptr()
        b.r_seed, b.r_a2sa, b.r_pl2sa, b.angle_interval = float(cfg.pl2seed_radius), float(cfg.a2sa_radius), float(cfg.pl2sa_radius), float(cfg.angle_interval)
        b.n_heading, b.force_enter, b.insert_k, b.max_new = int(360.0 / cfg.angle_interval), int(self.force_enter), self.insert_k, 10
        b.insert_temperature, b.insert_top_p = self.insert_temperature, self.insert_top_p
        if self.insert_rules is not None:
            b.max_new = self.insert_rules.per_step
        return b

    def _insert_step(self, t: int):
        """the insertion sub-loop of decode step t (reference agent_decoder.py:1773-2105).  The launches of an
        iteration are sequenced by the library (infgen_insert_seed -> decisions -> infgen_insert_heading: two C calls instead of
        ~60 Python-level launches); the data-dependent loop stays here.  A generator: once per iteration the per-scene decisions
        (inserted?, which row, still active?) arrive in pinned host memory asynchronously and the event of that copy is yielded -
        ``run`` just waits for it, ``rollout_many`` sequences other engines' streams meanwhile."""
        lib, I, S = self.lib, self.ins, self.S
        ctx = C.byref(self._ctx)
        if I.get('struct') is None:
            I['struct'] = self._insertion_struct()
        blk = C.byref(I['struct'])
        I['first_new'].copy_(self.n_agents)
        I['active'].fill_(1)
        I['n_new'].zero_()
        riders = riders_h = h_ready = False
        rule_args = self._insert_rule_args()
        hd = I['host_dec'].numpy()
        for it in range(10):
            st = self.ops.stream
            u = _lib.ptr(self._insert_u[t, it]) if self._insert_u is not None else None
            if rule_args is None:
                _lib.check(lib.infgen_insert_seed(ctx, blk, t, it, int(riders), u, st), 'infgen_insert_seed')
            else:
                _lib.check(lib.infgen_insert_seed_rules(ctx, blk, t, it, int(riders), u, *rule_args, st), 'infgen_insert_seed_rules')
            ev = I['host_ev']
            ev.record(torch.cuda.current_stream(self.device))
            yield ev
            ev.synchronize()
            ins_host = hd[0].copy()
            if (ins_host < 0).any():
                full = np.nonzero(ins_host < 0)[0]
                raise InsertionHeadroomError(
                    f'decode step {t}: scene(s) {full[:8].tolist()} have used all {self.A_cap} agent rows '
                    f'({int(self.n_agents[int(full[0])].item())} agents) and the seed head asks for another insertion; '
                    f're-run with a larger insert_headroom (rows per scene <= {self.lib.infgen_layout_query(_lib.Q_MAX_AGENTS)})',
                    needed=self.A_cap)
            ins_host = ins_host > 0
            if not ins_host.any():
                if self.insert_k > 1 and hd[2].any():
                    riders = False          # sampled cells were occupied everywhere: the iteration is spent, active scenes draw again
                    continue
                break
            ins_idx_host = np.nonzero(ins_host)[0]
            nr_host = hd[1][ins_idx_host].astype(np.int64)
            for s_i, r_i in zip(ins_idx_host, nr_host):
                I['inserted_rows'][int(s_i)].append((int(r_i), t))
            if self.seed_out is not None:
                # slot = the scene's insertion count of this step after the append (agent_decoder.py:2099-2105)
                ops, w = self.ops, self.w
                ins = torch.from_numpy(ins_idx_host.astype(np.int64)).to(self.device)
                so, slot = self.seed_out, I['n_new'][ins].long()
                XS_in = I['XS'][:S][ins].contiguous()
                so['state'][ins, slot, t] = torch.softmax(I['lg_state'][ins], dim=-1)[:, -1]
                if 'pos' in so:                  # (the grid's outputs: not recorded for use_grid_token = False)
                    so['pos'][ins, slot, t] = torch.softmax(I['lg_pos'][ins], dim=-1)
                    so['occ_a'][ins, slot, t] = ops.mlp_layer(XS_in, w.fwd_heads['grid_agent_occ_head'], D, self.G)
                    so['occ_p'][ins, slot, t] = ops.mlp_layer(XS_in, w.fwd_heads['grid_pt_occ_head'], D, self.G)
                    so['occ_gt'][ins, slot, t] = I['occ'][ins]
            # heading stage of the rows just appended; the rows of the previous heading stage ride along (their K / V of the motion
            # layers 0..2 are refreshed) - not necessarily the previous iteration's: an occupied sampled cell spends iterations
            _lib.check(lib.infgen_insert_heading(ctx, blk, t, int(h_ready), int(riders_h and h_ready), self.ops.stream), 'infgen_insert_heading')
            h_ready = True
            riders = riders_h = True

    def _build_ctx(self):
        cfg, w = self.cfg, self.w
        c = _lib.Rollout()
        c.S, c.A_cap, c.T, c.M_cap, c.W, c.ring, c.R = self.S, self.A_cap, self.T, self.M_cap, self.W, self.ring, self.R
        c.token_size, c.grid_size, c.num_layers = cfg.token_size, self.G, cfg.num_agent_layers
        c.force_valid, c.store_logits = int(self.force_valid), int(self.store_logits)
        c.no_grid_token, c.no_state_token = int(not cfg.use_grid_token), int(not cfg.use_state_token)
        c.r_map, c.r_agent = float(cfg.pl2a_radius), float(cfg.a2a_radius)
        P = _lib.ptr
        c.n_agents, c.n_map, c.av_index = P(self.n_agents), P(self.n_map), P(self.av)
        c.pos, c.head, c.state, c.token, c.grid = P(self.pos), P(self.head), P(self.state), P(self.token), P(self.gridtok)
        c.tmask, c.imask, c.catflag, c.type, c.bos = P(self.tmask), P(self.imask), P(self.catflag), P(self.atype), P(self.bos)
        c.map_pos, c.map_orient = P(self.map_pos), P(self.map_orient)
        c.map_scene = P(self.map_scene)
        c.tap_x = P(self.tap_x)
        for i in range(cfg.num_agent_layers):
            c.attn_t[i], c.attn_m[i], c.attn_a[i] = P(w.attn_t[i]), P(w.attn_m[i]), P(w.attn_a[i])
            c.ringK[i], c.ringV[i], c.mapK[i], c.mapV[i] = P(self.ringK[i]), P(self.ringV[i]), P(self.mapK[i]), P(self.mapV[i])
        c.four_t, c.four_m, c.four_a, c.four_xa = P(w.four_t), P(w.four_m), P(w.four_a), P(w.four_xa)
        c.fusion_pack, c.tok_head_pack, c.st_head_pack = P(w.fusion), P(w.tok_head), P(w.st_head)
        c.tok_tab, c.grid_tab, c.state_emb = P(self.tok_tab), P(self.grid_tab), P(w.state_a_emb)
        c.cat_agent, c.cat_seed, c.vocab, c.grid_xy = P(self.cat_agent), P(self.cat_seed), P(self.vocab), P(self.grid_xy)
        c.X, c.Q, c.U, c.Ka, c.Va, c.AGG, c.Z, c.SIG = (P(self.X), P(self.Q), P(self.U), P(self.Ka), P(self.Va),
                                                          P(self.AGG), P(self.Z), P(self.SIG))
        for name, field in (('t', 'et'), ('m', 'em'), ('a', 'ea')):
            e, b = self.edges[name], getattr(c, field)
            b.off, b.cnt, b.src, b.raw, b.rhat, b.total, b.cap = (P(e['off']), P(e['cnt']), P(e['src']), P(e['raw']),
                                                                   P(e['rhat']), P(e['total']), e['cap'])
        c.raw2, c.cat, c.fus_in, c.tmp1, c.tmp2 = P(self.raw2), P(self.cat), P(self.fus_in), P(self.tmp1), P(self.tmp2)
        c.next_token, c.next_state, c.logits = P(self.next_token), P(self.next_state), P(self.logits)
        c.teacher_token, c.teacher_state = P(self.teacher_token), P(self.teacher_state)
        c.teacher_grid = P(self.teacher_grid)
        c.teacher_pos, c.teacher_head = P(self.teacher_pos), P(self.teacher_head)
        c.replay_row = P(self.replay_row)
        c.pred_traj, c.pred_head, c.pred_state = P(self.pred_traj), P(self.pred_head), P(self.pred_state)
        if self.insertion:
            c.first_new, c.hv_ovr = P(self.ins['first_new']), P(self.ins['hv_ovr'])
        c.sample_k, c.sample_u, c.logits_scratch = self.sample_k, P(self.sample_u), P(self.logits_scratch)
        c.token_logprob = P(self.token_logprob)
        c.sample_logprob = P(self.sample_logprob)
        self._ctx = c
        self._apply_sampling()
        self._apply_token_masks(validate=False)      # (validated below, once the kernel switches and the scratch are in place)
        self._refresh_opts()
        _lib.check(self.lib.infgen_rollout_validate(C.byref(c)), 'infgen_rollout_validate')      # (the packs' headers, looked at afresh)

    def _refresh_opts(self, groups: bool = False):
        """the context carries its own kernel switches (InfgenRollout.opts, re-entrant): explicit ``options`` of this engine,
        otherwise a snapshot of the library's process-wide defaults (infgen_set_*) taken at every prologue / run"""
        o = self._ctx.opts
        _lib.check(self.lib.infgen_get_options(C.byref(o)), 'infgen_get_options')
        for k, v in (self.options or {}).items():
            setattr(o, k, int(v))
        o.use = 1
        if (int(o.gemm_terms) == 2) != (self.w.operand_bits == 8):
            raise ValueError(f'gemm_terms = {int(o.gemm_terms)} with packs of {self.w.operand_bits}-bit operands: the bf16 mode '
                             '(gemm_terms = 2) takes PackedWeights(..., operand_bits=8), every other mode operand_bits=11')
        # the temporal edges' time-gap input as a lookup of its r_t_emb branch (include/infgen_hip.h: four_t_dt), built once per
        # weight pack and arithmetic; INFGEN_NO_DT_TAB=1: evaluated per edge as before
        self._ctx.four_t_dt = None
        if o.fourier_mode != 0 and self.flags['dt_table']:
            self._ctx.four_t_dt = _lib.ptr(self.w.time_gap_table(self.lib, int(o.gemm_terms), self.ops.stream))
        # does a step read logits from memory?  The library's own rules (infgen_heads_sample_fused for a sampled step,
        # infgen_heads_logprob_fused for a greedy one with token_logprob) - every step of a rollout has the same rows, beam and
        # switches, so either all of them stay inside the heads kernel or none does
        if self.sample_k > 1:
            in_kernel = self.lib.infgen_heads_sample_fused(int(o.attn_mode), self.rows, self.sample_k)
        else:
            in_kernel = self.token_logprob is None or self.lib.infgen_heads_logprob_fused(int(o.attn_mode), self.rows)
        if not in_kernel and self.logits is None and self.logits_scratch is None:
            self.logits_scratch = torch.zeros(self.rows, self.cfg.token_size, device=self.device)
            self._ctx.logits_scratch = _lib.ptr(self.logits_scratch)
            self._drop_graphs()          # (a captured graph holds the old pointers)
        o.row_groups = o.n_row_groups = None
        o.row_group_margin = 0
        if groups and self.insertion and self.ins is not None and self.flags['row_groups']:
            # rows are padded to A_cap per scene: the split node kernels and the edge kernels visit only the 16-row groups
            # that hold agents (or may receive one of the <= 10 rows a step appends)
            o.row_groups, o.n_row_groups, o.row_group_margin = _lib.ptr(self.ins['groups']), _lib.ptr(self.ins['n_groups']), 10

    # ------------------------------------------------------------------ rollout
    def run(self, t0: int = 0, t1: Optional[int] = None):
        for _ in self.run_gen(t0, t1):      # (the generator waits for each event itself when it is resumed)
            pass

    def run_gen(self, t0: int = 0, t1: Optional[int] = None):
        """``run`` as a generator: yields a ``torch.cuda.Event`` wherever the host needs a result of the device (the insertion
        sub-loop's per-iteration decisions) - everything up to the event is already enqueued on the current stream.  Lets one
        host thread keep several engines on several streams busy (``rollout_many``)."""
        if not self._prologue_done:
            self.prologue()
        t1 = self.cfg.num_decode_steps if t1 is None else t1
        self._refresh_opts(groups=True)        # (the group list is rebuilt on the device at every decode step below)
        if not self.insertion:
            # a replay runs what was captured: fall back to the eager sequence while per-kernel profiling is on (events are not
            # part of the graph) and re-capture when the context's kernel switches changed since the capture
            if self.use_graph and (t0, t1) == (0, self.cfg.num_decode_steps) and not _lib.prof_active():
                self._run_graph(t0, t1)
                return
            _lib.check(self.lib.infgen_rollout_run(C.byref(self._ctx), t0, t1, self.ops.stream), 'infgen_rollout_run')
            return
        for t in range(t0, t1):
            yield from self._step_gen(t)

    def _step_gen(self, t: int):
        """decode step t as the host sequences it (scenario insertion on, or a closed-loop session stepping an engine without
        it): the row-group refresh, the step's insertion sub-loop, the motion stage.  A generator like ``run_gen``, which drives it
        for every step; ``ClosedLoopSession.advance`` drives it for one.  ``_refresh_opts(groups=True)`` comes first (once)."""
        if not self.insertion:
            self.step(t)
            return
        lib, I = self.lib, self.ins
        use_groups = bool(self._ctx.opts.row_groups)
        if use_groups:
            _lib.check(lib.infgen_active_row_groups(_lib.ptr(self.n_agents), self.S, self.A_cap, 10,
                                                    _lib.ptr(I['groups']), _lib.ptr(I['n_groups']), self.ops.stream),
                       'infgen_active_row_groups')
        if t > 0:
            yield from self._insert_step(t)
            live_shapes = [k['shape'] for k, on in ((self._coll, self.avoid_collisions), (self._road, self.stay_on_road),
                                                        (self._signal, self.obey_signals)) if on is not None]
            if live_shapes:
                # the boxes of the rows this step appended (they are obstacles, and get sets, from the next step on): one mask, merged
                # into the shape array of every per-step mask kernel that is on
                S, A_cap = self.S, self.A_cap
                new = ((self._coll_cols >= I['first_new'][:, None]) & (self._coll_cols < self.n_agents[:, None]))[..., None]
                for shp in live_shapes:
                    cs = shp.view(S, A_cap, 3)
                    cs.copy_(torch.where(new, I['shape_all'].view(S, A_cap, 3), cs))
        self._decoded_rows.add_(self.n_agents.sum())       # A_t: rows decoded at this step, incl. the inserted ones
        tight = use_groups and self.flags['row_groups_tight']
        if tight:
            # the step's insertions are done: the motion stage runs on exactly the rows that hold agents now - the ten rows of
            # head-room the sub-loop's lists carry put one more 16-row group per scene into 60 % of the node / edge launches
            _lib.check(lib.infgen_active_row_groups(_lib.ptr(self.n_agents), self.S, self.A_cap, 0,
                                                    _lib.ptr(I['groups']), _lib.ptr(I['n_groups']), self.ops.stream),
                       'infgen_active_row_groups')
            self._ctx.opts.row_group_margin = 0
        self.step(t)
        if tight:
            self._ctx.opts.row_group_margin = 10

    def session(self, pose: str = 'token', controlled=None):
        """a closed-loop stepping session on this engine (infgen_amd/closed_loop.py): the flagged rows take a command
        per decode step - a token id or a target pose, from device tensors - instead of a plan known up front.  ``controlled``:
        None (the rows ``replay=`` flagged), 'ego' or a bool tensor [S, rows]; ``pose``: 'token' (the stored pose is the
        commanded / matched token's integration) or 'exact' (the commanded pose itself is stored)."""
        from .closed_loop import ClosedLoopSession
        return ClosedLoopSession(self, pose=pose, controlled=controlled)

    def observe_rows(self, c: int, rows=None, neighbors: int = 8, radius: float = float('inf'), map_tokens: int = 0,
                     map_radius: float = float('inf'), out=None) -> Dict[str, torch.Tensor]:
        """the agent-frame observation of stored column ``c`` ("observations" of include/infgen_hip.h): for every row of
        ``rows`` - int tensor [N] of global rows s * A_cap + i, None: all S * A_cap in order - ``self_feat`` [N, 8], the
        ``neighbors`` nearest live agents within ``radius`` (``nbr_feat`` [N, K, 10], ``nbr_index`` [N, K], ``nbr_count`` [N]) and the
        ``map_tokens`` nearest map tokens within ``map_radius`` (``map_feat`` [N, Km, 6], ``map_index`` [N, Km], ``map_count`` [N]),
        in the row's own frame.  One launch of ``infgen_observe_rows`` on the engine's own buffers and the current stream, no host
        read; ``dt`` is the step length the step scores use by default.  ``out``: an earlier result of the same sizes, whose
        tensors are written again instead of new ones.  The scene is only read (``n_agents`` on the device, at launch), so an
        engine with scenario insertion observes like any other."""
        if getattr(self, '_shape10', None) is None:
            raise ValueError('observe_rows needs the rows\' shapes: this engine has no shape array')
        observe.check_params(c, self.T, constraints.STEP_SECONDS, neighbors, radius, map_tokens, map_radius, True)
        observe.check_rows(rows)
        r = None if rows is None else rows.to(self.device, torch.int32).contiguous()
        N = self.S * self.A_cap if r is None else int(r.numel())
        res = observe.outputs(N, int(neighbors), int(map_tokens), self.device, out)
        observe.launch(self.lib, self.ops.stream, self.pos, self.head, self.state, self.n_agents, self.atype, self._shape10, c,
                       constraints.STEP_SECONDS, self.map_pos, self.map_orient, self._map_cat[1], self.n_map, self.copies, r,
                       neighbors, radius, map_tokens, map_radius, res)
        return res

    def idm_command(self, c: int, ctl_row=None, routes=None, n_points=None, v_des=None, out=None, **params) -> Dict[str, torch.Tensor]:
        """the target poses of rule-based controlled rows from stored column ``c >= 1`` ("IDM commands" of
        include/infgen_hip.h): every row of ``ctl_row`` ([S, A_cap] uint8 / bool device tensor, None: ``replay_row``) that is live,
        of a ruled type and has a route follows that route under the intelligent-driver law behind the nearest agent ahead of it.
        ``routes`` [S0][A][P][2] / ``n_points`` [S0][A]: the routes (``constraints.routes_from_logged`` makes them from a log); the
        engine keeps tables of its own for them, built by ``infgen_route_records`` and rebuilt only when the routes change (the same
        array objects as at the last call count as unchanged: pass new arrays for new routes).
        Without ``routes`` the tables of ``follow_routes`` are read.  ``v_des`` [S0][A]: the rows' own desired speeds where > 0;
        ``params``: the keys of ``controllers.check_idm``.  One launch of ``infgen_idm_command`` on the engine's own buffers and the
        current stream, no host read.  -> dict(``pose`` [S, A_cap, 3] - written for ruled rows only, so ``out['pose']`` may hold a
        fill -, ``state`` [S * A_cap, 8], ``lead`` [S * A_cap]); ``out``: an earlier result, written again.  The scene is only read
        (``n_agents`` on the device, at launch): rows scenario insertion appends have no route, so they are never ruled, and count
        as obstacles once live."""
        if getattr(self, '_shape10', None) is None:
            raise ValueError('idm_command needs the rows\' shapes: this engine has no shape array')
        if not 1 <= int(c) < self.T:
            raise ValueError(f'idm_command: column {c} outside 1 .. {self.T - 1}')
        conf = controllers.check_idm(params)
        if routes is not None:
            if n_points is None:
                raise ValueError('idm_command: routes come with n_points')
            tab = self._idm_tables(routes, n_points)
        elif self._route is not None:
            tab = self._route
        else:
            raise ValueError('idm_command: no routes - pass routes= and n_points= (constraints.routes_from_logged makes them from '
                             'a log) or build the engine with follow_routes=')
        if ctl_row is None:
            ctl_row = self.replay_row
            if ctl_row is None:
                raise ValueError('idm_command: no controlled rows - pass ctl_row= or build the engine with replay=')
        if tuple(ctl_row.shape) != (self.S, self.A_cap):
            raise ValueError(f'idm_command: ctl_row must be {(self.S, self.A_cap)}, got {tuple(ctl_row.shape)}')
        ctl_row = ctl_row.to(self.device, torch.uint8).contiguous()
        vd = None
        if v_des is not None:
            vd = torch.as_tensor(v_des, dtype=torch.float32)
            if vd.dim() != 2 or vd.shape[0] != self.S0 or vd.shape[1] > self.A_cap:
                raise ValueError(f'idm_command: v_des must be [{self.S0}][<= {self.A_cap}], got {tuple(vd.shape)}')
            if vd.shape[1] < self.A_cap:
                vd = torch.nn.functional.pad(vd, (0, self.A_cap - vd.shape[1]))
            vd = vd.to(self.device).contiguous()
        res = controllers.idm_buffers(self.S, self.A_cap, self.device, out)
        pose = None if out is None else out.get('pose')
        if pose is None:
            pose = torch.zeros(self.S, self.A_cap, 3, device=self.device)
        elif tuple(pose.shape) != (self.S, self.A_cap, 3) or pose.dtype != torch.float32 or not pose.is_contiguous() \
                or pose.device != self.device:
            raise ValueError(f'idm: out[\'pose\'] must be a contiguous float32 tensor of shape {(self.S, self.A_cap, 3)} on {self.device}')
        controllers.launch(self.lib, self.ops.stream, self.pos, self.head, self.state, self.n_agents, self.atype, self._shape10, ctl_row,
                           c, tab['records'], tab['total'], self.copies, vd, conf, pose, res)
        res['pose'] = pose
        return res

    def _idm_tables(self, routes, n_points):
        """the engine's own route tables for ``idm_command(routes=...)``: uploaded and their records rebuilt only when the routes
        differ from the ones the tables were built from.  The same two array objects as last time are taken as unchanged
        routes without looking inside - the loop of ``run_idm`` costs no host work per step -, so new routes come as new arrays"""
        tab = getattr(self, '_idm_route', None)
        if tab is not None and routes is tab['src'][0] and n_points is tab['src'][1]:
            return tab
        r, n = constraints.route_arrays(routes, n_points, n_scenes=self.S0, a_cap=self.A_cap, what='idm_command')
        if tab is not None and tab['host'][0].shape == r.shape and np.array_equal(tab['host'][0], r, equal_nan=True) \
                and np.array_equal(tab['host'][1], n):
            tab['src'] = (routes, n_points)
            return tab
        P, A = int(r.shape[2]), int(r.shape[1])
        if tab is None or tab['P'] != P:
            dev = self.device
            tab = dict(P=P, routes=torch.zeros(self.S0, self.A_cap, P, 2, device=dev),
                       n_points=torch.zeros(self.S0, self.A_cap, dtype=torch.int32, device=dev),
                       records=torch.zeros(self.S0, self.A_cap, P - 1, 8, device=dev), total=torch.zeros(self.S0, self.A_cap, device=dev))
        full, cnt = np.zeros((self.S0, self.A_cap, P, 2), np.float32), np.zeros((self.S0, self.A_cap), np.int32)
        full[:, :A], cnt[:, :A] = r, n
        tab['routes'].copy_(torch.from_numpy(full))
        tab['n_points'].copy_(torch.from_numpy(cnt))
        _lib.check(self.lib.infgen_route_records(_lib.ptr(tab['routes']), _lib.ptr(tab['n_points']), self.S0, self.A_cap, P,
                                                 _lib.ptr(tab['records']), _lib.ptr(tab['total']), self.ops.stream), 'infgen_route_records')
        tab['host'], tab['src'] = (r.copy(), n.copy()), (routes, n_points)
        self._idm_route = tab
        return tab

    def _run_graph(self, t0, t1):
        """the decode steps as a HIP-graph replay.  Replays launched into the LEGACY DEFAULT stream fault now and then on this
        ROCm 7.2 stack (memory access fault inside the second or a later replay, 2 of 4 runs; never with AMD_SERIALIZE_KERNEL=3, never
        on a created stream: profiles/r03_graph_replay_fault.log), so capture and replay always run on a stream of the engine's
        own, fenced against the caller's stream on both sides."""
        cur = torch.cuda.current_stream(self.device)
        if getattr(self, '_gstream', None) is None:
            self._gstream = torch.cuda.Stream(device=self.device)
        gs = self._gstream
        gs.wait_stream(cur)
        with torch.cuda.stream(gs):
            snap = bytes(self._ctx.opts)[:_lib.OPTIONS_VALUE_BYTES] + bytes([self._ctx.four_t_dt is not None])
            if self._graph is not None and snap != self._graph_opts:
                self._graph = None
            if self._graph is None and not getattr(self, '_graph_warm', False):
                # the first rollout runs eagerly: kernels are loaded lazily at their first launch, which must not happen
                # inside a capture
                self._graph_warm = True
                _lib.check(self.lib.infgen_rollout_run(C.byref(self._ctx), t0, t1, self.ops.stream), 'infgen_rollout_run')
            else:
                if self._graph is None:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=gs):
                        _lib.check(self.lib.infgen_rollout_run(C.byref(self._ctx), t0, t1, self.ops.stream), 'infgen_rollout_run')
                    self._graph = g
                    self._graph_opts = snap
                self._graph.replay()
        cur.wait_stream(gs)

    def edge_totals(self):
        """(temporal, map, agent) edge counts of the last decode step's edge sets (one host sync)"""
        return tuple(int(self.edges[k]['total'].item()) for k in ('t', 'm', 'a'))

    def scenes_at_row_cap(self) -> int:
        """scenes whose insertion head-room ran out (n_agents == A_cap): their later insertions were dropped - give the engine a
        larger ``insert_headroom`` (A_cap <= 1024) to avoid that"""
        return int((self.n_agents >= self.A_cap).sum().item()) if self.insertion else 0

    def step(self, t: int):
        _lib.check(self.lib.infgen_decode_step(C.byref(self._ctx), t, self.ops.stream), 'infgen_decode_step')

    @property
    def branch_bad(self) -> torch.Tensor:
        """[1] int32 on the device: the entries of the last ``branch`` call's parent vector that broke the contract and were read
        as the identity (0 before the first call)"""
        if self._branch_bad is None:
            self._branch_bad = torch.zeros(1, device=self.device, dtype=torch.int32)
        return self._branch_bad

    def branch(self, parent, t: int):
        """branching rollouts ("branching" of include/infgen_hip.h): every slot s with ``parent[s] != s`` becomes a
        clone of slot ``parent[s]`` as of the boundary in front of decode step ``t`` (0 .. steps) - stored columns, the temporal
        K / V rings, the pending raw feature, ``pred_*`` and the logs of the steps that ran.  One launch of ``infgen_branch_scenes``
        on the current stream.  Each slot keeps its own uniforms, temperature, constraints, replay flags and commands, so a clone
        diverges from its parent at the next draw.  ``parent``: int [S] or [S0, copies], global slot indices; source and
        destination in one copy group, every source a fixed point (``infgen_amd.branching`` makes such vectors).  A device tensor
        is taken as it is - stream-ordered, no host read; entries that break the contract are treated as the identity and counted
        into ``branch_bad`` (a device int the call zeroes first).  A host tensor or array is checked here (``ValueError`` naming
        the first bad entry).  Eager: captured graphs stay as they are (``run(t0, t1)`` over a partial range is eager too).
        Refused on an engine with scenario insertion (row counts, types and shapes differ between the copies) and before
        ``prologue()``; with ``copies == 1`` only the identity is valid (a host vector is refused; the entries of a device one are
        all counted into ``branch_bad``)."""
        from . import branching
        if self.insertion:
            raise ValueError('branch: engines with scenario insertion cannot branch (row counts, types and shapes differ between '
                             'the copies): left out')
        if self._ctx is None or not self._prologue_done:
            raise RuntimeError('branch: run prologue() first - there is no rollout state to clone yet')
        steps = self.cfg.num_decode_steps
        if not 0 <= int(t) <= steps:
            raise ValueError(f'branch: t = {t} is outside 0 .. {steps}')
        p = parent if isinstance(parent, torch.Tensor) else torch.as_tensor(np.asarray(parent))
        if p.is_floating_point() or p.dtype == torch.bool:
            raise ValueError('parent holds integer slot indices')
        if tuple(p.shape) not in ((self.S,), (self.S0, self.copies)):
            raise ValueError(f'parent: expected shape {(self.S,)} or {(self.S0, self.copies)}, got {tuple(p.shape)}')
        if not p.is_cuda:
            if self.copies == 1 and not torch.equal(p.reshape(-1).long(), torch.arange(self.S)):
                raise ValueError('branch: an engine with copies == 1 has no copy to clone - only the identity is a valid parent')
            p = torch.from_numpy(branching.check_parent(p.numpy(), self.S0, self.copies))
        p = p.to(self.device, torch.int32).contiguous().view(-1)
        _lib.check(self.lib.infgen_branch_scenes(C.byref(self._ctx), int(t), _lib.ptr(p), _lib.ptr(self.branch_bad), self.ops.stream),
                   'infgen_branch_scenes')
        self._rollout_lp = self._rollout_slp = None

    # ------------------------------------------------------------------ snapshots
    def _check_snapshot_call(self, what: str, t: int):
        if self.insertion:
            raise ValueError(f'{what}: engines with scenario insertion are left out (row counts, types and shapes differ between '
                             'the copies, as for branch)')
        if self._ctx is None or not self._prologue_done:
            raise RuntimeError(f'{what}: run prologue() first - there is no rollout state yet')
        steps = self.cfg.num_decode_steps
        if not 0 <= int(t) <= steps:
            raise ValueError(f'{what}: t = {t} is outside 0 .. {steps}')

    def snapshot_buffer(self, n: Optional[int] = None):
        """an empty ``Snapshot`` with room for ``n`` slots (default: all) at any decode step - for ``snapshot(t, out=...)``"""
        from . import snapshots
        self._check_snapshot_call('snapshot_buffer', 0)
        return snapshots.allocate(self, self.S if n is None else int(n))

    def snapshot(self, t: int, slots=None, out=None):
        """snapshots ("snapshots" of include/infgen_hip.h): the decode state of the named slots as of the boundary in
        front of decode step ``t`` (0 .. steps) -> a ``snapshots.Snapshot`` on the device: what ``branch`` copies between slots
        (stored columns, the temporal K / V rings, the pending raw feature, ``pred_*``, the logs of the steps that ran, the
        step-score block), one entry per slot.  One launch of ``infgen_snapshot_scenes`` on the current stream; the engine is not
        written.  ``slots``: None (all), a host list (checked here: ``ValueError`` naming the first bad entry) or a device int
        tensor [n], taken as it is - stream-ordered, no host read; a slot out of range leaves an entry ``restore`` skips and is
        counted into ``snapshot_bad``.  ``out``: a ``Snapshot`` of this engine with enough capacity (``snapshot_buffer()``) to
        reuse instead of allocating - an entry is about ``2 * layers * ring * A_cap * 512`` bytes.  Refused on an engine with
        scenario insertion and before ``prologue()``."""
        from . import snapshots
        self._check_snapshot_call('snapshot', t)
        t = int(t)
        host = None
        if slots is None:
            host = np.arange(self.S, dtype=np.int32)
            sl = torch.arange(self.S, device=self.device, dtype=torch.int32)
        elif isinstance(slots, torch.Tensor) and slots.is_cuda:
            if slots.is_floating_point() or slots.dtype == torch.bool or slots.dim() != 1:
                raise ValueError('slots: a device tensor holds integer slot indices, shape [n]')
            if slots.numel() > 65535:
                raise ValueError('slots: at most 65535 entries')
            sl = slots.to(self.device, torch.int32).contiguous()
        else:
            host = snapshots.check_slots(slots.numpy() if isinstance(slots, torch.Tensor) else slots, self.S)
            sl = torch.from_numpy(host).to(self.device)
        n, need = int(sl.numel()), snapshots.entry_bytes(self, t)
        if out is None:
            out = snapshots.allocate(self, n, t)
        else:
            if not isinstance(out, snapshots.Snapshot) or out.signature != snapshots.signature(self):
                raise ValueError('snapshot: out= is no Snapshot of this engine\'s layout')
            if out.capacity < n or out.stride < need:
                raise ValueError(f'snapshot: out= holds {out.capacity} entries of {out.stride} bytes, {n} of {need} are needed')
        _lib.check(self.lib.infgen_snapshot_scenes(C.byref(self._ctx), t, _lib.ptr(sl), n, _lib.ptr(out.buf), out.stride,
                                                   _lib.ptr(out.head), _lib.ptr(self.snapshot_bad), self.ops.stream),
                   'infgen_snapshot_scenes')
        out.t, out.n, out.slots, out.slots_host, out.generation = t, n, sl, host, self._reload_gen
        return out

    def restore(self, snap, index=None):
        """the way back: slot s takes over entry ``index[s]`` of ``snap`` and stands at the boundary in front of decode step
        ``snap.t`` again (``run(snap.t, ...)`` or ``step(snap.t)`` continues from there, bit for bit as the saved slot would have,
        under the uniforms, temperatures, constraints and commands the engine has now).  ``index``: None - every saved slot back
        onto itself (built on the device) - or int [S] / [S0, copies] of entry numbers, -1 = keep the slot as it is; one entry may
        go to several slots of its copy group (the same as a branch from the saved slot).  A host ``index`` is checked here
        (``ValueError`` naming the first bad entry); a device tensor is taken as it is - stream-ordered, no host read - and the
        entries the kernel refuses (out of range, not valid, another step, another copy group) are read as -1 and counted into
        ``restore_bad``.  One launch of ``infgen_restore_scenes``.  Raises for a snapshot of another engine layout or from before
        a ``reload*()``, on engines with scenario insertion and before ``prologue()``.  Clears the cached rollout
        log-probabilities.  Eager: captured graphs stay as they are."""
        from . import snapshots
        if not isinstance(snap, snapshots.Snapshot):
            raise ValueError('restore takes a snapshots.Snapshot')
        self._check_snapshot_call('restore', snap.t)
        if snap.signature != snapshots.signature(self):
            raise ValueError('restore: the snapshot belongs to another engine layout')
        if snap.generation != self._reload_gen:
            raise ValueError('restore: the snapshot was taken before a reload: its scenes are no longer in this engine')
        if snap.n < 1:
            raise ValueError('restore: the snapshot holds no entry')
        if index is None:
            idx = snapshots.identity_index(snap, self.S)
        else:
            x = index if isinstance(index, torch.Tensor) else torch.as_tensor(np.asarray(index))
            if x.is_floating_point() or x.dtype == torch.bool:
                raise ValueError('index holds integer entry indices')
            if tuple(x.shape) not in ((self.S,), (self.S0, self.copies)):
                raise ValueError(f'index: expected shape {(self.S,)} or {(self.S0, self.copies)}, got {tuple(x.shape)}')
            if not x.is_cuda:
                x = torch.from_numpy(snapshots.check_index(x.numpy(), self.S, snap.n, self.copies, snap.slots_host))
            idx = x.to(self.device, torch.int32).contiguous().view(-1)
        _lib.check(self.lib.infgen_restore_scenes(C.byref(self._ctx), int(snap.t), _lib.ptr(idx), _lib.ptr(snap.buf), snap.stride,
                                                  _lib.ptr(snap.head), snap.n, _lib.ptr(self.restore_bad), self.ops.stream),
                   'infgen_restore_scenes')
        self._rollout_lp = self._rollout_slp = None

    def rollout_guided(self, every: int = 4, keep: Optional[int] = None, weights=None, u=None):
        """a guided rollout: ``prologue``, then for every block of ``every`` decode steps ``run(t0, t1)``,
        ``branching.score_log_weight`` over the block's step scores, ``branching.keep_best(.., keep)`` - or, with ``keep=None``,
        ``resample_parents(systematic_ancestors(.., u[b]))`` - and ``branch(parent, t1)``: the copies of every scene are pruned or
        resampled on overlaps, road departures and comfort while they run.  Everything is enqueued on the current stream; nothing
        is read on the host.  ``weights``: a dict with keys of ``branching.SCORE_WEIGHTS``; ``u``: the systematic resampler's
        uniforms [n_blocks, S0] in [0, 1) (an array or a tensor; needed when ``keep`` is None).  ``ancestry`` [n_blocks, S] int32
        holds the parent vector of every block, on the device.  Needs ``copies > 1``, ``step_scores`` and no scenario insertion."""
        from . import branching
        if self.copies <= 1:
            raise ValueError('rollout_guided: needs copies > 1 - there is nothing to prune or resample among one copy')
        if self.step_scores is None:
            raise ValueError('rollout_guided: needs step_scores (the engine logs no score to guide on)')
        if self.insertion:
            raise ValueError('rollout_guided: engines with scenario insertion cannot branch: left out')
        steps, every = self.cfg.num_decode_steps, int(every)
        if every < 1:
            raise ValueError('rollout_guided: every must be at least 1')
        weights = branching.check_score_weights(weights)
        if keep is not None and not 1 <= int(keep) <= self.copies:
            raise ValueError(f'rollout_guided: keep must be in 1 .. {self.copies}')
        blocks = [(t0, min(t0 + every, steps)) for t0 in range(0, steps, every)]
        if keep is None:
            if u is None:
                raise ValueError(f'rollout_guided: the systematic resampler (keep=None) needs uniforms u [{len(blocks)}, {self.S0}]')
            u = torch.as_tensor(u).to(self.device, torch.float32)
            if tuple(u.shape) != (len(blocks), self.S0):
                raise ValueError(f'rollout_guided: u must be [{len(blocks)}, {self.S0}], got {tuple(u.shape)}')
        self._bc_host = None
        self._end_session()
        self.prologue()
        self.ancestry = torch.empty(len(blocks), self.S, device=self.device, dtype=torch.int32)
        for b, (t0, t1) in enumerate(blocks):
            self.run(t0, t1)
            lw = branching.score_log_weight(self.step_score, t0, t1, weights, copies=self.copies)
            if keep is not None:
                parent = branching.keep_best(lw, int(keep))
            else:
                parent = branching.resample_parents(branching.systematic_ancestors(lw, u[b]), self.copies)
            self.ancestry[b].copy_(parent.reshape(-1))
            self.branch(self.ancestry[b], t1)

    def ctx_tensor(self) -> torch.Tensor:
        """the bytes of this engine's InfgenRollout block (after ``prologue``) - the state handle of
        ``torch.ops.infgen_hip.decode_step``"""
        assert self._ctx is not None, 'run prologue() first'
        self._refresh_opts(groups=True)
        return torch.frombuffer(bytearray(bytes(self._ctx)), dtype=torch.uint8)

    # ------------------------------------------------------------------ outputs (reference :2303-2389)
    def outputs(self) -> List[Dict[str, np.ndarray]]:
        """the reference's return dict per scene (agent_decoder.py:2303-2389); rows appended by the
        insertion loop follow the initial ones like in the reference"""
        if self._batch_lay is not None:
            raise RuntimeError('an ingested Batch has no host-side scenes: use outputs_batch() / outputs_device()')
        torch.cuda.synchronize(self.device)
        self._full_hosts()
        cfg, hc, H = self.cfg, self.hc, self.cfg.num_historical_steps
        pos, head = self.pos.cpu().numpy(), self.head.cpu().numpy()
        state, token = self.state.cpu().numpy(), self.token.cpu().numpy()
        ptraj, phead, pstate = self.pred_traj.cpu().numpy(), self.pred_head.cpu().numpy(), self.pred_state.cpu().numpy()
        logits = self.logits.cpu().numpy() if self.logits is not None else None
        x_pt = self.x_pt.cpu().numpy() if self.x_pt is not None else None
        tabs = self.vocab.cpu().numpy()
        n_fin = self.n_agents.cpu().numpy()
        atype_dev = self.atype.cpu().numpy()
        bos_dev = self.bos.cpu().numpy()
        shape_all = self.ins['shape_all'].cpu().numpy().reshape(self.S, self.A_cap, 3) if self.ins is not None else None
        replay_row = self.replay_row.cpu().numpy().astype(bool) if self.replay_row is not None else None
        tok_lp = self.token_logprob.cpu().numpy() if self.token_logprob is not None else None
        smp_lp = self.sample_logprob.cpu().numpy() if self.sample_logprob is not None else None
        outs = []
        for s, h in enumerate(self.hosts):
            A0, M = h['A'], h['M']
            A = int(n_fin[s])
            sc = self.scenes[s // self.copies]['agent']
            filt = h['filt']
            pos_a = pos[s, :, :A].transpose(1, 0, 2).copy()
            head_a = head[s, :, :A].T.copy()
            nstate = state[s, :, :A].T.astype(np.int64)
            ntok = token[s, :, :A].T.astype(np.int64)
            # history columns of next_token_idx / next_state_idx are the *input* tokens (:1733-1735)
            ntok[:A0, :hc] = np.asarray(sc['token_idx'])[filt][:, :hc]
            nstate[:A0, :hc] = np.asarray(sc['state_idx'])[filt][:, :hc]
            for a in range(A0, A):                      # inserted rows: no token up to and including bos (:2303-2305)
                ntok[a, :bos_dev[s, a] + 1] = -1
            pt = np.concatenate([np.zeros((A, H, 2), np.float32), ptraj[s, :A]], axis=1)
            ph = np.concatenate([np.zeros((A, H), np.float32), phead[s, :A]], axis=1)
            ps = np.concatenate([np.zeros((A, H), np.float32), pstate[s, :A]], axis=1)
            pt[:A0, 0] = np.asarray(sc['position'])[filt][:, 0, :2]
            ph[:A0, 0] = np.asarray(sc['heading'])[filt][:, 0]
            ps[:A0, 1:H] = np.repeat(np.asarray(sc['state_idx'])[filt][:, :hc], cfg.shift, axis=1)
            htok = np.asarray(sc['token_idx'])[filt][:, :hc].astype(np.int64).copy()
            htok[htok < 0] = 0
            atype0 = h['type']
            hcont = tabs[atype0[:, None], htok]                      # (A0, hc, 6, 4, 2)
            th = head_a[:A0, 0].astype(np.float32)
            cs, sn = np.cos(th)[:, None, None, None], np.sin(th)[:, None, None, None]
            x, y = hcont[..., 0], hcont[..., 1]
            hx = x * cs - y * sn + pos_a[:A0, 0, 0][:, None, None, None]
            hy = x * sn + y * cs + pos_a[:A0, 0, 1][:, None, None, None]
            pt[:A0, 1:H, 0] = hx[:, :, 1:].mean(axis=3).reshape(A0, -1)
            pt[:A0, 1:H, 1] = hy[:, :, 1:].mean(axis=3).reshape(A0, -1)
            ph[:A0, 1:H] = np.arctan2(hy[:, :, 1:, 0] - hy[:, :, 1:, 3], hx[:, :, 1:, 0] - hx[:, :, 1:, 3]).reshape(A0, -1)
            atype = atype_dev[s, :A].astype(np.int64)
            eval_shape = np.asarray(EVAL_SHAPE, np.float32)[atype]
            ids0 = np.asarray(sc['id'])[filt]
            ids = np.concatenate([ids0, ids0.max() + 1 + np.arange(A - A0, dtype=ids0.dtype)])
            pshape = np.asarray(sc['shape'])[filt][:, hc - 1].astype(np.float32)
            if A > A0:
                pshape = np.concatenate([pshape, shape_all[s, A0:A]])
            o = dict(ego_index=h['av'], agent_id=ids, valid_mask=h['valid'],
                     pos_a=pos_a, head_a=head_a, pred_traj=pt, pred_head=ph, pred_state=ps,
                     pred_valid=(ps != INVALID) & (ps != ENTER), pred_type=atype,
                     pred_shape=pshape, eval_shape=eval_shape,
                     pred_z=np.zeros_like(ph), next_token_idx=ntok, next_state_idx=nstate,
                     gt_traj=np.asarray(sc['position'])[filt][:, H:, :2].copy(), num_inserted=A - A0)
            if replay_row is not None:
                o['replay_mask'] = replay_row[s, :A].copy()        # the rows that followed their plan (inserted rows never do)
            if tok_lp is not None or smp_lp is not None:
                n_st = (tok_lp if tok_lp is not None else smp_lp).shape[0]
                first = np.full(A, hc, np.int64)
                first[A0:] = bos_dev[s, A0:A].astype(np.int64) + 1
                forced = replay_row[s, :A] if replay_row is not None else np.full(A, self.teacher_token is not None)
                m = logprob.logprob_mask(torch.from_numpy(ntok), torch.from_numpy(first), hc, n_st,
                                         torch.from_numpy(np.ascontiguousarray(forced))).numpy()
                for key, buf in (('next_token_logprob', tok_lp), ('next_token_sample_logprob', smp_lp)):
                    if buf is not None:
                        lp = np.zeros((A, self.T), np.float32)
                        lp[:, hc:hc + n_st] = buf[:, s * self.A_cap:s * self.A_cap + A].T
                        o[key] = np.where(m, lp, np.float32(0))
                o['next_token_logprob_mask'] = m
            if self.ins is not None:
                o['agent_labels'] = self._agent_labels(s, A)
            if self.seed_out is not None:
                so = self.seed_out
                for k_out, k_in in self._SEED_KEYS:
                    o[k_out] = so[k_in][s].cpu().numpy() if k_in in so else None
            if logits is not None:
                o['logits'] = logits[:, s * self.A_cap:s * self.A_cap + A].copy()
            if x_pt is not None:
                ms = s // self.copies
                o['x_pt'] = x_pt[ms * self.M_cap:ms * self.M_cap + M].copy()
            outs.append(o)
        return outs

    def _agent_labels(self, s: int, A: int):
        """[A][T] labels of scene s: 'A<k>' on the first column after the bos column of the k-th agent a step inserted (:1996-1999)"""
        labels = [[None] * self.T for _ in range(A)]
        per_step = {}
        for row, t_ in self.ins['inserted_rows'][s]:
            k_ = per_step[t_] = per_step.get(t_, 0) + 1
            a_ = row - s * self.A_cap
            if a_ < A and self.hc + t_ < self.T:
                labels[a_][self.hc + t_] = f'A{k_}'
        return labels

    def _epi_from_hosts(self):
        """the inputs of the device epilogue (``scene_setup.epilogue_inputs``) of a batch set up from host scenes, ground truths
        of differing lengths included: staged on the host, one upload per array"""
        H, n = self.cfg.num_historical_steps, self.copies
        hosts = self.hosts[::n]
        ag = scene_setup.stage_epilogue(self.scenes, [h['filt'] for h in hosts], self.cfg)
        valid = torch.from_numpy(scene_setup._stack([h['valid'] for h in hosts], False, bool))
        n0 = np.repeat(np.asarray([h['A'] for h in hosts], np.int64), n)
        if n > 1:
            ag = {k: v.repeat_interleave(n, dim=0) for k, v in ag.items()}
            valid = valid.repeat_interleave(n, dim=0)
        self._gt_len = [int(np.asarray(sc['agent']['position']).shape[1]) - H for sc in self.scenes for _ in range(n)]
        E = scene_setup.epilogue_inputs(ag, valid, self.A_cap, self.cfg, n0)
        return dict({k: v.to(self.device) for k, v in E.items()}, n0_host=n0)

    def _epilogue_arrays(self, detach: bool):
        """the batch-wide arrays of the epilogue of agent_decoder.py:2303-2389 ([S][A_cap][...], all on the device)"""
        cfg, hc, H, dev = self.cfg, self.hc, self.cfg.num_historical_steps, self.device
        S, A_cap, T, R = self.S, self.A_cap, self.T, self.R
        if getattr(self, '_epi', None) is None:
            self._epi = self._epi_from_hosts()
        E = self._epi
        n_fin = self.n_agents.long()
        row = torch.arange(A_cap, device=dev)[None, :]
        init = row < E['n0'][:, None]                                                 # rows of the initial agents
        pos_a = self.pos.permute(0, 2, 1, 3)                                          # [S, A_cap, T, 2]
        head_a = self.head.permute(0, 2, 1)
        lg_all, x_pt_all = self.logits, self.x_pt
        if detach:
            pos_a, head_a = pos_a.contiguous(), head_a.contiguous()
            lg_all = lg_all.clone() if lg_all is not None else None
            x_pt_all = x_pt_all.clone() if x_pt_all is not None else None
        nstate = self.state.permute(0, 2, 1).long().clone()
        ntok = self.token.permute(0, 2, 1).long().clone()
        # history columns of next_token_idx / next_state_idx are the input tokens (:1733-1735); inserted rows: no token up to and
        # including their bos column (:2303-2305)
        ntok[:, :, :hc] = torch.where(init[..., None], E['htok'], ntok[:, :, :hc])
        nstate[:, :, :hc] = torch.where(init[..., None], E['hst'], nstate[:, :, :hc])
        cols = torch.arange(T, device=dev)[None, None, :]
        ntok.masked_fill_((~init)[..., None] & (cols <= self.bos.long()[..., None]), -1)      # (a masked assignment would wait for the device)
        zf = lambda *shape: torch.zeros(*shape, device=dev)
        pt = torch.cat([zf(S, A_cap, H, 2), self.pred_traj], dim=2)
        ph = torch.cat([zf(S, A_cap, H), self.pred_head], dim=2)
        ps = torch.cat([zf(S, A_cap, H), self.pred_state], dim=2)
        # history prefill of the initial agents: step 0 = the logged pose, steps 1..H-1 from the history tokens' contours
        atype = self.atype.long()
        hcont = self.vocab[atype[..., None].expand(S, A_cap, hc), E['htok'].clamp(min=0)]        # [S, A_cap, hc, 6, 4, 2]
        th = head_a[:, :, 0]
        cs, sn = torch.cos(th)[..., None, None, None], torch.sin(th)[..., None, None, None]
        x, y = hcont[..., 0], hcont[..., 1]
        hx = x * cs - y * sn + pos_a[:, :, 0, 0][..., None, None, None]
        hy = x * sn + y * cs + pos_a[:, :, 0, 1][..., None, None, None]
        i3 = init[..., None, None]
        pt[:, :, 0] = torch.where(init[..., None], E['p0'], pt[:, :, 0])
        ph[:, :, 0] = torch.where(init, E['h0'], ph[:, :, 0])
        hist_xy = torch.stack([hx[:, :, :, 1:].mean(dim=4), hy[:, :, :, 1:].mean(dim=4)], dim=-1).reshape(S, A_cap, H - 1, 2)
        pt[:, :, 1:H] = torch.where(i3, hist_xy, pt[:, :, 1:H])
        hist_h = torch.atan2(hy[:, :, :, 1:, 0] - hy[:, :, :, 1:, 3], hx[:, :, :, 1:, 0] - hx[:, :, :, 1:, 3]).reshape(S, A_cap, H - 1)
        ph[:, :, 1:H] = torch.where(init[..., None], hist_h, ph[:, :, 1:H])
        ps[:, :, 1:H] = torch.where(init[..., None], E['hst'].float().repeat_interleave(cfg.shift, dim=2), ps[:, :, 1:H])
        pvalid = (ps != INVALID) & (ps != ENTER)
        pshape = E['shp']
        if self.ins is not None:
            pshape = torch.where(init[..., None], E['shp'], self.ins['shape_all'].view(S, A_cap, 3))
        eval_shape = E['eval_shape'][atype]
        batch = dict(agent_id=E['ids'], pos_a=pos_a, head_a=head_a, pred_traj=pt, pred_head=ph, pred_state=ps, pred_valid=pvalid,
                     pred_type=atype, pred_shape=pshape, eval_shape=eval_shape, next_token_idx=ntok, next_state_idx=nstate)
        if self.replay_row is not None:
            batch['replay_mask'] = self.replay_row.bool()
        if self.token_logprob is not None or self.sample_logprob is not None:
            steps = (self.token_logprob if self.token_logprob is not None else self.sample_logprob).shape[0]
            first = torch.where(init, torch.full_like(self.bos, hc, dtype=torch.long), self.bos.long() + 1)
            forced = (self.replay_row.bool() if self.replay_row is not None
                      else torch.full((S, A_cap), self.teacher_token is not None, device=dev))
            m = logprob.logprob_mask(ntok, first, hc, steps, forced) & (row < n_fin[:, None])[..., None]
            if self.token_logprob is not None:
                lp = zf(S, A_cap, T)
                lp[:, :, hc:hc + steps] = self.token_logprob.view(steps, S, A_cap).permute(1, 2, 0)
                batch['next_token_logprob'] = torch.where(m, lp, zf(()))
                self._rollout_lp = logprob.rollout_logprob(lp, m)
            if self.sample_logprob is not None:
                slp = zf(S, A_cap, T)
                slp[:, :, hc:hc + steps] = self.sample_logprob.view(steps, S, A_cap).permute(1, 2, 0)
                batch['next_token_sample_logprob'] = torch.where(m, slp, zf(()))
                self._rollout_slp = logprob.rollout_logprob(slp, m)
            batch['next_token_logprob_mask'] = m
        return batch, E, ph, lg_all, x_pt_all, n_fin

    def outputs_device(self, detach: bool = False) -> List[Dict[str, torch.Tensor]]:
        """``outputs`` without the host round trip: the same per-scene dicts as device tensors (views of the batch arrays where
        the layout allows), the epilogue of agent_decoder.py:2303-2389 evaluated for all scenes at once on the device.
        VIEWS: the per-scene tensors are slices of batch-wide results of this call (an in-place edit of one scene's tensor edits
        that slice only); ``pos_a`` / ``head_a`` / ``logits`` / ``x_pt`` additionally alias this engine's own buffers, which the next
        rollout overwrites - ``detach=True`` copies those four batch arrays once (what ``InfGenDecoder`` does, whose engines are
        reused across calls)."""
        if self._batch_lay is not None:
            self.batch_counts()
        batch, E, ph, lg_all, x_pt_all, n_fin = self._epilogue_arrays(detach)
        cfg, hc, H, dev = self.cfg, self.hc, self.cfg.num_historical_steps, self.device
        S, A_cap, T, R = self.S, self.A_cap, self.T, self.R
        # the only host copy: the final agent counts - known without asking when nothing can be inserted (then the call returns
        # with the epilogue enqueued behind the rollout and nothing waited for)
        n_host = n_fin.cpu().numpy() if self.insertion else E['n0_host']
        outs = []
        gt_all, val_all, gt_len = E['gt'], E['val'], self._gt_len
        seed_out, ins = self.seed_out, self.ins
        A_capl, M_capl = A_cap, self.M_cap

        def cut(t, s, A):          # (default arguments bind the loop variables: the thunk runs later)
            return lambda: t[s, :A]
        for s, h in enumerate(self.hosts):
            A, A0, M = int(n_host[s]), h['A'], h['M']
            lazy = {k: cut(t, s, A) for k, t in batch.items()}
            lazy['valid_mask'] = cut(val_all, s, A0)
            lazy['pred_z'] = (lambda s=s, A=A: torch.zeros_like(ph[s, :A]))
            lazy['gt_traj'] = (lambda s=s, A0=A0: gt_all[s, :A0, :gt_len[s]])
            o = LazyOut(dict(ego_index=h['av'], num_inserted=A - A0), lazy)
            if ins is not None:
                o.set_lazy('agent_labels', (lambda s=s, A=A: self._agent_labels(s, A)))
            if seed_out is not None:
                # (detach: the seed arrays are engine-owned and zeroed / rewritten by the next rollout of a reused engine - cloned NOW)
                for k_out, k_in in self._SEED_KEYS:
                    o[k_out] = None if k_in not in seed_out else seed_out[k_in][s].clone() if detach else seed_out[k_in][s]
            if lg_all is not None:
                o.set_lazy('logits', (lambda s=s, A=A: lg_all[:, s * A_capl:s * A_capl + A]))
            if x_pt_all is not None:
                o.set_lazy('x_pt', (lambda ms=s // self.copies, M=M: x_pt_all[ms * M_capl:ms * M_capl + M]))
            outs.append(o)
        return outs

    # the seed node's outputs (reference return dict key, seed_out key); the grid's are None for use_grid_token = False
    _SEED_KEYS = (('next_state_prob_seed', 'state'), ('next_pos_rel_prob_seed', 'pos'), ('grid_agent_occ_seed', 'occ_a'),
                  ('grid_pt_occ_seed', 'occ_p'), ('grid_agent_occ_gt_seed', 'occ_gt'))

    _PACK_FIN = ('agent_id', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state', 'pred_valid', 'pred_type', 'pred_shape',
                 'eval_shape', 'next_token_idx', 'next_state_idx')

    def outputs_batch(self) -> List[Dict]:
        """the batched epilogue of an ingested Batch: one dict per copy (``copies`` rollouts of every graph), each holding the B
        graphs' agents concatenated in graph order - graph s's rows are exactly ``outputs_device()``'s rows of its scene - plus
        ``agent_batch`` [N] / ``agent_ptr`` [B + 1] / ``ego_index`` [B] (rows into the concatenation) and ``x_pt`` [sum M][D] in
        pt_token order.  ``valid_mask`` / ``gt_traj`` hold the initial agents only (as per scene).  The rows are gathered by
        infgen_pack_rows (one launch per copy); the one host copy is ``batch_counts()``."""
        assert self._batch_lay is not None, 'outputs_batch() needs an engine set up from a Batch (reload_batch)'
        n_fin, c = self.batch_counts()
        batch, E, ph, lg_all, x_pt_all, _ = self._epilogue_arrays(False)
        S, A_cap, T, B, n, dev = self.S, self.A_cap, self.T, self.S0, self.copies, self.device
        fin, init = self.n_agents, self._ing['counts'][:, 0]
        pack_fin = self._PACK_FIN + tuple(k for k in ('replay_mask', 'next_token_logprob', 'next_token_sample_logprob',
                                                  'next_token_logprob_mask') if k in batch)
        keys = pack_fin + ('valid_mask', 'gt_traj')
        srcs = [batch[k].contiguous() for k in pack_fin] + [E['val'], E['gt']]
        x_pt = None
        if x_pt_all is not None:
            M = self._batch_lay['M']
            x_pt = pack_rows([x_pt_all.view(B, self.M_cap, -1)], [self.n_map], [int(M.sum())], B)[0]
        outs = []
        for j in range(n):
            f_j, i_j = n_fin[j::n], c[j::n, 0]
            tots = [int(f_j.sum())] * len(pack_fin) + [int(i_j.sum())] * 2
            cols = [fin] * len(pack_fin) + [init] * 2
            packed = dict(zip(keys, pack_rows(srcs, cols, tots, B, scene0=j, scene_step=n)))
            ptr = np.concatenate([[0], np.cumsum(f_j)])
            o = dict(packed)
            o['pred_z'] = torch.zeros(int(f_j.sum()), ph.shape[2], device=dev)
            o['agent_ptr'] = torch.from_numpy(ptr).to(dev)
            o['agent_batch'] = torch.repeat_interleave(torch.arange(B, device=dev), torch.from_numpy(f_j).to(dev), output_size=int(f_j.sum()))
            o['ego_index'] = torch.from_numpy(ptr[:-1] + c[j::n, 1]).to(dev)
            o['num_inserted'] = torch.from_numpy(f_j - i_j).to(dev)
            if x_pt is not None:
                o['x_pt'] = x_pt
            if self.ins is not None:
                labels = []
                for g in range(B):
                    labels.extend(self._agent_labels(g * n + j, int(n_fin[g * n + j])))
                o['agent_labels'] = labels
            if self.seed_out is not None:
                so = self.seed_out
                for k_out, k_in in self._SEED_KEYS:
                    v = so[k_in][j::n] if k_in in so else None
                    o[k_out] = None if v is None else v.reshape((-1,) + tuple(v.shape[2:])).clone()
            outs.append(o)
        return outs

    def rollout_logprob(self) -> torch.Tensor:
        """[S] float64 on the device: every scene's masked sum of ``next_token_logprob`` as of the last ``outputs_device()`` /
        ``outputs_batch()`` call, added up in an order that does not depend on the batch (``logprob.fixed_order_sum``)"""
        assert getattr(self, '_rollout_lp', None) is not None, 'needs token_logprob=True and an outputs_device() / outputs_batch() call'
        return self._rollout_lp

    def rollout_sample_logprob(self) -> torch.Tensor:
        """[S] float64 on the device: every scene's masked sum of ``next_token_sample_logprob``, as ``rollout_logprob`` sums"""
        assert getattr(self, '_rollout_slp', None) is not None, 'needs sample_logprob=True and an outputs_device() / outputs_batch() call'
        return self._rollout_slp

    def _initial_rows(self):
        """(int32 device tensor, stride): entry ``s * stride`` is scene s's initial agent count - no device work after the first
        call for a batch"""
        c = getattr(self, '_n0_dev', None)
        if c is None or c[0] != self._reload_gen:
            if self._batch_lay is not None:
                c = (self._reload_gen, self._ing['counts'], 3)            # [S][3]: kept rows first
            else:
                c = (self._reload_gen, torch.tensor([h['A'] for h in self.hosts], dtype=torch.int32).to(self.device), 1)
            self._n0_dev = c
        return c[1], c[2]

    def select_modes(self, k: int = 6, dist_thresh: float = 2.5, scores='density', t_goal: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """K representative futures per agent out of the ``copies`` rollouts of its scene, after a rollout with ``copies > 1``
        (``infgen_amd.modes``; "modes" of include/infgen_hip.h): candidate j of row a is agent a in copy j, its goal the (x, y) of
        ``pred_traj`` at step ``t_goal`` (None: the last of the R steps).  ``pred_traj`` is read in place - one launch, nothing
        read on the host.  A candidate is valid if its ``pred_state`` at ``t_goal`` is neither INVALID nor ENTER and the row is
        below the scene's initial agent count: with scenario insertion only the initial rows are the same agent in every copy, so
        rows at or above that count return index -1.  ``scores``: 'density' (the share of valid copies whose goal lies within
        ``dist_thresh``), 'logprob' (the softmax over the copies of the scene-level ``rollout_logprob()``, for every row; needs
        ``token_logprob=True`` and an ``outputs_device()`` / ``outputs_batch()`` call) or a tensor [S0, copies] >= 0.
        -> dict of device tensors: ``mode_idx`` [S0, A_cap, k] int32 (the copy; -1: none), ``mode_score``, ``mode_prob`` (the scores
        renormalised over the k slots), ``mode_traj`` [S0, A_cap, k, R, 2].  Tokens, poses and logits of the rollout are untouched.
        Before anything has run on the current batch (a new engine, or after a reload) the call raises RuntimeError."""
        modes.check_engine_args(self.copies, k, scores)
        if not self._prologue_done:
            raise RuntimeError('select_modes reads the pred_traj a rollout leaves behind: nothing has run on the current batch yet '
                               '(call rollout() first; a reload outdates the previous batch\'s rollout)')
        n, S0, A_cap, R, dev = self.copies, self.S0, self.A_cap, self.R, self.device
        t = R - 1 if t_goal is None else int(t_goal)
        if not -R <= t < R:
            raise ValueError(f't_goal = {t_goal} is outside the {R} predicted steps')
        sc = None
        if isinstance(scores, str) and scores == 'logprob':
            if self.token_logprob is None:
                raise ValueError("scores='logprob' needs an engine built with token_logprob=True")
            sc = torch.softmax(self.rollout_logprob().view(S0, n), dim=1).to(torch.float32).contiguous()
        elif torch.is_tensor(scores):
            if tuple(scores.shape) != (S0, n):
                raise ValueError(f'scores must be [scenes, copies] = {(S0, n)}, not {tuple(scores.shape)}')
            sc = scores.to(dev, torch.float32).contiguous()
        n0, n0_stride = self._initial_rows()
        traj = self.pred_traj.view(S0, n, A_cap, R, 2).permute(0, 2, 1, 3, 4)              # [S0, A_cap, copies, R, 2], in place
        state = self.pred_state.view(S0, n, A_cap, R).permute(0, 2, 1, 3)
        out, score, idx = modes.launch(traj, int(k), dist_thresh, t % R, scores=sc, score_per_group=True, cand_state=state,
                                       state_values=(float(INVALID), float(ENTER)), row_limit=n0, limit_stride=n0_stride * n)
        return dict(mode_idx=idx, mode_score=score, mode_prob=modes.mode_prob(score, idx), mode_traj=out)

    def agent_steps(self) -> int:
        """agent-steps (10 Hz) decoded by the last full rollout of this batch (the rows decoded at every step, incl. the
        ones scenario insertion appended, x 5 simulated steps per decode step)"""
        if self.insertion and self._prologue_done:
            return int(self._decoded_rows.item()) * self.cfg.shift
        if self.hosts is None:
            self.batch_counts()
        return int(sum(h['A'] for h in self.hosts)) * self.R


def rollout_many(engines: Sequence[RolloutEngine], streams: Optional[Sequence[torch.cuda.Stream]] = None):
    """Full rollouts of several engines (disjoint scene sets of one GPU), each on its own HIP stream, sequenced by ONE host
    thread: an engine runs until it needs a result of the device (``RolloutEngine.run_gen``), then the next engine's launches
    are enqueued, round robin.  With scenario insertion on, the sub-loop of a decode step is a chain of small dependent launches
    whose length is set by the slowest scene of the batch; several smaller batches in different phases fill the chip where one
    large batch leaves it idle.  Without insertion the engines' launch sequences simply interleave."""
    if not engines:
        return
    dev = engines[0].device
    if streams is None or len(engines) == 1:
        for e in engines:
            e.rollout()
        return
    # (k_layers_p launches of several streams: the library keeps every launch within the device's resident capacity and orders such
    # launches of different streams behind each other - csrc/api.hip: layers_p_launch - so engines of any size may share the GPU;
    # the launch itself is a plain one by default, cooperative with options['layers_p'] = 2)
    return _rollout_many_streams(engines, streams, dev)


def _rollout_many_streams(engines, streams, dev):
    cur = torch.cuda.current_stream(dev)
    if all(e._graph_all and not e.insertion for e in engines):
        # whole-rollout graphs: one replay per engine, nothing for the host to sequence
        try:
            for e, st in zip(engines, streams):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    e.rollout()
        finally:
            for st in streams:
                cur.wait_stream(st)
        return
    live = []
    try:
        for e, st in zip(engines, streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                e.prologue()
                live.append((e.run_gen(), st))
        while live:
            nxt = []
            for g, st in live:
                with torch.cuda.stream(st):
                    try:
                        next(g)
                        nxt.append((g, st))
                    except StopIteration:
                        pass
            live = nxt
    finally:
        for st in streams:          # also when a generator raised (InsertionHeadroomError): the caller's stream waits for all
            cur.wait_stream(st)
