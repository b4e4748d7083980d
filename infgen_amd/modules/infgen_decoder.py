"""InfGenDecoder: the drop-in boundary of the hot path (reference
infgen/modules/infgen_decoder.py:15-143).  Same constructor signature, same sub-module names
(``map_encoder`` / ``agent_encoder``), ``forward`` / ``inference`` / ``inference_no_map`` with the
reference's return dicts (``forward``: the teacher-forced open-loop pass, infgen_amd/forward_engine.py).  ``inference`` runs map encoder + closed-loop rollout on the GPU through
libinfgen_hip.so; ``inference_batch`` is the throughput entry (many scenes in lockstep).
"""
from __future__ import annotations

import functools
import os
import weakref
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, logprob, modes, scene_setup
from ..closed_loop import ClosedLoopSession, run_idm
from ..constraints import (TokenMasks, check_avoid_collisions, check_follow_routes, check_obey_signals, check_stay_on_road,
                           check_step_scores, check_type_selectors, road_key, route_key, score_key, signal_key)
from ..engine import InsertionHeadroomError, LazyOut, PackedWeights, RolloutEngine, read_batch_layout
from ..synth import RolloutConfig
from .agent_decoder import InfGenAgentDecoder
from .attr_tokenizer import Attr_Tokenizer
from .map_decoder import InfGenMapDecoder

_AGENT_KEYS = ('state_idx', 'valid_mask', 'id', 'raw_agent_valid_mask', 'token_pos', 'token_idx', 'token_heading',
               'shape', 'type', 'grid_token_idx', 'position', 'heading', 'av_index',
               'trajectory_token_veh', 'trajectory_token_ped', 'trajectory_token_cyc')


def _np(v):
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


def scene_from_data(data) -> Dict[str, Dict[str, np.ndarray]]:
    """the reference's HeteroData-style ``data`` (dict access) -> host scene dict of numpy arrays"""
    ag = data['agent']
    agent = {k: _np(ag[k]) for k in _AGENT_KEYS}
    pt = data['pt_token']
    ptd = {k: _np(pt[k]) for k in ('position', 'orientation', 'type', 'pl_type', 'token_idx')}
    key = ('pt_token', 'to', 'map_polygon')
    try:
        e = data[key]['edge_index']
    except (KeyError, TypeError):
        e = data['pt_token__to__map_polygon']['edge_index']
    return {'agent': agent, 'pt_token': ptd, 'map_polygon': {'light_type': _np(data['map_polygon']['light_type'])},
            'pt_token__to__map_polygon': {'edge_index': _np(e)}}


_FWD_AGENT_KEYS = ('state_idx', 'raw_agent_valid_mask', 'token_pos', 'token_idx', 'token_heading', 'shape', 'type',
                    'grid_token_idx', 'grid_offset_xy', 'heading_token_idx', 'sort_indices', 'pos_xy', 'heading_theta',
                    'pt_grid_token_idx', 'av_index', 'trajectory_token_veh', 'trajectory_token_ped', 'trajectory_token_cyc')


def batch_from_data(data) -> Dict[str, Dict[str, np.ndarray]]:
    """the (batched) ``data`` the reference's forward reads (agent_decoder.py:1108-1127, map_decoder.py:71-93) -> host dict of
    numpy arrays; ``ptr`` defaults to one scene"""
    ag, pt = data['agent'], data['pt_token']
    agent = {k: _np(ag[k]) for k in _FWD_AGENT_KEYS}
    A = agent['state_idx'].shape[0]
    agent['ptr'] = _np(ag['ptr']) if 'ptr' in ag else np.array([0, A], np.int64)
    ptd = {k: _np(pt[k]) for k in ('position', 'orientation', 'type', 'pl_type', 'token_idx')}
    ptd['ptr'] = _np(pt['ptr']) if 'ptr' in pt else np.array([0, ptd['position'].shape[0]], np.int64)
    key = ('pt_token', 'to', 'map_polygon')
    try:
        e = data[key]['edge_index']
    except (KeyError, TypeError):
        e = data['pt_token__to__map_polygon']['edge_index']
    return {'agent': agent, 'pt_token': ptd, 'map_polygon': {'light_type': _np(data['map_polygon']['light_type'])},
            'pt_token__to__map_polygon': {'edge_index': _np(e)}}


def scenes_from_datas(datas) -> List[Dict[str, Dict[str, np.ndarray]]]:
    """``scene_from_data`` for many scenes with ONE device -> host copy per key instead of one per key and scene (a 512-scene
    batch is ~12,000 small synchronous copies otherwise): tensors of a key are concatenated on their device, copied once and
    split into per-scene views on the host"""
    if len(datas) <= 1:
        return [scene_from_data(d) for d in datas]
    key = ('pt_token', 'to', 'map_polygon')

    def edge(d):
        try:
            return d[key]['edge_index']
        except (KeyError, TypeError):
            return d['pt_token__to__map_polygon']['edge_index']

    def split(vals, axis=0):
        """list of equal-rank arrays / tensors -> list of numpy views of one host copy"""
        if not all(isinstance(v, torch.Tensor) for v in vals):
            return [_np(v) for v in vals]
        if vals[0].dim() == 0:
            return list(torch.stack(vals).detach().cpu().numpy())
        sizes = [int(v.shape[axis]) for v in vals]
        host = torch.cat([v.detach() for v in vals], dim=axis).cpu().numpy()
        offs = np.concatenate([[0], np.cumsum(sizes)])
        return [host[offs[i]:offs[i + 1]] if axis == 0 else host[:, offs[i]:offs[i + 1]] for i in range(len(vals))]
    shared = ('trajectory_token_veh', 'trajectory_token_ped', 'trajectory_token_cyc')
    first = {k: _np(datas[0]['agent'][k]) for k in shared}
    cols = {}
    for k in _AGENT_KEYS:
        if k in shared:
            continue
        vals = [d['agent'][k] for d in datas]
        if k == 'av_index':
            vals = [v.reshape(-1) if isinstance(v, torch.Tensor) else np.asarray(v).reshape(-1) for v in vals]
        cols[k] = split(vals)
    pcols = {k: split([d['pt_token'][k] for d in datas]) for k in ('position', 'orientation', 'type', 'pl_type', 'token_idx')}
    light = split([d['map_polygon']['light_type'] for d in datas])
    edges = split([edge(d) for d in datas], axis=1)
    out = []
    for i in range(len(datas)):
        agent = {k: cols[k][i] for k in cols}
        agent.update(first)
        out.append({'agent': agent, 'pt_token': {k: pcols[k][i] for k in pcols}, 'map_polygon': {'light_type': light[i]},
                    'pt_token__to__map_polygon': {'edge_index': edges[i]}})
    return out


_STACK_AGENT_KEYS = ('state_idx', 'valid_mask', 'id', 'raw_agent_valid_mask', 'token_pos', 'token_idx', 'token_heading', 'shape',
                     'type', 'grid_token_idx', 'position', 'heading', 'av_index')
_STACK_PT_KEYS = ('position', 'orientation', 'type', 'pl_type', 'token_idx')


def stack_datas(datas, min_scenes: int = 8, any_device: bool = False):
    """a batch of ``data`` objects whose arrays are DEVICE tensors of one shape -> one stacked device tensor per key (what
    ``RolloutEngine.reload_device`` takes), or None when the batch is not of that kind (host arrays, ragged shapes, several
    devices, fewer than ``min_scenes`` scenes): then ``scenes_from_datas`` + the host setup take it.  No host copy.
    ``any_device``: CPU tensors count too (the CPU test of the device-side setup)."""
    if len(datas) < min_scenes:
        return None
    key = ('pt_token', 'to', 'map_polygon')

    def edge(d):
        try:
            return d[key]['edge_index']
        except (KeyError, TypeError):
            return d['pt_token__to__map_polygon']['edge_index']

    def stack(vals):
        v0 = vals[0]
        if not all(isinstance(v, torch.Tensor) and v.device == v0.device and v.shape == v0.shape for v in vals):
            raise TypeError('not a one-shape batch of tensors on one device')
        return torch.stack(vals)
    try:
        agent = {k: stack([d['agent'][k].reshape(-1)[:1] if k == 'av_index' else d['agent'][k] for d in datas])
                 for k in _STACK_AGENT_KEYS}
        if agent['state_idx'].device.type != 'cuda' and not any_device:
            return None
        return {'agent': agent, 'pt_token': {k: stack([d['pt_token'][k] for d in datas]) for k in _STACK_PT_KEYS},
                'light_type': stack([d['map_polygon']['light_type'] for d in datas]),
                'edge_index': stack([edge(d) for d in datas])}
    except (KeyError, TypeError, AttributeError, RuntimeError):
        return None


def _pt_mask(data, key) -> Optional[torch.Tensor]:
    """``data['pt_token'][key]`` (pt_pred_mask / pt_target_mask, filled by InfGen.sample_pt_pred) as a flat bool tensor; None
    when the data carries none"""
    try:
        m = data['pt_token'][key]
    except (KeyError, TypeError):
        return None
    return None if m is None else torch.as_tensor(m).reshape(-1).bool()


def _scatter_rows(pm: torch.Tensor, rowmap: torch.Tensor, n: int) -> torch.Tensor:
    """rowmap[pm] for a mask with n True entries, known on the host: no second count read (every index of the scatter is
    distinct: the unselected entries land past the first n)"""
    ar = torch.arange(pm.numel(), device=pm.device)
    dst = torch.where(pm, torch.cumsum(pm, 0) - 1, n + ar)
    return torch.empty(n + pm.numel(), dtype=torch.int64, device=pm.device).scatter_(0, dst, rowmap.to(torch.int64))[:n]


def num_graphs(data) -> int:
    """graphs in ``data``: ``num_graphs`` of a PyG-style Batch, else the length of ``agent.ptr`` - 1, else 1"""
    ng = getattr(data, 'num_graphs', None)
    if ng is None and isinstance(data, Mapping):
        ng = data.get('num_graphs')
    ag = data['agent']
    if 'ptr' in ag and ag['ptr'] is not None:
        ng = max(int(ng or 1), int(torch.as_tensor(ag['ptr']).numel()) - 1)
    return int(ng or 1)


def batch_datas(datas) -> Dict:
    """single-graph ``data`` dicts (device tensors) -> one PyG-style Batch dict, laid out like ``Batch.from_data_list`` of the
    reference's HeteroData: the rows of every key concatenated, ``agent.ptr`` / ``pt_token.ptr`` / ``*.batch``, the pt_token ->
    map_polygon edges offset by the token and polygon counts, ``num_graphs``; ``av_index`` in the global form (``av_index +
    ptr[:-1]``) that ``InfGen.validation_step`` hands to the decoder.  The trajectory-token vocabularies are taken from the first
    graph (they are one table)."""
    dev = torch.as_tensor(datas[0]['agent']['state_idx']).device
    cat = lambda vals: torch.cat([torch.as_tensor(v).to(dev) for v in vals])
    A = [int(d['agent']['state_idx'].shape[0]) for d in datas]
    M = [int(d['pt_token']['position'].shape[0]) for d in datas]
    L = [int(d['map_polygon']['light_type'].shape[0]) for d in datas]
    aptr, mptr, lptr = (torch.from_numpy(np.concatenate([[0], np.cumsum(x)])).to(dev) for x in (A, M, L))
    B = len(datas)
    agent = {k: cat([d['agent'][k] for d in datas]) for k in _STACK_AGENT_KEYS if k != 'av_index'}
    agent['av_index'] = cat([torch.as_tensor(d['agent']['av_index']).reshape(-1)[:1].to(dev) for d in datas]) + aptr[:-1]
    for k in ('trajectory_token_veh', 'trajectory_token_ped', 'trajectory_token_cyc'):
        agent[k] = datas[0]['agent'][k]
    agent['ptr'] = aptr
    agent['batch'] = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(A, device=dev))
    agent['num_nodes'] = sum(A)
    pt = {k: cat([d['pt_token'][k] for d in datas]) for k in _STACK_PT_KEYS}
    pt['ptr'] = mptr
    pt['batch'] = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(M, device=dev))
    pt['num_nodes'] = sum(M)
    key = ('pt_token', 'to', 'map_polygon')

    def edge(d):
        try:
            return d[key]['edge_index']
        except (KeyError, TypeError):
            return d['pt_token__to__map_polygon']['edge_index']
    off = lambda i: torch.tensor([[int(mptr[i])], [int(lptr[i])]], device=dev)
    out = {'agent': agent, 'pt_token': pt, 'map_polygon': {'light_type': cat([d['map_polygon']['light_type'] for d in datas])},
           key: {'edge_index': torch.cat([torch.as_tensor(edge(d)).to(dev) + off(i) for i, d in enumerate(datas)], dim=1)},
           'num_graphs': B}
    for k in ('agent_valid_mask', 'category', 'valid_mask', 'shape', 'batch_size_a'):
        if all(k in d for d in datas):
            out[k] = cat([d[k] for d in datas])
    if all('av_index' in d for d in datas):
        out['av_index'] = agent['av_index']
    if all('scenario_id' in d for d in datas):
        out['scenario_id'] = [x for d in datas for x in (d['scenario_id'] if isinstance(d['scenario_id'], (list, tuple))
                                                         else [d['scenario_id']])]
    return out


class _LazyScenes:
    """``scenes_from_datas(datas)``, made when first read (the device-side reload of a reused engine never reads it)"""

    def __init__(self, datas):
        self._datas, self._scenes = datas, None

    def _get(self):
        if self._scenes is None:
            self._scenes = scenes_from_datas(self._datas)
        return self._scenes

    def __len__(self):
        return len(self._datas)

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())


# ---------------------------------------------------------------------- the rollout driver's steps (InfGenDecoder._run_gen /
# _run_graphs_gen): plain functions over an engine dict and callables, so that they run without weights or a device
def _draw_uniforms(cfg, k: int, ik: int, S: int, ucols: int, sample_uniforms=None):
    """the uniforms of a stochastic decode from torch's RNG -> (sample_uniforms [steps][S][ucols] or the caller's, insert_uniforms
    [steps][10][S] or None).  Seeded callers depend on the stream: the motion draw comes first, each only under its condition."""
    if sample_uniforms is not None:
        sample_uniforms = _np(sample_uniforms)
    elif k > 1:
        # stochastic decode like the reference's default (top-k multinomial): one uniform per decode step and agent row - with
        # insertion on for every row a scene can ever hold (a row without its own uniform would be decoded greedily)
        sample_uniforms = torch.rand(cfg.num_decode_steps, S, ucols).numpy()
    insert_uniforms = None
    if ik > 1 and not cfg.disable_insertion and cfg.use_grid_token:
        # the cell of an inserted agent from the insert_beam_size most probable ones (agent_decoder.py:1900-1904)
        insert_uniforms = torch.rand(cfg.num_decode_steps, 10, S).numpy()
    return sample_uniforms, insert_uniforms


def _engine_key(*, graphs: bool, scenes: int, tables: bytes, disable_insertion: bool, steps: int, sample_k: int, insert_k: int,
                debug: bool, copies: int, replay: bool, token_logprob: bool, sample_logprob: bool, sampling: tuple,
                single: bool, map_only: bool, own_map: bool, seed_outputs: bool) -> tuple:
    """everything an engine is built from that its reload* cannot change -> its key in ``InfGenDecoder._engines``
    (``InfGenDecoder._make_engine`` reads the same facts: an engine argument is named here or it is reloaded).  A Batch's
    engines (set up by the ingest kernel) are apart from the list path's: 'graphs' leads their key."""
    return ('graphs' if graphs else 'scenes', scenes, tables, disable_insertion, steps, sample_k, insert_k, debug, copies, replay,
            token_logprob, sample_logprob, sampling, single, map_only, own_map, seed_outputs)


def _cached_engine(engines: Dict, key, attempts, make_engine):
    """one engine per batch layout is kept across calls: a second call of the same shape re-uploads the scene arrays into the
    first call's device buffers instead of building (and allocating) an engine again.  ``attempts``: (fits, reload) pairs over
    the held engine in order of preference; a reload that returns False has changed nothing and the next pair is tried.
    -> the reloaded engine, else a new one (two are held: the oldest goes)"""
    eng = engines.get(key)
    if eng is not None:
        for fits, reload in attempts:
            if fits(eng) and reload(eng) is not False:
                return eng
    eng = make_engine()
    if len(engines) >= 2:
        engines.pop(next(iter(engines)))
    engines[key] = eng
    return eng


def _rollout_or_yield(engines: Dict, key, eng, make_engine, amax: int, limit: int, session: bool = False, guided=None):
    """generator -> the engine after its rollout.  The reference's agent arrays grow without bound; here rows are pre-allocated
    per scene: if the inserted agents outgrow them the (deterministic) rollout is repeated with twice the rows (at most ``limit``,
    ``amax`` of them the scenes' own) instead of dropping insertions.  ``session``: yields the engine where ``rollout()`` would
    run - the caller steps a closed-loop session on it and resumes the generator for the epilogue - and otherwise never yields.
    ``guided``: the arguments of ``RolloutEngine.rollout_guided``, which then runs in place of ``rollout``."""
    while not session:
        try:
            if guided is not None:
                eng.rollout_guided(**guided)
            else:
                eng.rollout()
            return eng
        except InsertionHeadroomError:
            if eng.A_cap >= limit:
                raise
            eng = engines[key] = make_engine(headroom=min(2 * eng.A_cap, limit) - amax)
    yield eng
    return eng


class InfGenDecoder(nn.Module):

    def __init__(self, decoder_type: str, dataset: str, input_dim: int, hidden_dim: int, num_historical_steps: int,
                 pl2pl_radius: float, time_span: Optional[int], pl2a_radius: float, pl2seed_radius: float,
                 a2a_radius: float, a2sa_radius: float, pl2sa_radius: float, num_freq_bands: int, num_map_layers: int,
                 num_agent_layers: int, num_heads: int, head_dim: int, dropout: float, map_token: Dict,
                 token_size=512, attr_tokenizer: Attr_Tokenizer = None, predict_motion: bool = False,
                 predict_state: bool = False, predict_map: bool = False, predict_occ: bool = False,
                 use_grid_token: bool = True, use_head_token: bool = True, use_state_token: bool = True,
                 disable_insertion: bool = False, state_token: Dict[str, int] = None, seed_size: int = 5,
                 buffer_size: int = 32, num_recurrent_steps_val: int = -1, loss_weight: dict = None, logger=None) -> None:
        super().__init__()
        if decoder_type != 'agent_decoder':
            raise ValueError(f'Unsupport decoder type: {decoder_type} (the HIP path implements agent_decoder)')
        self.map_encoder = InfGenMapDecoder(dataset=dataset, input_dim=input_dim, hidden_dim=hidden_dim,
                                            num_historical_steps=num_historical_steps, pl2pl_radius=pl2pl_radius,
                                            num_freq_bands=num_freq_bands, num_layers=num_map_layers, num_heads=num_heads,
                                            head_dim=head_dim, dropout=dropout, map_token=map_token)
        self.agent_encoder = InfGenAgentDecoder(
            dataset=dataset, input_dim=input_dim, hidden_dim=hidden_dim, num_historical_steps=num_historical_steps,
            time_span=time_span, pl2a_radius=pl2a_radius, pl2seed_radius=pl2seed_radius, a2a_radius=a2a_radius,
            a2sa_radius=a2sa_radius, pl2sa_radius=pl2sa_radius, num_freq_bands=num_freq_bands, num_layers=num_agent_layers,
            num_heads=num_heads, head_dim=head_dim, dropout=dropout, token_size=token_size, attr_tokenizer=attr_tokenizer,
            predict_motion=predict_motion, predict_state=predict_state, predict_map=predict_map, predict_occ=predict_occ,
            state_token=state_token, use_grid_token=use_grid_token, use_head_token=use_head_token,
            use_state_token=use_state_token, disable_insertion=disable_insertion, seed_size=seed_size,
            buffer_size=buffer_size, num_recurrent_steps_val=num_recurrent_steps_val, loss_weight=loss_weight, logger=logger)
        ref = weakref.ref(self)
        self.map_encoder._owner = ref
        self.agent_encoder._owner = ref
        self.map_enc = None
        self.predict_motion, self.predict_state, self.predict_map, self.predict_occ = predict_motion, predict_state, predict_map, predict_occ
        self.data_keys = ["agent_valid_mask", "category", "valid_mask", "av_index", "scenario_id", "shape"]
        self._cfg_kw = dict(input_dim=input_dim, hidden_dim=hidden_dim, num_heads=num_heads, head_dim=head_dim,
                            num_freq_bands=num_freq_bands, num_map_layers=num_map_layers, num_agent_layers=num_agent_layers,
                            num_historical_steps=num_historical_steps, token_size=token_size, a2a_radius=a2a_radius,
                            pl2a_radius=pl2a_radius, pl2pl_radius=pl2pl_radius, a2sa_radius=a2sa_radius,
                            pl2sa_radius=pl2sa_radius, pl2seed_radius=pl2seed_radius,
                            time_span=time_span if time_span is not None else num_historical_steps,
                            seed_size=seed_size, buffer_size=buffer_size, disable_insertion=disable_insertion,
                            state_token=dict(state_token), use_grid_token=bool(use_grid_token),
                            use_head_token=bool(use_head_token), use_state_token=bool(use_state_token))
        # arithmetic of the rollout's GEMM kernels - the counterpart of the trainer's `precision` flag, which the reference's run.py
        # never passes (fp32): '32' (default) the fp32-accurate operand split; 'bf16' bf16 operands with fp32 accumulation (packs of
        # bf16 weights, InfgenOptions.gemm_terms = 2; BASELINE config C5); '16' fp16 operands (gemm_terms = 1).  Set it before a call.
        self.rollout_precision = '32'
        # True: inference / inference_batch / inference_rollouts (single graph or Batch) also return, per rollout,
        #   next_token_logprob [A][T_cols] float32   log-probability of the motion token the row emitted (laid out like next_token_idx)
        #   next_token_logprob_mask [A][T_cols] bool  decoded column, row alive, token >= 0, row neither replayed nor teacher-forced
        #   pred_prob [A][steps]                      exp(logprob) where masked, else 0 - the softmax probability of the chosen token, the
        #                                            array the reference allocates (agent_decoder.py:1689) and never fills (:2205)
        #   rollout_logprob                           the masked sum, float64 on the device ([B] for a Batch), added in a fixed order:
        #                                            bitwise reproducible, and the same from a Batch as from single calls
        # The value is the FULL-softmax log-probability; the probability renormalised over the top-k tokens, the distribution a
        # sampled rollout actually draws from, is ``sample_logprob``'s.  False (default): the dicts have exactly the keys they had.
        self.token_logprob = False
        # True: the same entries also return, per rollout, the probability under the sampler's OWN distribution (the softmax
        # re-normalised over the motion_beam_size best logits; what reweighting or fine-tuning on sampled rollouts needs)
        #   next_token_sample_logprob [A][T_cols] float32   laid out and masked like next_token_logprob (next_token_logprob_mask comes
        #                                                   with either flag); 0 where masked for a greedy rollout (a point mass)
        #   rollout_sample_logprob                          the masked sum, float64 on the device ([B] for a Batch), rollout_logprob's order
        # Independent of token_logprob.  False (default): the dicts have exactly the keys they had.
        self.sample_logprob = False
        # temperature and nucleus (top-p) truncation of the two top-k draws (RolloutEngine's arguments of the same names):
        # the motion token where motion_beam_size > 1 - sample_temperature may also hold one value per copy of inference_rollouts /
        # inference_batch(copies=n), 0 making that copy greedy - and the inserted agent's cell where insert_beam_size > 1.  The
        # defaults are the plain top-k samplers; next_token_logprob stays the model's own softmax at temperature 1.
        self.sample_temperature = 1.0
        self.sample_top_p = 1.0
        self.insert_temperature = 1.0
        self.insert_top_p = 1.0
        # constrained decoding (RolloutEngine's token_masks / token_mask_type): None, a constraints.TokenMasks - its own
        # per-type selection applies (TokenMasks.from_vocab) - or (TokenMasks, [vehicle, pedestrian, cyclist] set indices, -1 =
        # unconstrained).  Generated rows only emit motion tokens of their type's set; part of the engine cache key
        self.token_constraints = None
        # collision-aware decoding (RolloutEngine's avoid_collisions): False, True or dict(margin=, predict=).  Taken by
        # inference, inference_batch, inference_rollouts and closed_loop alike; part of the engine cache key
        self.avoid_collisions = False
        # road-aware decoding (RolloutEngine's stay_on_road): False, True or dict(margin=, sweep=, detail=, types=,
        # segments=).  Taken by the same entries; its settings are part of the engine cache key, explicit segments are contents that
        # every call loads again with its scenes
        self.stay_on_road = False
        # route-following decoding (RolloutEngine's follow_routes): False or dict(routes=, n_points=, corridor=, back=,
        # pace=, finish=, types=), routes [scenes][A][P][2] for the scenes of the call (with copies = n a scene's routes apply to each
        # of its copies).  Its scalars and P are part of the engine cache key; the routes are contents loaded with every call
        self.follow_routes = False
        # signal-aware decoding (RolloutEngine's obey_signals): False or dict(lines=, n_lines=, phase=, setback=, align=,
        # types=), lines [scenes][K][4] and phase [scenes][n_phase][K] for the scenes of the call (with copies = n a scene's lines
        # apply to each of its copies).  Its scalars, K and n_phase are part of the engine cache key; the tables are contents loaded
        # with every call
        self.obey_signals = False
        # step scores (RolloutEngine's step_scores): False, True or dict(road_margin=, sweep=, types=, detail=,
        # segments=, dt=) - every rollout dict then carries ``step_score`` [steps, 8]; keyed and loaded like stay_on_road.
        # guided_rollouts: None or a dict of RolloutEngine.rollout_guided's arguments (every=, keep=, weights=, u=): the copies of
        # inference_rollouts / inference_batch(copies=n) are pruned or resampled on those scores while they run
        self.step_scores = False
        self.guided_rollouts = None
        # insertion rules (RolloutEngine's insert_rules): None or dict(clearance=, ego_keepout=, edge_clearance=,
        # near_lane=, zones=, types=, max_agents=, per_step=); fixed per engine and part of its cache key (the zone table by content)
        self.insert_rules = None
        self._packed = None
        self._param_dicts = None
        self._last_w = None
        self._packed_ver = None
        self._engines = {}          # RolloutEngine per batch layout, reused across calls (RolloutEngine.reload)

    _PRECISIONS = {'32': None, 'bf16': {'gemm_terms': 2}, '16': {'gemm_terms': 1}}

    # ------------------------------------------------------------------ weights
    def _weights(self) -> PackedWeights:
        # every call checks that the packed copy still belongs to the module's parameters (their versions and storage); walking the
        # module tree for that took 3 ms of a 14 ms single-scene call, so the per-module parameter dicts are collected once (the
        # tree is built in __init__; a Parameter that is replaced inside its module is still seen - the dicts are read every call)
        if self._param_dicts is None:
            self._param_dicts = [m._parameters for m in self.modules() if m._parameters]
        ps = [p for d in self._param_dicts for p in d.values() if p is not None]
        dev = ps[0].device
        if dev.type != 'cuda':
            raise _lib.InfgenHipError('InfGenDecoder must live on a cuda device: the product path has no CPU fallback')
        tok = self.agent_encoder.attr_tokenizer
        R = self.agent_encoder.num_recurrent_steps_val
        # the rollout length and the tokenizer geometry are part of the key: changing num_recurrent_steps_val between calls
        # (80 -> 300 for long-term validation) must not be ignored
        prec = str(self.rollout_precision)
        if prec not in self._PRECISIONS:
            raise ValueError(f'rollout_precision must be one of {sorted(self._PRECISIONS)}, not {prec!r}')
        ver = (dev, tuple(p._version for p in ps), tuple(p.data_ptr() for p in ps), R, tok.grid_range, tok.grid_interval,
               tok.angle_interval, prec)
        if self._packed_ver != ver:
            cfg = RolloutConfig(num_recurrent_steps_val=R if R != -1 else 80, grid_range=tok.grid_range,
                                grid_interval=tok.grid_interval, angle_interval=tok.angle_interval, **self._cfg_kw)
            sd = {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}
            self._packed = PackedWeights(sd, cfg, dev, operand_bits=8 if prec == 'bf16' else 11)
            self._packed_ver = ver
            self._engines = {}
        return self._packed

    # ------------------------------------------------------------------ driver
    @staticmethod
    def _plan_list(replay_plan, counts) -> Optional[List[Dict]]:
        """``replay_plan`` (one dict over all rows in scene order, or one dict per scene) -> one dict per scene"""
        if replay_plan is None:
            return None
        if isinstance(replay_plan, (list, tuple)):
            if len(replay_plan) != len(counts):
                raise ValueError(f'replay_plan lists {len(replay_plan)} plans for {len(counts)} scenes')
            plans = [dict(p_) for p_ in replay_plan]
        else:
            scene_setup.check_plan(replay_plan)
            cut = {k_: torch.as_tensor(v_).split(list(counts)) for k_, v_ in replay_plan.items() if v_ is not None}
            plans = [{k_: v_[i] for k_, v_ in cut.items()} for i in range(len(counts))]
        for p_ in plans:
            scene_setup.check_plan(p_)
        return plans

    def _replay_forms(self, datas, stk, replay, replay_plan):
        """``replay`` / ``replay_plan`` of the public entries -> (device form for ``reload_device`` or None, a function that
        makes the per-scene host entries ``RolloutEngine(replay=...)`` takes).  The device form is built without a host copy."""
        if isinstance(replay, str) and replay != 'ego':
            raise ValueError(f"replay must be 'ego', a bool tensor or a list of bool tensors, not {replay!r}")
        counts = [int(d_['agent']['state_idx'].shape[0]) for d_ in datas]
        plans = self._plan_list(replay_plan, counts)
        if not isinstance(replay, str):                  # (the lengths are checked here, whichever path takes the batch)
            scene_setup.replay_rows(replay, counts, [0] * len(counts))
        dev_form = None
        if stk is not None:
            sag = stk['agent']
            S, A = (int(n) for n in sag['state_idx'].shape[:2])
            dev = sag['state_idx'].device
            if isinstance(replay, str):
                mask = torch.zeros(S, A, dtype=torch.bool, device=dev)
                mask.scatter_(1, sag['av_index'].reshape(S, -1)[:, :1].long(), True)
            else:
                mask = torch.stack([m.to(dev) for m in scene_setup.replay_rows(replay, counts, [0] * S)])
            dev_form = mask if plans is None else (mask, {k_: torch.stack([torch.as_tensor(p_[k_]).to(dev) for p_ in plans])
                                                          for k_ in scene_setup.PLAN_KEYS if plans[0].get(k_) is not None})

        def host_form():
            av = [int(_np(d_['agent']['av_index']).reshape(-1)[0]) for d_ in datas]
            masks = [_np(m) for m in scene_setup.replay_rows(replay, counts, av)]
            if plans is None:
                return masks
            return [(m, _np(p_['token_idx']), _np(p_['state_idx'])) +
                    ((_np(p_['token_pos']), _np(p_['token_heading'])) if p_.get('token_pos') is not None else ())
                    for m, p_ in zip(masks, plans)]
        return dev_form, host_form

    def _sampling_kw(self, n_scenes: int, copies: int, sample_temperature=None):
        """-> (the engine's constructor arguments, the value its reload* take): a scalar temperature, or one entry per copy spread
        over the agent-side scenes (scene i's copies are adjacent)"""
        t = np.asarray(self.sample_temperature if sample_temperature is None else sample_temperature, dtype=np.float32)
        if t.ndim == 0:
            temp = float(t)
        else:
            if t.shape != (copies,):
                raise ValueError(f'sample_temperature: a float or one value per copy ({copies}), got shape {t.shape}')
            temp = np.tile(t, n_scenes)
        # (the cell draw's two scalars are fixed per engine and key it; the motion draw's go through reload*, like the uniforms)
        fixed = dict(insert_temperature=float(self.insert_temperature), insert_top_p=float(self.insert_top_p))
        live = dict(sample_temperature=temp, sample_top_p=float(self.sample_top_p))
        key = tuple(fixed.values())
        tc = self.token_constraints
        if tc is not None:      # (fixed per engine: engines are not shared between different constraints)
            masks, sel = tc if isinstance(tc, (tuple, list)) else (tc, None)
            if not isinstance(masks, TokenMasks):
                raise ValueError('token_constraints: None, a TokenMasks or (TokenMasks, three per-type set indices)')
            sel = check_type_selectors(masks.type_sets if sel is None else sel, masks.n_sets)
            fixed.update(token_masks=masks, token_mask_type=sel)
            key += (masks.key(), tuple(sel))
        ac = check_avoid_collisions(self.avoid_collisions)
        if ac is not None:      # (fixed per engine, like the constraints)
            fixed.update(avoid_collisions=ac)
            key += (('avoid_collisions', ac['margin'], ac['predict']),)
        sr = check_stay_on_road(getattr(self, 'stay_on_road', False))      # (absent on a bare argument holder: off)
        if sr is not None:
            key += (('stay_on_road',) + road_key(sr),)
            if sr['segments'] is None:
                fixed.update(stay_on_road=sr)
            else:      # (world coordinates of this call's scenes: loaded with them, like the uniforms)
                live.update(stay_on_road=sr)
        fr = check_follow_routes(getattr(self, 'follow_routes', False), n_scenes=n_scenes)
        if fr is not None:      # (the engine takes the caller's own form; the waypoints are world coordinates of this call's scenes)
            key += (('follow_routes',) + route_key(fr) + (int(fr['routes'].shape[2]),),)
            live.update(follow_routes=self.follow_routes)
        og = check_obey_signals(getattr(self, 'obey_signals', False), n_scenes=n_scenes)      # (absent on a bare argument holder: off)
        if og is not None:      # (the engine takes the caller's own form; lines and phase are contents of this call's scenes)
            key += (('obey_signals',) + signal_key(og),)
            live.update(obey_signals=self.obey_signals)
        ss = check_step_scores(getattr(self, 'step_scores', False), stay_on_road=sr)
        if getattr(self, 'guided_rollouts', None) is not None and ss is None:
            raise ValueError('guided_rollouts needs step_scores')
        if ss is not None:
            key += (('step_scores',) + score_key(ss),)
            # (the engine takes the caller's own form: its check resolves it against its road table; explicit segments are
            # contents of this call's scenes, loaded with them)
            (fixed if ss['segments'] is None else live).update(step_scores=self.step_scores)
        ir = getattr(self, 'insert_rules', None)
        if ir is not None:      # (checked by the engine against its own scene counts; keyed by value, arrays by their bytes)
            if not isinstance(ir, dict):
                raise ValueError('insert_rules: None or dict(clearance=, ego_keepout=, edge_clearance=, near_lane=, zones=, types=, '
                                 'max_agents=, per_step=)')
            fixed.update(insert_rules=ir)
            by_value = lambda v: (tuple(np.asarray(x).tobytes() for x in v) if isinstance(v, tuple) and len(v) == 2 and np.ndim(v[0]) >= 2
                                  else np.asarray(v).tobytes() if isinstance(v, (np.ndarray, list)) else repr(v))
            key += (('insert_rules',) + tuple((k, by_value(v)) for k, v in sorted(ir.items())),)
        return dict(fixed, **live), live, key

    def _guided(self, copies: int):
        """``guided_rollouts`` as ``_rollout_or_yield`` takes it: None, or the driver's arguments (a dict)"""
        g = getattr(self, 'guided_rollouts', None)
        if g is None:
            return None
        if not isinstance(g, dict) or set(g) - {'every', 'keep', 'weights', 'u'}:
            raise ValueError('guided_rollouts: None or dict(every=, keep=, weights=, u=)')
        if int(copies) <= 1:
            raise ValueError('guided_rollouts needs copies > 1 (inference_rollouts, or inference_batch(copies=n))')
        return dict(g)

    @staticmethod
    def _drive(gen):
        """runs ``_run_gen`` / ``_run_graphs_gen`` / ``_inference_gen`` to the end -> its result (without ``session`` they never yield)"""
        try:
            next(gen)
        except StopIteration as e:
            return e.value
        raise RuntimeError('the run yielded an engine: only closed_loop() asks for a session')

    def _run(self, *args, **kw):
        return self._drive(self._run_gen(*args, **kw))

    def _begin(self, columns: int, replay, replay_plan):
        """what every rollout call starts with -> (the packed weights, motion_beam_size, insert_beam_size, DEBUG).  ``columns``: the
        time steps of the data's ``agent.position``, which set an unset rollout length."""
        if replay is None and replay_plan is not None:
            raise ValueError('replay_plan overrides the logged future of the rows replay= flags: give replay= too')
        ae = self.agent_encoder
        w = self._last_w = self._weights()
        if ae.num_recurrent_steps_val == -1:
            # sticky like the reference (agent_decoder.py:1633-1635)
            ae.num_recurrent_steps_val = int(columns) - ae.num_historical_steps
            w.cfg.num_recurrent_steps_val = ae.num_recurrent_steps_val
        w.cfg.disable_insertion = bool(ae.disable_insertion)
        # DEBUG=1 forces 'enter' (agent_decoder.py:1888)
        return w, int(getattr(ae, 'motion_beam_size', 1)), int(getattr(ae, 'insert_beam_size', 1)), bool(int(os.getenv('DEBUG', 0)))

    def _make_engine(self, w, facts: Dict, tables, uniforms, skw: Dict, source, headroom=None):
        """the facts ``_engine_key`` keys + the call's arrays -> a new engine.  ``tables``: (vocab, map_vocab, grid); ``source()``:
        the arguments of the data's form - scenes / x_pt_override of the list path, batch / batch_layout of a Batch, and replay in
        the form that path takes (made when an engine is built: the list path's costs a host copy)."""
        f = facts
        agents = not f['map_only']
        return RolloutEngine(w, vocab=tables[0], map_vocab=tables[1], grid=tables[2], insert_headroom=headroom,
                             force_enter=f['debug'], sample_k=f['sample_k'], sample_uniforms=uniforms[0], insert_k=f['insert_k'],
                             insert_uniforms=uniforms[1],
                             # the seed node's per-insertion outputs (plot inputs of the reference, 5.5 MB per scene): the
                             # single-scene entry, the n-copies batch of inference_rollouts and a Batch; the throughput entry
                             # (inference_batch) returns the zero arrays the reference initialises them to
                             seed_outputs=(f['single'] or f['seed_outputs']) and not f['disable_insertion'] and agents,
                             copies=f['copies'], options=self._PRECISIONS[str(self.rollout_precision)],
                             token_logprob=f['token_logprob'] and agents, sample_logprob=f['sample_logprob'] and agents,
                             **skw, **source())

    def _decorate(self, eng, rows, zeros):
        """completes epilogue dicts to the reference's key set.  ``rows``: per dict (o, sel, n_graphs, n_rows, inserted) - ``o`` one
        scene's LazyOut of the list path (its pending values stay pending) or a copy's dict over the ``n_graphs`` graphs of a Batch,
        ``sel`` its scenes in the engine's batch (an index or a slice), ``n_rows`` its agent rows, ``inserted`` the inserted agents
        per scene.  ``zeros(shape)`` makes the arrays nothing was recorded for."""
        cfg = eng.cfg
        steps, G, T_cols, hc = cfg.num_decode_steps, self.agent_encoder.grid_size, cfg.num_columns, cfg.hist_columns
        # without insertion (or in the batched entry) the seed node's outputs stay what the reference initialises them to
        # (:1746-1750, :1730), 11 rows per scene; use_grid_token = False: the grid's are None (reference :2376-2386)
        seed = [(k_, (steps,) if k_in == 'state' else (steps, G), cfg.use_grid_token or k_in == 'state') for k_, k_in in eng._SEED_KEYS]
        lp = eng.rollout_logprob() if eng.token_logprob is not None else None
        slp = eng.rollout_sample_logprob() if eng.sample_logprob is not None else None
        for o, sel, n_graphs, n_rows, inserted in rows:
            put = o.set_lazy if isinstance(o, LazyOut) else (lambda k_, thunk, o=o: o.__setitem__(k_, thunk()))
            for k_, shape, recorded in seed:
                if k_ not in o:
                    o[k_] = zeros((n_graphs * 11,) + shape) if recorded else None
            if 'agent_labels' not in o:
                put('agent_labels', lambda n=n_rows: [[None] * T_cols for _ in range(n)])
            if lp is not None:
                put('pred_prob', lambda o=o: logprob.pred_prob(o['next_token_logprob'], o['next_token_logprob_mask'], hc, steps))
                o['rollout_logprob'] = lp[sel]
            if slp is not None:
                o['rollout_sample_logprob'] = slp[sel]
            if eng.step_scores is not None:         # [steps, 8] of the rollout (a copy's dict over B graphs: [B, steps, 8])
                o['step_score'] = eng.step_score[sel].clone()
            o['log_message'] = '\n'.join('No agents inserted!' if x == 0 else f'Number of total inserted agents: {x}' for x in inserted)

    def _run_gen(self, data, x_pt=None, map_only=False, batch: Optional[Sequence] = None, sample_uniforms=None,
                 batch_seed_outputs: bool = False, copies: int = 1, replay=None, replay_plan=None, sample_temperature=None,
                 session: bool = False):
        """one scene, or a list of scenes (``batch``), through per-scene host dicts or a stacked device batch.  A generator (see
        ``_rollout_or_yield``): only ``closed_loop`` asks for a ``session``."""
        datas = list(batch) if batch is not None else [data]
        copies = int(copies)
        skw, live, skey = self._sampling_kw(len(datas), copies, sample_temperature)
        # copies = n: every scene of the batch is decoded n times in lockstep over ONE map encoding (RolloutEngine(copies=n));
        # the result list holds scene 0's n rollouts, then scene 1's, ...
        # a batch of device tensors of one shape is set up on the device (RolloutEngine.reload_device); its host form is only made
        # when something reads it (a new engine, a filtered row, the host-side outputs)
        stk = stack_datas(datas) if batch is not None and copies == 1 else None
        scenes = _LazyScenes(datas) if stk is not None else scenes_from_datas(datas)
        rp_dev, rp_host = self._replay_forms(datas, stk, replay, replay_plan) if replay is not None else (None, lambda: None)
        ag0 = datas[0]['agent']
        w, k, ik, debug = self._begin(ag0['position'].shape[1], replay, replay_plan)
        cfg = w.cfg
        if map_only:
            k = ik = 1
        vocab = {k_: _np(ag0[f'trajectory_token_{k_}']) for k_ in ('veh', 'ped', 'cyc')}
        map_vocab = _np(self.map_encoder.map_token['traj_src']).astype(np.float32)
        grid = self.agent_encoder.attr_tokenizer.grid.detach().cpu().numpy()
        xo = None
        if x_pt is not None:
            xo = [x_pt] if batch is None else list(x_pt)
        limit = int(_lib.load().infgen_layout_query(_lib.Q_MAX_AGENTS))
        ucols = max(int(d_['agent']['state_idx'].shape[0]) for d_ in datas) if cfg.disable_insertion else limit
        su, iu = _draw_uniforms(cfg, k, ik, len(datas) * copies, ucols, sample_uniforms)
        facts = dict(graphs=False, scenes=len(datas), disable_insertion=cfg.disable_insertion, steps=cfg.num_recurrent_steps_val,
                     tables=PackedWeights.tables_key(*(vocab[k_] for k_ in ('veh', 'ped', 'cyc')), grid, map_vocab),
                     sample_k=k, insert_k=ik if iu is not None else 1, debug=debug, copies=copies, replay=replay is not None,
                     token_logprob=bool(self.token_logprob), sample_logprob=bool(self.sample_logprob), sampling=skey,
                     single=batch is None, map_only=map_only, own_map=xo is None, seed_outputs=bool(batch_seed_outputs))
        ekey = _engine_key(**facts)
        make_engine = functools.partial(self._make_engine, w, facts, (vocab, map_vocab, grid), (su, iu), skw,
                                        lambda: dict(scenes=scenes, x_pt_override=xo, replay=rp_host()))
        up = dict(sample_uniforms=su, insert_uniforms=iu, x_pt_override=xo, **live)
        attempts = [(lambda e: e.fits(scenes), lambda e: e.reload(scenes, replay=rp_host(), **up))]
        if stk is not None:
            attempts.insert(0, (lambda e: e.fits_device(stk), lambda e: e.reload_device(stk, scenes, replay=rp_dev, **up)))
        eng = _cached_engine(self._engines, ekey, attempts, make_engine)
        if map_only:
            eng.prologue(map_only=True)
            return eng.x_pt[:eng.hosts[0]['M']].clone(), self._map_keys(eng, datas)[0]
        # (the scenes' own rows: their kept counts, which this path knows on the host and sizes the engine's rows from)
        eng = yield from _rollout_or_yield(self._engines, ekey, eng, make_engine, max(h['A'] for h in eng.hosts), limit, session,
                                           self._guided(copies))
        # the map-token head once per distinct scene (not with a caller's map encoding: inference_no_map passes its map_enc through)
        mk = self._map_keys(eng, datas) if xo is None else None
        # per-scene dicts of device tensors (no host round trip of the results), detached from the engine's buffers
        outs = eng.outputs_device(detach=True)
        self._last_engine = eng                 # (predict_modes reads the copies' pred_traj where the rollout left it)
        zero = {}                              # shared (read-only) zero tensors of the seed outputs a batch does not record

        def zeros(shape):
            if shape not in zero:
                zero[shape] = torch.zeros(shape, device=w.device)
            return zero[shape]
        if copies > 1:                          # scene i's copies are adjacent in the engine's batch
            datas = [d_ for d_ in datas for _ in range(copies)]
        # (a LazyOut per scene: its views are cut when a key is read, not here)
        self._decorate(eng, ((r, i_, 1, eng.hosts[i_]['A'] + r['num_inserted'], (r['num_inserted'],)) for i_, r in enumerate(outs)), zeros)
        for i_, (d, r) in enumerate(zip(datas, outs)):
            if mk is not None:                      # (copies of a scene share its tensors)
                for k_, v_ in mk[i_ // copies].items():
                    r[k_] = v_
            # the callee mutates data['batch_size_a'] like the reference (agent_decoder.py:1649)
            try:
                filt = eng.hosts[i_]['filt']
                if not filt.all():
                    av0 = int(np.asarray(scenes[i_ // copies]['agent']['av_index']).reshape(-1)[0])
                    removed = int((~filt[:av0]).sum())
                    if removed and i_ % copies == 0:          # (once per data object)
                        d['batch_size_a'] -= removed
            except (KeyError, TypeError):
                pass
        return outs if batch is not None else outs[0]

    def _empty_map_keys(self, dev) -> Dict[str, torch.Tensor]:
        return {'map_next_token_idx': torch.zeros(0, 10, dtype=torch.long, device=dev),
                'map_next_token_prob': torch.zeros(0, self.map_encoder.token_size, device=dev),
                'map_next_token_idx_gt': torch.zeros(0, dtype=torch.long, device=dev),
                'map_next_token_eval_mask': torch.zeros(0, dtype=torch.bool, device=dev)}

    def _gt_keys(self, data, dev) -> Dict[str, torch.Tensor]:
        """the empty head keys plus token_idx[pt_target_mask] (map_decoder.py:122) when the data carries the mask"""
        k = self._empty_map_keys(dev)
        tm = _pt_mask(data, 'pt_target_mask')
        if tm is not None:
            k['map_next_token_idx_gt'] = torch.as_tensor(data['pt_token']['token_idx']).to(dev)[tm.to(dev)]
        return k

    def _map_keys(self, eng: RolloutEngine, datas: Sequence) -> List[Dict[str, torch.Tensor]]:
        """the map-token head's keys of the reference's map encoder (map_decoder.py:119-129) for the distinct map scenes of ``eng``
        (map scene i = datas[i]): logits and top-10 of the pt_pred_mask rows, token_idx[pt_target_mask], the all-True evaluation
        mask.  One count read for all scenes, and one head launch when some scene has predicted rows."""
        dev = eng.device
        out = [self._gt_keys(d, dev) for d in datas]
        masks = [_pt_mask(d, 'pt_pred_mask') for d in datas]
        if all(m is None for m in masks):
            return out
        M = [int(d['pt_token']['position'].shape[0]) for d in datas]
        pm = torch.cat([(m if m is not None else torch.zeros(Mi, dtype=torch.bool)).to(dev) for m, Mi in zip(masks, M)])
        off = np.concatenate([[0], np.cumsum(M)]).astype(np.int64)
        ends = torch.nn.functional.pad(torch.cumsum(pm, 0), (1, 0))[torch.from_numpy(off).to(dev)].cpu().numpy()
        cnt, n = np.diff(ends), int(ends[-1])
        if n == 0:
            return out
        base = np.repeat(np.arange(len(M), dtype=np.int64) * eng.M_cap - off[:-1], M)
        rowmap = torch.arange(int(off[-1]), device=dev) + torch.from_numpy(base).to(dev)
        lg, top = eng.map_token_head(_scatter_rows(pm, rowmap, n))
        o = 0
        for i, c_ in enumerate(cnt.tolist()):
            if c_:
                out[i].update(map_next_token_idx=top[o:o + c_], map_next_token_prob=lg[o:o + c_],
                              map_next_token_eval_mask=torch.ones(c_, dtype=torch.bool, device=dev))
            o += c_
        return out

    _HOST_CACHE = 4             # entries of each host-copy cache below

    @staticmethod
    def _tensor_key(t):
        """identity of a tensor's contents for the host-copy caches: address, layout and version counter.  The cache entry
        keeps the tensor itself alive, so its storage cannot be freed and handed to another tensor while the key is held."""
        return (t.device, t.data_ptr(), t.dtype, tuple(t.shape), tuple(t.stride()), t._version)

    def _cached(self, name, tensors, make):
        cache = self.__dict__.setdefault(name, {})
        key = tuple(self._tensor_key(t) for t in tensors)
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= self._HOST_CACHE:
                cache.pop(next(iter(cache)))
            hit = cache[key] = (tuple(tensors), make())
        return hit[1]

    def _host_const(self, t):
        """host copy of a module constant (grid, map vocabulary), made again only when the tensor changes"""
        if not isinstance(t, torch.Tensor):
            return np.asarray(t)
        return self._cached('_host_consts', [t], lambda: t.detach().cpu().numpy())

    def _run_graphs(self, *args, **kw) -> List[Dict]:
        return self._drive(self._run_graphs_gen(*args, **kw))

    def _run_graphs_gen(self, data, sample_uniforms=None, copies: int = 1, mutate: bool = True, replay=None,
                        replay_plan=None, sample_temperature=None, session: bool = False):
        """a ragged multi-graph Batch of device tensors through RolloutEngine.reload_batch (the ingest kernel: filter, pad and
        set up every scene on the device) and the batched epilogue (outputs_batch: infgen_pack_rows).  One device -> host copy
        before the first launch (the offsets and av_index; the token vocabularies the tables are keyed by ride along unless the
        same vocabulary tensors were seen before) and one after the rollout (the agent counts).  -> ``copies`` dicts.  A
        generator like ``_run_gen``."""
        ae = self.agent_encoder
        ag = data['agent']
        copies = int(copies)
        w, k, ik, debug = self._begin(ag['position'].shape[1], replay, replay_plan)
        cfg = w.cfg
        limit = int(_lib.load().infgen_layout_query(_lib.Q_MAX_AGENTS))
        ts = cfg.token_size
        voc_t = [torch.as_tensor(ag[f'trajectory_token_{k_}']) for k_ in ('veh', 'ped', 'cyc')]
        map_vocab = np.asarray(self._host_const(self.map_encoder.map_token['traj_src']), np.float32)
        grid = self._host_const(ae.attr_tokenizer.grid)
        # the token vocabularies key the engine's tables by content: their host copy (1.2 MB) and hash are made once per set of
        # vocabulary tensors - the TokenProcessor hands the same module buffers every call; other tensors ride along with the
        # offsets in the one host copy
        cache = self.__dict__.setdefault('_vocab_host', {})
        src = self.map_encoder.map_token['traj_src'], ae.attr_tokenizer.grid
        keep = list(voc_t) + [t for t in src if isinstance(t, torch.Tensor)]
        # cached only for one table per type (what the TokenProcessor hands over): a collated Batch's per-graph copies are new
        # tensors every batch and would only be kept alive here; host-array constants have no identity to key by
        cacheable = all(isinstance(t, torch.Tensor) for t in src) and all(int(t.shape[0]) == ts for t in voc_t)
        key = tuple(self._tensor_key(t) for t in keep)
        hit = cache.get(key) if cacheable else None
        # the map-token head's row count per graph rides along too: the running count of pt_pred_mask at every pt_token.ptr entry
        pm = _pt_mask(data, 'pt_pred_mask')
        pm_ext = []
        if pm is not None:
            pm = pm.to(torch.as_tensor(ag['ptr']).device)
            mptr_d = torch.as_tensor(data['pt_token']['ptr']).to(pm.device, torch.int64)
            pm_ext = [torch.nn.functional.pad(torch.cumsum(pm, 0), (1, 0))[mptr_d]]
        lay = read_batch_layout(data, cfg.num_columns, cfg.hist_columns, limit,
                                extra=(() if hit is not None else tuple(t[:ts] for t in voc_t)) + tuple(pm_ext))
        if hit is None:
            vocab_ = {k_: np.asarray(v, np.float32) for k_, v in zip(('veh', 'ped', 'cyc'), lay['extra'])}
            tkey_ = PackedWeights.tables_key(*(vocab_[k_] for k_ in ('veh', 'ped', 'cyc')), grid, map_vocab)
            hit = (tuple(keep), vocab_, tkey_)
            if cacheable:
                if len(cache) >= self._HOST_CACHE:
                    cache.pop(next(iter(cache)))
                cache[key] = hit
        _, vocab, tkey = hit
        B = lay['B']
        skw, live, skey = self._sampling_kw(B, copies, sample_temperature)
        su, iu = _draw_uniforms(cfg, k, ik, B * copies, lay['amax'] if cfg.disable_insertion else limit, sample_uniforms)
        # log replay: the row mask in the Batch's global row order, on its device (the ingest kernel applies the row filter)
        rp = None
        if replay is not None:
            st_idx = torch.as_tensor(ag['state_idx'])
            rp = scene_setup.replay_global(replay, int(st_idx.shape[0]), torch.as_tensor(ag['av_index']).to(st_idx.device), B)
            if replay_plan is not None:
                if isinstance(replay_plan, (list, tuple)):
                    replay_plan = {k_: torch.cat([torch.as_tensor(p_[k_]) for p_ in replay_plan])
                                   for k_ in scene_setup.PLAN_KEYS if replay_plan[0].get(k_) is not None}
                scene_setup.check_plan(replay_plan)
                rp = (rp, {k_: v_ for k_, v_ in replay_plan.items() if v_ is not None})
        # (a Batch's rollouts always record the seed node's outputs)
        facts = dict(graphs=True, scenes=B, tables=tkey, disable_insertion=cfg.disable_insertion, steps=cfg.num_recurrent_steps_val,
                     sample_k=k, insert_k=ik if iu is not None else 1, debug=debug, copies=copies, replay=replay is not None,
                     token_logprob=bool(self.token_logprob), sample_logprob=bool(self.sample_logprob), sampling=skey,
                     single=False, map_only=False, own_map=True, seed_outputs=True)
        ekey = _engine_key(**facts)
        make_engine = functools.partial(self._make_engine, w, facts, (vocab, map_vocab, grid), (su, iu), skw,
                                        lambda: dict(scenes=None, batch=data, batch_layout=lay, replay=rp))
        eng = _cached_engine(self._engines, ekey, [(lambda e: e.fits_batch(lay), lambda e: e.reload_batch(
            data, sample_uniforms=su, insert_uniforms=iu, layout=lay, replay=rp, **live))], make_engine)
        # (the scenes' own rows: the kept counts stay on the device until the rollout is over - the engine's rows are sized from
        # the layout's unfiltered maximum, which the offsets give on the host, and so is the retry's head-room)
        eng = yield from _rollout_or_yield(self._engines, ekey, eng, make_engine, lay['amax'], limit, session, self._guided(copies))
        outs = eng.outputs_batch()
        self._last_engine = eng
        n_fin, c = eng.batch_counts()
        dev = w.device
        # the map-token head once per graph, one launch: the predicted rows of the Batch in graph order (graph g's token p sits at
        # row g * M_cap + p - ptr[g] of the engine's map encoding), shared by every copy
        map_keys = self._gt_keys(data, dev)
        n_pred = int(lay['extra'][-1][-1]) if pm is not None else 0
        if n_pred:
            ar = torch.arange(pm.numel(), device=pm.device)
            g = torch.searchsorted(mptr_d[1:], ar, right=True)
            lg, top = eng.map_token_head(_scatter_rows(pm, ar - mptr_d[g] + g * eng.M_cap, n_pred))
            map_keys.update(map_next_token_idx=top, map_next_token_prob=lg,
                            map_next_token_eval_mask=torch.ones(n_pred, dtype=torch.bool, device=dev))
        passthrough = {k_: data[k_] for k_ in self.data_keys if k_ in data}
        # (copy j's scenes are j, j + copies, ... of the engine's batch)
        self._decorate(eng, ((o, slice(j, None, copies), B, int(n_fin[j::copies].sum()), (n_fin - c[:, 0])[j::copies].tolist())
                             for j, o in enumerate(outs)), lambda shape: torch.zeros(shape, device=dev))
        res = [{**map_keys, **o, **passthrough} for o in outs]
        # the callee mutates data['batch_size_a'] like the reference (agent_decoder.py:1649), per graph
        removed = c[::copies, 2]
        if mutate and removed.any() and 'batch_size_a' in data:
            try:
                bsa = data['batch_size_a']
                bsa -= torch.as_tensor(removed, device=bsa.device, dtype=bsa.dtype) if isinstance(bsa, torch.Tensor) else removed
                data['batch_size_a'] = bsa
            except (KeyError, TypeError):
                pass
        return res

    def get_agent_inputs(self, data) -> Dict[str, torch.Tensor]:
        """the arrays of the reference's ``get_inputs`` (agent_decoder.py:933-992) that ``InfGen.check_inputs`` reads, as written
        there - ``next_state_idx_gt`` is the rolled TOKEN index (:947) -, on the data's device.  ``next_token_eval_mask`` (a Python
        loop over the enter / exit positions, :949-979; check_inputs clones it and never reads it) is not built."""
        ag = data['agent']
        tok = ag['token_idx']
        return {'token_pos': ag['token_pos'].clone(), 'token_heading': ag['token_heading'].clone(),
                'next_token_idx_gt': tok.roll(shifts=-1, dims=1), 'next_state_idx_gt': tok.roll(shifts=-1, dims=1),
                'raw_agent_valid_mask': ag['raw_agent_valid_mask'], 'state_token': ag['state_idx'].clone(),
                'grid_index': ag['grid_token_idx']}

    @torch.no_grad()
    def forward(self, data) -> Dict[str, torch.Tensor]:
        """map encoder + teacher-forced forward over every token column of the batch (reference infgen_decoder.py:114-121,
        agent_decoder.py:1104-1603) on the GPU (infgen_amd/forward_engine.py).  Evaluation only (no autograd
        through the HIP kernels).  The candidate rows of the refine stage and the neighbour-grid evaluation masks are drawn
        with ``torch.randperm`` from torch's CPU generator in the reference's order."""
        from ..forward_engine import ForwardEngine
        if self.map_only():
            return self._map_model(data)
        ae = self.agent_encoder
        for flag in ('use_grid_token', 'use_head_token', 'use_state_token'):
            if not getattr(ae, flag):
                raise NotImplementedError(f'InfGenDecoder.forward (teacher-forced) implements the full-token model only: {flag} is False '
                                          f'(the ablation models roll out through inference)')
        w = self._weights()                 # (raises on a CPU module: no CPU fallback)
        batch = batch_from_data(data)
        vocab = {k: batch['agent'][f'trajectory_token_{k}'] for k in ('veh', 'ped', 'cyc')}
        map_vocab = _np(self.map_encoder.map_token['traj_src']).astype(np.float32)
        grid = self.agent_encoder.attr_tokenizer.grid.detach().cpu().numpy()
        fe = ForwardEngine(w, batch, vocab, map_vocab, grid)
        out = fe.run()
        map_enc = self._flat_map_keys(out['x_pt'], data, fe.ops, w)
        return {**map_enc, **out, **{k: data[k] for k in self.data_keys if k in data}}

    def _flat_map_keys(self, x_pt, data, ops, w) -> Dict[str, torch.Tensor]:
        """the head's keys over an x_pt that holds the (batched) tokens in their own order: the rows are the mask's indices (one
        count read, like the reference's boolean index)"""
        dev = w.device
        keys = self._gt_keys(data, dev)
        pm = _pt_mask(data, 'pt_pred_mask')
        if pm is not None:
            rows = pm.to(dev).nonzero().reshape(-1)
            if rows.numel():
                lg, top = ops.map_token_head(x_pt, rows.to(torch.int32), w.map_head)
                keys.update(map_next_token_idx=top, map_next_token_prob=lg,
                            map_next_token_eval_mask=torch.ones(rows.numel(), dtype=torch.bool, device=dev))
        return keys

    def map_only(self) -> bool:
        """the map-pretraining model (configs/pretrain_scalable_map.yaml): no agent prediction, only the map-token head"""
        return not (self.predict_motion or self.predict_state or self.predict_occ)

    def _map_model(self, data) -> Dict[str, torch.Tensor]:
        """forward / inference of the map-pretraining model (infgen_decoder.py:114-130 with predict_motion / _state / _occ False): the
        map encoder's dict plus the data keys.  No agent decoding and no RolloutEngine: the map encoder runs alone
        (forward_engine.MapEncoder; a Batch's graphs through pt_token.ptr)"""
        from ..forward_engine import MapEncoder
        w = self._weights()
        pt = data['pt_token']
        ptd = {k: _np(pt[k]) for k in ('position', 'orientation', 'type', 'pl_type', 'token_idx')}
        ptd['ptr'] = _np(pt['ptr']) if 'ptr' in pt else np.array([0, ptd['position'].shape[0]], np.int64)
        key = ('pt_token', 'to', 'map_polygon')
        try:
            e = data[key]['edge_index']
        except (KeyError, TypeError):
            e = data['pt_token__to__map_polygon']['edge_index']
        enc = MapEncoder(w, {'pt_token': ptd, 'map_polygon': {'light_type': _np(data['map_polygon']['light_type'])},
                             'pt_token__to__map_polygon': {'edge_index': _np(e)}},
                         np.asarray(self._host_const(self.map_encoder.map_token['traj_src']), np.float32))
        x_pt = enc.run()
        return {'x_pt': x_pt, **self._flat_map_keys(x_pt, data, enc.ops, w), **{k: data[k] for k in self.data_keys if k in data}}

    @torch.no_grad()
    def inference(self, data, sample_uniforms=None, replay=None, replay_plan=None) -> Dict[str, torch.Tensor]:
        """map encoder + closed-loop rollout of one scene (reference infgen_decoder.py:123-130).
        Greedy unless ``agent_encoder.motion_beam_size > 1``; then tokens are drawn by inverse CDF over the
        top-k probabilities with ``sample_uniforms`` ([steps][1][A]) or torch.rand when omitted.
        A multi-graph ``data`` (a PyG-style Batch: ``num_graphs > 1`` / ``agent.ptr`` of more than 2 entries, ``av_index`` in
        the global form) is decoded as B scenes in lockstep (``_run_graphs``): one dict whose per-agent arrays concatenate the
        graphs' rows in graph order, with ``agent_batch`` / ``agent_ptr`` and ``ego_index`` [B]; ``sample_uniforms`` is then
        [steps][B][cols], graph s's slice indexed like a single-graph call's; cols must cover every graph's row count BEFORE
        the filter of agent_decoder.py:1609 (with insertion on: INFGEN_Q_MAX_AGENTS), since the kept counts are only known on
        the device when the uniforms are checked.
        The map-pretraining model (predict_motion / predict_state / predict_occ all False) returns the map encoder's dict plus the
        data keys, single graph or Batch, as the reference does (``_map_model``).
        ``replay`` (log replay; None: every agent is generated): 'ego', a bool tensor over ``data['agent']`` rows (the global row
        order of a Batch) or a list of such tensors, one per graph - the flagged agents follow their logged future (token_idx /
        state_idx / token_pos / token_heading from column hist_columns on) and the others are generated around them;
        ``replay_plan`` = dict(token_idx, state_idx[, token_pos, token_heading]) over the same rows replaces the logged future
        (a planner in the loop).  The dict then carries ``replay_mask`` (bool per returned row, after the row filter; inserted
        agents False); the flagged rows' ``next_token_idx`` / ``next_state_idx`` / ``pos_a`` / ``head_a`` are the plan's and their
        ``pred_traj`` / ``pred_head`` the plan's tokens integrated from the plan's poses."""
        if self.map_only():
            return self._map_model(data)
        return self._drive(self._inference_gen(data, sample_uniforms, replay, replay_plan))

    def _inference_gen(self, data, sample_uniforms=None, replay=None, replay_plan=None, session: bool = False):
        if num_graphs(data) > 1:
            rs = yield from self._run_graphs_gen(data, sample_uniforms=sample_uniforms, replay=replay, replay_plan=replay_plan,
                                                 session=session)
            return rs[0]
        r = yield from self._run_gen(data, sample_uniforms=sample_uniforms, replay=replay, replay_plan=replay_plan, session=session)
        x_pt = r.pop('x_pt')
        return r.merged(first={'x_pt': x_pt, **self._empty_map_keys(x_pt.device)}, last={k: data[k] for k in self.data_keys if k in data})

    @torch.no_grad()
    def closed_loop(self, data, controlled='ego', pose: str = 'token', idm=None):
        """a closed-loop stepping session over ``data`` (one graph or a Batch; infgen_amd/closed_loop.py): the
        ``controlled`` rows - 'ego' or a bool tensor / list of tensors as ``inference(replay=...)`` takes - are commanded step by
        step (``ses.observe()``, ``ses.command(tokens= | poses=)``, ``ses.advance()``), every other agent is generated around
        them.  ``pose``: 'token' stores the commanded / matched token's integration, 'exact' the commanded pose itself.  After
        the last step ``ses.outputs()`` is the dict ``inference(data, replay=controlled, replay_plan=<the commands>)`` returns,
        ``replay_mask`` included.  The engine is the cached one of ``inference``: another call on this module ends the session.
        ``idm=dict(routes=, n_points=, v_des=, ...)`` (the arguments of ``ClosedLoopSession.command_idm``; an empty dict reads the
        tables of ``follow_routes``): the controlled rows are driven by the rule-based IDM route follower to the last step
        (``closed_loop.run_idm``) and the finished outputs are returned instead of the session."""
        if self.map_only():
            raise ValueError('the map-pretraining model decodes no agents: nothing to control')
        gen = self._inference_gen(data, None, controlled, None, session=True)
        eng = next(gen)

        def finish():
            with torch.no_grad():
                return self._drive(gen)
        ses = ClosedLoopSession(eng, pose=pose, finish=finish)
        if idm is None:
            return ses
        return run_idm(ses, **idm).outputs()

    @torch.no_grad()
    def inference_no_map(self, data, map_enc) -> Dict[str, torch.Tensor]:
        r = self._run(data, x_pt=map_enc['x_pt'])
        r.pop('x_pt')
        return r.merged(first=map_enc)

    @torch.no_grad()
    def inference_rollouts(self, data, n: int, replay=None, replay_plan=None, sample_temperature=None,
                           sample_uniforms=None) -> List[Dict[str, torch.Tensor]]:
        """``n`` independent rollouts of ONE scene (the reference's ``n_rollout_close_val`` loop, infgen/model/infgen.py:704-706,
        which calls ``inference(data.clone())`` n times) as one batch of n copies decoded in lockstep: with
        ``motion_beam_size`` / ``insert_beam_size`` > 1 every copy draws its own uniforms from torch's RNG, so the results are n
        samples; greedy copies are identical.  ``data`` itself is not mutated (the copies are).  ``replay`` / ``replay_plan``
        as in ``inference``: every copy replays the same plan.  ``sample_temperature``: one temperature per copy (a sweep in one
        batch; 0: that copy decodes greedily) instead of the module's ``sample_temperature``; ``sample_uniforms``
        ([steps][graphs * n][A]): the copies' uniforms instead of torch's RNG."""
        # one engine batch of n copies of the scene over ONE map encoding (RolloutEngine(copies=n): the map-token graph, the map
        # encoder and the map K / V rows exist once - the reference offers inference_no_map(data, map_enc) for the same purpose);
        # every rollout carries what ``inference`` returns for it: the seed node's outputs and the map_next_token_* keys too
        if num_graphs(data) > 1:            # B graphs x n copies as one engine batch over B map encodings; n batched dicts
            return self._run_graphs(data, copies=int(n), mutate=False, replay=replay, replay_plan=replay_plan,
                                    sample_temperature=sample_temperature, sample_uniforms=sample_uniforms)
        return self.inference_batch([data.clone() if hasattr(data, 'clone') else dict(data)], seed_outputs=True, copies=int(n),
                                    replay=replay, replay_plan=replay_plan, sample_temperature=sample_temperature,
                                    sample_uniforms=sample_uniforms)

    @torch.no_grad()
    def predict_modes(self, data, n: int, k: int = 6, dist_thresh: float = 2.5, scores='density', **rollout_kwargs):
        """K representative futures per agent with probabilities - the 6-mode output of WOMD-style motion prediction - from ``n``
        rollouts of the scene: ``inference_rollouts(data, n, **rollout_kwargs)``, then ``RolloutEngine.select_modes`` on the
        copies where the rollout left them (one launch; ``infgen_amd.modes``).  ``scores``: 'density' or 'logprob' (needs
        ``token_logprob``).  -> per graph a dict of ``agent_id`` [A], ``pred_traj_modes`` [A, k, R, 2], ``pred_prob_modes`` [A, k]
        and ``mode_idx`` [A, k] (the rollout a mode came from; -1: fewer than k rollouts hold the agent at the goal step) over
        the graph's A initial agents: one dict for a single graph, a list for a multi-graph ``Batch``."""
        modes.check_engine_args(int(n), k, scores)
        B = num_graphs(data)
        self._last_engine = None                # (set by the rollout path that runs below: a stale engine is never read)
        self.inference_rollouts(data, int(n), **rollout_kwargs)
        eng = self._last_engine
        if eng is None:
            raise RuntimeError('predict_modes: the rollout path did not hand over its engine')
        m = eng.select_modes(k=k, dist_thresh=dist_thresh, scores=scores)
        ids = eng._epi['ids']
        res = []
        for g in range(B):
            A = int(eng.hosts[g * eng.copies]['A'])
            res.append(dict(agent_id=ids[g * eng.copies, :A], pred_traj_modes=m['mode_traj'][g, :A],
                            pred_prob_modes=m['mode_prob'][g, :A], mode_idx=m['mode_idx'][g, :A]))
        return res if B > 1 else res[0]

    @torch.no_grad()
    def inference_batch(self, datas: Sequence, seed_outputs: bool = False, copies: int = 1, replay=None,
                        replay_plan=None, sample_temperature=None, sample_uniforms=None) -> List[Dict[str, torch.Tensor]]:
        """throughput entry: many independent scenes decoded in lockstep on this GPU.  Every dict has the key set of
        ``inference``; the seed node's per-insertion arrays (``*_seed``) are recorded only with ``seed_outputs=True`` (5.5 MB per
        scene), otherwise they are the zero arrays the reference initialises them to (agent_decoder.py:1746-1750).
        ``replay``: 'ego', one bool tensor per scene, or one over all scenes' rows in order; ``replay_plan``: one dict per scene
        or one over all rows (see ``inference``)."""
        rs = self._run(None, batch=datas, batch_seed_outputs=seed_outputs, copies=copies, replay=replay, replay_plan=replay_plan,
                       sample_temperature=sample_temperature, sample_uniforms=sample_uniforms)
        if copies > 1:                          # ``copies`` rollouts per scene over one map encoding: scene 0's first, then scene 1's ...
            datas = [d for d in datas for _ in range(int(copies))]
        out = []
        map_keys = self._empty_map_keys(self._last_w.device)
        for d, r in zip(datas, rs):
            out.append(r.merged(first=map_keys, last={k: d[k] for k in self.data_keys if k in d}))
        return out
