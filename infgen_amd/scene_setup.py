"""Scene setup of a batch (reference agent_decoder.py:1609-1719: filter, pad, zero the future, bos / eos, tmask / imask /
catflag) and the inputs of the output epilogue - written ONCE, as torch statements over [S, A, ...] arrays on whatever
device the inputs live on.  Host scene lists are first staged into such arrays (``stage_agents``: the row filter and slice
copies, nothing else); a batch that arrives as stacked device tensors is passed as it is.  The ingest kernel
(k_ingest_batch) is the independent second implementation: tests/test_batch_inference_gpu.py compares the two bit for bit.
Nothing here reads engine state."""
from __future__ import annotations

from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from .synth import INVALID, ENTER, EXIT

INVALID_SHAPE = 0.1
# box (length, width, height) by agent type, of the reference's evaluation (agent_decoder.py:2380)
EVAL_SHAPE = ((4.3, 1.8, 1.0), (0.5, 0.5, 1.0), (1.9, 0.5, 1.0))


def _stack(xs: Sequence[np.ndarray], fill, dtype, width: Optional[int] = None) -> np.ndarray:
    """ragged [n_i, w_i, ...] arrays -> one [S, max n, max w, ...] array of ``dtype`` (columns beyond ``width`` cut), ``fill``
    where a scene has no entry"""
    if width is not None:
        xs = [x[:, :width] for x in xs]
    shapes = {x.shape for x in xs}
    if len(shapes) == 1:                                   # nothing to fill
        return np.stack(xs, dtype=dtype, casting='unsafe')
    out = np.full((len(xs),) + tuple(max(d) for d in zip(*shapes)), fill, dtype)
    for o, x in zip(out, xs):
        o[tuple(slice(n) for n in x.shape)] = x
    return out


def _rows(filts):
    """the row filters as indices: a scene that keeps every row is read without a copy"""
    return [slice(None) if f.all() else f for f in filts]


def _kept(scenes, filts, key, cut=None) -> List[np.ndarray]:
    """``agent[key]`` of every scene, the filtered rows dropped (``filts``: of ``_rows``; ``cut``: the leading columns only)"""
    xs = (np.asarray(sc['agent'][key]) for sc in scenes)
    return [(x if cut is None else x[:, :cut])[f] for x, f in zip(xs, filts)]


def stage_agents(scenes: Sequence[Mapping], cfg, T: int) -> Tuple[Dict[str, torch.Tensor], torch.Tensor, np.ndarray, List[np.ndarray]]:
    """host scenes -> (the agent arrays ``setup_agents`` takes, [S, max A, T0, ...] with each array's padding value in the
    missing rows / columns; ego rows [S]; agent counts [S]; row filters): rows invalid at the last history column are dropped
    and the ego index moves up by the rows dropped before it (reference :1609-1640); token columns beyond T are not read"""
    hc, H = cfg.hist_columns, cfg.num_historical_steps
    filts = [np.asarray(sc['agent']['state_idx'])[:, hc - 1] != INVALID for sc in scenes]
    av0 = [int(np.asarray(sc['agent']['av_index']).reshape(-1)[0]) for sc in scenes]
    av = np.asarray([a - int((~f[:a]).sum()) for a, f in zip(av0, filts)], np.int64)
    counts = np.asarray([int(f.sum()) for f in filts], np.int64)
    keep = _rows(filts)
    col = lambda key, c: [x[:, c] for x in _kept(scenes, keep, key, c + 1)]
    ag = dict(token_pos=_stack(_kept(scenes, keep, 'token_pos'), 0.0, np.float32, T),
              token_heading=_stack(_kept(scenes, keep, 'token_heading'), 0.0, np.float32, T),
              token_idx=_stack(_kept(scenes, keep, 'token_idx'), -1, np.int64, T),
              state_idx=_stack(_kept(scenes, keep, 'state_idx'), INVALID, np.int64, T),
              grid_token_idx=_stack(_kept(scenes, keep, 'grid_token_idx'), -1, np.int64, T),
              raw_agent_valid_mask=_stack(_kept(scenes, keep, 'raw_agent_valid_mask'), True, bool, T),
              eval_mask=_stack(col('valid_mask', H - 1), False, bool), type=_stack(_kept(scenes, keep, 'type'), 0, np.int64),
              shape10=_stack(col('shape', H - 1), INVALID_SHAPE, np.float32))
    return {k: torch.from_numpy(v) for k, v in ag.items()}, torch.from_numpy(av), counts, filts


def stage_map(scenes: Sequence[Mapping]) -> Tuple[Dict[str, np.ndarray], np.ndarray]:
    """host scenes -> (the map-token arrays [S, max M, ...], zero beyond a scene's tokens; token counts [S])"""
    pt = lambda key: [np.asarray(sc['pt_token'][key]) for sc in scenes]
    light = [np.asarray(sc['map_polygon']['light_type']).astype(np.int64)[
        np.asarray(sc['pt_token__to__map_polygon']['edge_index'])[1].astype(np.int64)] for sc in scenes]
    m = dict(map_pos=_stack(pt('position'), 0.0, np.float32, 2), map_orient=_stack(pt('orientation'), 0.0, np.float32),
             map_tok=_stack(pt('token_idx'), 0, np.int64), map_type=_stack(pt('type'), 0, np.int64),
             map_pl=_stack(pt('pl_type'), 0, np.int64), map_light=_stack(light, 0, np.int64))
    return m, np.asarray([len(x) for x in light], np.int64)


def setup_agents(ag: Mapping[str, torch.Tensor], av: torch.Tensor, cfg, T: int, counts=None) -> Dict[str, torch.Tensor]:
    """reference agent_decoder.py:1640-1719 for S scenes at once.  ``ag``: token_pos / token_heading / token_idx / state_idx /
    grid_token_idx / raw_agent_valid_mask [S, A, T0, ...], eval_mask / type [S, A], shape10 [S, A, 3] (rows already filtered);
    ``av`` [S]: the ego rows; ``counts`` [S]: the agents of every scene when they differ (the rows from a scene's count on
    then hold the padding values of the engine's buffers).  Returns pos / head / token / state / grid / valid / tmask / imask
    / catflag [S, A, T, ...] and bos / type / shape10 [S, A, ...]."""
    hc, H = cfg.hist_columns, cfg.num_historical_steps
    state0 = ag['state_idx'].long()
    S, A, T0 = state0.shape
    assert T0 <= T, 'token arrays longer than the rollout are not supported (SURVEY a-Q15)'
    dev = state0.device

    def pad(x, val):
        if x.shape[2] == T:
            return x.clone()
        shp = tuple(x.shape[:2]) + (T - x.shape[2],) + tuple(x.shape[3:])
        return torch.cat([x, torch.full(shp, val, dtype=x.dtype, device=dev)], dim=2)
    pos = pad(ag['token_pos'].float(), 0.0)
    head = pad(ag['token_heading'].float(), 0.0)
    token = pad(ag['token_idx'].long(), -1)
    state = pad(state0, INVALID)
    grid = pad(ag['grid_token_idx'].long(), -1)
    valid = pad(ag['raw_agent_valid_mask'].bool(), True)
    pos[:, :, hc:] = 0; head[:, :, hc:] = 0; token[:, :, hc:] = -1; state[:, :, hc:] = INVALID; grid[:, :, hc:] = -1
    valid[:, :, hc:] = True
    valid &= ag['eval_mask'].bool()[..., None]
    is_bos, is_eos = state == ENTER, state == EXIT
    bos = torch.where(is_bos.any(2), is_bos.int().argmax(2), 0)
    eos = torch.where(is_eos.any(2), is_eos.int().argmax(2), T - 1)
    cols = torch.arange(T, device=dev)[None, None, :]
    motion = (cols > bos[..., None]) & (cols <= eos[..., None])
    motion[:, :, H // cfg.shift:] = False
    tmask = torch.where(motion, valid, True)
    nonmotion = ~motion
    nonmotion[:, :, H // cfg.shift:] = False
    imask = ~nonmotion
    imask |= state == ENTER
    imask[torch.arange(S, device=dev), av] = True
    tmask[:, :, hc:] = True
    imask[:, :, hc:] = True
    catflag = state != INVALID
    out = dict(pos=pos, head=head, token=token, state=state, grid=grid, valid=valid, tmask=tmask, imask=imask, catflag=catflag,
               bos=bos, type=ag['type'].long(), shape10=ag['shape10'].float())
    if counts is not None:
        # (an all-INVALID padding row does not come out as padding by itself: bos = 0, eos = T - 1 puts column 1 into motion)
        absent = torch.arange(A, device=dev)[None, :] >= torch.as_tensor(counts, device=dev)[:, None]
        for k, val in (('token', -1), ('grid', -1), ('shape10', INVALID_SHAPE), ('pos', 0), ('head', 0), ('state', 0), ('valid', 0),
                       ('tmask', 0), ('imask', 0), ('catflag', 0), ('bos', 0), ('type', 0)):
            out[k][absent] = val
    return out


def stage_epilogue(scenes: Sequence[Mapping], filts: Sequence[np.ndarray], cfg) -> Dict[str, torch.Tensor]:
    """host scenes -> the agent arrays ``epilogue_inputs`` reads, [S, max A, ...], zero in the missing rows / steps"""
    hc, filts = cfg.hist_columns, _rows(filts)
    ag = dict(token_idx=_stack(_kept(scenes, filts, 'token_idx', hc), 0, np.int64),
              state_idx=_stack(_kept(scenes, filts, 'state_idx', hc), 0, np.int64),
              position=_stack([x[:, :, :2] for x in _kept(scenes, filts, 'position')], 0.0, np.float32),
              heading=_stack(_kept(scenes, filts, 'heading', 1), 0.0, np.float32),
              shape=_stack(_kept(scenes, filts, 'shape', hc), 0.0, np.float32), id=_stack(_kept(scenes, filts, 'id'), 0, np.int64))
    return {k: torch.from_numpy(v) for k, v in ag.items()}


def epilogue_inputs(ag: Mapping[str, torch.Tensor], valid: torch.Tensor, a_cap: int, cfg, counts=None) -> Dict[str, torch.Tensor]:
    """what the output epilogue reads besides the engine's buffers (``RolloutEngine._epilogue_arrays``), [S, a_cap, ...] on the
    device of ``ag``: history tokens / states, the logged first pose, ids (rows beyond a scene's agents: the ids scenario
    insertion hands out, max id + 1 ...), shapes, the ground-truth future and ``valid`` of ``setup_agents``"""
    hc, H = cfg.hist_columns, cfg.num_historical_steps
    S, A = ag['id'].shape
    dev = valid.device

    def rows(x, dtype):                     # [S, A, ...] -> [S, a_cap, ...], zero rows behind
        out = torch.zeros((S, a_cap) + tuple(x.shape[2:]), dtype=dtype, device=dev)
        out[:, :A] = x
        return out
    n0 = torch.full((S,), A, device=dev) if counts is None else torch.as_tensor(counts, device=dev)
    row = torch.arange(a_cap, device=dev)[None, :]
    init = row < n0[:, None]
    ids = rows(ag['id'], torch.int64)
    top = torch.where(init, ids, torch.iinfo(torch.int64).min).max(dim=1).values
    top = torch.where(n0 > 0, top, -1)
    ids = torch.where(init, ids, top[:, None] + 1 + row - n0[:, None])
    f32 = torch.float32
    return dict(htok=rows(ag['token_idx'][:, :, :hc], torch.int64), hst=rows(ag['state_idx'][:, :, :hc], torch.int64),
                p0=rows(ag['position'][:, :, 0, :2], f32), h0=rows(ag['heading'][:, :, 0], f32), ids=ids,
                shp=rows(ag['shape'][:, :, hc - 1], f32), gt=rows(ag['position'][:, :, H:, :2], f32), val=rows(valid, torch.bool),
                n0=n0, eval_shape=torch.tensor(EVAL_SHAPE, device=dev))
