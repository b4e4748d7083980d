"""Scene setup of a batch (reference agent_decoder.py:1609-1719: filter, pad, zero the future, bos / eos, tmask / imask /
catflag) and the inputs of the output epilogue - written ONCE, as torch statements over [S, A, ...] arrays on whatever
device the inputs live on (log replay included: ``replay_arrays``, the plan of the rows that follow their logged future).  Host scene lists are first staged into such arrays (``stage_agents``: the row filter and slice
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


# ------------------------------------------------------------------ log replay (RolloutEngine(replay=...))
PLAN_KEYS = ('token_idx', 'state_idx', 'token_pos', 'token_heading')


def replay_rows(replay, counts: Sequence[int], av: Sequence[int], device=None) -> List[torch.Tensor]:
    """the public forms of ``replay=`` -> one bool row mask per scene.  ``replay``: 'ego', a bool tensor over the rows of all
    scenes in scene order (the global row order of a Batch; for one scene its own rows), or one bool tensor per scene.
    ``counts`` [B]: rows per scene (before the row filter), ``av`` [B]: each scene's ego row, local.  Raises ValueError when a
    mask's length is not its scene's row count."""
    B = len(counts)
    if isinstance(replay, str):
        if replay != 'ego':
            raise ValueError(f"replay must be 'ego', a bool tensor or a list of bool tensors, not {replay!r}")
        out = [torch.zeros(int(n), dtype=torch.bool, device=device) for n in counts]
        for m, a in zip(out, av):
            m[int(a)] = True
        return out
    if isinstance(replay, (list, tuple)):
        if len(replay) != B:
            raise ValueError(f'replay lists {len(replay)} masks for {B} scenes')
        out = [torch.as_tensor(m).bool().reshape(-1) for m in replay]
    else:
        flat = torch.as_tensor(replay).bool().reshape(-1)
        if flat.numel() != int(sum(counts)):
            raise ValueError(f'replay mask of {flat.numel()} rows for {int(sum(counts))} agent rows')
        out = list(flat.split([int(n) for n in counts]))
    for s, (m, n) in enumerate(zip(out, counts)):
        if m.numel() != int(n):
            raise ValueError(f'replay mask of scene {s} has {m.numel()} rows, the scene has {int(n)}')
    return out


def replay_global(replay, n_rows: int, av_global: torch.Tensor, n_graphs: int) -> torch.Tensor:
    """``replay=`` of a ragged Batch -> one bool mask over its N concatenated rows, on the Batch's device and without a host
    copy ('ego': the global ego rows; a list: the graphs' masks concatenated)"""
    dev = av_global.device
    if isinstance(replay, str):
        if replay != 'ego':
            raise ValueError(f"replay must be 'ego', a bool tensor or a list of bool tensors, not {replay!r}")
        m = torch.zeros(n_rows, dtype=torch.bool, device=dev)
        m[av_global.reshape(-1).long()] = True
        return m
    if isinstance(replay, (list, tuple)):
        if len(replay) != n_graphs:
            raise ValueError(f'replay lists {len(replay)} masks for {n_graphs} graphs')
        replay = torch.cat([torch.as_tensor(m).reshape(-1) for m in replay])
    m = torch.as_tensor(replay).reshape(-1)
    if m.numel() != n_rows:
        raise ValueError(f'replay mask of {m.numel()} rows for {n_rows} agent rows')
    return m.to(dev).bool()


def check_plan(plan: Mapping) -> bool:
    """a plan names its tokens and states; poses come as a pair or not at all.  -> does it carry poses?"""
    if plan.get('token_idx') is None or plan.get('state_idx') is None:
        raise ValueError('a replay plan needs token_idx and state_idx (poses - token_pos and token_heading - are optional)')
    pose = [plan.get(k) is not None for k in ('token_pos', 'token_heading')]
    if pose[0] != pose[1]:
        raise ValueError('a replay plan carries token_pos and token_heading together or neither')
    return pose[0]


def stage_replay(scenes: Sequence[Mapping], filts: Sequence[np.ndarray], replay: Sequence, T: int
                 ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """host scenes + per-scene ``replay`` entries -> (row mask [S, max A] after the row filter, the plan ``replay_arrays``
    takes: token_idx / state_idx [S, max A, T0] and, unless an explicit plan comes without them, token_pos / token_heading).
    An entry is None (nothing replayed), a bool mask over the scene's rows - the plan is the scene's own logged future - or
    (mask, tokens, states[, pos, head]) with (A, T) / (A, T, 2) arrays over the same rows."""
    if len(replay) != len(scenes):
        raise ValueError(f'replay has {len(replay)} entries for {len(scenes)} scenes')
    masks, plans, poses = [], {k: [] for k in PLAN_KEYS}, set()
    for s, (sc, f, r) in enumerate(zip(scenes, filts, replay)):
        ag = sc['agent']
        n = int(np.asarray(ag['state_idx']).shape[0])
        src = {k: np.asarray(ag[k]) for k in PLAN_KEYS}
        if isinstance(r, (tuple, list)):
            if len(r) < 3 or r[1] is None or r[2] is None:
                raise ValueError(f'replay plan of scene {s}: (mask, tokens, states[, pos, head]) - tokens and states are required')
            m, explicit = r[0], dict(zip(PLAN_KEYS, list(r[1:]) + [None] * (5 - len(r))))
            has_pose = check_plan(explicit)
            src = {k: np.asarray(v) if v is not None else src[k] for k, v in explicit.items()}
            if np.asarray(m).any():
                poses.add(has_pose)
        else:
            m = np.zeros(n, bool) if r is None else r
            if np.asarray(m).any():
                poses.add(True)
        m = np.asarray(m).astype(bool).reshape(-1)
        if m.shape[0] != n:
            raise ValueError(f'replay mask of scene {s} has {m.shape[0]} rows, the scene has {n}')
        for k, v in src.items():
            if v.shape[0] != n or v.shape[1] < T:
                raise ValueError(f'replay plan of scene {s}: {k} has shape {v.shape}, need ({n}, >= {T} columns)')
            plans[k].append(v[f])
        masks.append(m[f])
    if len(poses) > 1:
        raise ValueError('the plans of one batch carry poses (the logged future always does) or none of them does')
    plan = dict(token_idx=_stack(plans['token_idx'], -1, np.int64, T), state_idx=_stack(plans['state_idx'], INVALID, np.int64, T))
    if poses != {False}:
        plan.update(token_pos=_stack(plans['token_pos'], 0.0, np.float32, T), token_heading=_stack(plans['token_heading'], 0.0, np.float32, T))
    mask = _stack([m[:, None] for m in masks], False, bool)[:, :, 0]
    return torch.from_numpy(mask), {k: torch.from_numpy(v) for k, v in plan.items()}


def replay_arrays(mask: torch.Tensor, plan: Mapping[str, torch.Tensor], hc: int, T: int, a_cap: int, copies: int = 1
                  ) -> Dict[str, torch.Tensor]:
    """the device arrays of a replayed batch in the engine's layout (InfgenRollout.teacher_* / replay_row), as torch statements
    on whatever device ``mask`` [S, A] and ``plan`` (token_idx / state_idx [S, A, T0], optional token_pos [S, A, T0, 2] /
    token_heading) live on: teacher_token / teacher_state int32 [S n][T][a_cap], teacher_pos / teacher_head, replay_row uint8
    [S n][a_cap].  Columns hc .. T - 1 of the flagged rows hold the plan, everything else -1 / INVALID / 0 (what
    k_ingest_batch writes); with ``copies`` = n every copy of a scene replays the same plan."""
    has_pose = check_plan(plan)
    tok, st = plan['token_idx'], plan['state_idx']
    S, A, T0 = st.shape
    if T0 < T:
        raise ValueError(f'the plan covers {T0} token columns, the rollout has {T}')
    if tuple(mask.shape) != (S, A) or A > a_cap:
        raise ValueError(f'replay mask {tuple(mask.shape)} against a plan of {(S, A)} rows (at most {a_cap} per scene)')
    dev = st.device
    on = mask.to(dev).bool()[:, :, None] & (torch.arange(T, device=dev) >= hc)[None, None, :]

    def put(x, fill, dtype):                 # [S, A, T0, ...] -> [S n][T][a_cap][...]
        x = x[:, :, :T].to(dtype)
        sel = on.reshape(on.shape + (1,) * (x.dim() - 3))
        x = torch.where(sel, x, torch.full((), fill, dtype=dtype, device=dev))
        out = torch.full((S, T, a_cap) + tuple(x.shape[3:]), fill, dtype=dtype, device=dev)
        out[:, :, :A] = x.transpose(1, 2)
        return out.repeat_interleave(copies, dim=0) if copies > 1 else out
    out = dict(teacher_token=put(tok, -1, torch.int32), teacher_state=put(st, INVALID, torch.int32))
    if has_pose:
        out.update(teacher_pos=put(plan['token_pos'][..., :2], 0.0, torch.float32), teacher_head=put(plan['token_heading'], 0.0, torch.float32))
    row = torch.zeros((S, a_cap), dtype=torch.uint8, device=dev)
    row[:, :A] = mask.to(dev).to(torch.uint8)
    out['replay_row'] = row.repeat_interleave(copies, dim=0) if copies > 1 else row
    return out
