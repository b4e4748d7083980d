"""Agent-centric observations ("observations" of include/infgen_hip.h): what ``torch.ops.infgen_hip.observe_rows``,
``RolloutEngine.observe_rows`` and ``ClosedLoopSession.observe(frame='agent')`` share - the argument checks (plain Python, no GPU),
the output tensors and the one call of ``infgen_observe_rows``."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import _lib

SELF, NBR, MAP, MAX_K = (_lib.HEADER.consts['INFGEN_OBS_' + n] for n in ('SELF', 'NBR', 'MAP', 'MAX_K'))
KEYS = ('self_feat', 'nbr_feat', 'nbr_index', 'nbr_count', 'map_feat', 'map_index', 'map_count')


def check_params(c: int, T: int, dt: float, neighbors: int, radius: float, map_tokens: int, map_radius: float, has_map: bool):
    """the scalar arguments, as the library refuses them: ``ValueError`` before anything is launched"""
    if not 0 <= int(c) < T:
        raise ValueError(f'observe: column {c} outside 0 .. {T - 1}')
    if not (math.isfinite(dt) and dt > 0):
        raise ValueError(f'observe: dt must be finite and > 0, not {dt}')
    for what, k in (('neighbors', neighbors), ('map_tokens', map_tokens)):
        if not 0 <= int(k) <= MAX_K:
            raise ValueError(f'observe: {what} must be in 0 .. {MAX_K}, not {k}')
    for what, r in (('radius', radius), ('map_radius', map_radius)):
        if not r >= 0:
            raise ValueError(f'observe: {what} must be >= 0 (inf: no limit), not {r}')
    if int(map_tokens) > 0 and not has_map:
        raise ValueError('observe: map_tokens > 0 needs the map arrays')


def check_rows(rows: Optional[torch.Tensor]):
    if rows is not None and (not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.is_floating_point()
                             or rows.dtype == torch.bool):
        raise ValueError('observe: rows is a 1-D integer tensor of global row indices s * A_cap + i')


def outputs(N: int, K: int, Km: int, dev, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """the seven result tensors: new ones, or those of an earlier result ``out`` (checked for shape, dtype and device)"""
    want = dict(self_feat=((N, SELF), torch.float32), nbr_feat=((N, K, NBR), torch.float32), nbr_index=((N, K), torch.int32),
                nbr_count=((N,), torch.int32), map_feat=((N, Km, MAP), torch.float32), map_index=((N, Km), torch.int32),
                map_count=((N,), torch.int32))
    if out is None:
        return {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in want.items()}
    res = {}
    for k, (shape, dt) in want.items():
        t = out.get(k)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or t.device != torch.device(dev) \
                or not t.is_contiguous():
            raise ValueError(f'observe: out[{k!r}] must be a contiguous {dt} tensor of shape {shape} on {dev}')
        res[k] = t
    return res


def launch(lib, stream, pos, head, state, n_agents, type, shape, c, dt, map_pos, map_orient, map_type, n_map, copies, rows,
           neighbors, radius, map_tokens, map_radius, res) -> None:
    """one ``infgen_observe_rows`` into the tensors of ``res``; every tensor is what the library reads (contiguous, fp32 / int32,
    ``map_type`` int64) - the callers see to that"""
    P = _lib.ptr
    S, T, A = (int(v) for v in pos.shape[:3])
    N = S * A if rows is None else int(rows.numel())
    if N == 0:
        return
    _lib.check(lib.infgen_observe_rows(
        P(pos), P(head), P(state), P(n_agents), P(type), P(shape), S, A, T, int(c), float(dt), P(map_pos), P(map_orient), P(map_type),
        P(n_map), 0 if map_pos is None else int(map_pos.shape[1]), int(copies), P(rows), N, int(neighbors), float(radius),
        int(map_tokens), float(map_radius), P(res['self_feat']), P(res['nbr_feat']), P(res['nbr_index']), P(res['nbr_count']),
        P(res['map_feat']), P(res['map_index']), P(res['map_count']), stream), 'infgen_observe_rows')
