"""K representative futures per agent from N candidate trajectories - the reference's ``batch_nms`` / ``new_batch_nms``
(infgen/utils/metrics.py:198-256, :143-195) on the device, one launch of ``k_select_modes`` (infgen_amd/csrc/mode_kernels.hip;
"modes" of include/infgen_hip.h states the semantics, the choices pinned by definition included): one wave per row, one candidate
per lane, ``1 <= N <= 64``, ``1 <= k <= min(N, 16)``.  Nothing is read on the host; the trajectory tensor is read in place.

    select_modes(traj, k, dist_thresh, scores=None | [B, N], valid=None | [B, N], t_goal=-1)  -> mode_traj, mode_score, mode_idx
    batch_nms(pred_trajs, pred_scores, dist_thresh, num_ret_modes)                            the reference's signature
    new_batch_nms(pred_trajs, dist_thresh, num_ret_modes)                                     scores = the goals' density
    mode_prob(mode_score)                                                                     scores renormalised over the K slots

``RolloutEngine.select_modes`` and ``InfGenDecoder.predict_modes`` run it over the copies of a rollout.
Not ported: ``batch_nms(mode='speed')`` and ``batch_nms_token``."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import InfgenHipError

MAX_CANDIDATES, MAX_MODES = 64, 16


def check_sizes(n: int, k: int, what: str = 'candidates') -> None:
    if not 1 <= int(n) <= MAX_CANDIDATES:
        raise ValueError(f'select_modes holds one candidate per lane of a 64-lane wave: 1..{MAX_CANDIDATES} {what}, not {int(n)}')
    if not 1 <= int(k) <= min(int(n), MAX_MODES):
        raise ValueError(f'select_modes returns 1..min({what}, {MAX_MODES}) modes: k = {int(k)} with {int(n)} {what}')


def check_engine_args(copies: int, k: int, scores) -> None:
    """the host-side checks of ``RolloutEngine.select_modes``, before anything touches the device"""
    if int(copies) == 1:
        raise ValueError('select_modes picks among the copies of a scene: this engine has copies = 1, so every agent has one '
                         'candidate (build the engine with copies = n, or call inference_rollouts / predict_modes)')
    if int(copies) > MAX_CANDIDATES:
        raise ValueError(f'select_modes holds one copy per lane of a 64-lane wave: copies = {int(copies)} > {MAX_CANDIDATES}')
    check_sizes(copies, k, 'copies')
    if isinstance(scores, str) and scores not in ('density', 'logprob'):
        raise ValueError(f"scores must be 'density', 'logprob' or a tensor [scenes, copies], not {scores!r}")
    if not isinstance(scores, str) and not torch.is_tensor(scores):
        raise ValueError(f"scores must be 'density', 'logprob' or a tensor [scenes, copies], not {type(scores).__name__}")


def _gpu(t: torch.Tensor, name: str, dev: Optional[torch.device] = None) -> torch.device:
    if not torch.is_tensor(t) or t.device.type != 'cuda':
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise InfgenHipError(f'{name} must be a GPU tensor (got {where}): select_modes runs on the device only')
    if dev is not None and t.device != dev:
        raise InfgenHipError(f'{name} is on {t.device}, expected {dev}')
    return t.device


def launch(traj: torch.Tensor, k: int, dist_thresh: float, t_goal: int, scores: Optional[torch.Tensor] = None,
           score_per_group: bool = False, valid: Optional[torch.Tensor] = None, with_traj: bool = True,
           cand_state: Optional[torch.Tensor] = None, state_values: Tuple[float, float] = (0.0, 0.0),
           row_limit: Optional[torch.Tensor] = None, limit_stride: int = 1):
    """``traj`` [G, Rg, N, T, F] float32 on the device, any strides with a unit inner one and a step stride of at least F (read in
    place); ``scores`` [G, Rg, N] ([G, N] with ``score_per_group``) float32 contiguous, ``valid`` [G, Rg, N] bytes contiguous;
    ``cand_state`` [G, Rg, N, T'] float32 with a unit inner stride: a candidate whose state at ``t_goal`` is one of
    ``state_values`` is invalid; ``row_limit`` int32, entry ``g * limit_stride``: rows at or above it are invalid.
    -> mode_traj [G, Rg, k, T, F] (None without ``with_traj``), mode_score [G, Rg, k], mode_idx [G, Rg, k] int32"""
    dev = traj.device
    G, Rg, N, T, F = (int(v) for v in traj.shape)
    B = G * Rg
    idx = torch.empty(G, Rg, k, dtype=torch.int32, device=dev)
    sc = torch.empty(G, Rg, k, dtype=torch.float32, device=dev)
    out = torch.empty(G, Rg, k, T, F, dtype=torch.float32, device=dev) if with_traj else None
    if B == 0:
        return out, sc, idx
    sg, sr, sn, st = (int(traj.stride(d)) if traj.shape[d] > 1 else 0 for d in range(4))
    if T == 1:
        st = F
    ssg = ssr = ssn = 0
    if cand_state is not None:
        ssg, ssr, ssn = (int(cand_state.stride(d)) if cand_state.shape[d] > 1 else 0 for d in range(3))
    _lib.check(_lib.load().infgen_select_modes(
        traj.data_ptr(), sg, sr, sn, st, Rg, B, N, T, F, int(t_goal), int(k), float(dist_thresh),
        scores.data_ptr() if scores is not None else None, int(bool(score_per_group)),
        valid.data_ptr() if valid is not None else None,
        cand_state.data_ptr() if cand_state is not None else None, ssg, ssr, ssn, float(state_values[0]), float(state_values[1]),
        row_limit.data_ptr() if row_limit is not None else None, int(limit_stride),
        idx.data_ptr(), sc.data_ptr(), out.data_ptr() if out is not None else None,
        torch.cuda.current_stream(dev).cuda_stream), 'infgen_select_modes')
    return out, sc, idx


def _in_place(traj: torch.Tensor) -> torch.Tensor:
    """float32, unit inner stride, non-negative strides, steps that do not overlap: else one contiguous copy"""
    if traj.dtype != torch.float32:
        traj = traj.to(torch.float32)
    F = int(traj.shape[-1])
    ok = (F == 1 or traj.stride(-1) == 1) and all(s >= 0 for s in traj.stride()) and (traj.shape[-2] == 1 or traj.stride(-2) >= F)
    return traj if ok else traj.contiguous()


def select_modes(traj: torch.Tensor, k: int = 6, dist_thresh: float = 2.5, scores: Optional[torch.Tensor] = None,
                 valid: Optional[torch.Tensor] = None, t_goal: int = -1, with_traj: bool = True):
    """``traj`` [B, N, T, F] (or [G, Rg, N, T, F]: B = G Rg rows; a strided view, such as a rollout's ``pred_traj`` seen as
    [S0, A_cap, copies, R, 2], is read in place), F >= 2 with (x, y) first.  ``scores`` [B, N] finite and >= 0 (the ``batch_nms``
    case) or None: the goals' density (``new_batch_nms``).  ``valid`` [B, N]: candidates that may be picked (None: all).
    ``t_goal``: the step whose (x, y) is a candidate's goal (negative: from the end).
    -> (mode_traj [B, k, T, F] or None, mode_score [B, k], mode_idx [B, k] int32; -1 / 0 / zeros where a row has fewer than k valid
    candidates), in the order ``batch_nms`` returns."""
    if not torch.is_tensor(traj) or traj.dim() not in (4, 5) or traj.shape[-1] < 2:
        raise ValueError('select_modes takes traj [B, N, T, F] or [G, Rg, N, T, F] with F >= 2')
    lead = tuple(traj.shape[:-3])
    N, T = int(traj.shape[-3]), int(traj.shape[-2])
    check_sizes(N, k)
    if T < 1 or not -T <= int(t_goal) < T:
        raise ValueError(f't_goal = {t_goal} is outside the {T} steps')
    for name, t in (('scores', scores), ('valid', valid)):
        if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != lead + (N,)):
            raise ValueError(f'{name} must be {lead + (N,)}, one entry per candidate')
    dev = _gpu(traj, 'traj')
    x = _in_place(traj)
    x5 = x if x.dim() == 5 else x.unsqueeze(1)
    s = v = None
    if scores is not None:
        _gpu(scores, 'scores', dev)
        s = scores.to(torch.float32).contiguous()
    if valid is not None:
        _gpu(valid, 'valid', dev)
        v = (valid.view(torch.uint8) if valid.dtype == torch.bool else valid if valid.dtype == torch.uint8
             else (valid != 0).view(torch.uint8)).contiguous()
    out, sc, idx = launch(x5, int(k), dist_thresh, int(t_goal) % T, scores=s, valid=v, with_traj=with_traj)
    shape = lead + (int(k),)
    return (out.view(shape + tuple(x.shape[-2:])) if out is not None else None), sc.view(shape), idx.view(shape)


def batch_nms(pred_trajs, pred_scores, dist_thresh, num_ret_modes=6, mode='static', speed=None):
    """the reference's ``batch_nms`` (:198-256): -> ret_trajs, ret_scores, ret_idxs (int64 like the reference's)"""
    if mode != 'static' or speed is not None:
        raise NotImplementedError("batch_nms(mode='speed') is not ported (nor is batch_nms_token): only the 'static' distance test is")
    t, s, i = select_modes(pred_trajs, k=num_ret_modes, dist_thresh=dist_thresh, scores=pred_scores)
    return t, s, i.long()


def new_batch_nms(pred_trajs, dist_thresh, num_ret_modes=6):
    """the reference's ``new_batch_nms`` (:143-195): the scores are the goals' density"""
    t, s, i = select_modes(pred_trajs, k=num_ret_modes, dist_thresh=dist_thresh, scores=None)
    return t, s, i.long()


def batch_nms_token(*args, **kwargs):
    raise NotImplementedError("batch_nms_token is not ported (nor is batch_nms(mode='speed')): use batch_nms / select_modes")


def mode_prob(mode_score: torch.Tensor, mode_idx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the scores of a row's K slots renormalised to sum 1; empty (-1) slots are 0.  A row whose scores are all 0 gives equal
    shares to its filled slots when ``mode_idx`` is given, else zeros.  No host read."""
    w = mode_score.clamp(min=0)
    if mode_idx is not None:
        filled = mode_idx >= 0
        w = torch.where(filled, w, torch.zeros_like(w))
        tot = w.sum(dim=-1, keepdim=True)
        w = torch.where(tot > 0, w, filled.to(w.dtype))
    tot = w.sum(dim=-1, keepdim=True)
    return torch.where(tot > 0, w / tot.clamp(min=torch.finfo(w.dtype).tiny), torch.zeros_like(w))
