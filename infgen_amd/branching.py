"""Branching rollouts: parent vectors for ``RolloutEngine.branch`` / ``ClosedLoopSession.branch``.

    anc = branching.systematic_ancestors(log_weight, u)        # or keep_best(score, keep), or a planner's own choice
    eng.branch(branching.resample_parents(anc, eng.copies), t) # slot s continues as a clone of slot parent[s] from step t on

A PARENT vector names, for every agent-side scene slot, the slot whose state it takes over ("branching" of include/infgen_hip.h):
global slot indices, source and destination in one copy group (the ``copies`` rollouts of one scene, slots g * copies ..
g * copies + copies - 1), and every source a fixed point (``parent[parent[s]] == parent[s]``).  ``resample_parents`` turns the
arbitrary ancestor indices a resampler draws into such a vector on the device (``infgen_resample_parents``); the two resamplers
here are plain torch on the device.  ``score_log_weight`` turns the engine's step scores ("step scores" of include/infgen_hip.h;
``RolloutEngine(step_scores=...)``, ``eng.step_score`` [S, steps, 8]) into the per-copy score those resamplers take.  No function
reads the device."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


# columns of a step score (include/infgen_hip.h, "step scores")
SCORE_N_LIVE, SCORE_N_OVERLAP, SCORE_MIN_SEP, SCORE_N_OFFROAD, SCORE_MAX_ACCEL, SCORE_MAX_YAW_RATE = range(6)
SCORE_WIDTH = 8
# score_log_weight's terms: weights (per count, per m/s^2, per rad/s, per metre) and the limits the comfort and gap terms start at
SCORE_WEIGHTS = dict(w_overlap=1.0, w_offroad=1.0, w_accel=0.0, w_yaw=0.0, w_gap=0.0, accel_limit=4.0, yaw_limit=1.0, gap_limit=0.5)


def check_score_weights(weights=None) -> dict:
    """``weights`` (None or a dict with keys of SCORE_WEIGHTS) -> the full dict of finite floats; ValueError otherwise"""
    out = dict(SCORE_WEIGHTS)
    if weights is not None:
        if not isinstance(weights, dict):
            raise ValueError('weights is a dict with keys of branching.SCORE_WEIGHTS')
        for k, v in weights.items():
            if k not in out:
                raise ValueError(f'weights: unknown key {k!r} (known: {sorted(out)})')
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not np.isfinite(v):
                raise ValueError(f'weights[{k!r}] must be a finite number')
            out[k] = float(v)
    return out


def score_log_weight(step_score: torch.Tensor, t0: int, t1: int, weights=None, copies: int = None) -> torch.Tensor:
    """step scores -> the log weight of every copy over the decode steps [t0, t1): ``step_score`` [S0 * n, steps, 8] (``copies`` = n)
    or [S0, n, steps, 8] -> [S0, n] float32, the negative sum over the steps of
    ``w_overlap n_overlap + w_offroad n_offroad + w_accel relu(max_accel - accel_limit) + w_yaw relu(max_yaw_rate - yaw_limit)
    + w_gap relu(gap_limit - min_sep)`` (a ``min_sep`` of +inf - fewer than two live rows - contributes 0).  Plain torch on the
    tensor's device; higher is better: feed it to ``keep_best`` or ``systematic_ancestors``."""
    w = check_score_weights(weights)
    x = step_score
    if x.dim() == 3 and copies is not None and int(copies) >= 1 and x.shape[0] % int(copies) == 0:
        x = x.view(-1, int(copies), x.shape[1], x.shape[2])
    if x.dim() != 4 or x.shape[3] != SCORE_WIDTH:
        raise ValueError('score_log_weight takes step_score [S0 * copies, steps, 8] with copies=, or [S0, copies, steps, 8]')
    t0, t1 = int(t0), int(t1)
    if not 0 <= t0 <= t1 <= x.shape[2]:
        raise ValueError(f'steps [{t0}, {t1}) are outside the log\'s 0 .. {x.shape[2]}')
    x = x[:, :, t0:t1].float()
    relu = torch.relu
    gap = relu(w['gap_limit'] - torch.clamp(x[..., SCORE_MIN_SEP], max=w['gap_limit']))
    cost = (w['w_overlap'] * x[..., SCORE_N_OVERLAP] + w['w_offroad'] * x[..., SCORE_N_OFFROAD]
            + w['w_accel'] * relu(x[..., SCORE_MAX_ACCEL] - w['accel_limit'])
            + w['w_yaw'] * relu(x[..., SCORE_MAX_YAW_RATE] - w['yaw_limit']) + w['w_gap'] * gap)
    return -cost.sum(dim=2)


def check_parent(parent, S0: int, copies: int) -> np.ndarray:
    """a HOST parent vector, [S0 * copies] or [S0, copies] integers -> int32 [S0 * copies]; ValueError naming the first entry that
    is out of range, in another copy group or no fixed point (what the kernel would treat as the identity and count)"""
    p = np.asarray(parent)
    S = S0 * copies
    if p.dtype.kind not in 'iu':
        raise ValueError('parent holds integer slot indices')
    if p.shape not in ((S,), (S0, copies)):
        raise ValueError(f'parent: expected shape {(S,)} or {(S0, copies)}, got {tuple(p.shape)}')
    p = p.reshape(-1).astype(np.int64)
    for s in range(S):
        q = int(p[s])
        if q == s:
            continue
        if not 0 <= q < S:
            raise ValueError(f'parent[{s}] = {q} is outside 0 .. {S - 1}')
        if q // copies != s // copies:
            raise ValueError(f'parent[{s}] = {q} is a slot of another copy group (scene {q // copies}, not {s // copies})')
        if int(p[q]) != q:
            raise ValueError(f'parent[{s}] = {q} is no fixed point: parent[{q}] = {int(p[q])} (a chain; sources keep themselves)')
    return p.astype(np.int32)


def _groups(x: torch.Tensor, copies: int, what: str) -> torch.Tensor:
    if x.dim() == 1 and copies >= 1 and x.numel() % copies == 0:
        return x.view(-1, copies)
    if x.dim() == 2 and x.shape[1] == copies:
        return x
    raise ValueError(f'{what}: expected shape [S0 * {copies}] or [S0, {copies}], got {tuple(x.shape)}')


def resample_parents(ancestor: torch.Tensor, copies: int) -> torch.Tensor:
    """arbitrary per-slot ancestors -> a valid parent vector of the same shape, int32 (``infgen_resample_parents``: one launch on
    the current stream).  ``ancestor``: a device int tensor [S0 * copies] or [S0, copies] of global slot indices inside the slot's
    own group (one outside counts as the slot itself).  A slot named at least once keeps itself; the unnamed slots, ascending,
    receive ancestor j's ``count[j] - 1`` extra copies in ascending j: the multiset of ancestors per group is preserved."""
    if not ancestor.is_cuda:
        raise _lib.InfgenHipError('resample_parents takes a device tensor: the HIP path has no CPU fallback')
    if ancestor.is_floating_point() or ancestor.dtype == torch.bool:
        raise ValueError('ancestor holds integer slot indices')
    copies = int(copies)
    if not 1 <= copies <= 1024:
        raise ValueError('copies must be in 1 .. 1024')
    a = _groups(ancestor, copies, 'ancestor').to(torch.int32).contiguous()
    out = torch.empty_like(a)
    if a.numel():
        stream = torch.cuda.current_stream(a.device).cuda_stream
        with torch.cuda.device(a.device):
            _lib.check(_lib.load().infgen_resample_parents(_lib.ptr(a), int(a.shape[0]), copies, _lib.ptr(out), stream),
                       'infgen_resample_parents')
    return out.view(ancestor.shape)


def systematic_ancestors(log_weight: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """systematic resampling per copy group: ``log_weight`` [S0, n] (unnormalised), ``u`` [S0] in [0, 1) -> ancestors [S0, n] int32,
    global slot indices.  With w the group's softmax and cdf its running sum, copy i takes the first j with
    ``cdf[j] > (u + i) / n`` (float64; the last slot where rounding leaves none) - slot j is drawn floor or ceil of n w[j] times."""
    if log_weight.dim() != 2 or u.shape != log_weight.shape[:1]:
        raise ValueError('systematic_ancestors takes log_weight [S0, n] and u [S0]')
    S0, n = log_weight.shape
    dev = log_weight.device
    cdf = torch.softmax(log_weight.double(), dim=1).cumsum(dim=1)
    at = (u.double()[:, None] + torch.arange(n, device=dev, dtype=torch.float64)[None, :]) / n
    j = torch.searchsorted(cdf, at, right=True).clamp_(max=n - 1)
    return (j + torch.arange(S0, device=dev)[:, None] * n).to(torch.int32)


def keep_best(score: torch.Tensor, keep: int) -> torch.Tensor:
    """best-of-n pruning per copy group: ``score`` [S0, n] (higher is better; equal scores: the lower slot first) -> ancestors
    [S0, n] int32, global slot indices.  The ``keep`` best copies keep themselves; the i-th of the others, in rank order, is
    replaced by the (i mod keep)-th best.  The result is a valid parent vector as it stands."""
    if score.dim() != 2:
        raise ValueError('keep_best takes score [S0, n]')
    S0, n = score.shape
    keep = int(keep)
    if not 1 <= keep <= n:
        raise ValueError(f'keep must be in 1 .. {n}')
    dev = score.device
    order = torch.argsort(score, dim=1, descending=True, stable=True)          # [S0, n]: slots by rank
    rank = torch.arange(n, device=dev)
    src_rank = torch.where(rank < keep, rank, (rank - keep) % keep)            # the rank whose slot the slot of this rank takes
    anc = torch.empty_like(order)
    anc.scatter_(1, order, order[:, src_rank])
    return (anc + torch.arange(S0, device=dev)[:, None] * n).to(torch.int32)
