"""Branching rollouts: parent vectors for ``RolloutEngine.branch`` / ``ClosedLoopSession.branch``.

    anc = branching.systematic_ancestors(log_weight, u)        # or keep_best(score, keep), or a planner's own choice
    eng.branch(branching.resample_parents(anc, eng.copies), t) # slot s continues as a clone of slot parent[s] from step t on

A PARENT vector names, for every agent-side scene slot, the slot whose state it takes over ("branching" of include/infgen_hip.h):
global slot indices, source and destination in one copy group (the ``copies`` rollouts of one scene, slots g * copies ..
g * copies + copies - 1), and every source a fixed point (``parent[parent[s]] == parent[s]``).  ``resample_parents`` turns the
arbitrary ancestor indices a resampler draws into such a vector on the device (``infgen_resample_parents``); the two resamplers
here are plain torch on the device.  No function reads the device."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib


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
