"""Per-token log-probabilities of a rollout: which entries count, and what is derived from them.

The rollout kernels write the FULL-softmax log-probability of the motion token every row emitted at every decode step
(``InfgenRollout.token_logprob``).  This module holds the pure-torch part around that buffer - no library call, so it runs on
the CPU as well as on the device:

    logprob_mask      which (row, column) entries are log-probabilities of a token the model itself chose
    pred_prob         exp(logprob) per decode step where masked, else 0 (the reference allocates this array as ``pred_prob``,
                      agent_decoder.py:1689, and leaves the line that fills it, :2205, commented out)
    rollout_logprob   the masked sum in float64, added up in an order that depends on nothing but the element positions

The value is the log-probability under the full softmax over the vocabulary.  A sampled rollout draws from the distribution
renormalised over its top-k tokens; that probability is a different quantity, written by the same kernels into
``InfgenRollout.sample_logprob`` (``RolloutEngine(sample_logprob=True)``: ``next_token_sample_logprob``, under the same mask and
summed by the same ``rollout_logprob``).
"""
from __future__ import annotations

from typing import Optional

import torch


def logprob_mask(token: torch.Tensor, first_col: torch.Tensor, hist_cols: int, steps: int,
                 forced: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``token`` [..., A, T]: the final ``next_token_idx``; ``first_col`` [..., A]: the first column the row was decoded for
    (``hist_cols`` for the initial rows, the column after its bos column for an inserted row); ``forced`` [..., A] bool: rows that
    follow a plan (log replay, teacher forcing) instead of their own token.  -> bool [..., A, T], True exactly where the column
    is a decoded one, the row existed at that step, the emitted token is >= 0 and the row is not forced."""
    T = token.shape[-1]
    cols = torch.arange(T, device=token.device)
    mask = (cols >= hist_cols) & (cols < hist_cols + steps) & (cols >= first_col.long()[..., None]) & (token >= 0)
    if forced is not None:
        mask = mask & ~forced.bool()[..., None]
    return mask


def pred_prob(logprob: torch.Tensor, mask: torch.Tensor, hist_cols: int, steps: int) -> torch.Tensor:
    """[..., A, T] -> [..., A, steps]: softmax probability of the chosen token per decode step, 0 where the mask is False"""
    sl = slice(hist_cols, hist_cols + steps)
    return torch.where(mask[..., sl], torch.exp(logprob[..., sl]), torch.zeros_like(logprob[..., sl]))


def fixed_order_sum(x: torch.Tensor) -> torch.Tensor:
    """float64 sum over the last dimension by a pairwise tree over the element INDICES (neighbours first): element-wise adds only,
    so the result is bitwise the same on every device and for every amount of trailing zero padding (x + 0 = x)"""
    x = x.double()
    n = x.shape[-1]
    p = 1
    while p < n:
        p *= 2
    if p != n:
        x = torch.cat([x, x.new_zeros(x.shape[:-1] + (p - n,))], dim=-1)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0] if n else x.new_zeros(x.shape[:-1])


def rollout_logprob(logprob: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """[..., A, T] -> [...] float64: the log-likelihood of the rollout's own tokens, rows in row-major (row, column) order.  Rows
    beyond A that a padded layout carries must be masked out; they then change nothing (``fixed_order_sum``)."""
    v = torch.where(mask, logprob.double(), torch.zeros((), dtype=torch.float64, device=logprob.device))
    return fixed_order_sum(v.reshape(v.shape[:-2] + (-1,)))
