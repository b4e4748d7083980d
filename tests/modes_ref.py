"""Restatement of the mode selection ("modes" of include/infgen_hip.h) and of minMultiFDE / minMultiADE in numpy - the yardstick
of infgen_amd/modes.py and of the two metric classes where no fixture of the reference exists, itself checked against the
reference's fixtures (tests/golden/modes_*.npz) by tests/test_modes_cpu.py.  Distances are float64 (of the float32 inputs), the
order is a stable sort; ``near_threshold`` reports the pairs whose distance lies within a relative 1e-5 of the threshold, where
the float32 kernel and this float64 text may disagree - a test asserts there are none.
``batch_nms_torch`` is the reference's batch_nms ALGORITHM (sort, gather, N x N distances, K arg-max rounds) written with torch
ops for the timing comparison of tools/time_mode_selection.py: a test helper, not product code."""
import numpy as np


def _goals(traj, t_goal):
    t = np.asarray(traj)
    return t[:, :, t_goal, 0].astype(np.float64), t[:, :, t_goal, 1].astype(np.float64)


def pair_dist(traj, t_goal=-1):
    """[B, N, N] float64 goal distances"""
    x, y = _goals(traj, t_goal)
    return np.sqrt((x[:, :, None] - x[:, None, :]) ** 2 + (y[:, :, None] - y[:, None, :]) ** 2)


def near_threshold(traj, dist_thresh, t_goal=-1, valid=None, rel=1e-5):
    """(b, i, j) of the pairs of valid candidates with |dist - dist_thresh| <= rel * dist_thresh"""
    d = pair_dist(traj, t_goal)
    bad = np.abs(d - float(dist_thresh)) <= rel * float(dist_thresh)
    if valid is not None:
        v = np.asarray(valid).astype(bool)
        bad &= v[:, :, None] & v[:, None, :]
    return np.argwhere(bad)


def density(traj, dist_thresh, t_goal=-1, valid=None):
    """float32 [B, N]: float(count) / float(N), count over the valid candidates within the threshold (0 for an invalid one)"""
    d = pair_dist(traj, t_goal)
    B, N = d.shape[:2]
    v = np.ones((B, N), bool) if valid is None else np.asarray(valid).astype(bool)
    cnt = ((d < float(np.float32(dist_thresh))) & v[:, None, :]).sum(-1)
    return np.where(v, cnt.astype(np.float32) / np.float32(N), np.float32(0)).astype(np.float32)


def select_modes(traj, k, dist_thresh, scores=None, valid=None, t_goal=-1):
    """-> mode_traj [B, k, T, F], mode_score [B, k] float32, mode_idx [B, k] int32 by the definition: order = (score descending,
    index ascending); k times the largest value among the unselected valid candidates (score, or 0 once covered), ties to the
    earlier of the order; the pick covers every candidate within the threshold of its goal, itself included"""
    traj = np.asarray(traj, np.float32)
    B, N, T, F = traj.shape
    d = pair_dist(traj, t_goal)
    thr = float(np.float32(dist_thresh))
    v = np.ones((B, N), bool) if valid is None else np.asarray(valid).astype(bool)
    s = density(traj, dist_thresh, t_goal, v) if scores is None else np.asarray(scores, np.float32)
    idx = np.full((B, k), -1, np.int32)
    sc = np.zeros((B, k), np.float32)
    out = np.zeros((B, k, T, F), np.float32)
    for b in range(B):
        order = np.lexsort((np.arange(N), -s[b].astype(np.float64)))          # stable: score descending, index ascending
        selected, covered = np.zeros(N, bool), np.zeros(N, bool)
        for kk in range(k):
            best, best_val = -1, -1.0
            for j in order:
                if not v[b, j] or selected[j]:
                    continue
                val = 0.0 if covered[j] else float(s[b, j])
                if val > best_val:
                    best, best_val = j, val
            if best < 0:
                break
            selected[best] = True
            covered |= v[b] & (d[b, best] < thr)
            covered[best] = True
            idx[b, kk], sc[b, kk], out[b, kk] = best, s[b, best], traj[b, best]
    return out, sc, idx


def multi_traj_error(pred, target, prob=None, valid=None, max_guesses=6, keep_invalid_final_step=True, min_criterion='FDE'):
    """minMultiADE.update / minMultiFDE.update -> ade_sum, fde_sum (float64), count; ``topk`` ties to the lower index, the
    guess with the smallest final error is the first minimum in guess order"""
    if min_criterion not in ('FDE', 'ADE'):
        raise ValueError('{} is not a valid criterion'.format(min_criterion))
    p, q = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    N, M, T = p.shape[:3]
    v = np.ones((N, T), bool) if valid is None else np.asarray(valid).astype(bool)
    G = min(int(max_guesses), M)
    ade = fde = 0.0
    count = 0
    for r in range(N):
        if not (v[r].any() if keep_invalid_final_step else v[r, -1]):
            continue
        guesses = np.arange(G)
        if prob is not None and G < M:
            guesses = np.lexsort((np.arange(M), -np.asarray(prob[r], np.float64)))[:G]
        last = int(np.flatnonzero(v[r])[-1])
        d = np.sqrt(((p[r, guesses] - q[r][None]) ** 2).sum(-1))                  # [G, T]
        f = d[:, last]
        mean = (d * v[r][None]).sum(-1) / v[r].sum()
        fde += f.min()
        ade += mean.min() if min_criterion == 'ADE' else mean[int(np.argmin(f))]
        count += 1
    return float(ade), float(fde), count


def guess_errors(pred, target, prob, valid, max_guesses):
    """per row taking part (any valid step): (final errors [G], masked means [G]) of its guesses - for the fixtures' no-tie check"""
    p, q, v = np.asarray(pred, np.float64), np.asarray(target, np.float64), np.asarray(valid).astype(bool)
    N, M, T = p.shape[:3]
    G = min(int(max_guesses), M)
    out = []
    for r in range(N):
        if not v[r].any():
            continue
        guesses = np.arange(G) if prob is None or G == M else np.lexsort((np.arange(M), -np.asarray(prob[r], np.float64)))[:G]
        d = np.sqrt(((p[r, guesses] - q[r][None]) ** 2).sum(-1))
        out.append((d[:, int(np.flatnonzero(v[r])[-1])], (d * v[r][None]).sum(-1) / v[r].sum()))
    return out


def batch_nms_torch(trajs, scores, dist_thresh, k):
    """the reference's batch_nms algorithm with torch ops on whatever device the tensors live on: sort the candidates by score,
    gather the whole trajectory tensor in that order, one [B, N, N] goal-distance tensor, k rounds of arg-max / cover / mark,
    gather the k winners.  -> trajs [B, k, T, F], scores [B, k], original indices [B, k]"""
    import torch
    B, N = scores.shape
    s_sorted, order = torch.sort(scores, dim=-1, descending=True, stable=True)
    rows = torch.arange(B, device=scores.device)
    t_sorted = trajs[rows[:, None], order]
    goal = t_sorted[:, :, -1, :2]
    cover = torch.cdist(goal, goal, compute_mode='donot_use_mm_for_euclid_dist') < dist_thresh
    val = s_sorted.clone()
    gone = torch.zeros_like(val)
    pick = torch.zeros(B, k, dtype=torch.long, device=scores.device)
    for i in range(k):
        cur = val.argmax(dim=-1)
        pick[:, i] = cur
        val = val * (~cover[rows, cur]).to(val.dtype)
        gone[rows, cur] = -1
        val = val + gone
    return t_sorted[rows[:, None], pick], s_sorted[rows[:, None], pick], order[rows[:, None], pick]
