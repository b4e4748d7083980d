"""Vectorised numpy restatement of the reference's validation metrics (infgen/utils/metrics.py) - the yardstick the device
classes of infgen_amd/utils/metrics.py are compared with where no fixture of the reference exists (end-to-end tests), itself
checked against the reference's fixtures (tests/golden/valmetrics_*.npz) by tests/test_val_metrics_cpu.py.  Integers are exact,
floating sums float64."""
import numpy as np

STATE_TOKEN = dict(invalid=0, valid=1, enter=2, exit=3)


def state_accuracy(state, mask=None, state_token=STATE_TOKEN):
    """StateAccuracy.update (:499-543) -> int64 [4]: valid, valid_count, invalid, invalid_count"""
    s = np.asarray(state).astype(np.int64)
    N, T = s.shape
    inv_s, val_s, ent, ext = (int(state_token[k]) for k in ('invalid', 'valid', 'enter', 'exit'))
    cols = np.arange(T)[None]

    def first(m):
        return m.any(1), m.argmax(1)

    hb, bos = first(s == ent)
    he, eos = first(s == ext)
    b, e = np.where(hb, bos, 0)[:, None], np.where(he, eos, T - 1)[:, None]
    is_inv = s == inv_s
    invalid = (is_inv & hb[:, None] & (cols < bos[:, None])).sum() + (is_inv & he[:, None] & (cols > eos[:, None])).sum()
    invalid_count = (hb * bos).sum() + (he * (T - 1 - eos)).sum()
    valid = ((s == val_s) & (cols > b) & (cols < e)).sum()
    valid_count = np.maximum(e - b - 1, 0).sum()
    if mask is not None:
        m = np.asarray(mask).astype(np.int64)
        r = np.roll(s, 1, axis=1)
        hb, bos = first(r == ent)
        is_x = r == ext
        he, eos = is_x.any(1), T - 1 - is_x[:, ::-1].argmax(1)
        b, e = np.where(hb, bos, 0)[:, None], np.where(he, eos, T - 1)[:, None]
        invalid += ((m == 0) & hb[:, None] & (cols < bos[:, None])).sum() + ((m != 0) & he[:, None] & (cols > eos[:, None])).sum()
        invalid_count += (hb * bos).sum() + (he * (T - 1 - eos)).sum()
        inr = (cols >= b) & (cols <= e)
        differs = (r > 0).astype(np.int64) != m
        invalid += (inr & (m == 0) & differs).sum()
        invalid_count += (inr & (m == 0)).sum()
        valid += (inr & (m == 1) & differs).sum()
        valid_count += (inr & (m == 1)).sum()
    return np.array([valid, valid_count, invalid, invalid_count], np.int64)


def grid_overlap(state, grid, num_step, enter_state, seed_size, ptr=None):
    """GridOverlapRate.update (:574-591) per row range of ptr -> int64 [4][num_step]: overlap, insert, total, exceed_seed, with the
    closed form overlap = inserted rows - distinct inserted cells that no non-enter in-range row occupies"""
    s, g = np.asarray(state).astype(np.int64), np.asarray(grid).astype(np.int64)
    ptr = np.array([0, s.shape[0]]) if ptr is None else np.asarray(ptr).astype(np.int64)
    out = np.zeros((4, num_step), np.int64)
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        for t in range(num_step):
            cell, st = g[lo:hi, t], s[lo:hi, t]
            inr = cell != -1
            ins = inr & (st == enter_state)
            free = np.setdiff1d(np.unique(cell[ins]), np.unique(cell[inr & ~ins]))
            out[0, t] += ins.sum() - free.size
            out[1, t] += ins.sum()
            out[2, t] += inr.sum()
            out[3, t] += int(ins.sum() >= seed_size)
    return out


def traj_error(pred, target, valid):
    """minADE.update (:462-464) / minFDE.update (:384-387) -> ade_sum, ade_count, fde_sum, fde_count"""
    p, q, v = np.asarray(pred, np.float64), np.asarray(target, np.float64), np.asarray(valid)
    T = p.shape[1]
    E = min(70, T)
    d = np.sqrt(((p - q) ** 2).sum(-1))
    ade = ((d[:, :E] * v[:, :E]).sum(-1) / T).sum()
    ade_count = int(v[:, :E].any(-1).sum())
    F = E - 1
    fde = (d[:, F - 1:F] * v[:, F - 1][:, None]).sum()
    return float(ade), ade_count, float(fde), int(v[:, F - 1].sum())


def expand_logits(a, u, b, v):
    """the fixtures' logits [R, C] = a u^T + b v^T in float32 (two exactly rounded products and one sum per element)"""
    a, u, b, v = (np.asarray(x, np.float32) for x in (a, u, b, v))
    return (a[:, None] * u[None, :]) + (b[:, None] * v[None, :])


def ce_sums(logits, target, mask, weight=None):
    """-> S1 = sum w_y (-log p_y), S2 = sum_i sum_c w_c (-log p_ic), S3 = sum w_y over the rows with mask (float64)"""
    x = np.asarray(logits, np.float64)[np.asarray(mask).astype(bool)]
    y = np.asarray(target).astype(np.int64)[np.asarray(mask).astype(bool)]
    C = x.shape[1]
    w = np.ones(C) if weight is None else np.asarray(weight, np.float64)
    mx = x.max(1, keepdims=True) if x.size else np.zeros((0, 1))
    nlp = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True))) - x
    s1 = (w[y] * nlp[np.arange(len(y)), y]).sum()
    return float(s1), float((nlp * w[None]).sum()), float(w[y].sum())


def ce_loss(logits, target, mask, weight=None, eps=0.0):
    s1, s2, s3 = ce_sums(logits, target, mask, weight)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.float64((1.0 - eps) * s1 + eps / np.asarray(logits).shape[1] * s2) / np.float64(s3)
