"""NumPy restatements for the branching tests ("branching" of include/infgen_hip.h): the parent-vector contract, what
infgen_resample_parents computes, the two resamplers of infgen_amd/branching.py, and the gather itself.  Not a test module."""
import numpy as np


def sanitise(ancestor, copies):
    """ancestors [S0 * copies] -> the same with every entry outside its slot's group replaced by the slot itself"""
    a = np.asarray(ancestor, np.int64).reshape(-1).copy()
    s = np.arange(a.size)
    out = (a < 0) | (a >= a.size) | (a // copies != s // copies)
    a[out] = s[out]
    return a


def resample_parents(ancestor, copies):
    """a slot named at least once keeps itself; the unnamed slots, ascending, receive ancestor j's count[j] - 1 extra copies in
    ascending j"""
    a = sanitise(ancestor, copies)
    parent = np.empty_like(a)
    for g0 in range(0, a.size, copies):
        grp = a[g0:g0 + copies]
        count = np.bincount(grp - g0, minlength=copies)
        free = [g0 + j for j in range(copies) if count[j] == 0]
        surplus = [g0 + j for j in range(copies) for _ in range(max(count[j] - 1, 0))]
        assert len(free) == len(surplus)
        for j in range(copies):
            if count[j]:
                parent[g0 + j] = g0 + j
        for f, j in zip(free, surplus):
            parent[f] = j
    return parent


def bad_entries(parent, copies):
    """the slots whose entry breaks the contract (out of range, another group, a source that is itself moved)"""
    p = np.asarray(parent, np.int64).reshape(-1)
    S = p.size
    bad = []
    for s in range(S):
        q = int(p[s])
        if q == s:
            continue
        if not 0 <= q < S or q // copies != s // copies or int(p[q]) != q:
            bad.append(s)
    return bad


def effective(parent, copies):
    """the parent vector the kernel applies: bad entries read as the identity"""
    p = np.asarray(parent, np.int64).reshape(-1).copy()
    for s in bad_entries(parent, copies):
        p[s] = s
    return p


def systematic_ancestors(log_weight, u):
    lw = np.asarray(log_weight, np.float64)
    S0, n = lw.shape
    w = np.exp(lw - lw.max(axis=1, keepdims=True))
    cdf = np.cumsum(w / w.sum(axis=1, keepdims=True), axis=1)
    out = np.empty((S0, n), np.int64)
    for g in range(S0):
        at = (float(u[g]) + np.arange(n)) / n
        out[g] = np.minimum(np.searchsorted(cdf[g], at, side='right'), n - 1) + g * n
    return out


def keep_best(score, keep):
    sc = np.asarray(score)
    S0, n = sc.shape
    out = np.empty((S0, n), np.int64)
    for g in range(S0):
        order = sorted(range(n), key=lambda j: (-sc[g, j], j))
        best = order[:keep]
        for j in best:
            out[g, j] = g * n + j
        for i, j in enumerate(order[keep:]):
            out[g, j] = g * n + best[i % keep]
    return out
