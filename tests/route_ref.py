"""numpy restatement of route-following decoding's allowed-token sets ("route masks" of include/infgen_hip.h), written
twice - in float32 with the kernel's operation order (it decides bits) and in float64 (it decides which tokens are too close to a
threshold to pin) - and the operator-level cases the CPU and GPU tests share.  numpy only."""
from __future__ import annotations

import functools

import numpy as np

INVALID = 0
BAND = 1e-4          # metres (m^2 for a tie of two segments' d2): a decision closer than this to its threshold may fall either way
DEAD = np.array([0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0])
CORRIDOR, BACK, FINISH, TYPES = 2.0, 0.5, 1.0, (1, 0, 1)
PACES = (0.0, 0.5, 1.0)


# ---------------------------------------------------------------------------------------- the definition
def end_centres(vocab, dt):
    """vocab [3][K][6][4][2] -> the end boxes' centres [3][K][2]: the mean of the last contour's corners, summed in corner order"""
    last = np.asarray(vocab, np.float32)[:, :, -1].astype(dt)
    return (((last[:, :, 0] + last[:, :, 1]) + last[:, :, 2]) + last[:, :, 3]) * dt(0.25)


def records(routes, n_points, dt=np.float32):
    """routes [S0][A][P][2] float32, n_points [S0][A] -> records [S0][A][P - 1][8], total [S0][A] in dtype dt, cum summed in order"""
    routes = np.asarray(routes, np.float32)
    S0, A, P, _ = routes.shape
    rec = np.tile(DEAD.astype(dt), (S0, A, P - 1, 1))
    total = np.zeros((S0, A), dt)
    with np.errstate(all='ignore'):
        for s in range(S0):
            for i in range(A):
                n = min(max(int(n_points[s, i]), 0), P)
                run = dt(0.0)
                for j in range(n - 1):
                    a, b = routes[s, i, j].astype(dt), routes[s, i, j + 1].astype(dt)
                    dx, dy = b[0] - a[0], b[1] - a[1]
                    L = np.sqrt(dx * dx + dy * dy)
                    if L > 0 and np.isfinite(L) and np.isfinite(a).all():
                        rec[s, i, j] = [a[0], a[1], dx / L, dy / L, L, run, 0, 0]
                        run = dt(run + L)
                total[s, i] = run
    return rec, total


def _frame(rec, px, py, h, dt):
    """the live records of a row, in order, in the row's frame: [m][6] = q0 x, y, u x, y, L, cum; and |p0 - pos| per live record"""
    live = rec[rec[:, 4] > 0].astype(dt)
    ci, si = np.cos(dt(h)), np.sin(dt(h))
    dx, dy = live[:, 0] - dt(px), live[:, 1] - dt(py)
    out = np.stack([dx * ci + dy * si, dy * ci - dx * si, live[:, 2] * ci + live[:, 3] * si, live[:, 3] * ci - live[:, 2] * si,
                    live[:, 4], live[:, 5]], 1).astype(dt)
    return out, np.abs(dx) + np.abs(dy)


def _project(ex, ey, segs, dt):
    """points (ex, ey) [K] on the segments [m][6] -> (s, d2, index) of the first least d2, and the [m][K] tables of s and d2"""
    ex, ey = np.asarray(ex, dt), np.asarray(ey, dt)
    S_all, D_all = np.zeros((len(segs),) + ex.shape, dt), np.zeros((len(segs),) + ex.shape, dt)
    s, best, idx = np.zeros(ex.shape, dt), np.full(ex.shape, np.inf, dt), np.zeros(ex.shape, np.int64)
    for e, g in enumerate(segs):
        rx, ry = ex - g[0], ey - g[1]
        t = np.fmin(np.fmax(rx * g[2] + ry * g[3], dt(0.0)), g[4])
        fx, fy = rx - t * g[2], ry - t * g[3]
        d2 = fx * fx + fy * fy
        S_all[e], D_all[e] = g[5] + t, d2
        take = d2 < best
        s, best, idx = np.where(take, g[5] + t, s), np.where(take, d2, best), np.where(take, e, idx)
    return s, best, idx, S_all, D_all


def _interval(S_all, D_all, best):
    """what a tie of d2 within BAND leaves open: the ranges of s and d over every segment that close to the least d2"""
    tied = D_all <= best[None] + BAND
    d = np.sqrt(D_all)
    big = np.float64(np.inf)
    return (np.where(tied, S_all, big).min(0), np.where(tied, S_all, -big).max(0), np.where(tied, d, big).min(0), np.where(tied, d, -big).max(0))


def _unsure_le(xlo, xhi, ylo, yhi):
    """the comparison x <= y (or <) of two ranges is open: they come within BAND of each other"""
    return (xlo - BAND <= yhi) & (xhi + BAND >= ylo)


def reference(case, pace, dt=np.float32, first_new=None):
    """the definition, row by row, in dtype dt.  -> dict: allowed (after the fallback) / pre (before it) bool [rows][K], base, count [rows]
    (of pre), progress [rows][4], ruled [rows] (the rule was applied: in the scene, a route, type on, not finished), scale [rows] (|dx| +
    |dy| of the chosen segment's p0 from the row).  dt float64 adds near bool [rows][K] and row_open [rows]: the row's own decisions
    (finished, gmax > 0, s0 across a tie) are within BAND of flipping"""
    f64 = dt == np.float64
    pos, head, state, n_agents, atype = case['pos'], case['head'], case['state'], case['n_agents'], case['atype']
    S, T, A = state.shape
    K, c, copies = case['token_size'], case['c'], case['copies']
    rec, total = records(case['routes'], case['n_points'], dt)
    centre = end_centres(case['vocab'], dt)
    base = np.ones((S * A, K), bool) if case['base_rows'] is None else case['base_rows'].copy()
    pre = base.copy()
    progress = np.zeros((S * A, 4), dt)
    ruled, scale = np.zeros(S * A, bool), np.zeros(S * A)
    near, row_open = np.zeros((S * A, K), bool), np.zeros(S * A, bool)
    corridor, back, finish = dt(CORRIDOR), dt(BACK), dt(FINISH)
    for s in range(S):
        n = min(int(n_agents[s]), A) if first_new is None else min(int(n_agents[s]), int(first_new[s]), A)
        for i in range(A):
            row = s * A + i
            ty = int(atype[s, i]) if 0 <= int(atype[s, i]) <= 2 else 0
            tot = total[s // copies, i]
            progress[row, 2] = tot
            if not (i < n and state[s, c, i] != INVALID and TYPES[ty] and tot > 0):
                continue
            segs, dist = _frame(rec[s // copies, i], pos[s, c, i, 0], pos[s, c, i, 1], head[s, c, i], dt)
            s0, b0, i0, S0a, D0a = _project(np.zeros(1), np.zeros(1), segs, dt)
            s0, d0 = s0[0], np.sqrt(b0[0])
            finished = not (s0 < tot - finish)
            progress[row] = [s0, d0, tot, 2 if finished else 1]
            scale[row] = dist[i0[0]]
            if f64:
                s0lo, s0hi, d0lo, d0hi = (v[0] for v in _interval(S0a, D0a, b0))
                row_open[row] = _unsure_le(s0lo, s0hi, tot - finish, tot - finish)
            if finished:
                continue
            ruled[row] = True
            sk, bk, _, Sa, Da = _project(centre[ty, :, 0], centre[ty, :, 1], segs, dt)
            dk = np.sqrt(bk)
            lo = s0 - back
            on = ((dk <= corridor) | (dk < d0)) & (sk >= lo)
            gain = sk - s0
            cand = base[row] & on
            gmax = gain[cand].max() if cand.any() else dt(-np.inf)
            keep = on.copy()
            if pace > 0 and gmax > 0:
                keep &= ~(gain < dt(pace) * gmax)
            pre[row] = base[row] & keep
            if f64:
                slo, shi, dlo, dhi = _interval(Sa, Da, bk)
                in_corr, in_corr_sure = dlo <= corridor + BAND, dhi <= corridor - BAND
                closer, closer_sure = dlo - BAND < d0hi, dhi + BAND < d0lo
                ahead, ahead_sure = shi + BAND >= s0lo - back, slo - BAND >= s0hi - back
                maybe, sure = (in_corr | closer) & ahead, (in_corr_sure | closer_sure) & ahead_sure
                near[row] = maybe & ~sure
                if pace > 0:
                    glo, ghi = slo - s0hi, shi - s0lo
                    g_sure = glo[base[row] & sure].max() if (base[row] & sure).any() else -np.inf
                    g_maybe = ghi[base[row] & maybe].max() if (base[row] & maybe).any() else -np.inf
                    row_open[row] |= (g_maybe > -BAND) != (g_sure > BAND)
                    if g_maybe > 0:
                        at_bar = maybe & _unsure_le(glo, ghi, pace * max(g_sure, 0.0), pace * g_maybe)
                        if pace == 1 and (base[row] & sure).any():
                            # the bar is the largest gain itself: the token that holds it alone - no other within 2 BAND - is at the
                            # bar in every precision (x < x is false), not near it
                            top = int(np.argmax(np.where(base[row] & sure, glo, -np.inf)))
                            rivals = base[row] & maybe & (ghi >= glo[top] - 2 * BAND)
                            rivals[top] = False
                            if not rivals.any():
                                at_bar[top] = False
                        near[row] |= at_bar
    empty = ~pre.any(axis=1)
    allowed = pre.copy()
    allowed[empty] = base[empty]
    out = dict(allowed=allowed, pre=pre, base=base, count=pre.sum(axis=1), progress=progress, ruled=ruled, scale=scale)
    if f64:
        out.update(near=near & base, row_open=row_open)
    return out


# ---------------------------------------------------------------------------------------- the operator-level cases
# S = 4 row-scenes, 2 scenes x 2 copies; T = 6; the route rows of scene 0: 0 a plain route, 1 no points, 2 one point, 3 a dead segment
# in the middle, 4 a NaN waypoint; of scene 1: 0 starts 3 corridors off its route, 1 past total - finish, 2 a U-turn whose legs run 1.5 m
# apart, 3 a pedestrian (type off), 4 at first_new.  Further rows (A = 32): random routes of 2 .. P points.
CASES = {
    'k64_a5_p2': dict(token_size=64, A=5, P=2, seed=1),
    'k96_a5_p3': dict(token_size=96, A=5, P=3, seed=2),
    'k2048_a32_p32': dict(token_size=2048, A=32, P=32, seed=3),
    'k4096_a5_p32': dict(token_size=4096, A=5, P=32, seed=4),
    'k64_a32_p32': dict(token_size=64, A=32, P=32, seed=5),
}
S_CASE, T_CASE, C_CASE, COPIES = 4, 6, 3, 2
ORIGIN = np.array([5000.0, -5000.0])      # the routes lie 5 km from the origin: the exact-difference rule matters
FIRST_NEW = np.array([32, 32, 4, 4], np.int32)


def _walk(rng, n, start, h):
    pts = [np.asarray(start, np.float64)]
    stretch = max(1.0, 16.0 / max(n - 1, 1))              # few points: long segments, so that no token reaches the route's end
    for _ in range(n - 1):
        h += rng.uniform(-0.4, 0.4)
        pts.append(pts[-1] + stretch * rng.uniform(3.0, 6.0) * np.array([np.cos(h), np.sin(h)]))
    return np.array(pts)


def _at(pts, frac, lateral):
    """the point at `frac` of the polyline's length, moved `lateral` metres to its left, and the tangent's heading there"""
    seg = np.diff(pts, axis=0)
    L = np.linalg.norm(seg, axis=1)
    keep = np.isfinite(L) & (L > 0)
    cum = np.concatenate([[0.0], np.cumsum(np.where(keep, L, 0.0))])
    want = frac * cum[-1]
    j = next(k for k in range(len(L)) if keep[k] and cum[k + 1] >= want - 1e-9)
    u = seg[j] / L[j]
    return pts[j] + (want - cum[j]) * u + lateral * np.array([-u[1], u[0]]), np.arctan2(u[1], u[0])


def thin_vocab(vocab, token_size):
    n = next(iter(vocab.values())).shape[0]
    if token_size == n:
        return vocab
    keep = np.sort(np.random.default_rng(0).choice(n, token_size, replace=False))
    return {k: np.ascontiguousarray(v[keep]) for k, v in vocab.items()}


@functools.lru_cache(maxsize=None)
def _vocab(token_size):
    from infgen_amd import synth
    return thin_vocab(synth.make_agent_vocab(4096 if token_size == 4096 else 2048), token_size)


@functools.lru_cache(maxsize=None)
def make_case(name, with_base=False):
    k = CASES[name]
    rng = np.random.default_rng(k['seed'])
    A, K, P, S, T, c = k['A'], k['token_size'], k['P'], S_CASE, T_CASE, C_CASE
    S0 = S // COPIES
    routes, n_points = np.zeros((S0, A, P, 2), np.float32), np.zeros((S0, A), np.int32)
    pos = (ORIGIN + rng.uniform(-50.0, 50.0, (S, T, A, 2))).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, (S, T, A)).astype(np.float32)
    atype = np.where(rng.random((S, A)) < 0.7, 0, 2).astype(np.int32)
    place = {}                                            # (scene, row) -> (fraction of the length, lateral offset)
    for s0 in range(S0):
        for i in range(A):
            n = P if i < 5 else int(rng.integers(2, P + 1))
            pts = _walk(rng, n, ORIGIN + rng.uniform(-40.0, 40.0, 2), rng.uniform(-np.pi, np.pi))
            where = (rng.uniform(0.0, 0.6), rng.uniform(-1.5, 1.5))
            if (s0, i) == (0, 1):
                n = 0
            elif (s0, i) == (0, 2):
                n = 1
            elif (s0, i) == (0, 3) and P >= 4:
                pts[P // 2] = pts[P // 2 - 1]             # a repeated point: the segment between the two has L == 0
            elif (s0, i) == (0, 4) and P >= 5:
                pts[P - 2] = np.nan                       # two dead segments near the end; the row stands in front of them
                where = (rng.uniform(0.0, 0.3), where[1])
            elif (s0, i) == (1, 0):
                where = (where[0], 3.0 * CORRIDOR)
            elif (s0, i) == (1, 1):
                where = (-0.3, 0.2)                       # 0.3 m in front of the route's end
            elif (s0, i) == (1, 2) and P >= 5:
                th = rng.uniform(-np.pi, np.pi)
                R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
                turn = np.array([[0.0, 0.0], [20.0, 0.0], [21.0, 0.75], [20.0, 1.5], [0.0, 1.5]])
                pts, n = pts[0] + turn @ R.T, 5
                where = (rng.uniform(0.15, 0.3), 0.3)     # on the first leg, the second 1.2 m to its left
            routes[s0, i, :n], n_points[s0, i] = pts[:n].astype(np.float32), n
            place[s0, i] = where
    for s in range(S):
        for i in range(A):
            n = int(n_points[s // COPIES, i])
            if n >= 2:
                frac, lat = place[s // COPIES, i]
                pts = routes[s // COPIES, i, :n].astype(np.float64)
                if frac < 0:
                    frac = 1.0 + frac / np.linalg.norm(np.diff(pts, axis=0), axis=1).sum()
                elif s % COPIES:                          # the copies stand elsewhere on the same route
                    frac = frac + rng.uniform(0.0, 0.1)
                p, h = _at(pts, frac, lat + (rng.uniform(-0.3, 0.3) if s % COPIES else 0.0))
                pos[s, c, i], head[s, c, i] = p.astype(np.float32), np.float32(h + rng.uniform(-0.4, 0.4))
    atype[COPIES:, 3] = 1                                 # scene 1, row 3: a pedestrian
    atype[COPIES:, :3] = np.where(atype[COPIES:, :3] == 1, 0, atype[COPIES:, :3])
    state = np.ones((S, T, A), np.int32)
    n_agents = np.full(S, A, np.int32)
    if A > 8:
        n_agents[1], state[0, c, 7] = 20, INVALID         # padding rows, and a row that is not in the scene at c
    shape = np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1).astype(np.float32)
    v = _vocab(K)
    out = dict(k, name=name, S=S, T=T, c=c, copies=COPIES, pos=pos, head=head, state=state, n_agents=n_agents, atype=atype, shape=shape,
               routes=routes, n_points=n_points, first_new=np.minimum(FIRST_NEW, A).astype(np.int32),
               vocab=np.stack([v[t] for t in ('veh', 'ped', 'cyc')]).astype(np.float32), base_rows=None)
    if with_base:      # static sets, some of them so small that the route rule empties the row: set 3 holds the reversing tokens only
        sets = rng.random((4, K)) < 0.5
        sets[:, 0] = True
        centre = end_centres(out['vocab'], np.float64)
        sets[3] = centre[0, :, 0] < -0.55
        assert sets[3].any()
        mask_row = rng.choice(np.array([-1, -1, 0, 1, 3], np.int32), S * A).astype(np.int32)
        mask_row[0] = 3                                   # scene 0's plain route: backwards only, all behind s0 - back
        sel = np.where(mask_row >= 0, mask_row, atype.reshape(-1))
        out.update(sets=sets, mask_row=mask_row, mask_type=[0, 1, 2], base_rows=sets[sel])
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name, with_base, pace, f64, first_new=False):
    case = make_case(name, with_base)
    return reference(case, pace, np.float64 if f64 else np.float32, case['first_new'] if first_new else None)
