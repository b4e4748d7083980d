"""numpy restatement of the "observations" block of include/infgen_hip.h, and the named inputs the observation tests share.

``evaluate(case)`` follows the definition twice:
  * in float32, operation by operation as the header writes it (numpy rounds every operation, no fused multiply-add): this
    evaluation DECIDES membership, order, indices and counts, and gives the fields that are copies or flags;
  * in float64 from the same float32 inputs, for the values (rotated positions, headings, velocities, the yaw rate) of the entries
    the float32 evaluation selected.
It also returns the float32-formed differences the tests' bars are made of.
"""
from __future__ import annotations

import numpy as np

SELF, NBR, MAP, MAX_K = 8, 10, 6, 64
F32 = np.float32
PI_F, TWO_PI_F = F32(3.14159274), F32(6.28318548)


def clamp_type(t):
    return 0 if t < 0 or t > 2 else int(t)


def d2_f32(px, py, qx, qy):
    """fl(fl(dx * dx) + fl(dy * dy)) of q - p, every operation rounded to float32"""
    dx = np.asarray(qx, F32) - F32(px)
    dy = np.asarray(qy, F32) - F32(py)
    return (dx * dx).astype(F32) + (dy * dy).astype(F32), dx, dy


def d2_f64(px, py, qx, qy):
    dx = np.asarray(qx, np.float64) - np.float64(px)
    dy = np.asarray(qy, np.float64) - np.float64(py)
    return dx * dx + dy * dy


def select(d2, idx, r2, k):
    """candidates idx with distances d2: (the first k by ascending d2, ties by ascending index, among d2 <= r2; their number)"""
    keep = d2 <= r2
    idx, d2 = idx[keep], d2[keep]
    order = np.lexsort((idx, d2))
    return idx[order][:k], int(keep.sum())


def wrap64(a):
    return (a + np.pi) % (2.0 * np.pi) - np.pi


def wrap32(a):
    r = np.fmod(F32(a) + PI_F, TWO_PI_F)
    if r < 0:
        r = F32(r + TWO_PI_F)
    return F32(r - PI_F)


def live(case, s, col, i):
    n = min(int(case['n_agents'][s]), case['pos'].shape[2])
    return 0 <= col and i < n and case['state'][s, col, i] != 0


def rows_of(case):
    S, _, A = case['pos'].shape[:3]
    return np.arange(S * A, dtype=np.int32) if case.get('rows') is None else np.asarray(case['rows'], np.int32)


def _rot(dx, dy, ci, si):
    return dx * ci + dy * si, dy * ci - dx * si


def evaluate(case):
    """-> dict: the seven outputs with float64 values (``*_feat``), the same in float32 arithmetic (``*_feat32``), and the bars'
    scales: ``self_scale`` [N] = |dx| + |dy| of the row's own displacement, ``nbr_scale`` [N, K, 2] = that of (position
    difference, displacement of j), ``map_scale`` [N, Km]"""
    pos, head, state = case['pos'], case['head'], case['state']
    S, T, A = pos.shape[:3]
    c, dt, K, Km, copies = case['c'], case['dt'], case['K'], case['Km'], case.get('copies', 1)
    rows = rows_of(case)
    N = len(rows)
    out = dict(self_feat=np.zeros((N, SELF)), nbr_feat=np.zeros((N, K, NBR)), nbr_index=np.full((N, K), -1, np.int32),
               nbr_count=np.zeros(N, np.int32), map_feat=np.zeros((N, Km, MAP)), map_index=np.full((N, Km), -1, np.int32),
               map_count=np.zeros(N, np.int32), self_scale=np.zeros(N), nbr_scale=np.zeros((N, K, 2)), map_scale=np.zeros((N, Km)))
    for k in ('self_feat', 'nbr_feat', 'map_feat'):
        out[k + '32'] = np.zeros(out[k].shape, F32)
    r2 = F32(case['radius']) * F32(case['radius'])
    mr2 = F32(case['map_radius']) * F32(case['map_radius'])
    has_map = case.get('map_pos') is not None
    for n, row in enumerate(rows):
        if not 0 <= row < S * A:
            continue
        s, i = divmod(int(row), A)
        if not live(case, s, c, i):
            continue
        px, py, ph = pos[s, c, i, 0], pos[s, c, i, 1], head[s, c, i]
        frames = {F32: (np.cos(F32(ph)), np.sin(F32(ph))), np.float64: (np.cos(np.float64(ph)), np.sin(np.float64(ph)))}

        def velocity(j, ft):
            """j's displacement c - 1 -> c over dt in row i's frame, (0, 0) without a previous pose; and |dx| + |dy| (float32)"""
            if not live(case, s, c - 1, j):
                return ft(0), ft(0), 0.0
            ux32, uy32 = pos[s, c, j, 0] - pos[s, c - 1, j, 0], pos[s, c, j, 1] - pos[s, c - 1, j, 1]
            ux = (ft(pos[s, c, j, 0]) - ft(pos[s, c - 1, j, 0])) / ft(dt)
            uy = (ft(pos[s, c, j, 1]) - ft(pos[s, c - 1, j, 1])) / ft(dt)
            return _rot(ux, uy, *frames[ft]) + (float(abs(ux32)) + float(abs(uy32)),)

        for ft, key in ((np.float64, 'self_feat'), (F32, 'self_feat32')):
            vx, vy, scale = velocity(i, ft)
            hp = live(case, s, c - 1, i)
            yaw = 0.0
            if hp:
                yaw = wrap64(np.float64(ph) - np.float64(head[s, c - 1, i])) / dt if ft is np.float64 else \
                    wrap32(F32(ph) - head[s, c - 1, i]) / F32(dt)
            out[key][n] = [1.0, vx, vy, yaw, case['shape'][s, i, 0], case['shape'][s, i, 1], clamp_type(case['type'][s, i]), float(hp)]
            out['self_scale'][n] = scale

        # neighbours: decided in float32
        na = min(int(case['n_agents'][s]), A)
        cand = np.array([j for j in range(max(na, 0)) if j != i and state[s, c, j] != 0], np.int64)
        d2, dx32, dy32 = d2_f32(px, py, pos[s, c, cand, 0], pos[s, c, cand, 1])
        sel, out['nbr_count'][n] = select(d2, cand, r2, K)
        out['nbr_index'][n, :len(sel)] = sel
        for e, j in enumerate(sel):
            for ft, key in ((np.float64, 'nbr_feat'), (F32, 'nbr_feat32')):
                ci, si = frames[ft]
                dx, dy = ft(pos[s, c, j, 0]) - ft(px), ft(pos[s, c, j, 1]) - ft(py)
                cj, sj = np.cos(ft(head[s, c, j])), np.sin(ft(head[s, c, j]))
                vx, vy, vscale = velocity(j, ft)
                out[key][n, e] = [*_rot(dx, dy, ci, si), cj * ci + sj * si, sj * ci - cj * si, vx, vy, case['shape'][s, j, 0],
                                  case['shape'][s, j, 1], clamp_type(case['type'][s, j]), 1.0]
            out['nbr_scale'][n, e] = [float(abs(F32(pos[s, c, j, 0]) - F32(px))) + float(abs(F32(pos[s, c, j, 1]) - F32(py))), vscale]

        # map tokens of map scene s // copies
        if has_map:
            ms = s // copies
            nm = min(max(int(case['n_map'][ms]), 0), case['map_pos'].shape[1])
            cand = np.arange(nm, dtype=np.int64)
            mp = case['map_pos'][ms]
            d2, _, _ = d2_f32(px, py, mp[:nm, 0], mp[:nm, 1])
            sel, out['map_count'][n] = select(d2, cand, mr2, Km)
            out['map_index'][n, :len(sel)] = sel
            for e, m in enumerate(sel):
                for ft, key in ((np.float64, 'map_feat'), (F32, 'map_feat32')):
                    ci, si = frames[ft]
                    dx, dy = ft(mp[m, 0]) - ft(px), ft(mp[m, 1]) - ft(py)
                    cm, sm = np.cos(ft(case['map_orient'][ms, m])), np.sin(ft(case['map_orient'][ms, m]))
                    out[key][n, e] = [*_rot(dx, dy, ci, si), cm * ci + sm * si, sm * ci - cm * si, float(case['map_type'][ms, m]), 1.0]
                out['map_scale'][n, e] = float(abs(F32(mp[m, 0]) - F32(px))) + float(abs(F32(mp[m, 1]) - F32(py)))
    return out


# ---------------------------------------------------------------------------------------------- cases
# (the seeds of the random cases are chosen so that every row's candidates are separated: tests/test_observe_cpu.py asserts it)
def _scene(seed, S, T, A, n_agents, M, n_map, copies=1, centre=(0.0, 0.0), extent=40.0, grid=None, speed=6.0):
    """random scenes: agents move on straight lines from column to column; ``grid``: coordinates are multiples of it (distances are
    then exact in float32, and equal ones are exact ties)"""
    rng = np.random.default_rng(seed)
    S0 = S // copies

    def coords(*shape):
        x = rng.uniform(-extent, extent, shape)
        return (np.round(x / grid) * grid if grid else x)

    p0 = coords(S, 1, A, 2)
    v = rng.uniform(-speed, speed, (S, 1, A, 2)) * 0.5
    if grid:
        v = np.round(v / grid) * grid
    pos = (p0 + v * np.arange(T)[None, :, None, None] + np.asarray(centre)).astype(F32)
    head = (rng.uniform(-3.0, 3.0, (S, 1, A)) + rng.uniform(-0.2, 0.2, (S, T, A))).astype(F32)
    state = np.ones((S, T, A), np.int32)
    return dict(pos=pos, head=head, state=state, n_agents=np.asarray(n_agents, np.int32),
                type=rng.integers(0, 3, (S, A)).astype(np.int32),
                shape=np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1).astype(F32),
                map_pos=(coords(S0, M, 2) + np.asarray(centre)).astype(F32), map_orient=rng.uniform(-3.1, 3.1, (S0, M)).astype(F32),
                map_type=rng.integers(0, 20, (S0, M)).astype(np.int64), n_map=np.asarray(n_map, np.int32), copies=copies,
                c=T - 1, dt=0.5, rows=None, K=8, radius=np.inf, Km=16, map_radius=np.inf)


def _ragged():
    k = _scene(101, 3, 4, 70, (70, 5, 1), 130, (130, 3, 0))
    k['state'][0, 3, [4, 9, 33, 69]] = 0              # skipped as neighbours, all-zero as observed rows
    k['state'][1, 3, 2] = 0
    k['state'][0, 2, [5, 12]] = 0                     # live now, not before: no velocity
    k['type'][0, 7], k['type'][0, 8] = 5, -1          # clamped to 0
    k.update(radius=30.0, map_radius=25.0)
    return k


def _ties_and_boundary():
    """integer coordinates around row 0 at the origin: mirrored neighbours of equal d2, a row at the same position as another, one
    exactly on the radius (3, 4 with radius 5) and one just outside (d2 = 26); the same for the map"""
    pts = [(0, 0), (2, 0), (-2, 0), (0, 2), (0, -2), (3, 4), (1, 5), (5, 1), (0, 0), (-4, 3), (4, 4), (1, 1), (1, 1)]
    mpts = [(3, 4), (-3, -4), (1, 5), (5, -1), (0, 0), (0, 0), (1, 0), (-1, 0), (0, 5), (4, 3), (6, 0)]
    A, M = len(pts), len(mpts)
    k = _scene(12, 1, 3, A, (A,), M, (M,))
    k['pos'][0, :, :, :] = np.asarray(pts, F32)[None]
    k['pos'][0, 1] += F32(0.5)                        # column 1 differs: velocities are not zero
    k['pos'][0, 2] = np.asarray(pts, F32)
    k['map_pos'][0] = np.asarray(mpts, F32)
    k.update(K=16, radius=5.0, Km=16, map_radius=5.0)
    return k


def _first_column():
    k = _scene(13, 2, 3, 9, (9, 6), 20, (20, 11))
    k.update(c=0, K=4, Km=4)
    return k


def _prev_not_live():
    k = _scene(14, 2, 3, 9, (9, 6), 20, (20, 11))
    k['state'][0, 1, [1, 3]] = 0                      # neighbours (and observed rows) that were not in the scene at c - 1
    k['state'][1, 1, 0] = 0
    k['head'][0, 1, 2], k['head'][0, 2, 2] = F32(3.1), F32(-3.1)     # the heading difference wraps
    k.update(c=2, K=8, Km=4)
    return k


def _many():
    k = _scene(15, 1, 2, 200, (200,), 1030, (1030,), extent=30.0, grid=0.5, speed=4.0)
    k.update(K=64, radius=200.0, Km=64, map_radius=90.0)
    k['rows'] = np.arange(0, 200, 7, dtype=np.int32)  # (every row sees the same 199 candidates: a sample keeps the test quick)
    return k


def _copies():
    k = _scene(16, 4, 3, 10, (10, 7, 4, 9), 40, (40, 17), copies=2)
    k.update(K=4, radius=35.0, Km=8, map_radius=30.0)
    return k


def _far_world():
    k = _scene(27, 2, 3, 12, (12, 8), 40, (40, 25), centre=(8000.0, -6000.0))
    k.update(K=6, radius=45.0, Km=8, map_radius=40.0)
    return k


def _rows(K=5, Km=6):
    k = _scene(18, 2, 3, 10, (10, 6), 30, (30, 12))
    k['state'][0, 2, 3] = 0
    #                   repeated   not live (state)  padding row  out of range
    k['rows'] = np.asarray([4, 4, 12, 3, 10 + 8, 20, -1, 1000000, 0, 15], np.int32)
    k.update(K=K, radius=50.0, Km=Km, map_radius=45.0)
    return k


CASES = dict(ragged=_ragged(), ties_and_boundary=_ties_and_boundary(), first_column=_first_column(), prev_not_live=_prev_not_live(),
             many=_many(), copies=_copies(), far_world=_far_world(), rows=_rows(), rows_k0=_rows(K=0), rows_km0=_rows(Km=0))
