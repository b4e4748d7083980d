"""numpy restatement of signal-aware decoding's allowed-token sets ("signal masks" of include/infgen_hip.h), written
twice - in float32 with the header's operation order (it decides bits) and in float64 (it decides which tokens are too close to a
threshold to pin) - and the hand-built operator-level cases the CPU and GPU tests share.  numpy only.

NEAR: each of g0, g_k, l0, l_k (and v.x) may carry an error of up to BAND in fp32; a (row, token) pair is NEAR when moving them by
that much can flip one of the rule's comparisons - for the cross-multiplied crossing test D = (half + hwa)(g_k - g0) - |l0 g_k - l_k g0|
that is |D| < BAND (2 (half + hwa) + |l0| + |l_k| + |g_k| + |g0|), its first-order sensitivity."""
from __future__ import annotations

import functools

import numpy as np

INVALID = 0
BAND = 1e-4          # metres (plain units for v.x): a decision closer than this to its threshold may fall either way
DEAD = np.array([0.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0])
SETBACK, ALIGN, TYPES = 0.5, 0.5, (1, 0, 1)
STEPS = (0, 1, 2, 4)                      # decode steps the cases are evaluated at: n_phase = 3, so t = 4 reads the row of t = 1


# ---------------------------------------------------------------------------------------- the definition
def end_poses(vocab, dt=np.float32):
    """vocab [3][K][6][4][2] -> ([3][K][4] = dx, dy, cos, sin of the last contour; [3] the largest displacement per type), the
    operations of infgen_collision_end_poses in their order"""
    last = np.asarray(vocab, np.float32)[:, :, -1].astype(dt)          # [3][K][4 corners][2]
    ctr = (((last[:, :, 0] + last[:, :, 1]) + last[:, :, 2]) + last[:, :, 3]) * dt(0.25)
    h = last[:, :, 0] - last[:, :, 3]                                   # front-left minus rear-left
    ln = np.sqrt(h[..., 0] * h[..., 0] + h[..., 1] * h[..., 1])
    with np.errstate(all='ignore'):
        cd, sd = np.where(ln > 0, h[..., 0] / ln, dt(1.0)), np.where(ln > 0, h[..., 1] / ln, dt(0.0))
    dmax = np.sqrt(ctr[..., 0] * ctr[..., 0] + ctr[..., 1] * ctr[..., 1]).max(axis=1)
    return np.stack([ctr[..., 0], ctr[..., 1], cd, sd], -1).astype(dt), dmax.astype(dt)


def records(lines, n_lines, dt=np.float32):
    """lines [S0][K][4] float32, n_lines [S0] -> records [S0][K][8] in dtype dt"""
    lines = np.asarray(lines, np.float32)
    S0, K, _ = lines.shape
    rec = np.tile(DEAD.astype(dt), (S0, K, 1))
    with np.errstate(all='ignore'):
        for s in range(S0):
            for j in range(min(max(int(n_lines[s]), 0), K)):
                ax, ay, bx, by = lines[s, j].astype(dt)
                dx, dy = bx - ax, by - ay
                L = np.sqrt(dx * dx + dy * dy)
                if L > 0 and np.isfinite(L) and np.isfinite(ax) and np.isfinite(ay):
                    ux, uy = dx / L, dy / L
                    rec[s, j] = [ax + dt(0.5) * dx, ay + dt(0.5) * dy, -uy, ux, dt(0.5) * L, 0, 0, 0]
    return rec


def reference(case, t, dt=np.float32, first_new=None):
    """the definition at decode step t, row by row, in dtype dt.  -> dict: allowed (after the fallback) / pre (before it) bool
    [rows][K], base, count [rows] (of pre), info [rows][4], ruled [rows], governed [rows] (some record governs the row), scale [rows]
    (|dx| + |dy| of info's record from the row, + hla + setback: the magnitudes that enter gap).  dt float64 adds near bool [rows][K],
    row_open [rows] (a governs decision is within BAND of flipping) and info_open [rows] (so is a decision of out_info)"""
    f64 = dt == np.float64
    pos, head, state, n_agents, atype, shape = (case[k] for k in ('pos', 'head', 'state', 'n_agents', 'atype', 'shape'))
    S, T, A = state.shape
    K, c, copies, n_phase = case['token_size'], case['c'], case['copies'], case['phase'].shape[1]
    # the records are the rule's INPUT as the table stores them, float32: the stored midpoint is the line (rounding a + 0.5 d to a
    # float32 world coordinate moves the line by up to half an ulp - 0.25 mm at 5 km -, which is no error of the rule)
    rec = records(case['lines'], case['n_lines'], np.float32).astype(dt)
    pose, dmax = end_poses(case['vocab'], dt)
    base = np.ones((S * A, K), bool) if case['base_rows'] is None else case['base_rows'].copy()
    pre = base.copy()
    info = np.tile(np.array([0.0, -1.0, 0.0, 0.0], dt), (S * A, 1))
    ruled, governed, scale = np.zeros(S * A, bool), np.zeros(S * A, bool), np.zeros(S * A)
    near, row_open, info_open = np.zeros((S * A, K), bool), np.zeros(S * A, bool), np.zeros(S * A, bool)
    setback, align = dt(SETBACK), dt(ALIGN)
    for s in range(S):
        n = min(int(n_agents[s]), A) if first_new is None else min(int(n_agents[s]), int(first_new[s]), A)
        s0 = s // copies
        closed = case['phase'][s0, t % n_phase] != 0
        for i in range(A):
            row = s * A + i
            ty = int(atype[s, i]) if 0 <= int(atype[s, i]) <= 2 else 0
            if not (i < n and state[s, c, i] != INVALID and TYPES[ty]):
                continue
            ruled[row] = True
            r = rec[s0]
            px, py, h = dt(pos[s, c, i, 0]), dt(pos[s, c, i, 1]), dt(head[s, c, i])
            ci, si = np.cos(h), np.sin(h)
            hla, hwa = dt(0.5) * dt(shape[s, i, 0]), dt(0.5) * dt(shape[s, i, 1])
            dx, dy = r[:, 0] - px, r[:, 1] - py
            qx, qy = dx * ci + dy * si, dy * ci - dx * si
            vx, vy = r[:, 2] * ci + r[:, 3] * si, r[:, 3] * ci - r[:, 2] * si
            ex, ey = hla - qx, dt(0.0) - qy
            g0 = (ex * vx + ey * vy) + setback
            l0 = ex * vy - ey * vx
            w = r[:, 4] + hwa
            on = closed & (r[:, 4] >= 0)
            gov = on & (vx >= align) & (g0 <= 0)
            governed[row] = gov.any()
            cand = gov & (np.abs(l0) <= w)
            flag = 1.0
            if cand.any():
                gap = np.where(cand, dt(0.0) - g0, dt(np.inf))
                j = int(np.argmin(gap))                                 # (the first least: ties go to the smaller index)
                flag = 2.0 if gap[j] <= dmax[ty] else 1.0
                info[row] = [gap[j], j, flag, 0.0]
                scale[row] = float(abs(dx[j]) + abs(dy[j]) + hla + setback)
            else:
                info[row] = [0.0, -1.0, 1.0, 0.0]
            fx, fy = pose[ty, :, 0] + hla * pose[ty, :, 2], pose[ty, :, 1] + hla * pose[ty, :, 3]
            runs = np.zeros(K, bool)
            for j in np.flatnonzero(gov):
                kx, ky = fx - qx[j], fy - qy[j]
                gk = (kx * vx[j] + ky * vy[j]) + setback
                lk = kx * vy[j] - ky * vx[j]
                cross = l0[j] * gk - lk * g0[j]
                reachw = w[j] * (gk - g0[j])
                runs |= (gk > 0) & (np.abs(cross) <= reachw)
                if f64:
                    D = reachw - np.abs(cross)
                    sens = BAND * (2 * w[j] + abs(l0[j]) + np.abs(lk) + np.abs(gk) + abs(g0[j]))
                    near[row] |= (np.abs(gk) < BAND) | ((gk > -BAND) & (np.abs(D) < sens))
            pre[row] = base[row] & ~runs
            if f64:
                row_open[row] = bool((on & (np.abs(vx - align) < BAND) & (g0 <= BAND)).any() or
                                     (on & (np.abs(g0) < BAND) & (vx >= align - BAND)).any())
                info_open[row] = bool((gov & (np.abs(np.abs(l0) - w) < BAND)).any())
                if cand.any():
                    gaps = np.sort(-g0[cand])
                    info_open[row] |= abs(gaps[0] - dmax[ty]) < BAND or (len(gaps) > 1 and gaps[1] - gaps[0] < BAND)
    empty = ~pre.any(axis=1)
    allowed = pre.copy()
    allowed[empty] = base[empty]
    out = dict(allowed=allowed, pre=pre, base=base, count=pre.sum(axis=1), info=info, ruled=ruled, governed=governed, scale=scale)
    if f64:
        out.update(near=near & base, row_open=row_open, info_open=info_open | row_open)
    return out


# ---------------------------------------------------------------------------------------- the operator-level cases
# S = 6 slots = 3 map scenes x 2 copies, A_cap = 5 (the last workgroup of four rows is ragged), T = 6, column 3; K = 64 line slots
# with n_lines = 0, 1 and 64; n_phase = 3.  Map scene 0 has no line: every row keeps its base.  Map scene 1 has one line, closed in
# phase rows 0 and 1 and open in row 2; its rows, slot 2: 0 in front of it, 1 astride it (the bumper is across), 2 past it, 3 facing
# against it, 4 off its right end so that the lateral test decides; slot 3: 0 a pedestrian (type off), 1 invalid at the column, 2 one
# metre in front - with a base table its set holds forward tokens only, so the fallback is taken -, 3 and 4 >= first_new.  Map scene 2
# has 64 lines - 1 of zero length, 2 with a NaN end (dead records, phase closed) - scattered over a 60 m square, its rows in front of
# five of them; the phase rows close about half the lines each, with bytes 1, 2 and 255.
CASES = {
    'k64': dict(token_size=64, seed=1),
    'k2048': dict(token_size=2048, seed=2),
    'k4096': dict(token_size=4096, seed=3),
}
S_CASE, A_CASE, T_CASE, C_CASE, COPIES, K_LINES, N_PHASE = 6, 5, 6, 3, 2, 64, 3
N_LINES = np.array([0, 1, 64], np.int32)
ORIGIN = np.array([5000.0, -5000.0])      # the lines lie 5 km from the origin: the exact-difference rule matters
FIRST_NEW = np.array([5, 5, 5, 3, 5, 4], np.int32)
FALLBACK_ROW = 3 * A_CASE + 2             # slot 3, row 2


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


def _line(mid, theta, half):
    """the line whose lawful direction of travel has heading theta: a (left) and b (right) as that traffic sees them"""
    left = np.array([-np.sin(theta), np.cos(theta)])
    return np.concatenate([mid + half * left, mid - half * left])


def _stand(mid, theta, gap, lateral, hla, turn=0.0):
    """the pose of a row whose front bumper is `gap` metres in front of the line (negative: across it) and `lateral` metres to the
    left of its midpoint, heading theta + turn"""
    fwd, left = np.array([np.cos(theta), np.sin(theta)]), np.array([-np.sin(theta), np.cos(theta)])
    front = mid - gap * fwd + lateral * left
    h = theta + turn
    return front - hla * np.array([np.cos(h), np.sin(h)]), h


@functools.lru_cache(maxsize=None)
def make_case(name, with_base=False):
    k = CASES[name]
    rng = np.random.default_rng(k['seed'])
    S, A, T, c, K = S_CASE, A_CASE, T_CASE, C_CASE, k['token_size']
    S0 = S // COPIES
    pos = (ORIGIN + rng.uniform(-30.0, 30.0, (S, T, A, 2))).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, (S, T, A)).astype(np.float32)
    atype = np.where(rng.random((S, A)) < 0.7, 0, 2).astype(np.int32)
    shape = np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1).astype(np.float32)
    state = np.ones((S, T, A), np.int32)
    lines = np.zeros((S0, K_LINES, 4), np.float32)
    lines[0] = rng.uniform(-30.0, 30.0, (K_LINES, 4)) + np.tile(ORIGIN, 2)      # beyond n_lines = 0: never read as lines
    # map scene 1: one line
    mid1, th1, half1 = ORIGIN + rng.uniform(-10.0, 10.0, 2), rng.uniform(-np.pi, np.pi), 3.0
    lines[1, 0] = _line(mid1, th1, half1)
    lines[1, 1:] = lines[1, 0]                                                   # beyond n_lines = 1: dead whatever they hold

    def put(s, i, mid, th, gap, lat, turn=0.0):
        p, h = _stand(mid, th, gap + SETBACK, lat, 0.5 * float(shape[s, i, 0]), turn)
        pos[s, c, i], head[s, c, i] = p.astype(np.float32), np.float32(h)

    put(2, 0, mid1, th1, 2.5, 0.4, 0.1)                                          # in front
    put(2, 1, mid1, th1, -1.0, -0.3)                                             # astride: the bumper is a metre across
    put(2, 2, mid1, th1, -9.0, 0.2)                                              # past
    put(2, 3, mid1, th1 + np.pi, -4.0, 0.5)                                      # oncoming: faces against the line, beyond it
    put(2, 4, mid1, th1, 2.0, -(half1 + 1.6), 0.15)                              # off the right end, steering towards it
    put(3, 0, mid1, th1, 2.0, 0.0)
    atype[3, 0] = 1                                                              # a pedestrian
    put(3, 1, mid1, th1, 2.0, 1.0)
    state[3, c, 1] = INVALID
    put(3, 2, mid1, th1, 1.0, 0.0)                                               # the fallback row of the base variant
    put(3, 3, mid1, th1, 1.5, -1.0)                                              # >= first_new
    put(3, 4, mid1, th1, 1.5, 1.0)
    atype[2, :] = np.where(atype[2, :] == 1, 0, atype[2, :])
    atype[3, 1:] = 0
    # map scene 2: 64 lines
    mids = ORIGIN + rng.uniform(-30.0, 30.0, (K_LINES, 2))
    ths = rng.uniform(-np.pi, np.pi, K_LINES)
    for j in range(K_LINES):
        lines[2, j] = _line(mids[j], ths[j], rng.uniform(2.0, 6.0))
    lines[2, 7, 2:] = lines[2, 7, :2]                                            # L == 0
    lines[2, 21, 2] = np.nan
    lines[2, 40, 0] = np.inf
    front = [3, 12, 30, 45, 63]
    for s in (4, 5):
        for i in range(A):
            put(s, i, mids[front[i]], ths[front[i]], rng.uniform(0.3, 5.0), rng.uniform(-1.5, 1.5), rng.uniform(-0.3, 0.3))
    put(5, 1, mids[7], ths[7], 1.0, 0.0)                                         # in front of the zero-length line
    put(5, 2, mids[21], ths[21], 1.0, 0.0)                                       # and of the NaN line
    atype[4:] = np.where(atype[4:] == 1, 0, atype[4:])
    phase = np.zeros((S0, N_PHASE, K_LINES), np.uint8)
    phase[0] = 1                                                                 # closed, but map scene 0 has no live line
    phase[1, :2] = 1
    phase[2] = rng.choice(np.array([0, 0, 0, 1, 2, 255], np.uint8), (N_PHASE, K_LINES))
    phase[2, 0, front] = [1, 2, 255, 1, 0]
    phase[2, 1, front] = [0, 1, 1, 0, 1]
    phase[2, 2, front] = [1, 1, 1, 1, 1]
    phase[2, :, [7, 21, 40]] = 1
    v = _vocab(K)
    out = dict(k, name=name, S=S, A=A, T=T, c=c, copies=COPIES, K=K_LINES, pos=pos, head=head, state=state,
               n_agents=np.full(S, A, np.int32), atype=atype, shape=shape, lines=lines, n_lines=N_LINES.copy(), phase=phase,
               first_new=FIRST_NEW.copy(), vocab=np.stack([v[t] for t in ('veh', 'ped', 'cyc')]).astype(np.float32), base_rows=None)
    if with_base:      # static sets; set 3 holds only tokens that carry the front point more than 2.5 m straight ahead
        sets = rng.random((4, K)) < 0.5
        sets[:, 0] = True
        pose, _ = end_poses(out['vocab'], np.float64)
        sets[3] = (pose[0, :, 0] > 2.5) & (np.abs(pose[0, :, 1]) < 0.5)
        assert sets[3].any()
        mask_row = rng.choice(np.array([-1, -1, 0, 1, 2], np.int32), S * A).astype(np.int32)
        mask_row[FALLBACK_ROW] = 3
        sel = np.where(mask_row >= 0, mask_row, atype.reshape(-1))
        out.update(sets=sets, mask_row=mask_row, mask_type=[0, 1, 2], base_rows=sets[sel])
    return out


@functools.lru_cache(maxsize=None)
def case_reference(name, with_base, t, f64, first_new=False):
    case = make_case(name, with_base)
    return reference(case, t, np.float64 if f64 else np.float32, case['first_new'] if first_new else None)
