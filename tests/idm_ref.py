"""numpy restatement of the IDM commands ("IDM commands" of include/infgen_hip.h), row by row, with a dtype argument -
float32 with the kernel's operation order, float64 to decide which rows lie too close to a decision to pin - and the operator-level
cases the CPU and GPU tests share.  numpy only; the route records, the frame and the projection are route_ref's."""
from __future__ import annotations

import functools

import numpy as np

import route_ref as rr

INVALID, BAND = rr.INVALID, rr.BAND
DEFAULTS = dict(dt=0.5, v0=(15.0, 1.5, 6.0), headway=1.5, s_min=2.0, a_max=1.5, b_comf=2.0, b_max=6.0, lateral=0.5, keep=0.5,
                types=(1, 0, 1), stop_at_end=1)
STATE = ('s0', 'e0', 'v', 'gap', 'acc', 'v1', 's1')
EPS32 = 2.0 ** -23
ILL_GAP = 1.0        # metres: with a lead this close and acc not at its clamp, q = sstar / g turns an ulp of the gap into far more of acc


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


# ---------------------------------------------------------------------------------------- the definition
def law(v, vl, gap, v0, has_lead, par, dt=np.float64):
    """the car-following law on scalars of dtype dt -> (acc, v1, advance = 0.5 (v + v1) dt, q, r)"""
    f = lambda k: dt(par[k])
    v, vl, gap, v0 = dt(v), dt(vl), dt(gap), dt(v0)
    g = np.maximum(gap, dt(0.1))
    sstar = f('s_min') + np.maximum(dt(0.0), v * f('headway') + v * (v - vl) / (dt(2.0) * np.sqrt(f('a_max') * f('b_comf'))))
    r = v / v0
    free = dt(1.0) - (r * r) * (r * r)
    q = sstar / g if has_lead else dt(0.0)
    acc = np.minimum(np.maximum(f('a_max') * (free - q * q), -f('b_max')), f('a_max'))
    v1 = np.maximum(dt(0.0), v + acc * f('dt'))
    return acc, v1, dt(0.5) * (v + v1) * f('dt'), q, r


def reference(case, par, dt=np.float32):
    """the definition in dtype dt -> dict: state [rows][8], lead [rows], pose [rows][3] (NaN where cmd_pose is not written), ruled [rows],
    and the magnitudes that enter, [rows] each: scale (|dx| + |dy| of the chosen segment's p0 and of the lead from the row, + total, metres),
    world (|x| + |y| of the row), mv (|dx| + |dy| of the two speed differences / dt).  dt float64 adds, [rows] each: near - some
    decision of the row (a tie of two segments' d2, a candidate's d_j or s_j at its threshold, two gaps that tie, s1 at the joint of two
    segments) lies inside BAND; ambiguous - the part of near that changes float outputs even where the lead agrees: the segment of the
    row's own projection, of its lead's projection or of its target is open; ill - a lead nearer than ILL_GAP with acc off its clamp"""
    f64 = dt == np.float64
    pos, head, state, n_agents, atype, shape, ctl = (case[k] for k in ('pos', 'head', 'state', 'n_agents', 'atype', 'shape', 'ctl'))
    S, T, A = state.shape
    c, copies, v_des = case['c'], case['copies'], par.get('v_des')
    rec, total = rr.records(case['routes'], case['n_points'], dt)
    rows = S * A
    out_state, lead_out, pose = np.zeros((rows, 8), dt), np.full(rows, -1, np.int64), np.full((rows, 3), np.nan, dt)
    ruled, near, amb, ill = np.zeros(rows, bool), np.zeros(rows, bool), np.zeros(rows, bool), np.zeros(rows, bool)
    scale, world, mv = np.zeros(rows), np.zeros(rows), np.zeros(rows)
    step, lateral, keep, half = dt(par['dt']), dt(par['lateral']), dt(par['keep']), dt(0.5)
    for s in range(S):
        n = min(int(n_agents[s]), A)
        for i in range(A):
            row = s * A + i
            ty = int(atype[s, i]) if 0 <= int(atype[s, i]) <= 2 else 0
            tot = total[s // copies, i]
            if not (ctl[s, i] != 0 and i < n and state[s, c, i] != INVALID and par['types'][ty] and tot > 0):
                continue
            ruled[row] = True
            px, py = dt(pos[s, c, i, 0]), dt(pos[s, c, i, 1])
            h = dt(head[s, c, i])
            ci, si = np.cos(h), np.sin(h)
            v = dt(0.0)
            if state[s, c - 1, i] != INVALID:
                dx, dy = px - dt(pos[s, c - 1, i, 0]), py - dt(pos[s, c - 1, i, 1])
                v = np.sqrt(dx * dx + dy * dy) / step
                mv[row] = (abs(dx) + abs(dy)) / float(step)
            segs, dist = rr._frame(rec[s // copies, i], pos[s, c, i, 0], pos[s, c, i, 1], head[s, c, i], dt)
            wdir = rec[s // copies, i][rec[s // copies, i][:, 4] > 0][:, 2:4].astype(dt)
            s0a, b0, i0, S0a, D0a = rr._project(np.zeros(1), np.zeros(1), segs, dt)
            s0, g0 = s0a[0], segs[i0[0]]
            rx, ry = dt(0.0) - g0[0], dt(0.0) - g0[1]
            t = np.fmin(np.fmax(rx * g0[2] + ry * g0[3], dt(0.0)), g0[4])
            fx, fy = rx - t * g0[2], ry - t * g0[3]
            e0 = fx * (-g0[3]) + fy * g0[2]
            scale[row] = dist[i0[0]] + float(tot)
            world[row] = abs(float(px)) + abs(float(py))
            if f64 and (D0a[:, 0] <= b0[0] + BAND).sum() > 1:
                near[row] = amb[row] = True
            # the lead search
            li, wi = dt(shape[s, i, 0]), dt(shape[s, i, 1])
            js = np.array([j for j in range(n) if j != i and state[s, c, j] != INVALID], np.int64)
            lead, gap, vl = -1, dt(np.inf), dt(0.0)
            entries = []                                   # (lowest gap, highest gap, sure, ambiguous segment) of whatever may lead
            if len(js):
                jx, jy = pos[s, c, js, 0].astype(dt), pos[s, c, js, 1].astype(dt)
                dxw, dyw = jx - px, jy - py
                sj, bj, gj, Sa, Da = rr._project(dxw * ci + dyw * si, dyw * ci - dxw * si, segs, dt)
                thr = lateral + half * (wi + shape[s, js, 1].astype(dt))
                cand = (np.sqrt(bj) <= thr) & (sj > s0)
                hl = half * (li + shape[s, js, 0].astype(dt))
                gaps = (sj - s0) - hl
                if cand.any():
                    k = int(np.argmin(np.where(cand, gaps, np.inf)))           # (the first of equal gaps: the lowest j)
                    lead, gap = int(js[k]), gaps[k]
                    if f64 and (Da[:, k] <= bj[k] + BAND).sum() > 1:
                        amb[row] = True                    # the lead's own segment is open: vl may differ
                    if state[s, c - 1, lead] != INVALID:
                        vx, vy = jx[k] - dt(pos[s, c - 1, lead, 0]), jy[k] - dt(pos[s, c - 1, lead, 1])
                        u = segs[gj[k]]
                        vl = np.maximum(dt(0.0), ((vx * ci + vy * si) * u[2] + (vy * ci - vx * si) * u[3]) / step)
                        mv[row] = max(mv[row], (abs(vx) + abs(vy)) / float(step))
                    scale[row] += abs(float(dxw[k])) + abs(float(dyw[k]))
                if f64:
                    slo, shi, dlo, dhi = rr._interval(Sa, Da, bj)
                    maybe = (dlo <= thr + BAND) & (shi + BAND > s0)
                    sure = (dhi <= thr - BAND) & (slo - BAND > s0)
                    tied = (Da <= bj[None] + BAND).sum(0) > 1
                    entries = [((slo[k] - s0) - hl[k], (shi[k] - s0) - hl[k], bool(sure[k]), bool(tied[k])) for k in np.flatnonzero(maybe)]
            if par['stop_at_end']:
                end_gap = (tot - s0) - half * li
                if end_gap < gap:
                    lead, gap, vl = -2, end_gap, dt(0.0)
                entries.append((end_gap, end_gap, True, False))
            if f64 and entries:
                best_hi = min([hi for lo, hi, ok, _ in entries if ok], default=np.inf)
                rivals = [e for e in entries if e[0] <= best_hi + BAND]
                if len(rivals) != 1 or not rivals[0][2] or rivals[0][3]:
                    near[row] = True
            # the law
            v0 = dt(par['v0'][ty])
            if v_des is not None and v_des[s // copies, i] > 0:
                v0 = dt(v_des[s // copies, i])
            acc, v1, adv, q, r = law(v, vl, gap, v0, lead != -1, par, dt)
            s1 = np.minimum(s0 + adv, tot)
            # the target
            at = len(segs) - 1
            for e, seg in enumerate(segs):
                if s1 <= seg[5] + seg[4]:
                    at = e
                    break
            if f64 and any(abs(float(s1) - float(seg[5] + seg[4])) <= BAND for seg in segs[:-1]):
                near[row] = amb[row] = True                # the target's segment is open: heading and normal may differ
            if f64 and lead != -1 and float(gap) < ILL_GAP and float(acc) > -par['b_max']:
                ill[row] = True
            seg = segs[at]
            a1 = np.minimum(np.maximum(s1 - seg[5], dt(0.0)), seg[4])
            ke = keep * e0
            tx = (seg[0] + a1 * seg[2]) + ke * (-seg[3])
            tz = (seg[1] + a1 * seg[3]) + ke * seg[2]
            pose[row] = [px + (tx * ci - tz * si), py + (tx * si + tz * ci), np.arctan2(wdir[at][1], wdir[at][0])]
            out_state[row] = [s0, e0, v, gap, acc, v1, s1, 1]
            lead_out[row] = lead
    out = dict(state=out_state, lead=lead_out, pose=pose, ruled=ruled, scale=scale, world=world, mv=mv)
    if f64:
        out.update(near=near, ambiguous=amb, ill=ill)
    return out


def floors(r64, par):
    """per output the magnitude that enters, [rows] each (the operator bar's floor is 8 * 2^-23 times it, row by row): for the arc
    lengths, offsets and gaps the metres |dx| + |dy| + total; for v the speed differences / dt; for acc the width of its clamp,
    a_max + b_max; for v1 and s1 what one step adds to those; for x and y the world coordinate itself plus the metres; pi for the
    heading.  No factor for how the law amplifies an error of the gap: rows where it does so without bound are ``ill``"""
    step = float(par['dt'])
    m, mv = r64['scale'], np.maximum(r64['mv'], 1e-3)
    ma = np.full_like(m, par['a_max'] + par['b_max'])
    mv1 = mv + ma * step
    ms1 = m + mv1 * step
    return dict(s0=m, e0=m, v=mv, gap=m, acc=ma, v1=mv1, s1=ms1, x=r64['world'] + ms1, y=r64['world'] + ms1,
                heading=np.full_like(m, np.pi))


def outputs(res):
    """name -> [rows] of the ten float outputs of a result of ``reference`` (or of the device's arrays in the same layout)"""
    out = {k: res['state'][:, n] for n, k in enumerate(STATE)}
    out.update(x=res['pose'][:, 0], y=res['pose'][:, 1], heading=res['pose'][:, 2])
    return out


# ---------------------------------------------------------------------------------------- the operator-level cases
# a scene is built of roles, one per row; a role's place is given on the route of the follower it belongs to:
#   F  a follower: controlled, a vehicle, moving along its own route            L  its leader: in lane 8 .. 15 m ahead, standing
#   O  4 .. 7 m ahead of it, just outside the lateral bound (controlled)        B  5 m behind it, in lane (controlled, a cyclist)
#   X  3 m ahead of it, in lane, but not live at c (controlled)                 N  its leader, not live at c - 1 (controlled, no route)
#   Q  its leader, faster than the follower (not controlled)                    P  a controlled pedestrian behind it
#   R  a controlled row with its own route, somewhere else                      1  like R, with a one-point route
# rows beyond n_agents are padding
CASES = {
    'a5_p2': dict(S=2, A=5, P=2, copies=1, seed=11, roles=['FLOBX', 'FNPR.']),
    'a70_p32': dict(S=2, A=70, P=32, copies=1, seed=12, roles=None),
    'a32_p3_c2': dict(S=4, A=32, P=3, copies=2, seed=13, roles=None),
}
CYCLE = 'FLOBXFQPFNR1'
T_CASE, C_CASE = 4, 2
# stop_at_end, with v_des, types
VARIANTS = {'stop': (1, False, (1, 0, 1)), 'free': (0, False, (1, 0, 1)), 'stop_vdes': (1, True, (1, 0, 1)),
            'free_vdes': (0, True, (1, 0, 1)), 'stop_nocyc': (1, False, (1, 1, 0))}


def _arc(pts, s, lateral):
    L = np.linalg.norm(np.diff(pts, axis=0), axis=1).sum()
    return rr._at(pts, min(max(s / L, 0.0), 1.0), lateral)


@functools.lru_cache(maxsize=None)
def make_case(name):
    k = CASES[name]
    rng = np.random.default_rng(k['seed'])
    S, A, P, copies, T, c = k['S'], k['A'], k['P'], k['copies'], T_CASE, C_CASE
    S0, step = S // copies, DEFAULTS['dt']
    roles = [(k['roles'][s0] if k['roles'] else (CYCLE * A)[:A - 3] + '...') for s0 in range(S0)]
    routes, n_points = np.zeros((S0, A, P, 2), np.float32), np.zeros((S0, A), np.int32)
    for s0 in range(S0):
        for i in range(A):
            n = P if i < 5 else int(rng.integers(2, P + 1))
            pts = rr._walk(rng, n, rr.ORIGIN + rng.uniform(-400.0, 400.0, 2), rng.uniform(-np.pi, np.pi))
            if P >= 8 and i % 12 == 0 and n >= 8:
                pts[n // 2] = pts[n // 2 - 1]             # a repeated point: a zero-length (dead) segment in the middle
                pts[3] = pts[2]
            role = roles[s0][i]
            n = 0 if role in 'N.' else 1 if role == '1' else n
            routes[s0, i, :n], n_points[s0, i] = pts[:n].astype(np.float32), n
    pos = (rr.ORIGIN + rng.uniform(-400.0, 400.0, (S, T, A, 2))).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, (S, T, A)).astype(np.float32)
    state = np.ones((S, T, A), np.int32)
    atype = np.zeros((S, A), np.int32)
    ctl = np.ones((S, A), np.uint8)
    shape = np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1).astype(np.float32)
    n_agents = np.full(S, A, np.int32)

    def put(s, j, pts, at, lateral, speed):
        """row j at arc length `at` of the polyline, `lateral` to its left, having come along it at `speed`"""
        for col, back in ((c, 0.0), (c - 1, speed * step), (c - 2, 2 * speed * step)):
            p, h = _arc(pts, at - back, lateral)
            pos[s, col, j], head[s, col, j] = p.astype(np.float32), np.float32(h + rng.uniform(-0.2, 0.2))

    for s in range(S):
        s0, f, fi, vf, sf = s // copies, None, 0, 0.0, 0.0
        n_agents[s] = A - roles[s0].count('.')
        for i, role in enumerate(roles[s0]):
            own = routes[s0, i, :n_points[s0, i]].astype(np.float64)
            if role == 'F':
                f, fi, vf = own, i, rng.uniform(4.0, 8.0)
                sf = rng.uniform(0.1, 0.3) * np.linalg.norm(np.diff(f, axis=0), axis=1).sum()
                put(s, i, f, sf, rng.uniform(-0.3, 0.3), vf)
                continue
            wide = DEFAULTS['lateral'] + 0.5 * (float(shape[s, i, 1]) + float(shape[s, fi, 1]))      # the follower's lateral bound for this row
            if role in 'LNQ':
                put(s, i, f, sf + rng.uniform(8.0, 15.0), rng.uniform(-1.0, 1.0), 1.5 * vf if role == 'Q' else 0.0)
                ctl[s, i] = role == 'N'
                if role == 'N':
                    state[s, :c, i] = INVALID
            elif role == 'O':
                put(s, i, f, sf + rng.uniform(4.0, 7.0), wide + rng.uniform(0.05, 0.3), 0.5 * vf)
            elif role == 'B':
                put(s, i, f, sf - 5.0, rng.uniform(-0.5, 0.5), vf)
                atype[s, i] = 2
            elif role == 'X':
                put(s, i, f, sf + 3.0, 0.0, 0.0)
                state[s, c, i] = INVALID
            elif role == 'P':
                put(s, i, f, max(sf - 9.0, 0.0), 0.3, 1.0)
                atype[s, i] = 1
            elif role == 'R':
                put(s, i, own, rng.uniform(0.2, 0.6) * np.linalg.norm(np.diff(own, axis=0), axis=1).sum(), rng.uniform(-1.0, 1.0),
                    rng.uniform(0.0, 10.0))
                atype[s, i] = 2 if rng.random() < 0.3 else 0
    v_des = np.where(rng.random((S0, A)) < 0.6, rng.uniform(3.0, 12.0, (S0, A)), rng.choice([0.0, -1.0], (S0, A))).astype(np.float32)
    return dict(k, name=name, T=T, c=c, pos=pos, head=head, state=state, n_agents=n_agents, atype=atype, shape=shape, ctl=ctl,
                routes=routes, n_points=n_points, v_des=v_des, role=[(r * copies) for r in roles])


def variant_params(case, variant):
    stop, with_vdes, types = VARIANTS[variant]
    return params(stop_at_end=stop, types=types, v_des=case['v_des'] if with_vdes else None)


@functools.lru_cache(maxsize=None)
def case_reference(name, variant, f64):
    case = make_case(name)
    return reference(case, variant_params(case, variant), np.float64 if f64 else np.float32)


# ---------------------------------------------------------------------------------------- the platoon scenario
PLATOON = dict(length=150.0, standing=140.0, start=(60.0, 40.0, 20.0), speed=8.0, steps=40)


def platoon_case():
    """one scene on a straight 150 m route: row 0 stands, uncontrolled, near the end; rows 1 .. 3 come up behind it at one speed"""
    k, step = PLATOON, DEFAULTS['dt']
    th = 0.3
    u = np.array([np.cos(th), np.sin(th)])
    A, T, c = 4, 3, 1
    line = np.stack([rr.ORIGIN, rr.ORIGIN + k['length'] * u])
    routes = np.tile(line.astype(np.float32), (1, A, 1, 1))
    at = np.array((k['standing'],) + k['start'])
    pos = np.zeros((1, T, A, 2), np.float32)
    pos[0, c] = (rr.ORIGIN + at[:, None] * u).astype(np.float32)
    pos[0, c - 1] = (rr.ORIGIN + (at - np.array([0.0, 1.0, 1.0, 1.0]) * k['speed'] * step)[:, None] * u).astype(np.float32)
    return dict(S=1, A=A, P=2, copies=1, T=T, c=c, pos=pos, head=np.full((1, T, A), th, np.float32), state=np.ones((1, T, A), np.int32),
                n_agents=np.array([A], np.int32), atype=np.zeros((1, A), np.int32), ctl=np.array([[0, 1, 1, 1]], np.uint8),
                shape=np.tile(np.array([4.5, 1.9, 1.5], np.float32), (1, A, 1)), routes=routes, n_points=np.full((1, A), 2, np.int32))


def platoon_feed(case, pose, ruled):
    """the next step's inputs: column c becomes c - 1, the targets of the ruled rows become column c (fill: stand still)"""
    c = case['c']
    nxt = dict(case, pos=case['pos'].copy(), head=case['head'].copy())
    nxt['pos'][:, c - 1], nxt['head'][:, c - 1] = case['pos'][:, c], case['head'][:, c]
    tgt = pose.reshape(case['S'], case['A'], 3).astype(np.float32)
    m = ruled.reshape(case['S'], case['A'])
    nxt['pos'][:, c][m], nxt['head'][:, c][m] = tgt[m][:, :2], tgt[m][:, 2]
    return nxt
