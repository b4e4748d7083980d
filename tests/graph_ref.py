"""Plain references of the integer-and-geometry kernels (edge builders, insertion decisions, top-k sampling) and the input
generators their tests share.  numpy only, float64, loops over scenes and destinations; written from the header comments of
infgen_amd/csrc/edge_kernels.hip and the reference lines they cite (agent_decoder.py:540-904, 1852-2074, 2162-2195;
map_decoder.py:91-93; attr_tokenizer.py:91-110) - nothing is shared with oracle/ or infgen_amd/.  The step-advance kernels
(k_integrate, the raw-feature gather: agent_decoder.py:2168-2285, :426-447) and the two geometry kernels of the teacher-forced
forward, k_radius_edges and k_motion_features of infgen_amd/csrc/forward_kernels.hip, follow: the latter from the text of
include/infgen_hip.h ("edge sets of the teacher-forced forward") and the lines it cites (agent_decoder.py:595-601, :632, :710,
:722-723, :780, :875, :426-447, :1327; map_decoder.py:91).  compare_lists is what every GPU test of an edge builder asserts of a
device CSR against these lists; test_graph_ref_cpu.py runs the deliberately wrong variants of the references (mutate=...) through
the same comparison, so that the generated inputs are known to tell those errors apart.

A scene block (`new_state`) is a dict of numpy arrays in the device layout of InfgenRollout (include/infgen_hip.h): the per-column
arrays are [S][T][A_cap], the map side [Sm][M_cap]."""
import math

import numpy as np

INVALID, VALID, ENTER, EXIT = 0, 1, 2, 3
MOTION_GAP = HEADING_GAP = 1.0
INVALID_MOTION = INVALID_HEAD = -2.0
NUM_SEED_FEATURE = 10            # the last 10 rows of a scene are never temporal destinations
A2A_CANDIDATES = 300 + 1         # radius_graph(max_num_neighbors=300): 301 candidates, self among them
MAP_NBR = 5
RULED_DIST, RULED_DTH = 1, 2        # edge_raw: which features of an edge are a gap rule's constants

# Which edges exist is compared exactly, so no candidate may sit closer to a radius than this (relative, in d^2): fp32 rounding
# of the device's dx*dx + dy*dy and r*r is ~1e-6 at a few hundred metres
MARGIN = 1e-4
# the same for the inverse-CDF draws: |u * sum(p) - cdf_j| / sum(p) over the boundaries that change the pick
CDF_MARGIN = 1e-5

# Largest error of a plain fp32 numpy evaluation of the raw edge features against float64 over the inputs of all generators below:
# distance [m], bearing [rad], heading difference [rad], angles modulo 2 pi.  The figures are the ones tests/test_graph_ref_cpu.py
# measures (and asserts not to be exceeded), rounded up in the fourth digit.  The device bar is four times the figure: atan2f /
# sincosf are a few ulp, not correctly rounded, and a subtraction may be fused.
FP32_ERR_DIST, FP32_ERR_BEARING, FP32_ERR_DTH = 3.907e-5, 3.595e-7, 5.922e-7
BAR_DIST, BAR_BEARING, BAR_DTH = 4 * FP32_ERR_DIST, 4 * FP32_ERR_BEARING, 4 * FP32_ERR_DTH
# occupancy embedding: fp32 numpy in the kernel's summation order (ascending cell) against float64 on gen_occupancy's pack
FP32_ERR_OCC_EMB = 1.086e-6
BAR_OCC_EMB = 4 * FP32_ERR_OCC_EMB
# poses written by the insertion kernels, coordinates within +-200 m: 1e-5 m and 1e-6 rad against float64 - unless the fp32 numpy
# evaluation already exceeds that, then four times its error.  It does for the position (half an ulp of 200 m is 7.6e-6 m, and the
# rotation adds to it), it does not for the heading (half an ulp of pi is 1.2e-7 rad).
FP32_ERR_INS_POS, FP32_ERR_INS_HEAD = 1.301e-5, 2.678e-7
BAR_INS_POS = 1e-5 if FP32_ERR_INS_POS <= 1e-5 else 4 * FP32_ERR_INS_POS
BAR_INS_HEAD = 1e-6 if FP32_ERR_INS_HEAD <= 1e-6 else 4 * FP32_ERR_INS_HEAD


def wrap(a, f=np.float64):
    """wrap_angle(a) = -pi + (a + pi) % (2 pi), python-style remainder"""
    a = np.asarray(a, dtype=f)
    return f(-math.pi) + np.mod(a + f(math.pi), f(2 * math.pi))


def ang_err(a, b):
    """|a - b| modulo 2 pi"""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % (2 * math.pi)
    return np.minimum(d, 2 * math.pi - d)


def first_k_within(centre_xy, cand_xy, r, k):
    """torch_cluster.radius for one centre: the first k candidates in ascending index with d^2 < r^2 (strict), and the smallest
    relative gap |d^2 - r^2| / r^2 over ALL candidates (inf without candidates)"""
    cand = np.asarray(cand_xy, np.float64).reshape(-1, 2)
    cx, cy = float(centre_xy[0]), float(centre_xy[1])
    r2 = float(r) * float(r)
    d2 = (cx - cand[:, 0]) ** 2 + (cy - cand[:, 1]) ** 2
    hits = np.nonzero(d2 < r2)[0][:k]
    gap = float(np.min(np.abs(d2 - r2)) / r2) if len(cand) else math.inf
    return hits, gap


def edge_raw(dst_pose, src_pose, dst_inv, src_inv, kind, hv=None, dt=0.0, f=np.float64):
    """(|d|, bearing of d in the destination's heading frame, wrap(theta_src - theta_dst), dt) of the edges src -> dst, one
    destination (x, y, theta) and arrays of sources; d = src - dst.  Gap rules by `kind`:
      'temporal' / 'agent': source INVALID only: d = (-1, -1), dth = -1; destination INVALID only: d = (1, 1) (dth kept);
                            both: d = (-2, -2), dth = -2
      'map': destination INVALID: d = (1, 1), dth = 1       'point': none
    hv: the destination's (cos, sin) when it is overridden.  Also returns per edge which features are a rule's constants, exact in
    fp32: bit RULED_DIST the distance (sqrt 2 or 2 sqrt 2: the correctly rounded root of 2 or 8), bit RULED_DTH the heading difference."""
    xd, yd, td = (f(v) for v in dst_pose)
    xs, ys, ts = (np.atleast_1d(np.asarray(v, dtype=f)) for v in src_pose)
    dx, dy = xs - xd, ys - yd
    dth = wrap(ts - td, f)
    s_inv = np.broadcast_to(np.asarray(src_inv, bool), xs.shape)
    d_inv = bool(dst_inv)
    ruled = np.zeros(xs.shape, np.int8)
    if kind in ('temporal', 'agent'):
        if not d_inv:
            dx, dy, dth = (np.where(s_inv, f(v), x) for v, x in ((-MOTION_GAP, dx), (-MOTION_GAP, dy), (-HEADING_GAP, dth)))
            ruled = np.where(s_inv, RULED_DIST | RULED_DTH, 0).astype(np.int8)
        else:
            dx = np.where(s_inv, f(INVALID_MOTION), f(MOTION_GAP)) + 0 * dx
            dy = dx.copy()
            dth = np.where(s_inv, f(INVALID_HEAD), dth)
            ruled = np.where(s_inv, RULED_DIST | RULED_DTH, RULED_DIST).astype(np.int8)      # (destination only: dth is kept)
    elif kind == 'map':
        if d_inv:
            dx, dy, dth = (np.full(xs.shape, f(v)) for v in (MOTION_GAP, MOTION_GAP, HEADING_GAP))
            ruled = np.full(xs.shape, RULED_DIST | RULED_DTH, np.int8)
    else:
        assert kind == 'point'
    c, s = (np.cos(td), np.sin(td)) if hv is None else (f(hv[0]), f(hv[1]))
    dist = np.sqrt(dx * dx + dy * dy)
    # (the dot product as a sum that starts from +0, like torch's: a source exactly at the destination has bearing +-0, never +-pi)
    bearing = np.arctan2(c * dy - s * dx, (f(0) + c * dx) + s * dy)
    raw = np.stack([dist, bearing, dth, np.full(xs.shape, f(dt))], axis=-1).astype(f)
    return raw, ruled


# ------------------------------------------------------------------------------------------------ scene blocks
def new_state(S, A_cap, T, M_cap, Sm=None, W=12, ring=13, r_map=30.0, r_agent=60.0, G=0, R=5):
    Sm = S if Sm is None else Sm
    z = lambda *sh, dt=np.float32: np.zeros(sh, dt)
    return dict(S=S, A_cap=A_cap, T=T, M_cap=M_cap, Sm=Sm, W=W, ring=ring, R=R, grid_size=G,
                r_map=float(np.float32(r_map)), r_agent=float(np.float32(r_agent)),
                n_agents=z(S, dt=np.int32), n_map=z(Sm, dt=np.int32), av_index=z(S, dt=np.int32),
                pos=z(S, T, A_cap, 2), head=z(S, T, A_cap), state=z(S, T, A_cap, dt=np.int32), token=z(S, T, A_cap, dt=np.int32),
                grid=z(S, T, A_cap, dt=np.int32), tmask=np.ones((S, T, A_cap), np.uint8), imask=np.ones((S, T, A_cap), np.uint8),
                catflag=np.ones((S, T, A_cap), np.uint8), type=z(S, A_cap, dt=np.int32), bos=z(S, A_cap, dt=np.int32),
                map_pos=z(Sm, M_cap, 2), map_orient=z(Sm, M_cap), map_scene=None, first_new=None, hv_ovr=None,
                grid_xy=z(max(G, 1), 2), pred_traj=z(S * A_cap, R, 2), pred_head=z(S * A_cap, R), pred_state=z(S * A_cap, R))


def take_scenes(st, scenes):
    """the block of a subset of scenes (the map side is kept whole, reached through map_scene)"""
    scenes = list(scenes)
    out = dict(st)
    out['S'] = len(scenes)
    for k in ('n_agents', 'av_index', 'pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag', 'type', 'bos',
              'first_new', 'hv_ovr'):
        if st[k] is not None:
            out[k] = np.ascontiguousarray(st[k][scenes])
    ms = st['map_scene'] if st['map_scene'] is not None else np.arange(st['S'], dtype=np.int32)
    out['map_scene'] = np.ascontiguousarray(ms[scenes]).astype(np.int32)
    return out


def _map_slot(st, s):
    return int(st['map_scene'][s]) if st['map_scene'] is not None else s


def build_edges_ref(st, c, f=np.float64):
    """the three CSR edge sets into column c, per destination row (S * A_cap lists per kind): {'t' | 'm' | 'a': [(src, raw, ruled)]}
    with src in ascending order.  The lists are always chosen in float64; f is the type the features are evaluated in.
      temporal  columns j in [c - W, c) with j >= bos and tmask[j], destinations < A - 10, dt = j - c, src = (j % ring) * rows + row
      map       the first 5 tokens (ascending) within r_map; destination needs imask; src = slot * M_cap + m
      agent     the first 301 rows (ascending, all rows < A, self among them) within r_agent, then self and imask == 0 sources
                dropped; destination needs imask; src = s * A_cap + j
    rows >= first_new[s] carry the head vector hv_ovr[s]."""
    S, A_cap, W, ring, M_cap = st['S'], st['A_cap'], st['W'], st['ring'], st['M_cap']
    rows = S * A_cap
    empty = (np.zeros(0, np.int64), np.zeros((0, 4), f), np.zeros(0, np.int8))
    out = {k: [empty] * rows for k in 'tma'}
    for s in range(S):
        A = int(st['n_agents'][s])
        ms = _map_slot(st, s)
        M = int(st['n_map'][ms])
        P, Hd, St = st['pos'][s], st['head'][s], st['state'][s]
        mp, mo = st['map_pos'][ms, :M], st['map_orient'][ms, :M]
        for a in range(A):
            row = s * A_cap + a
            hv = None
            if st['first_new'] is not None and a >= st['first_new'][s]:
                hv = st['hv_ovr'][s]
            dpose = (P[c, a, 0], P[c, a, 1], Hd[c, a])
            d_inv = St[c, a] == INVALID
            if a < A - NUM_SEED_FEATURE:
                js = np.asarray([j for j in range(max(c - W, 0), c) if j >= st['bos'][s, a] and st['tmask'][s, j, a]], np.int64)
                if len(js):
                    raw, ruled = edge_raw(dpose, (P[js, a, 0], P[js, a, 1], Hd[js, a]), d_inv, St[js, a] == INVALID, 'temporal',
                                          hv=hv, f=f)
                    raw[:, 3] = (js - c).astype(f)
                    out['t'][row] = ((js % ring) * rows + row, raw, ruled)
            if not st['imask'][s, c, a]:
                continue
            m, _ = first_k_within(dpose[:2], mp, st['r_map'], MAP_NBR)
            if len(m):
                raw, ruled = edge_raw(dpose, (mp[m, 0], mp[m, 1], mo[m]), d_inv, False, 'map', hv=hv, f=f)
                out['m'][row] = (ms * M_cap + m, raw, ruled)
            j, _ = first_k_within(dpose[:2], P[c, :A], st['r_agent'], A2A_CANDIDATES)
            j = j[(j != a) & (st['imask'][s, c, j] != 0)]
            if len(j):
                raw, ruled = edge_raw(dpose, (P[c, j, 0], P[c, j, 1], Hd[c, j]), d_inv, St[c, j] == INVALID, 'agent', hv=hv, f=f)
                out['a'][row] = (s * A_cap + j, raw, ruled)
    return out


def build_edges_margin(st, c):
    """smallest relative gap of any (destination, candidate) pair of the map and agent searches of column c"""
    g = math.inf
    for s in range(st['S']):
        A = int(st['n_agents'][s])
        ms = _map_slot(st, s)
        M = int(st['n_map'][ms])
        for a in range(A):
            g = min(g, first_k_within(st['pos'][s, c, a], st['map_pos'][ms, :M], st['r_map'], 1)[1],
                    first_k_within(st['pos'][s, c, a], st['pos'][s, c, :A], st['r_agent'], 1)[1])
    return g


def point_edges_ref(st, c, centre_row, active, exclude_centre, r_agent, k_agent, r_map, k_map, f=np.float64):
    """one query point per scene (the pose of row centre_row[s] at column c): the first K agents / map tokens within a radius in
    ascending index; among the agents the imask == 0 ones and (exclude_centre) the centre itself are dropped AFTER the cap.
    -> {'a' | 'm': [(src, raw)] per scene}; inactive scenes have no edges"""
    out = {'a': [], 'm': []}
    for s in range(st['S']):
        A, ms = int(st['n_agents'][s]), _map_slot(st, s)
        M = int(st['n_map'][ms])
        cr = int(centre_row[s])
        P, Hd = st['pos'][s, c], st['head'][s, c]
        pose = (P[cr, 0], P[cr, 1], Hd[cr])
        on = active is None or active[s] != 0
        j = first_k_within(pose[:2], P[:A], r_agent, k_agent)[0] if on else np.zeros(0, np.int64)
        j = j[st['imask'][s, c, j] != 0]
        if exclude_centre:
            j = j[j != cr]
        out['a'].append((s * st['A_cap'] + j, edge_raw(pose, (P[j, 0], P[j, 1], Hd[j]), False, False, 'point', f=f)[0]))
        m = first_k_within(pose[:2], st['map_pos'][ms, :M], r_map, k_map)[0] if on else np.zeros(0, np.int64)
        out['m'].append((ms * st['M_cap'] + m,
                         edge_raw(pose, (st['map_pos'][ms, m, 0], st['map_pos'][ms, m, 1], st['map_orient'][ms, m]), False, False,
                                  'point', f=f)[0]))
    return out


def map_graph_ref(n_map, pos, orient, radius, max_nbr, f=np.float64):
    """radius_graph(loop=False, max_num_neighbors=max_nbr) per scene: per centre the first max_nbr + 1 tokens in ascending index
    within the radius (self among them), self dropped.  -> ([(src, raw)] per row of [S][M_cap], smallest relative gap)"""
    S, M_cap = pos.shape[:2]
    out, gap = [], math.inf
    for s in range(S):
        M = int(n_map[s])
        for i in range(M_cap):
            if i >= M:
                out.append((np.zeros(0, np.int64), np.zeros((0, 4), f)))
                continue
            m, g = first_k_within(pos[s, i], pos[s, :M], radius, max_nbr + 1)
            cand = np.delete(pos[s, :M].astype(np.float64), i, axis=0)          # (the centre itself sits at distance 0)
            gap = min(gap, first_k_within(pos[s, i], cand, radius, 1)[1])
            m = m[m != i]
            raw = edge_raw((pos[s, i, 0], pos[s, i, 1], orient[s, i]), (pos[s, m, 0], pos[s, m, 1], orient[s, m]), False, False,
                           'point', f=f)[0]
            out.append((s * M_cap + m, raw))
    return out, gap


def raw_errors(ref_lists, other_lists):
    """largest per-feature difference of two evaluations of the same edge lists: (distance, bearing, heading difference)"""
    e = np.zeros(3)
    for a, b in zip(ref_lists, other_lists):
        ra, rb = np.asarray(a[1], np.float64), np.asarray(b[1], np.float64)
        if len(ra):
            e = np.maximum(e, [np.abs(ra[:, 0] - rb[:, 0]).max(), ang_err(ra[:, 1], rb[:, 1]).max(), ang_err(ra[:, 2], rb[:, 2]).max()])
    return e


def compare_lists(kind, off, cnt, src, raw, ref, cap=None, written=None):
    """what the GPU tests of the edge builders assert of a device CSR (off / cnt per destination row, src / raw [cap][4] in fp32)
    against reference lists: per row the count, the source list in order, raw features within the bars, raw[:, 3] and the rule
    constants exact.  With cap: rows whose range passes it are compared for their count only (written = False) or must report
    cnt = 0 (written = None: the compacting kernels).  -> the largest device errors (distance, bearing, heading difference)"""
    err = np.zeros(3)
    for row, r in enumerate(ref):
        want_src, want_raw = r[0], np.asarray(r[1], np.float64)
        n = len(want_src)
        over = cap is not None and off[row] + n > cap
        if over and written is None:
            assert cnt[row] == 0, (kind, row)
            continue
        assert cnt[row] == n, (kind, row, cnt[row], n)
        if n == 0 or over:
            continue
        o = off[row]
        assert 0 <= o and (cap is None or o + n <= cap)
        assert np.array_equal(src[o:o + n], want_src), (kind, row, src[o:o + n], want_src)
        got = raw[o:o + n].astype(np.float64)
        e = [np.abs(got[:, 0] - want_raw[:, 0]).max(), ang_err(got[:, 1], want_raw[:, 1]).max(), ang_err(got[:, 2], want_raw[:, 2]).max()]
        assert e[0] <= BAR_DIST and e[1] <= BAR_BEARING and e[2] <= BAR_DTH, (kind, row, e)
        assert np.array_equal(got[:, 3], want_raw[:, 3]), (kind, row)
        if len(r) > 2 and r[2].any():                  # gap rules: -1 / 1 / -2, and the distance float32(sqrt 2) / float32(2 sqrt 2)
            dth_c, dist_c = (r[2] & RULED_DTH) != 0, (r[2] & RULED_DIST) != 0
            assert np.array_equal(got[dth_c, 2], want_raw[dth_c, 2]), (kind, row, 'a gap-rule constant is not exact')
            assert np.array_equal(raw[o:o + n][dist_c, 0], want_raw[dist_c, 0].astype(np.float32)), (kind, row, 'a gap-rule distance is not exact')
        err = np.maximum(err, e)
    return err


# ------------------------------------------------------------------------------------------------ insertion / sampling
def occupancy_ref(st, c):
    """[S][G] 0 / 1: the cells named by the grid tokens of the scene's first n_agents rows at column c (tokens outside [0, G) none)"""
    G = st['grid_size']
    occ = np.zeros((st['S'], G))
    for s in range(st['S']):
        for a in range(int(st['n_agents'][s])):
            g = int(st['grid'][s, c, a])
            if 0 <= g < G:
                occ[s, g] = 1.0
    return occ


def mlp_layer_ref(x01, w0, b0, ln_g, ln_b, w3, b3, f=np.float64):
    """MLPLayer of a 0 / 1 vector: Linear -> LayerNorm (biased variance, eps 1e-5) -> ReLU -> Linear; torch weight layout [out][in].
    With f = float32 the sums run one term after the other in ascending input index, as the kernel's do."""
    w0, b0, ln_g, ln_b, w3, b3 = (np.asarray(v, f) for v in (w0, b0, ln_g, ln_b, w3, b3))
    h = np.zeros(w0.shape[0], f)
    for g in np.nonzero(np.asarray(x01) != 0)[0]:
        h = h + w0[:, g]
    h = h + b0
    mean = h.sum(dtype=f) / f(h.size)
    d = h - mean
    var = (d * d).sum(dtype=f) / f(h.size)
    hv = np.maximum(d * (f(1.0) / np.sqrt(var + f(1e-5))) * ln_g + ln_b, f(0))
    acc = np.zeros(w3.shape[0], f)
    for k in range(w3.shape[1]):
        acc = acc + hv[k] * w3[:, k]
    return acc + b3


def topk_pick(v, k, u):
    """the k largest of v in (value descending, index ascending) order; p_j = exp(v_j - v_0); the pick is the first j with
    u * sum(p) < cdf_j, else the last.  -> (index, smallest |u sum - cdf_j| / sum over the boundaries j < k - 1, the order)"""
    v = np.asarray(v, np.float64)
    order = np.lexsort((np.arange(v.size), -v))[:k]
    if k == 1:
        return int(order[0]), math.inf, order
    p = np.exp(v[order] - v[order[0]])
    cdf = np.cumsum(p)
    x = float(u) * cdf[-1]
    pick = k - 1
    for j in range(k):
        if x < cdf[j]:
            pick = j
            break
    return int(order[pick]), float(np.min(np.abs(x - cdf[:-1])) / cdf[-1]), order


def sample_topk_ref(logits, k, uniform):
    toks, margins = zip(*[topk_pick(row, k, u)[:2] for row, u in zip(logits, uniform)])
    return np.asarray(toks, np.int32), np.asarray(margins)


def decode_pos(gxy, ego, f=np.float64):
    """grid_xy[cell] @ Rot(theta_ego - pi / 2) + ego position, Rot(phi) = [[cos, sin], [-sin, cos]] (row vector on the left)"""
    gx, gy, ex, ey, eh = f(gxy[0]), f(gxy[1]), f(ego[0]), f(ego[1]), f(ego[2])
    phi = eh - f(math.pi / 2)
    cs, sn = np.cos(phi), np.sin(phi)
    return (gx * cs + gy * (-sn)) + ex, (gx * sn + gy * cs) + ey


def decode_heading(idx, angle_interval, eh, f=np.float64):
    """wrap((idx * interval - 180) / 360 * 2 pi + ego heading)"""
    dec = (f(idx) * f(angle_interval) - f(180.0)) / f(360.0) * f(2 * math.pi)
    return wrap(dec + f(eh), f)


def new_decisions(S, G, n_heading=0):
    z = lambda *sh, dt=np.float32: np.zeros(sh, dt)
    return dict(lg_state=z(S, 2), lg_type=z(S, 3), shape=z(S, 3), lg_pos=z(S, G), occ=z(S, G), uniform=z(S),
                active=np.ones(S, np.int32), n_new=z(S, dt=np.int32), inserted=np.full(S, 77, np.int32),
                new_row=np.full(S, -5, np.int32), new_shape=np.full((S, 3), -9.0, np.float32), new_cell=np.full(S, -7, np.int32),
                lg_heading=z(S, max(n_heading, 1)), offset=z(S, 2))


def insert_decide_ref(st, dec, s, t, force_enter, max_new, sample_k=1, kgrid=True, r_seed=0.0):
    """k_insert_decide for scene s, in place on float64 / integer copies of the block and the decision arrays (as_ref)"""
    c, A_cap, G = 1 + t, st['A_cap'], st['grid_size']
    if not dec['active'][s]:
        dec['inserted'][s] = 0
        return
    cell = -1
    if kgrid and np.all(np.isnan(dec['lg_pos'][s])):      # no cell can be ranked: the scene stops without a row
        dec['inserted'][s], dec['active'][s] = 0, 0
        return
    if kgrid:
        cell = topk_pick(dec['lg_pos'][s], max(sample_k, 1), dec['uniform'][s])[0]
    enter = bool(dec['lg_state'][s, 1] > dec['lg_state'][s, 0]) or bool(force_enter)
    ty = 0
    for k in (1, 2):
        if dec['lg_type'][s, k] > dec['lg_type'][s, ty]:
            ty = k
    occupied = kgrid and dec['occ'][s, cell] != 0
    A = int(st['n_agents'][s])
    if occupied and sample_k > 1:             # the iteration is spent, the next one draws again
        dec['inserted'][s] = 0
        return
    ok = enter and not occupied and dec['n_new'][s] + 1 <= max_new
    if ok and A >= A_cap:                     # no row left: reported, nothing touched
        dec['inserted'][s], dec['active'][s] = -1, 0
        return
    if not ok:
        dec['inserted'][s], dec['active'][s] = 0, 0
        return
    av = int(st['av_index'][s])
    ego = (st['pos'][s, c, av, 0], st['pos'][s, c, av, 1], st['head'][s, c, av])
    if kgrid:
        nx, ny = decode_pos(st['grid_xy'][cell], ego)
    else:
        nx, ny = (math.tanh(dec['lg_pos'][s, k]) * r_seed + ego[k] for k in (0, 1))
    row = s * A_cap + A
    st['pos'][s, :, A] = 0.0
    st['head'][s, :, A] = 0.0
    st['state'][s, :, A], st['token'][s, :, A], st['grid'][s, :, A], st['tmask'][s, :, A] = INVALID, -1, -1, 1
    st['imask'][s, :, A] = st['catflag'][s, :, A] = (np.arange(st['T']) >= c)
    st['pos'][s, c, A] = (nx, ny)
    st['head'][s, c, A] = ego[2]
    st['state'][s, c, A], st['token'][s, c, A], st['grid'][s, c, A] = ENTER, -2, cell
    st['type'][s, A], st['bos'][s, A] = ty, c
    dec['new_shape'][s], dec['new_cell'][s] = dec['shape'][s], cell
    if t > 0:
        k = slice((t - 1) * 5, (t - 1) * 5 + 5)
        st['pred_traj'][row, k] = (nx, ny)
        st['pred_head'][row, k] = ego[2]
        st['pred_state'][row, k] = float(ENTER)
    st['n_agents'][s] = A + 1
    dec['n_new'][s] += 1
    dec['new_row'][s], dec['inserted'][s] = row, 1


def insert_finalize_ref(st, dec, c, angle_interval, hv_ovr, head_token=True, xy_offset=True):
    """k_insert_finalize, in place: for the scenes with inserted > 0 the heading (arg-max token, first index on ties, decoded and
    wrapped - or tanh(lg[0]) * pi + ego heading, not wrapped) and the xy offset tanh(offset) * 2 of row new_row[s], and
    hv_ovr[s] = (cos, sin) of the heading.  inserted 0 and -1: nothing."""
    for s in range(st['S']):
        if dec['inserted'][s] <= 0:
            continue
        a = int(dec['new_row'][s]) - s * st['A_cap']
        eh = st['head'][s, c, int(st['av_index'][s])]
        lh = dec['lg_heading'][s]
        if head_token:
            bi = 0
            for k in range(1, lh.size):
                if lh[k] > lh[bi]:
                    bi = k
            nh = float(decode_heading(bi, angle_interval, eh))
        else:
            nh = math.tanh(lh[0]) * math.pi + eh
        st['head'][s, c, a] = nh
        if xy_offset:
            st['pos'][s, c, a] += np.tanh(dec['offset'][s].astype(np.float64)) * 2.0
        hv_ovr[s] = (math.cos(nh), math.sin(nh))


_F64_KEYS = ('pos', 'head', 'pred_traj', 'pred_head', 'pred_state')


def as_ref(d):
    """a deep copy of a block / decision dict for the in-place references: the float arrays they write in float64"""
    return {k: (v.astype(np.float64) if k in _F64_KEYS else v.copy()) if isinstance(v, np.ndarray) else v for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ generators
def _resample(rng, draw, offenders, tries=200):
    """draw() -> points; offenders(points) -> indices of points within MARGIN of a radius; those are drawn again"""
    pts = draw(None)
    for _ in range(tries):
        bad = offenders(pts)
        if len(bad) == 0:
            return pts
        pts[bad] = draw(len(bad))
    raise AssertionError('generator could not clear the radius margin')


def _pairs_near(d2, r):
    r2 = float(r) ** 2
    return np.abs(d2 - r2) / r2 < 2 * MARGIN


def _cloud_offenders(r, fixed=None, r_fixed=None, self_pairs=True):
    """points within twice the margin of radius r of another point of the cloud (or of r_fixed of a fixed cloud)"""
    def off(p):
        q = p.astype(np.float64)
        bad = np.zeros(len(q), bool)
        if self_pairs and len(q) > 1:
            d2 = ((q[:, None] - q[None]) ** 2).sum(-1)
            near = _pairs_near(d2, r)
            np.fill_diagonal(near, False)
            bad |= np.triu(near, 1).any(0)        # (the later point of a pair moves)
        if fixed is not None and len(fixed):
            d2 = ((q[:, None] - fixed.astype(np.float64)[None]) ** 2).sum(-1)
            bad |= _pairs_near(d2, r_fixed).any(1)
        return np.nonzero(bad)[0]
    return off


MAP_GRAPH_CASES = {
    # name: (n_map per scene, M_cap, radius, max_nbr, extent [m], what it is for)
    'lds_1024': ([1024, 0, 1, 700], 1024, 12.0, 8, 200.0, 'positions in LDS, ragged n_map with 0 and 1, the cap reached'),
    'global_1000': ([1000, 37, 1000], 1000, 12.0, 8, 200.0, 'global scan; a workgroup of 32 centres spans two scenes'),
    'global_40': ([40, 0, 1, 17, 40], 40, 8.0, 4, 30.0, 'global scan; S * M_cap not a multiple of 32'),
    'nomask_4160': ([4160, 4096], 4160, 12.0, 8, 400.0, 'more than 4096 tokens: no lane masks'),
    'dense_200': ([600, 1024], 1024, 25.0, 200, 200.0, 'a cluster: more than 128 neighbours kept, the chunk path'),
}


def gen_map_graph(name, seed=0):
    n_map, M_cap, radius, max_nbr, ext, _ = MAP_GRAPH_CASES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    S = len(n_map)
    radius = float(np.float32(radius))
    pos = rng.uniform(-500, 500, (S, M_cap, 2)).astype(np.float32)          # (slots >= n_map hold values that must not be read)
    orient = rng.uniform(-math.pi, math.pi, (S, M_cap)).astype(np.float32)
    for s, M in enumerate(n_map):
        def draw(n, M=M, s=s):
            k = M if n is None else n
            p = rng.uniform(-ext / 2, ext / 2, (k, 2))
            if name == 'dense_200' and n is None:
                nc = M // 2 + 60
                ang, rad = rng.uniform(0, 2 * math.pi, nc), 9.0 * np.sqrt(rng.uniform(0, 1, nc))
                p[:nc] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
                p = p[rng.permutation(k)]
            elif name == 'dense_200':
                p = rng.uniform(-9.0 / 1.5, 9.0 / 1.5, (k, 2))
            return p.astype(np.float32)
        if M:
            pos[s, :M] = _resample(rng, draw, _cloud_offenders(radius))
    return dict(n_map=np.asarray(n_map, np.int32), pos=pos, orient=orient, radius=radius, max_nbr=max_nbr, M_cap=M_cap, S=S)


BUILD_EDGES_CASES = {
    # name: (A per scene, A_cap, n_map per map slot, M_cap, map_scene, T, c, overrides, what it is for)
    'cap32': ([1, 10, 11, 32], 32, [0, 3, 700], 704, [2, 1, 0, 2], 18, None, True, 'A = 1 / 10 / 11: the A - 10 rule; shared, permuted map slots'),
    'cap256': (([1, 10, 11, 63, 64, 65, 200] * 19)[:130], 256, [0, 3, 700], 704, None, 18, 12, True,
               '130 scenes: the 256-thread instantiation; scans over several 64-lane trips'),
    'cap1024': ([700, 65], 1024, [4160, 700], 4160, [0, 1], 18, 11, True,
                'a cluster with more than 301 rows in radius; map tokens scanned in global memory'),
}


def gen_build_edges(name, c=None, seed=0, overrides=None):
    """a random block for infgen_build_edges: states with INVALID, imask / tmask zeros, bos inside the window, rows >= A filled with
    plausible values that must not be read; the agent-agent and agent-map pairs of column c clear the margin"""
    As, A_cap, n_map, M_cap, map_scene, T, c0, ovr, _ = BUILD_EDGES_CASES[name]
    c = c0 if c is None else c
    ovr = ovr if overrides is None else overrides
    rng = np.random.default_rng([seed, sum(map(ord, name)), c])
    S, Sm = len(As), len(n_map)
    st = new_state(S, A_cap, T, M_cap, Sm=Sm, W=12, ring=13, r_map=30.0, r_agent=60.0)
    st['n_agents'][:] = As
    st['n_map'][:] = n_map
    st['map_scene'] = (np.arange(S) % Sm if map_scene is None else np.asarray(map_scene)).astype(np.int32)
    ext = 300.0
    for m in range(Sm):
        st['map_pos'][m] = rng.uniform(-ext / 2, ext / 2, (M_cap, 2)).astype(np.float32)
        st['map_orient'][m] = rng.uniform(-math.pi, math.pi, M_cap).astype(np.float32)
    st['pos'][:] = rng.uniform(-ext / 2, ext / 2, st['pos'].shape).astype(np.float32)
    st['head'][:] = rng.uniform(-math.pi, math.pi, st['head'].shape).astype(np.float32)
    st['state'][:] = rng.choice([INVALID, VALID, VALID, ENTER, EXIT, INVALID], st['state'].shape)
    st['imask'][:] = rng.uniform(size=st['imask'].shape) > 0.15
    st['tmask'][:] = rng.uniform(size=st['tmask'].shape) > 0.15
    st['bos'][:] = np.where(rng.uniform(size=st['bos'].shape) < 0.5, 0, rng.integers(0, max(c, 1) + 1, st['bos'].shape))
    st['av_index'][:] = [rng.integers(0, A) for A in As]
    for s, A in enumerate(As):
        ms = int(st['map_scene'][s])
        fixed = st['map_pos'][ms, :n_map[ms]]

        def draw(n, A=A):
            k = A if n is None else n
            p = rng.uniform(-ext / 2, ext / 2, (k, 2))
            if A == 700:                          # the cluster: 400 rows within 15 m of each other, far inside r_agent
                nc = 400 if n is None else k
                ang, rad = rng.uniform(0, 2 * math.pi, nc), 15.0 * np.sqrt(rng.uniform(0, 1, nc))
                p[:nc] = np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
                if n is None:
                    p = p[rng.permutation(k)]
            return p.astype(np.float32)
        st['pos'][s, c, :A] = _resample(rng, draw, _cloud_offenders(st['r_agent'], fixed, st['r_map']))
    if ovr:
        st['first_new'] = np.asarray([A - min(3, A) if s % 2 == 0 else A_cap for s, A in enumerate(As)], np.int32)
        ang = rng.uniform(-math.pi, math.pi, S)
        st['hv_ovr'] = np.stack([np.cos(ang), np.sin(ang)], -1).astype(np.float32)
    return st, c


POINT_EDGES_CASES = {
    # name: (r_agent, k_agent, r_map, k_map, hit rates of the agents / map tokens per scene, what it is for)
    'heading_24_128': (10.0, 24, 10.0, 128, [(0.3, 0.6), (0.9, 0.9), (0.05, 0.1), (0.0, 0.0), (0.35, 0.55), (0.3, 0.6)],
                       'production heading stage: the 24th agent in the second trip, the 128th token in the fourth'),
    'seed_300_2048': (75.0, 300, 75.0, 2048, [(0.6, 0.75), (0.2, 0.3), (0.0, 0.0), (0.9, 0.95)],
                      'production seed stage: K = 300 / 2048 over 700 agents / 3000 tokens'),
}


def gen_point_edges(name, seed=0):
    """scenes of 700 agents / 3000 map tokens (two map slots, shared): every candidate sits either inside 0.8 r or outside 1.3 r of
    the centre row's position, with a per-scene hit rate; one scene has no hit at all"""
    ra, ka, rm, km, rates, _ = POINT_EDGES_CASES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    S, Sm, A, M = len(rates), 2, 700, 3000
    st = new_state(S, 1024, 3, 3008, Sm=Sm)
    c = 1
    st['n_agents'][:] = A
    st['n_agents'][-1] = 650
    st['n_map'][:] = [M, 2900]
    st['map_scene'] = (np.arange(S) % Sm)[::-1].astype(np.int32).copy()
    st['head'][:] = rng.uniform(-math.pi, math.pi, st['head'].shape).astype(np.float32)
    st['map_orient'][:] = rng.uniform(-math.pi, math.pi, st['map_orient'].shape).astype(np.float32)
    st['imask'][:] = rng.uniform(size=st['imask'].shape) > 0.2
    st['av_index'][:] = 0
    centre_row = rng.integers(1, 600, S).astype(np.int32)

    def ring_points(n, rate, r):
        hit = rng.uniform(size=n) < rate
        rad = np.where(hit, r * 0.8 * np.sqrt(rng.uniform(0.0004, 1, n)), r * rng.uniform(1.3, 3.0, n))
        ang = rng.uniform(0, 2 * math.pi, n)
        return np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)
    # the two map slots are shared by the scenes, so all centres sit at the origin of the map frame, rotated hit patterns apart
    for m in range(Sm):
        rate = max(r[1] for s, r in enumerate(rates) if st['map_scene'][s] == m)
        st['map_pos'][m] = ring_points(st['M_cap'], rate, rm).astype(np.float32)
    for s, (rate_a, rate_m) in enumerate(rates):
        st['pos'][s, c] = ring_points(1024, rate_a, ra).astype(np.float32)
        st['pos'][s, c, centre_row[s]] = 0.0
        if rate_m == 0.0:                         # the scene without hits: its centre far from every map token and agent
            st['pos'][s, c, centre_row[s]] = (5000.0, 5000.0)
    return dict(st=st, c=c, centre_row=centre_row, r_agent=float(np.float32(ra)), k_agent=ka, r_map=float(np.float32(rm)), k_map=km)


def gen_strict_radius():
    """integer coordinates, on which fp32 is exact: points at (3, 4), (6, 8), (5, 12) around the origin are at exactly 5, 10, 13"""
    pts = np.asarray([[0, 0], [3, 4], [6, 8], [5, 12], [100, 100]], np.float32)
    cases = []
    for i, r in ((1, 5.0), (2, 10.0), (3, 13.0)):
        cases.append((np.float32(r), i, False))
        cases.append((np.nextafter(np.float32(r), np.float32(np.inf)), i, True))
    return pts, cases


def gen_occupancy(G, seed=0, out_of_range=True):
    """64 scenes of 0 .. 64 agents (A_cap 64): grid tokens with -1, duplicates, 0 and G - 1 - and, once the kernels guard, values
    >= G; rows >= n_agents hold valid cells that must not be marked"""
    rng = np.random.default_rng([seed, G])
    S, A_cap = 64, 64
    st = new_state(S, A_cap, 3, 32, G=G)
    st['n_agents'][:] = np.arange(S)
    st['n_agents'][5] = A_cap
    st['n_agents'][7] = 0
    g = rng.integers(0, G, (S, A_cap))
    g[rng.uniform(size=g.shape) < 0.15] = -1
    g[:, 3] = g[:, 2]
    g[:, 10], g[:, 11] = 0, G - 1
    if out_of_range:
        g[:, 20], g[:, 21], g[30:, 22] = G, G + 5, 1 << 20
    g[9, :] = -1                                  # a scene of 9 agents without an occupied cell
    st['grid'][:, 1] = g
    st['grid'][:, 0] = rng.integers(0, G, (S, A_cap))            # (another column: not read)
    return st, 1


def gen_mlp_layer(G, seed=0):
    rng = np.random.default_rng([seed, G, 17])
    p = 'occ'
    return {f'{p}.mlp.0.weight': (rng.standard_normal((128, G)) / 8).astype(np.float32),
            f'{p}.mlp.0.bias': rng.standard_normal(128).astype(np.float32) * 0.1,
            f'{p}.mlp.1.weight': (1 + 0.1 * rng.standard_normal(128)).astype(np.float32),
            f'{p}.mlp.1.bias': rng.standard_normal(128).astype(np.float32) * 0.1,
            f'{p}.mlp.3.weight': (rng.standard_normal((128, 128)) / 11).astype(np.float32),
            f'{p}.mlp.3.bias': rng.standard_normal(128).astype(np.float32) * 0.1}, p


def gen_sample_topk(rows, n, k, seed=0):
    """logits on a 0.25 grid in [-4, 4] (ties inside and across the k-th place), -inf entries (fewer than n - k), rows whose k
    largest are all equal (probabilities exactly 1: u = j / k lands on a partial sum exactly), u = 0 and u = 1 - 2^-24; the other
    uniforms are drawn until they clear CDF_MARGIN"""
    rng = np.random.default_rng([seed, rows, n, k])
    lg = (rng.integers(-16, 17, (rows, n)) * 0.25).astype(np.float32)
    u = rng.uniform(0, 1, rows).astype(np.float32)
    kinds = []
    for r in range(rows):
        kind = ('ties', 'zero', 'one', 'random', 'neg_inf', 'tied_kth')[r % 6] if rows > 1 else 'ties'
        if kind == 'ties':                        # the k largest all equal 5.0, at random places
            lg[r, rng.choice(n, k, replace=False)] = 5.0
            u[r] = np.float32((r // 6) % k) / np.float32(k) if k in (1, 2, 16) else u[r]
        elif kind == 'zero':
            u[r] = 0.0
        elif kind == 'one':
            u[r] = np.float32(1.0) - np.float32(2.0 ** -24)
        elif kind == 'neg_inf':
            lg[r, rng.choice(n, max(min(n - k - 1, n // 3), 0), replace=False)] = -np.inf
        elif kind == 'tied_kth':                  # k + 2 copies of the k-th value: the tie runs across the k-th place
            lg[r, rng.choice(n, min(k + 2, n), replace=False)] = 4.5
        if kind in ('random', 'neg_inf', 'tied_kth'):
            for _ in range(100):
                if topk_pick(lg[r], k, u[r])[1] > CDF_MARGIN:
                    break
                u[r] = np.float32(rng.uniform(0, 1))
        kinds.append(kind)
    return lg, u, kinds


INSERT_DECIDE_BRANCHES = [
    # name, expected (inserted, active after) without force_enter (insert_decide_expect for the rest)
    ('inactive', 0, 0), ('enter_below', 0, 0), ('enter_equal', 0, 0), ('enter_above', 1, 1), ('force_enter', 1, 1),
    ('type_tie_01', 1, 1), ('type_tie_12', 1, 1), ('occupied', 0, None), ('max_new_reached', 0, 0), ('rows_full', -1, 0),
    ('cell_tie', 1, 1), ('u_zero', 1, 1), ('u_partial_sum', 1, 1), ('u_one', 1, 1), ('nan_logits', 0, 0), ('ego_not_first', 1, 1),
]
# the calls of the GPU test, each of which the CPU test runs through the generator and the reference as well:
# (sample_k, through infgen_insert_decide_topk?, t, force_enter)
INSERT_DECIDE_CASES = [(1, False, 0, 0), (1, False, 2, 0), (1, True, 2, 1), (2, True, 0, 0), (16, True, 2, 0), (16, True, 0, 1)]


def insert_decide_expect(name, sample_k, force_enter):
    """(inserted, active afterwards) of a named branch: force_enter makes the enter-logit rows enter (strict > otherwise, so equal
    logits do not); an occupied cell stops the scene when the choice is greedy and spends the iteration when it is sampled"""
    ins, act = {b[0]: b[1:] for b in INSERT_DECIDE_BRANCHES}[name]
    if name in ('enter_below', 'enter_equal') and force_enter:
        ins, act = 1, 1
    if name == 'occupied':
        act = 1 if sample_k > 1 else 0
    return ins, act


def gen_insert_decide(G, grid_xy, sample_k, t, force_enter=0, seed=0):
    """one scene per named branch of k_insert_decide (INSERT_DECIDE_BRANCHES; with force_enter the enter-logit rows all enter).
    A_cap = 32, T = 4; every array of a scene is filled with values that a reset must replace; poses within +-200 m.
    -> (block, decisions, names, max_new)"""
    rng = np.random.default_rng([seed, sample_k, t, force_enter])
    names = [b[0] for b in INSERT_DECIDE_BRANCHES]
    S, A_cap, T, max_new = len(names), 32, 4, 10
    c = 1 + t
    st = new_state(S, A_cap, T, 32, G=G, R=15)
    st['grid_xy'] = np.asarray(grid_xy, np.float32).copy()
    st['pos'][:] = rng.uniform(-200, 200, st['pos'].shape).astype(np.float32)
    st['head'][:] = rng.uniform(-math.pi, math.pi, st['head'].shape).astype(np.float32)
    for k, hi in (('state', 4), ('token', 2048), ('grid', G), ('type', 3), ('bos', T)):
        st[k][:] = rng.integers(0, hi, st[k].shape)
    for k in ('tmask', 'imask', 'catflag'):
        st[k][:] = rng.integers(0, 2, st[k].shape)
    for k in ('pred_traj', 'pred_head', 'pred_state'):
        st[k][:] = rng.uniform(-5, 5, st[k].shape).astype(np.float32)
    st['n_agents'][:] = rng.integers(3, 20, S)
    st['av_index'][:] = 0
    dec = new_decisions(S, G)
    dec['lg_pos'][:] = (rng.integers(-12, 13, (S, G)) * 0.25).astype(np.float32)
    dec['lg_type'][:] = rng.standard_normal((S, 3)).astype(np.float32)
    dec['shape'][:] = rng.uniform(0.5, 5, (S, 3)).astype(np.float32)
    dec['lg_state'][:] = (0.0, 1.0)
    dec['n_new'][:] = rng.integers(0, 5, S)
    dec['uniform'][:] = rng.uniform(0, 1, S).astype(np.float32)
    k = max(sample_k, 1)
    for s, name in enumerate(names):
        top = rng.choice(G, 16, replace=False)
        dec['lg_pos'][s, top] = 4.0 + 0.5 * rng.permutation(16).astype(np.float32)      # 16 distinct leaders
        if name == 'inactive':
            dec['active'][s] = 0
        elif name == 'enter_below':
            dec['lg_state'][s] = (0.5, 0.25)
        elif name == 'enter_equal':
            dec['lg_state'][s] = (0.5, 0.5)
        elif name == 'type_tie_01':
            dec['lg_type'][s] = (1.5, 1.5, 0.0)
        elif name == 'type_tie_12':
            dec['lg_type'][s] = (0.0, 1.5, 1.5)
        elif name == 'max_new_reached':
            dec['n_new'][s] = max_new
        elif name == 'rows_full':
            st['n_agents'][s] = A_cap
        elif name in ('cell_tie', 'u_partial_sum', 'occupied'):
            dec['lg_pos'][s, top] = 9.0           # the 16 leaders all equal: probabilities exactly 1, the lowest index first
            if name == 'u_partial_sum':
                dec['uniform'][s] = np.float32(k // 2) / np.float32(k)
        elif name == 'u_zero':
            dec['uniform'][s] = 0.0
        elif name == 'u_one':
            dec['uniform'][s] = np.float32(1.0) - np.float32(2.0 ** -24)
        elif name == 'nan_logits':
            dec['lg_pos'][s] = np.nan
        elif name == 'ego_not_first':
            st['av_index'][s] = st['n_agents'][s] - 1
        if name not in ('u_zero', 'u_one', 'u_partial_sum', 'nan_logits'):
            for _ in range(100):
                if topk_pick(dec['lg_pos'][s], k, dec['uniform'][s])[1] > CDF_MARGIN:
                    break
                dec['uniform'][s] = np.float32(rng.uniform(0, 1))
        # occupancy: a few cells, never the one this scene picks - except in the 'occupied' scene, where it is exactly that one
        dec['occ'][s, rng.choice(G, 12, replace=False)] = 1.0
        if name != 'nan_logits':
            cell = topk_pick(dec['lg_pos'][s], k, dec['uniform'][s])[0]
            dec['occ'][s, cell] = 1.0 if name == 'occupied' else 0.0
    return st, dec, names, max_new


def gen_insert_finalize(seed=0, angle_interval=3.0):
    """scenes after a decide: inserted in {1, 0, -1}; heading logits with ties at the maximum; a decoded heading whose sum with the
    ego heading crosses +-pi; offsets with tanh saturating.  new_row of the 0 / -1 scenes names an existing row that must stay."""
    rng = np.random.default_rng([seed, 99])
    n_heading = int(360.0 / angle_interval)
    S, A_cap, T, c = 12, 32, 4, 2
    st = new_state(S, A_cap, T, 32)
    st['pos'][:] = rng.uniform(-200, 200, st['pos'].shape).astype(np.float32)
    st['head'][:] = rng.uniform(-math.pi, math.pi, st['head'].shape).astype(np.float32)
    st['n_agents'][:] = rng.integers(4, 20, S)
    st['av_index'][:] = rng.integers(0, 3, S)
    dec = new_decisions(S, 1, n_heading)
    dec['lg_heading'][:] = (rng.integers(-8, 9, (S, n_heading)) * 0.25).astype(np.float32)
    dec['offset'][:] = rng.standard_normal((S, 2)).astype(np.float32)
    dec['inserted'][:] = [1, 1, 0, -1, 1, 1, 1, 0, -1, 1, 1, 1]
    dec['new_row'][:] = np.arange(S) * A_cap + st['n_agents'] - 1
    st['head'][0, c, st['av_index'][0]] = 3.0      # + decoded (119 * 3 - 180) deg = 3.09 rad: beyond pi
    dec['lg_heading'][0, 119] = 7.0
    st['head'][1, c, st['av_index'][1]] = -3.0     # + decoded (0 * 3 - 180) deg = -pi: below -pi
    dec['lg_heading'][1, 0] = 7.0
    dec['lg_heading'][4, [17, 40, 90]] = 6.0       # ties at the maximum: the first index wins
    dec['lg_heading'][5, :] = 1.0                  # all equal: index 0
    dec['offset'][6] = (30.0, -30.0)               # tanh saturates at +-1
    dec['offset'][9] = (1e-4, 0.0)
    return st, dec, c, angle_interval, n_heading


# ------------------------------------------------------------------------------------------------ step advance: integrate, raw feature
TOKEN_SIZE, EMB = 2048, 128
SCRATCH_FILL = -7.25e30            # the scratch outputs of a block start out with it: what a kernel leaves alone is seen


def step_vocab(seed=0):
    """[3][2048][6][4][2] contours: per (type, token) a random rectangle (0.5 .. 6 m by 0.4 .. 2.5 m) moving on an arc, corners in
    the order front-left, front-right, rear-right, rear-left (corner 0 - corner 3 points along the heading)"""
    if seed not in _VOCAB:
        rng = np.random.default_rng([seed, 4242])
        n = 3 * TOKEN_SIZE
        L, Wd = rng.uniform(0.5, 6.0, n), rng.uniform(0.4, 2.5, n)
        dist, dth = rng.uniform(-1.0, 12.0, n), rng.uniform(-0.6, 0.6, n)
        k = np.arange(6) / 5.0
        ang = k[None] * dth[:, None]
        ctr = np.stack([dist[:, None] * k[None] * np.cos(ang / 2), dist[:, None] * k[None] * np.sin(ang / 2)], -1)       # [n][6][2]
        cor = np.stack([np.stack([L / 2, Wd / 2], -1), np.stack([L / 2, -Wd / 2], -1), np.stack([-L / 2, -Wd / 2], -1),
                        np.stack([-L / 2, Wd / 2], -1)], 1)                                                             # [n][4][2]
        cs, sn = np.cos(ang)[:, :, None], np.sin(ang)[:, :, None]
        x = cor[:, None, :, 0] * cs - cor[:, None, :, 1] * sn + ctr[:, :, None, 0]
        y = cor[:, None, :, 0] * sn + cor[:, None, :, 1] * cs + ctr[:, :, None, 1]
        _VOCAB[seed] = np.stack([x, y], -1).astype(np.float32).reshape(3, TOKEN_SIZE, 6, 4, 2)
    return _VOCAB[seed]


_VOCAB, _CASES = {}, {}


def step_grid(G, seed=0, spacing=3.0):
    """the G innermost points of a square lattice (a circular mask, like the real 1961-cell grid), in shuffled order: the two cells
    nearest to an agent fall in the same lane of the search (indices equal modulo 64) or in different ones"""
    rng = np.random.default_rng([seed, G, 7])
    h = int(math.ceil(math.sqrt(G / math.pi))) + 2
    ij = np.mgrid[-h:h + 1, -h:h + 1].reshape(2, -1).T
    keep = np.lexsort((np.arange(len(ij)), (ij ** 2).sum(1)))[:G]
    assert len(keep) == G
    return (ij[keep][rng.permutation(G)] * spacing).astype(np.float32)


def new_step_ext(st, scratch=False):
    """what infgen_integrate / infgen_raw_feature read beside a new_state block (kept apart: the dicts of the other tests' callers do
    not change): scalars, next_token / next_state [S * A_cap], the optional teacher arrays [S][T][A_cap] and replay_row [S][A_cap],
    the contour vocabulary, the embedding tables and - with scratch - the raw-feature outputs"""
    rows = st['S'] * st['A_cap']
    ext = dict(force_valid=0, no_state_token=0, no_grid_token=0,
               next_token=np.zeros(rows, np.int32), next_state=np.zeros(rows, np.int32),
               teacher_token=None, teacher_state=None, teacher_grid=None, teacher_pos=None, teacher_head=None, replay_row=None,
               vocab=step_vocab(), tok_tab=None, grid_tab=None, state_emb=None, cat_agent=None, cat_seed=None)
    if scratch:
        for k, w in (('raw2', 4), ('cat', EMB), ('fus_in', 4 * EMB), ('tmp1', EMB), ('tmp2', EMB), ('X', EMB)):
            ext[k] = np.full((rows, w), SCRATCH_FILL, np.float32)
    return ext


def integrate_ref(st, ext, t, f=np.float64, mutate=None):
    """k_integrate: one decode step of column c = 1 + t into n = c + 1 (reference agent_decoder.py:2168-2239, attr_tokenizer.py:77-89)
    -> the arrays of the block after the step (floats in f), plus per row < n_agents: 'new_pose' (x, y, theta before an INVALID row
    is zeroed), 'search' (the first cell at the smallest distance, before teacher_grid) and 'gap' (second-smallest minus smallest
    distance; inf with one cell).  Order of the state rules: index 2 -> EXIT, the ego VALID, no_state_token EXIT -> VALID,
    force_valid all VALID.  Device-only (kernel header): teacher_token (negative: contour of token 0, the stored token stays),
    teacher_state, teacher_pos / teacher_head (the stored pose, not pred_*), teacher_grid (where >= -1) - each only for the rows
    replay_row flags (all rows without it); the ego's own flag decides the pose the search is centred on.
    mutate: a deliberately wrong variant, for the tests that show the cases tell it apart ('old_ego': search centred on the ego's
    pose of column c; 'dup_ignores_flag': rows outside the ego's 16-row group see the ego's generated pose; 'grid_ge0': teacher_grid
    honoured from 0 only)."""
    S, A_cap, G = st['S'], st['A_cap'], st['grid_size']
    c, n = 1 + t, 2 + t
    assert n < st['T'] and t * 5 + 5 <= st['R']
    out = {k: st[k].copy() for k in ('state', 'token', 'grid', 'imask', 'catflag')}
    for k in ('pos', 'head', 'pred_traj', 'pred_head', 'pred_state'):
        out[k] = st[k].astype(f)
    out['gap'] = np.full((S, A_cap), math.inf)
    out['search'] = np.full((S, A_cap), -1, np.int64)
    out['new_pose'] = np.zeros((S, A_cap, 3), f)
    gxy = st['grid_xy'][:G].astype(f)
    rr = None if ext['replay_row'] is None else ext['replay_row'].reshape(S, A_cap)
    sl = slice(t * 5, t * 5 + 5)
    for s in range(S):
        A, av = int(st['n_agents'][s]), int(st['av_index'][s])
        if A == 0:
            continue
        assert 0 <= av < A
        rows = s * A_cap + np.arange(A)
        tok, ns = ext['next_token'][rows].copy(), ext['next_state'][rows].copy()
        ns[ns == 2] = EXIT
        ns[av] = VALID
        if ext['no_state_token']:
            ns[ns == EXIT] = VALID
        if ext['force_valid']:
            ns[:] = VALID
        forced = np.ones(A, bool) if rr is None else rr[s, :A] != 0
        stored_tok = tok.copy()
        if ext['teacher_token'] is not None:
            tt = ext['teacher_token'][s, n, :A]
            stored_tok = np.where(forced, tt, tok)
            tok = np.where(forced, np.maximum(tt, 0), tok)
        if ext['teacher_state'] is not None:
            ns = np.where(forced, ext['teacher_state'][s, n, :A], ns)
        th = st['head'][s, c, :A].astype(f)
        cs, sn = np.cos(th)[:, None, None], np.sin(th)[:, None, None]
        b = st['pos'][s, c, :A].astype(f)
        ct = ext['vocab'][st['type'][s, :A], tok][:, 1:].astype(f)                 # [A][5][4][2]
        x, y = ct[..., 0], ct[..., 1]
        cx = (x * cs + y * (-sn)) + b[:, 0, None, None]                             # [x y] @ [[cos, sin], [-sin, cos]] + pos
        cy = (x * sn + y * cs) + b[:, 1, None, None]
        mx = (((cx[..., 0] + cx[..., 1]) + cx[..., 2]) + cx[..., 3]) / f(4)
        my = (((cy[..., 0] + cy[..., 1]) + cy[..., 2]) + cy[..., 3]) / f(4)
        hh = np.arctan2(cy[..., 0] - cy[..., 3], cx[..., 0] - cx[..., 3])
        out['pred_traj'][rows, sl, 0], out['pred_traj'][rows, sl, 1] = mx, my
        out['pred_head'][rows, sl] = hh
        out['pred_state'][rows, sl] = ns[:, None]
        lx, ly, lth = mx[:, 4].copy(), my[:, 4].copy(), hh[:, 4].copy()
        own = (lx[av], ly[av], lth[av])                                             # the ego's generated pose
        if ext['teacher_pos'] is not None:
            lx = np.where(forced, ext['teacher_pos'][s, n, :A, 0].astype(f), lx)
            ly = np.where(forced, ext['teacher_pos'][s, n, :A, 1].astype(f), ly)
            lth = np.where(forced, ext['teacher_head'][s, n, :A].astype(f), lth)
        ex, ey, eth = (np.full(A, v) for v in (lx[av], ly[av], lth[av]))
        if mutate == 'old_ego':
            ex, ey, eth = (np.full(A, v) for v in (b[av, 0], b[av, 1], th[av]))
        if mutate == 'dup_ignores_flag' and A_cap > 16 and S <= 128:
            other = np.arange(A) // 16 != av // 16
            ex, ey, eth = (np.where(other, o, e) for o, e in zip(own, (ex, ey, eth)))
        phi = -(eth - f(np.float32(math.pi / 2)))           # pi / 2 as the fp32 reference rounds it (tensor - python scalar), in every f
        pc, ps = np.cos(phi), np.sin(phi)
        dx, dy = lx - ex, ly - ey
        rx, ry = dx * pc + dy * (-ps), dx * ps + dy * pc
        ux, uy = rx[:, None] - gxy[None, :, 0], ry[:, None] - gxy[None, :, 1]
        d = np.sqrt(ux * ux + uy * uy)
        cell = d.argmin(1)                                                          # (the first of equal minima)
        if G > 1:
            two = np.partition(d, 1, axis=1)
            out['gap'][s, :A] = two[:, 1] - two[:, 0]
        out['search'][s, :A] = cell
        out['new_pose'][s, :A] = np.stack([lx, ly, lth], -1)
        inv = ns == INVALID
        if ext['teacher_grid'] is not None:
            tg = ext['teacher_grid'][s, n, :A]
            cell = np.where(forced & (tg >= (0 if mutate == 'grid_ge0' else -1)), tg, cell)
        out['state'][s, n, :A] = ns
        out['pos'][s, n, :A, 0], out['pos'][s, n, :A, 1] = np.where(inv, f(0), lx), np.where(inv, f(0), ly)
        out['head'][s, n, :A] = np.where(inv, f(0), lth)
        out['grid'][s, n, :A] = np.where(inv, -1, cell)
        out['token'][s, n, :A] = np.where(inv, -1, stored_tok)
        out['imask'][s, n, :A] = np.where(inv, 0, st['imask'][s, n, :A])
        out['catflag'][s, n, :A] = np.where(inv, 0, st['catflag'][s, n, :A])
    return out


def step_errors(ref, other, st, t):
    """largest difference of two evaluations of a step over the rows < n_agents: (position [m] of the stored pose and pred_traj,
    heading [rad] of the stored pose and pred_head, modulo 2 pi)"""
    n, sl = 2 + t, slice(t * 5, t * 5 + 5)
    live = np.arange(st['A_cap'])[None] < st['n_agents'][:, None]
    if not live.any():
        return np.zeros(2)
    lr = live.reshape(-1)
    f8 = lambda a: np.asarray(a, np.float64)
    ep = max(np.abs(f8(ref['pos'])[:, n][live] - f8(other['pos'])[:, n][live]).max(),
             np.abs(f8(ref['pred_traj'])[lr, sl] - f8(other['pred_traj'])[lr, sl]).max())
    eh = max(ang_err(ref['head'][:, n][live], other['head'][:, n][live]).max(),
             ang_err(ref['pred_head'][lr, sl], other['pred_head'][lr, sl]).max())
    return np.asarray([ep, eh])


def rawfeat_prep_ref(st, ext, col, rows=None, mask=None, f=np.float64):
    """k_rawfeat_prep of column col (agent_decoder.py:2265-2285, _build_vector_a: 426-447) for every row of [S][A_cap] - or for the
    compact slots of a row subset, a masked-off slot reading row 0.  -> raw2 (motion norm, bearing of the motion in the heading
    frame), 'ruled' (1: the motion is a gap rule's (+-1, +-1), 2: (-2, -2); the norm is then the rounded root of 2 or 8), the
    categorical row (cat_agent[row] where catflag, else cat_seed) and the token / state / grid embedding rows, by python indexing
    (token -1 / -2 and grid -1 count from the end of their tables); grid None with no_grid_token"""
    A_cap = st['A_cap']
    if rows is None:
        rows = np.arange(st['S'] * A_cap)
    rows = np.asarray(rows, np.int64)
    if mask is not None:
        rows = np.where(np.asarray(mask) != 0, rows, 0)
    s, ag = rows // A_cap, rows % A_cap
    stj = st['state'][s, col, ag]
    inv = stj == INVALID
    m = np.zeros((len(rows), 2), f)
    ruled = np.zeros(len(rows), np.int8)
    if col > 0:
        m = st['pos'][s, col, ag].astype(f) - st['pos'][s, col - 1, ag].astype(f)
        pinv = st['state'][s, col - 1, ag] == INVALID
        m[inv], ruled[inv] = f(INVALID_MOTION), 2
        m[pinv & ~inv], ruled[pinv & ~inv] = f(MOTION_GAP), 1
        m[~pinv & inv], ruled[~pinv & inv] = f(-MOTION_GAP), 1
    else:
        m[inv], ruled[inv] = f(INVALID_MOTION), 2
        m[stj == ENTER], ruled[stj == ENTER] = f(MOTION_GAP), 1
    h = st['head'][s, col, ag].astype(f)
    hc, hs = np.cos(h), np.sin(h)
    mx, my = m[:, 0], m[:, 1]
    raw2 = np.stack([np.sqrt(mx * mx + my * my), np.arctan2(hc * my - hs * mx, (f(0) + hc * mx) + hs * my)], -1)
    cat = np.where(st['catflag'][s, col, ag][:, None] != 0, ext['cat_agent'][rows], ext['cat_seed'][None])
    tok = np.stack([ext['tok_tab'][int(ty)][int(k)] for ty, k in zip(st['type'][s, ag], st['token'][s, col, ag])])
    grid = None if ext['no_grid_token'] else np.stack([ext['grid_tab'][int(g)] for g in st['grid'][s, col, ag]])
    return dict(raw2=raw2, ruled=ruled, cat=cat, tok=tok, state=ext['state_emb'][stj], grid=grid)


# Largest error of a plain fp32 numpy evaluation of a step (integrate_ref, the kernel's operation order) and of the raw feature's
# motion pair against float64 over the inputs of gen_integrate (all INTEGRATE_CASES) and gen_rawfeat: position [m] and heading [rad]
# of the stored pose and of pred_*, motion norm [m], motion bearing [rad].  As above: the figures tests/test_graph_ref_cpu.py
# measures, rounded up in the fourth digit; the device bars are four times the figure.
FP32_ERR_STEP_POS, FP32_ERR_STEP_HEAD, FP32_ERR_MOTION_NORM, FP32_ERR_MOTION_BEARING = 2.099e-5, 2.521e-5, 9.639e-7, 2.877e-7
BAR_STEP_POS, BAR_STEP_HEAD = 4 * FP32_ERR_STEP_POS, 4 * FP32_ERR_STEP_HEAD
BAR_MOTION_NORM, BAR_MOTION_BEARING = 4 * FP32_ERR_MOTION_NORM, 4 * FP32_ERR_MOTION_BEARING
# Which cell is nearest is compared exactly, so outside the tie case no agent's nearest and second-nearest cell may be closer in
# distance [m] than ten times the position bar
GRID_MARGIN = 10 * BAR_STEP_POS

STEP_T, STEP_R = 6, 20             # columns / pred slots of the integrate blocks: the last step t = 3 fills both to the end
_RAGGED = [0, 1, 16, 17, -1]       # n_agents of the scenes of a batch, cycled (-1: A_cap)
INTEGRATE_CASES = {
    # name: (S, A_cap, n_agents (cycled; -1: A_cap), ego row (cycled; -1: the last row), G, step, force_valid, no_state_token,
    #        teacher: None | 'all' (no flags) | 'ego' (mixed flags, the ego flagged) | 'noego' (mixed, the ego generated), what for)
    'g2_first': (3, 32, [32, 17, 1], [0, 16, 0], 1961, 'first', 0, 0, None, '2 workgroups; the ego in the first / the second'),
    'g2_last': (3, 32, [16, 0, 32], [15, 0, 31], 63, 'last', 0, 1, None, 'the last step that fits T and R; a scene without agents'),
    'g2_force': (3, 32, [17, 32, 16], [0, 16, 15], 64, 'first', 1, 0, None, 'force_valid; a second workgroup with one row'),
    'g2_both': (3, 32, [32, 1, 17], [-1, 0, 16], 65, 'last', 1, 1, None, 'force_valid and no_state_token'),
    'g2_grid1': (3, 32, [17, 1, 32], [15, -1, 16], 1, 'first', 0, 0, None, 'a grid of one cell'),
    'g64_global': (1, 1024, [1024], [-1], 2049, 'first', 0, 0, None, '64 workgroups, the ego in the last; the grid in global memory'),
    'g64_lds': (1, 1024, [700], [0], 2048, 'last', 0, 1, 'ego', '64 workgroups, 20 of them empty, flags; the largest grid held in LDS'),
    'g1_32': (129, 32, _RAGGED, [0, 15, 16, -1], 1961, 'first', 0, 0, None, '1 workgroup per scene: S > 128'),
    'g1_96': (129, 96, _RAGGED + [65], [0, 15, 16, -1], 2049, 'last', 0, 0, 'noego', '16 waves loop over up to 96 agents; global grid'),
    'teach_all': (3, 32, [32, 17, 16], [0, 16, 15], 1961, 'first', 0, 0, 'all', 'the five teacher arrays, no flags'),
    'replay_ego': (3, 32, [32, 32, 17], [0, -1, 16], 1961, 'last', 0, 0, 'ego', 'flagged ego in another workgroup than flagged rows'),
    'replay_noego': (3, 32, [32, 17, 32], [16, 0, 15], 65, 'first', 0, 1, 'noego', 'a generated ego among flagged rows'),
    'replay_g1': (129, 32, _RAGGED, [16, 0, -1, 15], 64, 'last', 0, 0, 'ego', 'flags with one workgroup per scene'),
    'ties': (3, 32, [32, 17, 32], [16, 0, -1], 197, 'first', 0, 0, 'all', 'agents exactly between 2 or 4 cells: the lowest index'),
}


def integrate_groups(S, A_cap):
    """workgroups per scene of k_integrate (api.hip: integrate_groups)"""
    return A_cap // 16 if S <= 128 and A_cap > 16 and A_cap % 16 == 0 else 1


def gen_integrate(name, seed=0):
    """-> (block, ext, t) of a named case.  Every array is filled: columns other than n, rows >= n_agents and the pred_* slots of
    other steps hold values a step must leave alone.  Poses within +-200 m, headings over the full circle with +-pi among them,
    types 0..2, tokens with 0 and 2047, next_state over {0, 1, 2} with an ego that predicts INVALID.  Outside 'ties' every agent
    whose two nearest cells are closer in distance than twice GRID_MARGIN is drawn again.  Cached: do not write to the result."""
    if (name, seed) in _CASES:
        return _CASES[name, seed]
    S, A_cap, nag, avs, G, step, force_valid, no_state, teacher, _ = INTEGRATE_CASES[name]
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    T, R = STEP_T, STEP_R
    t = 0 if step == 'first' else min(T - 3, R // 5 - 1)
    c, n = 1 + t, 2 + t
    st = new_state(S, A_cap, T, 32, G=G, R=R)
    st['grid_xy'] = step_grid(G) if name != 'ties' else _tie_lattice(G, rng)
    st['n_agents'][:] = [A_cap if nag[s % len(nag)] < 0 else nag[s % len(nag)] for s in range(S)]
    st['av_index'][:] = [max(min(avs[s % len(avs)] if avs[s % len(avs)] >= 0 else A - 1, A - 1), 0) for s, A in enumerate(st['n_agents'])]
    centre = rng.uniform(-120, 120, (S, 1, 1, 2))
    draw_pos = lambda s, k=None: (centre[s, 0, 0] + rng.uniform(-70, 70, (2,) if k is None else (k, 2))).astype(np.float32)
    st['pos'][:] = (centre + rng.uniform(-70, 70, st['pos'].shape)).astype(np.float32)
    st['head'][:] = rng.uniform(-math.pi, math.pi, st['head'].shape).astype(np.float32)
    edge = np.float32(math.pi)
    st['head'][:, c, 1::7], st['head'][:, c, 2::7] = edge, -edge
    st['head'][:, c, 3::7], st['head'][:, c, 4::7] = np.nextafter(edge, np.float32(0)), -np.nextafter(edge, np.float32(0))
    st['state'][:] = rng.integers(0, 4, st['state'].shape)
    st['token'][:] = rng.integers(-1, TOKEN_SIZE, st['token'].shape)
    st['grid'][:] = rng.integers(-1, G, st['grid'].shape)
    for k in ('tmask', 'imask', 'catflag'):
        st[k][:] = rng.integers(0, 2, st[k].shape)
    st['type'][:] = rng.integers(0, 3, st['type'].shape)
    st['bos'][:] = rng.integers(0, T, st['bos'].shape)
    for k in ('pred_traj', 'pred_head', 'pred_state'):
        st[k][:] = rng.uniform(-5, 5, st[k].shape).astype(np.float32)
    ext = new_step_ext(st)
    ext['force_valid'], ext['no_state_token'] = force_valid, no_state
    ext['next_token'][:] = rng.integers(0, TOKEN_SIZE, S * A_cap)
    ext['next_token'][0::5], ext['next_token'][3::5] = 0, TOKEN_SIZE - 1
    ext['next_state'][:] = rng.integers(0, 3, S * A_cap)
    ext['next_state'][np.arange(S) * A_cap + st['av_index']] = np.arange(S) % 3          # an ego predicting INVALID / VALID / EXIT
    if teacher:
        sh = (S, T, A_cap)
        ext['teacher_token'] = rng.integers(0, TOKEN_SIZE, sh).astype(np.int32)
        ext['teacher_token'][:, :, 1::5] = -1
        ext['teacher_token'][:, :, 2::11], ext['teacher_token'][:, :, 3::11] = TOKEN_SIZE - 1, 0
        ext['teacher_state'] = rng.choice([INVALID, VALID, VALID, VALID, ENTER, EXIT], sh).astype(np.int32)
        ext['teacher_grid'] = rng.integers(0, G, sh).astype(np.int32)
        ext['teacher_grid'][:, :, 0::3], ext['teacher_grid'][:, :, 1::6] = -2, -1
        ext['teacher_pos'] = (centre + rng.uniform(-70, 70, sh + (2,))).astype(np.float32)
        ext['teacher_head'] = rng.uniform(-math.pi, math.pi, sh).astype(np.float32)
        for s in range(S):
            ext['teacher_state'][s, :, st['av_index'][s]] = VALID
        if teacher != 'all':
            ext['replay_row'] = rng.integers(0, 2, (S, A_cap)).astype(np.uint8)
            ext['replay_row'][np.arange(S), st['av_index']] = 1 if teacher == 'ego' else 0
    if name == 'ties':
        _place_ties(st, ext, n, rng)
    else:
        for _ in range(100):
            gap = integrate_ref(st, ext, t)['gap']
            bad = np.argwhere(gap < 2 * GRID_MARGIN)
            if len(bad) == 0:
                break
            for s, a in bad:
                st['pos'][s, c, a] = draw_pos(s)
                if teacher:
                    ext['teacher_pos'][s, n, a] = draw_pos(s)
        else:
            raise AssertionError('generator could not clear the grid margin')
    _CASES[name, seed] = (st, ext, t)
    return _CASES[name, seed]


def _tie_lattice(G, rng):
    """the G innermost points of the lattice of spacing 2, shuffled"""
    h = int(math.ceil(math.sqrt(G / math.pi))) + 2
    ij = np.mgrid[-h:h + 1, -h:h + 1].reshape(2, -1).T
    keep = np.lexsort((np.arange(len(ij)), (ij ** 2).sum(1)))[:G]
    return (ij[keep][rng.permutation(G)] * 2).astype(np.float32)


def _place_ties(st, ext, n, rng):
    """every value of the search exact in fp32: the ego's teacher pose at integer coordinates with heading float32(pi / 2) (the frame
    rotation is then by exactly 0), every other row's at integer offsets of at most 9 from it, teacher_grid -2 everywhere (the search
    decides).  A row at (odd, even) or (even, odd) is equidistant from 2 cells, at (odd, odd) from 4.  The cell order is then
    rearranged so that the two cells of four 2-way rows have indices 64 apart (the same lane) and those of four others sit in
    different lanes with the lower index in the higher lane."""
    S, A_cap = st['S'], st['A_cap']
    ext['teacher_grid'][:] = -2
    ext['teacher_state'][:, n] = np.where(ext['teacher_state'][:, n] == INVALID, VALID, ext['teacher_state'][:, n])
    for s in range(S):
        av = int(st['av_index'][s])
        e = rng.integers(-150, 150, 2)
        off = rng.integers(-9, 10, (A_cap, 2))
        off[av] = 0
        ext['teacher_pos'][s, n] = (e + off).astype(np.float32)
        ext['teacher_head'][s, n, av] = np.float32(math.pi / 2)
    g = st['grid_xy']
    index_of = lambda p: int(np.nonzero((g == np.asarray(p, np.float32)).all(1))[0][0])
    used = set()

    def put(cell_xy, index):                      # move the cell at cell_xy to `index` by swapping
        i = index_of(cell_xy)
        g[[i, index]] = g[[index, i]]
        used.update((index,))
    s, av = 0, int(st['av_index'][0])
    e = ext['teacher_pos'][0, n, av].astype(np.int64)
    rows = [a for a in range(int(st['n_agents'][0])) if a != av][:8]
    for k, a in enumerate(rows):
        odd = (2 * (k % 4) + 1) * (1 if k % 2 else -1)
        off = np.asarray([odd, 2 * (k - 3)]) if k < 4 else np.asarray([2 * (k - 6), 2 * (k - 4) + 3])      # 2-way ties, disjoint cells
        ext['teacher_pos'][0, n, a] = (e + off).astype(np.float32)
        # in the ego frame (rotation by 0) the row sits at `off`: its two nearest cells differ by +-1 in the odd coordinate
        d = np.asarray([1, 0]) if k < 4 else np.asarray([0, 1])
        lo, hi = (3 + k, 3 + k + 64) if k < 4 else (70 + k, 10 + k)                               # same lane / lower index in the higher lane
        put(off - d, min(lo, hi))
        put(off + d, max(lo, hi))


def gen_rawfeat(seed=0):
    """-> (block, ext): S = 3, A_cap = 32, T = 4, G = 65, poses a random walk within +-200 m (steps up to 12 m, some of exactly 0).
    Scene 0 starts with hand-set rows over columns 0, 1, 2 - previous INVALID and current valid, previous valid and current
    INVALID, both INVALID, ENTER at column 0, tokens -1 and -2, grid -1, catflag 0 and 1 - the rest is random over the same values;
    rows >= n_agents are gathered like any other row and hold valid indices"""
    if ('rawfeat', seed) in _CASES:
        return _CASES['rawfeat', seed]
    rng = np.random.default_rng([seed, 515])
    S, A_cap, T, G = 3, 32, 4, 65
    st = new_state(S, A_cap, T, 32, G=G)
    st['n_agents'][:] = [32, 17, 1]
    p = rng.uniform(-150, 150, (S, 1, A_cap, 2)) + np.cumsum(rng.uniform(-8.5, 8.5, (S, T, A_cap, 2)), 1)
    st['pos'][:] = p.astype(np.float32)
    st['pos'][:, 2, 5::6] = st['pos'][:, 1, 5::6]                 # stationary rows
    st['head'][:] = rng.uniform(-math.pi, math.pi, st['head'].shape).astype(np.float32)
    st['state'][:] = rng.choice([INVALID, VALID, VALID, ENTER, EXIT], st['state'].shape)
    st['token'][:] = rng.integers(-2, TOKEN_SIZE, st['token'].shape)
    st['token'][:, :, 3::7], st['token'][:, :, 4::7] = -1, -2
    st['grid'][:] = rng.integers(-1, G, st['grid'].shape)
    st['grid'][:, :, 2::5] = -1
    st['catflag'][:] = rng.integers(0, 2, st['catflag'].shape)
    st['type'][:] = rng.integers(0, 3, st['type'].shape)
    hand = [(VALID, VALID, VALID), (INVALID, VALID, INVALID), (INVALID, INVALID, VALID), (ENTER, VALID, EXIT),
            (VALID, INVALID, INVALID), (EXIT, ENTER, VALID), (INVALID, ENTER, INVALID)]
    for a, states in enumerate(hand):
        st['state'][0, :3, a] = states
        st['type'][0, a] = a % 3
        st['catflag'][0, :3, a] = (a % 2, 1 - a % 2, a % 2)
    st['token'][0, :3, 0], st['token'][0, :3, 1], st['grid'][0, :3, 2] = (-1, -2, 5), (-2, -1, 0), (-1, 7, -1)
    st['token'][0, :3, 3], st['token'][0, :3, 4], st['token'][0, :3, 5] = (0, TOKEN_SIZE - 1, -1), (TOKEN_SIZE - 1, 0, 0), (3, 3, TOKEN_SIZE - 1)
    st['token'][0, :3, 6] = (-1, -2, 0)
    st['grid'][0, :3, 3], st['grid'][0, :3, 4], st['grid'][0, :3, 5] = (G - 1, 0, -1), (0, G - 1, G - 1), (G - 1, 0, 0)
    ext = new_step_ext(st, scratch=True)
    rows = S * A_cap
    ext['tok_tab'] = rng.standard_normal((3, TOKEN_SIZE + 2, EMB)).astype(np.float32)
    ext['grid_tab'] = rng.standard_normal((G + 1, EMB)).astype(np.float32)
    ext['state_emb'] = rng.standard_normal((4, EMB)).astype(np.float32)
    ext['cat_agent'] = (rng.standard_normal((rows, EMB)) * 0.1).astype(np.float32)
    ext['cat_seed'] = (rng.standard_normal(EMB) * 0.1).astype(np.float32)
    _CASES['rawfeat', seed] = (st, ext)
    return _CASES['rawfeat', seed]


def take_step_scenes(st, ext, scenes):
    """the block and ext of a list of scenes (repeats allowed): every per-scene array gathered, the shared ones kept"""
    scenes = np.asarray(list(scenes))
    S, A_cap = st['S'], st['A_cap']
    o_st, o_ext = dict(st), dict(ext)
    o_st['S'] = len(scenes)
    for d, o in ((st, o_st), (ext, o_ext)):
        for k, v in d.items():
            if not isinstance(v, np.ndarray) or k in ('grid_xy', 'vocab', 'tok_tab', 'grid_tab', 'state_emb', 'cat_seed', 'map_pos',
                                                      'map_orient', 'n_map'):
                continue
            if v.shape[0] == S * A_cap and k not in ('n_agents', 'av_index'):
                o[k] = np.ascontiguousarray(v.reshape((S, A_cap) + v.shape[1:])[scenes].reshape((-1,) + v.shape[1:]))
            else:
                assert v.shape[0] == S, k
                o[k] = np.ascontiguousarray(v[scenes])
    return o_st, o_ext


# ------------------------------------------------------------------------------------------------ teacher-forced forward: edge builder, motion features
def pack_lists(lists, e_base=0, f=np.float32):
    """reference lists [(src, raw, ...)] as a compact CSR in list order: (off, cnt, src, raw [total][4] in f, total); off carries
    e_base, src / raw start at the zone's first edge"""
    cnt = np.asarray([len(r[0]) for r in lists], np.int64)
    off = e_base + np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    src = np.concatenate([np.asarray(r[0], np.int64) for r in lists] + [np.zeros(0, np.int64)])
    raw = np.concatenate([np.asarray(r[1], f).reshape(-1, 4) for r in lists] + [np.zeros((0, 4), f)])
    pad_i, pad_f = np.zeros(e_base, np.int64), np.zeros((e_base, 4), f)
    return off, cnt, np.concatenate([pad_i, src]), np.concatenate([pad_f, raw]), total


RADIUS_EDGES_MUTANTS = ('filtered_not_counted', 'le_radius', 'pair_abs_index', 'index_diff_sign', 'rule1_dst_dth', 'rule2_keep_dth',
                        'bearing_pre_override')
_GAP_KIND = {0: 'point', 1: 'agent', 2: 'map'}


def radius_edges_ref(case, f=np.float64, mutate=None):
    """infgen_radius_edges (include/infgen_hip.h, "edge sets of the teacher-forced forward"; agent_decoder.py:632, :710, :780, :875,
    map_decoder.py:91 with the filters the reference applies after the radius call, gap rules :595-601 / :722-723) of a case dict
    (gen_radius_edges: the fields of InfgenRadiusEdges as numpy arrays or None, n_nodes).  Per query q: candidates [q_c0, q_c1) in
    ascending index, the first K with d^2 < r^2 (strict) are found; of those the ones with index != q_self, c_ok[index] and
    pair_ok[q_pair_off + index - q_c0] (q_pair_off < 0: no pair filter) are emitted with src = c_src[index] (else the index) and
    raw = (|d|, bearing in the query's heading frame, wrap(c_head - p_head), index_diff ? index - q_pt : 0), gap_rule 1 = edge_raw's
    'agent', 2 = 'map', 0 = 'point'.  Which candidates are found is decided in float64; f is the type of the features.
    -> ([(src in order, raw [n][4], ruled bits)] per destination NODE (nodes without a query: empty), the smallest relative gap
    |d^2 - r^2| / r^2 of any (query, candidate) pair).
    mutate: one deliberate deviation, for the tests that show the cases tell it apart - 'filtered_not_counted' (the filters run
    before the K cap), 'le_radius' (d^2 <= r^2), 'pair_abs_index' (pair_ok read at q_pair_off + index), 'index_diff_sign',
    'rule1_dst_dth' (gap rule 1, destination invalid only: dth = the gap too), 'rule2_keep_dth' (gap rule 2 leaves dth),
    'bearing_pre_override' (the bearing of d before a gap rule replaced it)."""
    assert mutate is None or mutate in RADIUS_EDGES_MUTANTS
    g = case
    K, kind, r = int(g['K']), _GAP_KIND[g['gap_rule']], float(g['radius'])
    empty = (np.zeros(0, np.int64), np.zeros((0, 4), f), np.zeros(0, np.int8))
    out, gap = [empty] * g['n_nodes'], math.inf
    opt = lambda k, i, d: d if g[k] is None else g[k][i]
    for q in range(len(g['q_node'])):
        node, qp, c0, c1 = (int(g[k][q]) for k in ('q_node', 'q_pt', 'q_c0', 'q_c1'))
        idx = np.arange(c0, c1)
        centre = g['p_pos'][qp]
        found, gq = first_k_within(centre, g['c_pos'][c0:c1], r, 10 ** 9 if mutate == 'filtered_not_counted' else K)
        gap = min(gap, gq)
        if mutate == 'le_radius':
            cand = g['c_pos'][c0:c1].astype(np.float64).reshape(-1, 2)
            d2 = (float(centre[0]) - cand[:, 0]) ** 2 + (float(centre[1]) - cand[:, 1]) ** 2
            found = np.nonzero(d2 <= r * r)[0][:K]
        m = idx[found]
        keep = np.ones(len(m), bool)
        if g['q_self'] is not None:
            keep &= m != int(g['q_self'][q])
        if g['c_ok'] is not None:
            keep &= g['c_ok'][m] != 0
        if g['pair_ok'] is not None and g['q_pair_off'] is not None and g['q_pair_off'][q] >= 0:
            at = int(g['q_pair_off'][q]) + (m if mutate == 'pair_abs_index' else m - c0)
            keep &= g['pair_ok'].reshape(-1)[at % g['pair_ok'].size] != 0           # (the modulus only keeps the mutant inside the array)
        m = m[keep]
        if mutate == 'filtered_not_counted':
            m = m[:K]
        if len(m) == 0:
            continue
        assert out[node] is empty, 'two queries of one destination node'
        dpose = (g['p_pos'][qp, 0], g['p_pos'][qp, 1], g['p_head'][qp])
        spose = (g['c_pos'][m, 0], g['c_pos'][m, 1], g['c_head'][m])
        d_inv, s_inv = bool(opt('p_inv', qp, 0)), np.asarray(opt('c_inv', m, np.zeros(len(m), np.uint8))) != 0
        raw, ruled = edge_raw(dpose, spose, d_inv, s_inv, kind, f=f)
        plain = edge_raw(dpose, spose, False, False, 'point', f=f)[0]
        if mutate == 'rule1_dst_dth' and kind == 'agent' and d_inv:
            raw[~s_inv, 2] = f(HEADING_GAP)
        if mutate == 'rule2_keep_dth' and kind == 'map':
            raw[:, 2] = plain[:, 2]
        if mutate == 'bearing_pre_override':
            raw[:, 1] = plain[:, 1]
        if g['index_diff']:
            raw[:, 3] = ((qp - m) if mutate == 'index_diff_sign' else (m - qp)).astype(f)
        out[node] = (np.asarray(opt('c_src', m, m), np.int64), raw, ruled)
    return out, gap


MOTION_FEATURES_MUTANTS = ('swap_invalid_and_leave', 'gap_mask_first', 't0_reads_previous_row', 'no_gap_mask')


def motion_features_ref(pos, head, state, gap_mask, f=np.float64, mutate=None, with_ruled=False):
    """infgen_motion_features (_build_vector_a, agent_decoder.py:426-447, gap mask :1327) of agent-major [rows][T] arrays: the motion
    vector pos[t] - pos[t - 1], (0, 0) at t = 0; then, in this order, (1) INVALID: (-2, -2), (2) previous INVALID and this not -
    at t = 0: state == ENTER - : (1, 1), (3) t > 0, previous not INVALID and this INVALID: (-1, -1), (4) gap_mask: (1, 1).
    -> [rows][T][4] = (norm, angle(head vector, motion vector), 0, 0) [, ruled [rows][T]: 1 the motion is a rule's (+-1, +-1), 2
    (-2, -2): the norm is then the rounded root of 2 or 8].
    mutate: 'swap_invalid_and_leave' (rule 3 before rule 1), 'gap_mask_first' (rule 4 before the others), 't0_reads_previous_row'
    (column 0 treated like any other column of the flat arrays: it reads the previous row's last column), 'no_gap_mask'."""
    assert mutate is None or mutate in MOTION_FEATURES_MUTANTS
    pos, state = np.asarray(pos), np.asarray(state)
    rows, T = state.shape
    p = pos.astype(f).reshape(rows * T, 2)
    st = state.reshape(-1)
    first = np.arange(rows * T) % T == 0
    if mutate == 't0_reads_previous_row':
        first = np.arange(rows * T) == 0
    prev = np.maximum(np.arange(rows * T) - 1, 0)
    m = np.where(first[:, None], f(0), p - p[prev])
    inv = st == INVALID
    pinv = np.where(first, False, st[prev] == INVALID)
    enter = np.where(first, st == ENTER, pinv & ~inv)
    leave = ~first & ~pinv & inv
    gm = np.zeros(rows * T, bool) if gap_mask is None or mutate == 'no_gap_mask' else np.asarray(gap_mask).reshape(-1) != 0
    rules = [(inv, INVALID_MOTION, 2), (enter, MOTION_GAP, 1), (leave, -MOTION_GAP, 1), (gm, MOTION_GAP, 1)]
    if mutate == 'swap_invalid_and_leave':
        rules = [rules[2], rules[1], rules[0], rules[3]]
    if mutate == 'gap_mask_first':
        rules = [rules[3]] + rules[:3]
    ruled = np.zeros(rows * T, np.int8)
    for mask, value, bit in rules:
        m = np.where(mask[:, None], f(value), m)
        ruled = np.where(mask, bit, ruled).astype(np.int8)
    h = np.asarray(head).astype(f).reshape(-1)
    hc, hs = np.cos(h), np.sin(h)
    mx, my = m[:, 0], m[:, 1]
    out = np.stack([np.sqrt(mx * mx + my * my), np.arctan2(hc * my - hs * mx, (f(0) + hc * mx) + hs * my),
                    np.zeros(rows * T, f), np.zeros(rows * T, f)], -1).astype(f).reshape(rows, T, 4)
    return (out, ruled.reshape(rows, T)) if with_ruled else out


# Largest error of a plain fp32 numpy evaluation of motion_features_ref against float64 over gen_motion_features (all shapes, with
# and without the gap mask): norm [m], angle [rad].  The figures tests/test_graph_ref_cpu.py measures, rounded up in the fourth
# digit; the device bar is four times the figure, as above.  (Apart from FP32_ERR_MOTION_NORM / _BEARING of the rollout's raw
# feature: the last column of these rows jumps by up to 300 m.)
FP32_ERR_MOTION_FEAT_NORM, FP32_ERR_MOTION_FEAT_ANGLE = 2.363e-5, 2.863e-7
BAR_MOTION_FEAT_NORM, BAR_MOTION_FEAT_ANGLE = 4 * FP32_ERR_MOTION_FEAT_NORM, 4 * FP32_ERR_MOTION_FEAT_ANGLE



def compare_motion(got, ref, ruled):
    """what the GPU test asserts of infgen_motion_features' fp32 output [rows][T][4] against motion_features_ref(with_ruled=True):
    columns 2 and 3 exactly 0, the norm of a ruled motion exactly float32(sqrt 2) / float32(2 sqrt 2), norm and angle within the
    bars.  -> the largest errors (norm, angle)"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got[..., 2:].view(np.int32), np.zeros(got[..., 2:].shape, np.int32)), 'columns 2 and 3 are not +0'
    want = np.where(ruled == 2, np.float32(math.sqrt(8.0)), np.float32(math.sqrt(2.0)))
    assert np.array_equal(got[..., 0][ruled != 0], want[ruled != 0]), 'the norm of a rule constant is not exact'
    e = np.asarray([np.abs(got[..., 0].astype(np.float64) - ref[..., 0]).max(), ang_err(got[..., 1], ref[..., 1]).max()])
    assert e[0] <= BAR_MOTION_FEAT_NORM and e[1] <= BAR_MOTION_FEAT_ANGLE, e
    return e


RADIUS_EDGES_CASES = {
    # name: (radius, K, gap_rule, index_diff, what it is for) - the forward's use it stands for in forward_engine.py
    'temporal': (1e30, 12, 1, 1, '5 agents x 20 columns, window 12: r * r overflows in fp32, history mask, permuted node map, empty ranges'),
    'agent': (60.0, 301, 1, 0, 'scenes of 1 / 70 / 330 agents in one launch: self dropped, the cap truncates after several chunks'),
    'seed_pair': (50.0, 300, 0, 0, 'per-pair filter with per-query offsets (some -1); the upper zone of a shared buffer'),
    'map': (30.0, 5, 2, 0, '200 map tokens per scene (one scene without): no candidate validity, queries valid and invalid'),
    'map_graph': (20.0, 101, 0, 0, 'the map-token graph: no validity arrays at all, self dropped, scenes of 150 tokens and 1'),
}


def _new_radius_case(name, n_nodes, **kw):
    radius, K, gap_rule, index_diff, _ = RADIUS_EDGES_CASES[name]
    g = dict(name=name, n_nodes=n_nodes, radius=float(np.float32(radius)), K=K, gap_rule=gap_rule, index_diff=index_diff, e_base=0,
             q_self=None, q_pair_off=None, p_inv=None, c_inv=None, c_ok=None, c_src=None, pair_ok=None)
    g.update(kw)
    for k in ('q_node', 'q_pt', 'q_c0', 'q_c1', 'q_self', 'q_pair_off', 'c_src'):
        if g[k] is not None:
            g[k] = np.ascontiguousarray(g[k], np.int32)
    for k in ('p_inv', 'c_inv', 'c_ok', 'pair_ok'):
        if g[k] is not None:
            g[k] = np.ascontiguousarray(g[k], np.uint8)
    for k in ('p_pos', 'p_head', 'c_pos', 'c_head'):
        if k in g:
            g[k] = np.ascontiguousarray(g[k], np.float32)
    return g


def _disc(rng, n, radius):
    ang, rad = rng.uniform(0, 2 * math.pi, n), radius * np.sqrt(rng.uniform(0, 1, n))
    return np.stack([rad * np.cos(ang), rad * np.sin(ang)], -1)


def gen_radius_edges(name, seed=0):
    """-> the case dict of a RADIUS_EDGES_CASES entry: the arrays of InfgenRadiusEdges (None: a null pointer), n_nodes (rows of off /
    cnt), e_base.  Coordinates within +-200 m; every (query, candidate) pair clears MARGIN.  Cached: do not write to the result."""
    if ('radius_edges', name, seed) in _CASES:
        return _CASES['radius_edges', name, seed]
    rng = np.random.default_rng([seed, sum(map(ord, name)), 31])
    r = float(np.float32(RADIUS_EDGES_CASES[name][0]))
    heads = lambda n: rng.uniform(-math.pi, math.pi, n).astype(np.float32)
    if name == 'temporal':
        A, T, W, N = 5, 20, 12, 7                 # N rows per column: the agents and two rows that are never a destination
        pos = (rng.uniform(-150, 150, (A, 1, 2)) + np.cumsum(rng.uniform(-2.5, 2.5, (A, T, 2)), 1)).astype(np.float32)
        inv = rng.uniform(size=(A, T)) < 0.4
        hist = rng.uniform(size=(A, T)) > 0.25
        hist[:, 0] = [1, 1, 0, 1, 1]
        hist[2, :4] = 0                           # an agent whose history starts late
        rowp = rng.permutation(N)[:A]
        node_of = np.arange(T)[None, :] * N + rowp[:, None]
        qa, qj = np.nonzero(hist)
        g = _new_radius_case(name, T * N, q_node=node_of[qa, qj], q_pt=qa * T + qj, q_c0=qa * T + np.maximum(qj - W, 0), q_c1=qa * T + qj,
                             p_pos=pos.reshape(-1, 2), p_head=heads(A * T), p_inv=inv.reshape(-1), c_ok=hist.reshape(-1),
                             c_src=node_of.reshape(-1))
        g['c_pos'], g['c_head'], g['c_inv'] = g['p_pos'], g['p_head'], g['p_inv']
    elif name == 'agent':
        sizes = [1, 70, 330]
        start = np.concatenate([[0], np.cumsum(sizes)])
        n = int(start[-1])
        pos = np.zeros((n, 2), np.float32)
        for s, A in enumerate(sizes):
            centre = rng.uniform(-100, 100, 2)

            def draw(k, A=A, centre=centre):
                if A == 330:                      # 312 rows within 25 m of the centre (all inside each other's radius), 18 far out
                    nc = 312 if k is None else k
                    p = centre + _disc(rng, nc, 25.0)
                    if k is None:
                        p = np.concatenate([p, centre + rng.uniform(-95, 95, (A - nc, 2))])[rng.permutation(A)]
                    return p.astype(np.float32)
                return (centre + rng.uniform(-80, 80, (A if k is None else k, 2))).astype(np.float32)
            pos[start[s]:start[s + 1]] = _resample(rng, draw, _cloud_offenders(r))
        ok = rng.uniform(size=n) > 0.12
        ok[0] = True
        if ok.sum() % 4 == 0:
            ok[start[2] + 5] = not ok[start[2] + 5]
        qd = np.nonzero(ok)[0]
        scene = np.searchsorted(start, qd, side='right') - 1
        inv = rng.uniform(size=n) < 0.3
        g = _new_radius_case(name, n, q_node=qd, q_pt=qd, q_c0=start[scene], q_c1=start[scene + 1], q_self=qd, p_pos=pos, p_head=heads(n),
                             p_inv=inv, c_ok=ok)
        g['c_pos'], g['c_head'], g['c_inv'] = g['p_pos'], g['p_head'], g['p_inv']
    elif name == 'seed_pair':
        NS, sizes = 3, [40, 90]                   # scene-contiguous rows: the agents, then NS seed rows at the ego's pose
        grp = np.concatenate([[0], np.cumsum([A + NS for A in sizes])])
        n = int(grp[-1])
        pos, is_agent = np.zeros((n, 2), np.float32), np.zeros(n, bool)
        for s, A in enumerate(sizes):
            centre = rng.uniform(-80, 80, 2)
            ego = rng.integers(0, A)
            ext = 45.0 if s == 0 else 90.0

            def draw(k, A=A, centre=centre, ext=ext):
                return (centre + rng.uniform(-ext, ext, (A if k is None else k, 2))).astype(np.float32)

            def offenders(p, ego=ego):            # the seed rows sit at the ego: only the distances to the ego decide
                d2 = ((p.astype(np.float64) - p[ego].astype(np.float64)[None]) ** 2).sum(-1)
                bad = _pairs_near(d2, r)
                return np.nonzero(bad)[0]
            p = _resample(rng, draw, offenders)
            pos[grp[s]:grp[s] + A] = p
            pos[grp[s] + A:grp[s + 1]] = p[ego]
            is_agent[grp[s]:grp[s] + A] = True
        ok = is_agent & (rng.uniform(size=n) > 0.1)
        qs = np.nonzero(~is_agent)[0]
        scene = np.searchsorted(grp, qs, side='right') - 1
        width = max(sizes) + NS
        pair = (rng.uniform(size=(len(qs), width)) > 0.35).astype(np.uint8)
        pair_off = np.arange(len(qs)) * width
        pair_off[[1, 4]] = -1                     # one seed row of each scene without a pair filter
        g = _new_radius_case(name, n, q_node=qs, q_pt=qs, q_c0=grp[scene], q_c1=grp[scene + 1], q_pair_off=pair_off, p_pos=pos,
                             p_head=heads(n), p_inv=rng.uniform(size=n) < 0.3, c_ok=ok, pair_ok=pair, e_base=1000)
        g['c_pos'], g['c_head'], g['c_inv'] = g['p_pos'], g['p_head'], g['p_inv']
    elif name == 'map':
        n_map, n_ag = [200, 0, 200], [12, 9, 6]
        mp = np.concatenate([[0], np.cumsum(n_map)])
        ag = np.concatenate([[0], np.cumsum(n_ag)])
        M, n = int(mp[-1]), int(ag[-1])
        map_pos, pos = np.zeros((M, 2), np.float32), np.zeros((n, 2), np.float32)
        for s in range(3):
            centre = rng.uniform(-60, 60, 2)
            map_pos[mp[s]:mp[s + 1]] = (centre + rng.uniform(-90, 90, (n_map[s], 2))).astype(np.float32)
            fixed = map_pos[mp[s]:mp[s + 1]]

            def draw(k, s=s, centre=centre):
                return (centre + rng.uniform(-125, 125, (n_ag[s] if k is None else k, 2))).astype(np.float32)
            pos[ag[s]:ag[s + 1]] = _resample(rng, draw, _cloud_offenders(r, fixed, r, self_pairs=False))
        scene = np.repeat(np.arange(3), n_ag)
        inv = np.arange(n) % 3 == 1
        g = _new_radius_case(name, n + 3, q_node=np.arange(n), q_pt=np.arange(n), q_c0=mp[scene], q_c1=mp[scene + 1], p_pos=pos,
                             p_head=heads(n), p_inv=inv, c_pos=map_pos, c_head=heads(M))
    else:
        assert name == 'map_graph'
        sizes = [150, 1]
        start = np.concatenate([[0], np.cumsum(sizes)])
        n = int(start[-1])
        pos = np.zeros((n, 2), np.float32)
        for s, Mn in enumerate(sizes):
            centre = rng.uniform(-100, 100, 2)

            def draw(k, Mn=Mn, centre=centre):
                if Mn == 150:                     # 115 tokens within 8 m of the centre, 35 spread out
                    nc = 115 if k is None else k
                    p = centre + _disc(rng, nc, 8.0)
                    if k is None:
                        p = np.concatenate([p, centre + rng.uniform(-95, 95, (Mn - nc, 2))])[rng.permutation(Mn)]
                    return p.astype(np.float32)
                return (centre + rng.uniform(-95, 95, (Mn if k is None else k, 2))).astype(np.float32)
            pos[start[s]:start[s + 1]] = _resample(rng, draw, _cloud_offenders(r))
        scene = np.repeat(np.arange(2), sizes)
        g = _new_radius_case(name, n, q_node=np.arange(n), q_pt=np.arange(n), q_c0=start[scene], q_c1=start[scene + 1], q_self=np.arange(n),
                             p_pos=pos, p_head=heads(n))
        g['c_pos'], g['c_head'] = g['p_pos'], g['p_head']
    _CASES['radius_edges', name, seed] = g
    return g


def gen_strict_radius_edges():
    """gen_strict_radius's exact-coordinate points as infgen_radius_edges cases: one query at the origin over all five points, self
    dropped.  -> [(case, index of the point at exactly the rounded radius, present?)]; the margin does not hold here by design"""
    pts, cases = gen_strict_radius()
    n = len(pts)
    out = []
    for r, i, present in cases:
        g = dict(name='strict', n_nodes=1, radius=float(r), K=16, gap_rule=0, index_diff=0, e_base=0, q_self=np.zeros(1, np.int32),
                 q_pair_off=None, p_inv=None, c_inv=None, c_ok=None, c_src=None, pair_ok=None, q_node=np.zeros(1, np.int32),
                 q_pt=np.zeros(1, np.int32), q_c0=np.zeros(1, np.int32), q_c1=np.full(1, n, np.int32), p_pos=pts.copy(),
                 p_head=np.zeros(n, np.float32), c_pos=pts.copy(), c_head=np.zeros(n, np.float32))
        out.append((g, i, present))
    return out


MOTION_FEATURES_SHAPES = [(7, 1), (3, 2), (37, 19)]


def gen_motion_features(seed=0):
    """-> [dict(pos [rows][T][2], head, state, gap_mask)] for MOTION_FEATURES_SHAPES (37 * 19 = 703 elements: not a multiple of the
    256-thread workgroup).  Poses a random walk within +-60 m of the origin with steps up to 9 m, the last column of every row a
    jump to the far side (|coordinate| up to 200 m): a column 0 that reads across the row boundary shows.  States over all four
    values with hand-set rows, so that every rule, every pair of rules that can coincide and EXIT occur at t = 0 and at t > 0; the
    gap mask (the GPU test also runs without it) hits every rule.  Cached: do not write to the result."""
    if ('motion_features', seed) in _CASES:
        return _CASES['motion_features', seed]
    out = []
    for rows, T in MOTION_FEATURES_SHAPES:
        rng = np.random.default_rng([seed, rows, T, 808])
        pos = rng.uniform(-60, 60, (rows, 1, 2)) + np.cumsum(rng.uniform(-9, 9, (rows, T, 2)), 1)
        far = np.where(pos[:, -1] >= 0, -1.0, 1.0) * rng.uniform(120, 200, (rows, 2))
        pos[:, -1] = far
        state = rng.choice([INVALID, VALID, VALID, ENTER, EXIT], (rows, T))
        gm = rng.uniform(size=(rows, T)) < 0.25
        # hand-set heads of rows: (state at t = 0, mask at t = 0[, state at t = 1, mask at t = 1])
        hand = [(INVALID, 0, VALID, 0), (VALID, 0, INVALID, 0), (ENTER, 0, EXIT, 0), (EXIT, 0, INVALID, 1), (INVALID, 1, INVALID, 1),
                (ENTER, 1, VALID, 1), (VALID, 1, EXIT, 1), (INVALID, 0, ENTER, 1), (EXIT, 1, EXIT, 0), (INVALID, 0, INVALID, 0)]
        for a, hs in enumerate(hand[:rows]):
            state[a, 0], gm[a, 0] = hs[0], hs[1]
            if T > 1:
                state[a, 1], gm[a, 1] = hs[2], hs[3]
        out.append(dict(pos=pos.astype(np.float32), head=rng.uniform(-math.pi, math.pi, (rows, T)).astype(np.float32),
                        state=state.astype(np.int32), gap_mask=gm.astype(np.uint8)))
    _CASES['motion_features', seed] = out
    return out
