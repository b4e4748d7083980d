"""numpy restatement of the insertion rules of include/infgen_hip.h ("INSERTION RULES"): the cell verdicts of k_insert_cell_mask and
the decision under them (k_insert_decide<true, true>).  ``cell_verdicts(case, s, f)`` follows the header operation by operation in
the float type ``f``: np.float32 is the kernel's own arithmetic (up to the last bits of cosf / sinf), np.float64 the reference the
GPU tests compare with.  Next to each verdict it returns the cell's MARGIN: the smallest |distance - threshold| over every
comparison of a distance rule that the cell took part in - a cell whose margin is below BAND may fall either way on the device.
Not a test module; imports graph_ref for the decision's shared pieces and leaves it alone."""
import math

import numpy as np

import graph_ref as gr

BAND = 1e-4                 # metres: the header's "may fall either way"
BAND_SHARE = 0.005          # at most this share of a case's cells may sit in the band (the generators are checked against it)
KEEPOUT, CLEARANCE, EDGES, LANES, ZONES = 1, 2, 4, 8, 16
INVALID = 0


def words_for(G):
    """32-bit words of one scene's set: ceil(G / 32) rounded up to a multiple of 4"""
    return (G + 127) // 128 * 4


def pack_bits(ok, W=None):
    """bool [..., G] -> uint32 [..., W], bit g of word g // 32 (little-endian inside the word), bits >= G zero"""
    ok = np.asarray(ok, bool)
    G = ok.shape[-1]
    W = words_for(G) if W is None else W
    pad = np.zeros(ok.shape[:-1] + (32 * W,), bool)
    pad[..., :G] = ok
    b = pad.reshape(ok.shape[:-1] + (W, 32)).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def unpack_bits(words, G):
    """uint32 [..., W] -> bool [..., G]; also returns whether every bit at a position >= G is zero"""
    w = np.asarray(words).astype(np.uint32)
    bits = ((w[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool).reshape(w.shape[:-1] + (-1,))
    return bits[..., :G], not bits[..., G:].any()


def new_rules(**kw):
    """a rule set in the kernel's terms; None switches a rule off.  keepout (back, front, half_width); clearance; edge_clearance
    with records [S0][rec_cap][8] / n_records [S0]; near_lane (dist, types) with map_pos [S0][M_cap][2] / map_type [S0][M_cap] /
    n_map [S0]; zones [S0][Z][4] / n_zones [S0]; copies"""
    r = dict(keepout=None, clearance=None, edge_clearance=None, records=None, n_records=None, near_lane=None, map_pos=None,
             map_type=None, n_map=None, zones=None, n_zones=None, copies=1)
    assert set(kw) <= set(r), set(kw) - set(r)
    r.update(kw)
    return r


def rule_bits(rules):
    return (KEEPOUT * (rules['keepout'] is not None) | CLEARANCE * (rules['clearance'] is not None)
            | EDGES * (rules['edge_clearance'] is not None) | LANES * (rules['near_lane'] is not None) | ZONES * (rules['zones'] is not None))


def lane_type_mask(types):
    m = 0
    for t in types:
        assert 0 <= int(t) < 32
        m |= 1 << int(t)
    return m


def in_scene(st, s, c):
    """bool [A_cap]: the rows of scene s that are in the scene at column c"""
    A_cap = st['A_cap']
    n = min(max(int(st['n_agents'][s]), 0), A_cap)
    return (np.arange(A_cap) < n) & (np.asarray(st['state'][s, c]) != INVALID)


def _rot(dx, dy, cs, sn):
    return dx * cs + dy * sn, dy * cs - dx * sn


def cell_verdicts(st, shape, rules, s, c, f=np.float64):
    """-> dict(static [G] bool: no static rule bans the cell, allowed [G] bool, margin [G] float64, live int) of scene s at column c.
    st: a graph_ref block (pos [S][T][A_cap][2], head, state, n_agents, av_index, grid_xy); shape [S * A_cap][3]."""
    A_cap = st['A_cap']
    grid = np.asarray(st['grid_xy'], f)
    gx, gy = grid[:, 0], grid[:, 1]
    G = grid.shape[0]
    ms = s // rules['copies']
    av = min(max(int(st['av_index'][s]), 0), A_cap - 1)
    pos, head = np.asarray(st['pos'][s, c]), np.asarray(st['head'][s, c])
    # the exact difference is formed in the stored precision's own terms: float32 inputs subtract exactly enough in either type,
    # but the float64 reference subtracts the float32 VALUES (no rounding at all)
    e = pos[av].astype(f)
    eh = f(head[av])
    phi = eh - f(np.float32(math.pi / 2))
    cs, sn = np.cos(phi), np.sin(phi)
    ban = np.zeros(G, bool)
    margin = np.full(G, np.inf)

    def note(dist, thr):
        """fold |dist - thr| of a [G][N] comparison table into the cells' margins"""
        if dist.shape[1]:
            np.minimum(margin, np.abs(dist.astype(np.float64) - float(thr)).min(1), out=margin)

    if rules['keepout'] is not None:
        back, front, half = (f(v) for v in rules['keepout'])
        ban |= (-back <= gy) & (gy <= front) & (np.abs(gx) <= half)
    if rules['edge_clearance'] is not None:
        n = min(max(int(rules['n_records'][ms]), 0), rules['records'].shape[1])
        rec = np.asarray(rules['records'][ms, :n])
        rec = rec[rec[:, 7] >= 0]
        r = rec.astype(f)
        mx, my = _rot((r[:, 0] - e[0]) + r[:, 2], (r[:, 1] - e[1]) + r[:, 3], cs, sn)
        ux, uy = _rot(r[:, 4], r[:, 5], cs, sn)
        fx, fy = gx[:, None] - mx[None], gy[:, None] - my[None]
        al, ac = fx * ux + fy * uy, fy * ux - fx * uy
        ox = np.maximum(np.abs(al) - r[:, 6][None], f(0))
        dist = np.sqrt(ox * ox + ac * ac)
        thr = f(rules['edge_clearance'])
        ban |= (dist < thr).any(1)
        note(dist, thr)
    if rules['near_lane'] is not None:
        d, types = rules['near_lane']
        n = min(max(int(rules['n_map'][ms]), 0), rules['map_pos'].shape[1])
        ty = np.asarray(rules['map_type'][ms, :n])
        keep = np.isin(ty, [int(t) for t in types]) & (ty >= 0) & (ty < 32)
        mp = np.asarray(rules['map_pos'][ms, :n])[keep].astype(f)
        qx, qy = _rot(mp[:, 0] - e[0], mp[:, 1] - e[1], cs, sn)
        fx, fy = gx[:, None] - qx[None], gy[:, None] - qy[None]
        d2 = fx * fx + fy * fy
        ban |= ~(d2 <= f(d) * f(d)).any(1)
        note(np.sqrt(d2.astype(np.float64)), d)
    if rules['zones'] is not None:
        n = min(max(int(rules['n_zones'][ms]), 0), rules['zones'].shape[1])
        z = np.asarray(rules['zones'][ms, :n])
        live = np.isfinite(z[:, 2]) & (z[:, 2] > 0) & ((z[:, 3] == 0) | (z[:, 3] == 1))
        z = z[live]
        zf = z.astype(f)
        qx, qy = _rot(zf[:, 0] - e[0], zf[:, 1] - e[1], cs, sn)
        fx, fy = gx[:, None] - qx[None], gy[:, None] - qy[None]
        d2 = fx * fx + fy * fy
        inside = d2 <= (zf[:, 2] * zf[:, 2])[None]
        ban |= inside[:, z[:, 3] == 0].any(1)
        if (z[:, 3] == 1).any():
            ban |= ~inside[:, z[:, 3] == 1].any(1)
        if z.shape[0]:
            np.minimum(margin, np.abs(np.sqrt(d2.astype(np.float64)) - z[:, 2].astype(np.float64)[None]).min(1), out=margin)
    static = ~ban
    rows = in_scene(st, s, c)
    near = np.zeros(G, bool)
    if rules['clearance'] is not None:
        j = np.nonzero(rows)[0]
        p = pos[j].astype(f)
        qx, qy = _rot(p[:, 0] - e[0], p[:, 1] - e[1], cs, sn)
        hj = head[j].astype(f)
        ux, uy = _rot(np.cos(hj), np.sin(hj), cs, sn)
        sh = np.asarray(shape).reshape(-1, A_cap, 3)[s, j].astype(f)
        hl, hw = np.maximum(f(0.5) * sh[:, 0], f(0)), np.maximum(f(0.5) * sh[:, 1], f(0))
        fx, fy = gx[:, None] - qx[None], gy[:, None] - qy[None]
        lx, ly = fx * ux + fy * uy, fy * ux - fx * uy
        ox, oy = np.maximum(np.abs(lx) - hl, f(0)), np.maximum(np.abs(ly) - hw, f(0))
        dist = np.sqrt(ox * ox + oy * oy)
        thr = f(rules['clearance'])
        rr = (hl + hw) + thr
        reach = fx * fx + fy * fy < (rr * rr)[None]          # the circle test: a row beyond it is skipped
        near = ((dist < thr) & reach).any(1)
        note(dist, thr)
    return dict(static=static, allowed=static & ~near, margin=margin, live=int(rows.sum()))


def decide_mask_ref(st, dec, s, t, force_enter, max_new, sample_k, allowed, type_allowed, max_agents=None, live=None):
    """k_insert_decide<true, true> for scene s, in place on float64 / integer copies (graph_ref.as_ref) like
    graph_ref.insert_decide_ref: allowed bool [G] of the scene, type_allowed three ints, max_agents / live ints or None.
    With every cell and type allowed and no budget this is graph_ref.insert_decide_ref."""
    c, A_cap = 1 + t, st['A_cap']
    if not dec['active'][s]:
        dec['inserted'][s] = 0
        return
    lg = np.asarray(dec['lg_pos'][s], np.float64)
    cand = np.nonzero(np.asarray(allowed, bool) & ~np.isnan(lg))[0]
    if cand.size == 0:                                       # no cell: the scene stops, nothing else is touched
        dec['inserted'][s], dec['active'][s] = 0, 0
        return
    k = min(max(sample_k, 1), cand.size)
    cell = int(cand[gr.topk_pick(lg[cand], k, dec['uniform'][s])[0]])
    enter = bool(dec['lg_state'][s, 1] > dec['lg_state'][s, 0]) or bool(force_enter)
    if max_agents is not None and live >= max_agents:
        enter = False
    ty = -1
    for j in range(3):
        if type_allowed[j] and (ty < 0 or dec['lg_type'][s, j] > dec['lg_type'][s, ty]):
            ty = j
    assert ty >= 0, 'a rule set without a type is refused at configuration time'
    occupied = dec['occ'][s, cell] != 0
    A = int(st['n_agents'][s])
    if occupied and sample_k > 1:
        dec['inserted'][s] = 0
        return
    ok = enter and not occupied and dec['n_new'][s] + 1 <= max_new
    if ok and A >= A_cap:
        dec['inserted'][s], dec['active'][s] = -1, 0
        return
    if not ok:
        dec['inserted'][s], dec['active'][s] = 0, 0
        return
    av = int(st['av_index'][s])
    ego = (st['pos'][s, c, av, 0], st['pos'][s, c, av, 1], st['head'][s, c, av])
    nx, ny = gr.decode_pos(st['grid_xy'][cell], ego)
    row = s * A_cap + A
    st['pos'][s, :, A] = 0.0
    st['head'][s, :, A] = 0.0
    st['state'][s, :, A], st['token'][s, :, A], st['grid'][s, :, A], st['tmask'][s, :, A] = INVALID, -1, -1, 1
    st['imask'][s, :, A] = st['catflag'][s, :, A] = (np.arange(st['T']) >= c)
    st['pos'][s, c, A] = (nx, ny)
    st['head'][s, c, A] = ego[2]
    st['state'][s, c, A], st['token'][s, c, A], st['grid'][s, c, A] = gr.ENTER, -2, cell
    st['type'][s, A], st['bos'][s, A] = ty, c
    dec['new_shape'][s], dec['new_cell'][s] = dec['shape'][s], cell
    if t > 0:
        sl = slice((t - 1) * 5, (t - 1) * 5 + 5)
        st['pred_traj'][row, sl] = (nx, ny)
        st['pred_head'][row, sl] = ego[2]
        st['pred_state'][row, sl] = float(gr.ENTER)
    st['n_agents'][s] = A + 1
    dec['n_new'][s] += 1
    dec['new_row'][s], dec['inserted'][s] = row, 1


# ------------------------------------------------------------------------------------------------ generated cases
# consecutive pairs share a map scene (copies = 2): the names are paired so that a pair can share its tables
SCENES = ('empty', 'full', 'ego_not_first', 'ego_heading_pi', 'far_away', 'appended_row', 'all_banned', 'all_banned_copy',
          'allow_zones_only', 'allow_zones_copy', 'void_tables', 'plain')


def segment_records(segs):
    """road records (8 floats) of explicit world segments [(x0, y0, x1, y1)], by the road masks' rule: anchor p0, offset of the
    midpoint from it, unit direction, half length, radius; a zero-length or non-finite segment is the void record of radius -1"""
    out = np.zeros((len(segs), 8), np.float32)
    for i, (x0, y0, x1, y1) in enumerate(np.asarray(segs, np.float32)):
        dx, dy = np.float32(x1 - x0), np.float32(y1 - y0)
        L = np.sqrt(dx * dx + dy * dy, dtype=np.float32)
        if not (np.isfinite(L) and L > 0 and np.isfinite(x0) and np.isfinite(y0)):
            out[i] = (0, 0, 0, 0, 1, 0, 0, -1)
        else:
            out[i] = (x0, y0, np.float32(0.5) * ((x1 - x0) + np.float32(0)), np.float32(0.5) * ((y1 - y0) + np.float32(0)), dx / L,
                      dy / L, np.float32(0.5) * L, np.float32(0.5) * L)
    return out


def gen_case(grid_xy, seed=0, A_cap=33, T=3, M_cap=48, Z=6, rec_cap=24, copies=2):
    """the named scenes of SCENES (map-side tables for S / copies map scenes: scene s reads those of s // copies), column c = 1.
    The thresholds carry odd fractions of a millimetre so that no cell of the 3 m lattice sits on one by construction.
    -> (block, shape [S * A_cap][3], rules, c)"""
    rng = np.random.default_rng([seed, 1961])
    S, c = len(SCENES), 1
    S0 = S // copies
    grid_xy = np.asarray(grid_xy, np.float32)
    G = grid_xy.shape[0]
    R = float(np.abs(grid_xy).max())
    st = gr.new_state(S, A_cap, T, M_cap, G=G)
    st['grid_xy'] = grid_xy.copy()
    shape = np.full((S, A_cap, 3), 0.1, np.float32)
    st['state'][:] = 0
    zones = np.zeros((S0, Z, 4), np.float32)
    n_zones = np.zeros(S0, np.int32)
    records = np.zeros((S0, rec_cap, 8), np.float32)
    n_records = np.zeros(S0, np.int32)
    map_pos = np.zeros((S0, M_cap, 2), np.float32)
    map_type = np.zeros((S0, M_cap), np.int64)
    n_map = np.zeros(S0, np.int32)
    origin = {}
    for s, name in enumerate(SCENES):
        n = dict(empty=0, full=A_cap, appended_row=9).get(name, int(rng.integers(5, 14)))
        if s % copies == 0:                                  # the scenes of a pair lie in the same place: they share a map
            off = np.float32(1e4) if name == 'far_away' else np.float32(0)
            o = (rng.uniform(-50, 50, 2).astype(np.float32) + off).astype(np.float32)
        origin[s] = o
        st['n_agents'][s] = n
        st['av_index'][s] = 0 if n == 0 else (n - 1 if name == 'ego_not_first' else 0)
        rad = R if n else 0.0
        ang, rr = rng.uniform(0, 2 * math.pi, (T, A_cap)), rad * np.sqrt(rng.uniform(0, 1, (T, A_cap)))
        st['pos'][s, :, :, 0] = (o[0] + rr * np.cos(ang)).astype(np.float32)
        st['pos'][s, :, :, 1] = (o[1] + rr * np.sin(ang)).astype(np.float32)
        st['head'][s] = rng.uniform(-math.pi, math.pi, (T, A_cap)).astype(np.float32)
        st['state'][s, :, :n] = rng.integers(1, 4, (T, n))
        if n > 3:
            st['state'][s, c, 1] = 0                         # a row that left: no obstacle, not counted
        st['state'][s, :, n:] = rng.integers(0, 4, (T, A_cap - n))      # padding rows: never looked at, whatever they hold
        av = int(st['av_index'][s])
        st['state'][s, c, av] = 1
        if name == 'ego_heading_pi':
            st['head'][s, c, av] = np.float32(math.pi) - np.float32(1e-6)
        if name == 'empty':                                   # n_agents = 0: the ego pose is still read from row av = 0
            st['pos'][s, c, 0] = o
        shape[s, :, 0] = rng.uniform(0.6, 6.0, A_cap)
        shape[s, :, 1] = rng.uniform(0.4, 2.4, A_cap)
        shape[s, :, 2] = rng.uniform(1.0, 2.0, A_cap)
        if name == 'appended_row':                            # row 8 was appended by an earlier iteration of this step: state ENTER
            st['state'][s, c, 8] = 2
            st['state'][s, :c, 8] = 0
            st['pos'][s, c, 8] = (o + np.float32(0.5 * R) * np.array([0.6, -0.8], np.float32)).astype(np.float32)
    for m in range(S0):
        o = origin[m * copies]
        k = int(rng.integers(M_cap // 2, M_cap))
        n_map[m] = k
        a_, r_ = rng.uniform(0, 2 * math.pi, M_cap), R * np.sqrt(rng.uniform(0, 1, M_cap))
        map_pos[m, :, 0], map_pos[m, :, 1] = o[0] + r_ * np.cos(a_), o[1] + r_ * np.sin(a_)
        map_type[m] = rng.choice([0, 1, 2, 12, 15, 40, -1], M_cap)
        segs = []
        for _ in range(rec_cap - 3):
            p = o + rng.uniform(-R, R, 2)
            d = rng.uniform(-25, 25, 2)
            segs.append((p[0], p[1], p[0] + d[0], p[1] + d[1]))
        segs += [(o[0], o[1], o[0], o[1]), (np.inf, 0, 1, 1)]           # void records (radius -1)
        rec = segment_records(segs)
        records[m, :len(segs)] = rec
        n_records[m] = len(segs)
        zc = o + rng.uniform(-0.6 * R, 0.6 * R, (Z, 2))
        zones[m, :, :2] = zc
        zones[m, :, 2] = rng.uniform(8, 30, Z) + 0.00037
        zones[m, :, 3] = [0, 1, 0, 1, 0, 0]
        zones[m, 4, 2], zones[m, 5, 2] = -3.0, np.inf                   # void zones
        n_zones[m] = Z
    by = {n: i for i, n in enumerate(SCENES)}
    m = by['all_banned'] // copies
    zones[m, 0] = (*origin[m * copies], 4 * R, 0)                       # a ban zone over the whole disc
    m = by['allow_zones_only'] // copies
    zones[m, :, 3] = 1
    zones[m, 4, 2], zones[m, 5, 2] = -3.0, np.nan
    m = by['void_tables'] // copies
    zones[m, :, 2] = (-1.0, 0.0, np.inf, np.nan, -np.inf, -2.0)         # every zone void: the rule bans nothing
    records[m, :, 7] = -1.0                                             # every record void
    rules = new_rules(keepout=(6.0005, 40.0005, 4.4995), clearance=10.00037, edge_clearance=2.50041, records=records,
                      n_records=n_records, near_lane=(12.00053, (0, 1, 2, 15)), map_pos=map_pos, map_type=map_type, n_map=n_map,
                      zones=zones, n_zones=n_zones, copies=copies)
    return st, shape.reshape(S * A_cap, 3), rules, c


def band_share(st, shape, rules, c):
    """per scene: the share of cells whose float64 margin is below BAND"""
    G = st['grid_xy'].shape[0]
    return [float((cell_verdicts(st, shape, rules, s, c)['margin'] < BAND).sum()) / G for s in range(st['S'])]
