"""float64 restatement of road-aware decoding's allowed-token sets ("road masks" of include/infgen_hip.h) from the same
fp32 inputs, and the operator-level cases the CPU and GPU tests share.  numpy only."""
from __future__ import annotations

import numpy as np

from collision_ref import sat_sep, thin_vocab, token_end_poses      # noqa: F401  (thin_vocab: re-exported for the tests)

INVALID = 0
EDGE = 12            # the map-token type whose polylines are road edges
BAND = 1e-4          # metres: a decision whose |sep| is below this may fall either way in fp32
NO_RECORD = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, -1.0])


def _record(anchor, p0, p1):
    """one record (anchor x, y | midpoint offset x, y | cos, sin | half length | radius) of the segment p0 -> p1 given relative to
    the anchor; zero length or a non-finite coordinate: NO_RECORD"""
    d = p1 - p0
    L = float(np.hypot(d[0], d[1]))
    if not (np.isfinite(L) and L > 0 and np.isfinite(anchor).all() and np.isfinite(p0).all()):
        return NO_RECORD.copy()
    return np.array([anchor[0], anchor[1], 0.5 * (p0[0] + p1[0]), 0.5 * (p0[1] + p1[1]), d[0] / L, d[1] / L, 0.5 * L, 0.5 * L])


def records_from_map(map_pos, map_orient, map_type, map_tok, n_map, map_vocab, detail=2):
    """-> one float64 array [R][8] per scene: `detail` chords of every EDGE token's vocabulary polyline, tokens in order"""
    map_pos, map_orient, vocab = np.asarray(map_pos, np.float64), np.asarray(map_orient, np.float64), np.asarray(map_vocab, np.float64)
    vocab = vocab.reshape(vocab.shape[0], 11, 2)
    hop, out = 10 // detail, []
    for s in range(map_pos.shape[0]):
        rec = []
        for m in range(min(int(n_map[s]), map_pos.shape[1])):
            tk = int(map_tok[s][m])
            if int(map_type[s][m]) != EDGE or not 0 <= tk < vocab.shape[0]:
                continue
            with np.errstate(invalid='ignore'):
                co, so = np.cos(map_orient[s, m]), np.sin(map_orient[s, m])
            rot = lambda q: np.array([q[0] * co - q[1] * so, q[0] * so + q[1] * co])
            for j in range(detail):
                rec.append(_record(map_pos[s, m], rot(vocab[tk, j * hop]), rot(vocab[tk, (j + 1) * hop])))
        out.append(np.array(rec).reshape(-1, 8))
    return out


def records_from_segments(segments, n_segments):
    """segments [S0][E][4] = (x0, y0, x1, y1) fp32 world coordinates -> one float64 array [n_segments[s]][8] per scene"""
    seg = np.asarray(segments, np.float64)
    return [np.array([_record(g[:2], np.zeros(2), g[2:] - g[:2]) for g in seg[s, :int(n_segments[s])]]).reshape(-1, 8)
            for s in range(seg.shape[0])]


def reference(pos, head, state, n_agents, atype, shape, vocab, c, records, copies=1, sweep=1, margin=0.0, types=(1, 0, 1), base=None,
              first_new=None):
    """the definition, row by row, in float64.  Scene arrays as collision_ref.reference; records: the per-map-scene arrays of
    records_from_*.  -> dict: allowed (after the fallback) / pre (before it) bool [S * A][K], count [S * A] (of pre), live [S * A]
    (the rule applies to the row), base, min_abs_sep [S * A][K] (the smallest |sep| over both shapes and the row's obstacles; inf
    without one), min_sep [S * A][K] (the deepest overlap: the smallest sep), straddle_sep [S * A] -> array [R] (sep of the obstacle rectangle against the row's current box; < 0: straddled),
    straddle_band [S * A] (a straddle decision inside the band), sep_end / sep_path: row -> [K][R] (inf: no obstacle / not tested),
    kept [S * A] (obstacles that are neither out of reach nor straddled)"""
    pos, head, shape = (np.asarray(x, np.float64) for x in (pos, head, shape))
    state, atype = np.asarray(state), np.asarray(atype)
    S, T, A = state.shape
    centre, dth = token_end_poses(vocab)
    K = centre.shape[1]
    base = np.ones((S * A, K), bool) if base is None else np.asarray(base, bool)
    pre, live = base.copy(), np.zeros(S * A, bool)
    min_abs, min_sep = np.full((S * A, K), np.inf), np.full((S * A, K), np.inf)
    straddle_band, kept = np.zeros(S * A, bool), np.zeros(S * A, int)
    straddle_sep, sep_end, sep_path = {}, {}, {}
    disp = np.linalg.norm(centre, axis=-1)                                     # [3][K]
    for s in range(S):
        n = min(int(n_agents[s]), A)
        if first_new is not None:
            n = min(n, int(first_new[s]))
        rec = records[s // copies]
        ok = rec[:, 7] >= 0
        for i in range(n):
            ty = int(atype[s, i]) if 0 <= int(atype[s, i]) <= 2 else 0
            if state[s, c, i] == INVALID or not types[ty]:
                continue
            row = s * A + i
            live[row] = True
            if not ok.any():
                continue
            own = 0.5 * shape[s, i, :2]
            rel = (rec[:, 0:2] - pos[s, c, i]) + rec[:, 2:4]                   # the obstacles' centres in the row's (unrotated) frame
            oh = np.arctan2(rec[:, 5], rec[:, 4])
            oe = np.stack([rec[:, 6] + margin, np.full(len(rec), float(margin))], -1)
            st = np.where(ok, sat_sep(np.zeros(2), head[s, c, i], own, rel, oh, oe), np.inf)
            straddle_sep[row] = st
            straddle_band[row] = bool((np.abs(st[ok]) <= BAND).any())
            # obstacles: valid, not straddled, and - only to keep this restatement quick - not hopelessly far (a metre of slack)
            far = np.linalg.norm(rel, axis=1) > np.hypot(*own) + disp[ty].max() + np.hypot(oe[:, 0], oe[:, 1]) + 1.0
            obs = np.flatnonzero(ok & ~(st < 0) & ~far)
            kept[row] = obs.size
            if obs.size == 0:
                continue
            ci, si = np.cos(head[s, c, i]), np.sin(head[s, c, i])
            cc = np.stack([centre[ty, :, 0] * ci - centre[ty, :, 1] * si, centre[ty, :, 0] * si + centre[ty, :, 1] * ci], -1)   # [K][2]
            se = np.full((K, len(rec)), np.inf)
            se[:, obs] = sat_sep(cc[:, None, :], (head[s, c, i] + dth[ty])[:, None], np.broadcast_to(own, (K, 1, 2)),
                                 rel[obs][None], oh[obs][None], oe[obs][None])
            sp = np.full((K, len(rec)), np.inf)
            if sweep:
                moving = disp[ty] > 0
                pe = np.stack([0.5 * disp[ty], np.full(K, own[1])], -1)[:, None, :]
                pth = sat_sep(0.5 * cc[:, None, :], np.arctan2(cc[:, 1], cc[:, 0])[:, None], pe, rel[obs][None], oh[obs][None], oe[obs][None])
                sp[:, obs] = np.where(moving[:, None], pth, np.inf)
            sep_end[row], sep_path[row] = se, sp
            both = np.minimum(se, sp)
            pre[row] &= ~(both < 0).any(axis=1)
            min_abs[row] = np.minimum(np.abs(se), np.abs(sp)).min(axis=1)
            min_sep[row] = both.min(axis=1)
    count = pre.sum(axis=1)
    allowed = np.where((count == 0)[:, None], base, pre)
    return dict(allowed=allowed, pre=pre, count=count, live=live, base=base, min_abs_sep=min_abs, min_sep=min_sep, straddle_sep=straddle_sep,
                straddle_band=straddle_band, sep_end=sep_end, sep_path=sep_path, kept=kept)


# ------------------------------------------------------------------------------------------ the shared operator-level cases
# token_size 2048 and 64 (lanes without a word), A_cap 8 and 33, copies 1 and 2 (the scene division), sweep 0 / 1, margin 0 / 0.5, with
# and without a base table.  Seeds chosen so the band conditions hold (tests/test_road_masks_cpu.py checks them)
CASES = {
    'k2048_a8_c1_s1_m0': dict(token_size=2048, A=8, copies=1, sweep=1, margin=0.0, base=False, seed=21),
    'k2048_a33_c2_s1_m05_base': dict(token_size=2048, A=33, copies=2, sweep=1, margin=0.5, base=True, seed=22),
    'k64_a33_c1_s0_m0_base': dict(token_size=64, A=33, copies=1, sweep=0, margin=0.0, base=True, seed=23),
    'k64_a8_c2_s1_m05': dict(token_size=64, A=8, copies=2, sweep=1, margin=0.5, base=False, seed=24),
    'k2048_a33_c1_s0_m0': dict(token_size=2048, A=33, copies=1, sweep=0, margin=0.0, base=False, seed=25),
    'k2048_a8_c2_s0_m05_base': dict(token_size=2048, A=8, copies=2, sweep=0, margin=0.5, base=True, seed=26),
}
T_CASE, C_CASE = 3, 1
ORIGIN = np.array([5000.0, -5000.0])      # the 40 m square lies 5 km from the origin: the exact-difference rule matters
SIDE = 40.0
# the map scenes: their record counts, and what row 0 (a vehicle) of the scene's FIRST copy meets there
MIXED, EMPTY, THIN_WALL, N63, N64, RING, WALLED = range(7)
N_RECORDS = {MIXED: 65, EMPTY: 0, THIN_WALL: 1, N63: 63, N64: 64, RING: 150, WALLED: 22}
ASTRIDE_ROW, PED_ROW, ZERO_LENGTH = 0, 1, 5      # of scene MIXED: row 0 sits astride segment 0, the pedestrian row 1 beside segment 1


def _frame(p, h):
    u, v = np.array([np.cos(h), np.sin(h)]), np.array([-np.sin(h), np.cos(h)])
    return lambda x, y: p + x * u + y * v


def walls_around(p, h, hl, hw, margin):
    """22 segments that wall in a box of half extents (hl, hw) at pose (p, h): walls a centimetre outside it (beyond the margin) on
    all four sides and, in front and behind, every 1.5 m out to 16 m - closer together than a vehicle is wide, so a box that jumps
    one wall ends on the next"""
    at, gx, gy = _frame(np.asarray(p, np.float64), float(h)), hl + margin + 0.01, hw + margin + 0.01
    seg = [np.concatenate([at(-gx - 15.0, gy), at(gx + 15.0, gy)]), np.concatenate([at(-gx - 15.0, -gy), at(gx + 15.0, -gy)])]
    for j in range(10):
        seg.append(np.concatenate([at(gx + 1.5 * j, -16.0), at(gx + 1.5 * j, 16.0)]))
        seg.append(np.concatenate([at(-gx - 1.5 * j, -16.0), at(-gx - 1.5 * j, 16.0)]))
    return np.array(seg)


def make_case(name, vocab):
    """-> the arrays of an operator-level case: seven map scenes (N_RECORDS), `copies` row scenes each.  Row 0 of every scene is a
    vehicle of 4.5 m x 2 m, row 1 a pedestrian, row 2 a cyclist.  Scene MIXED: random segments, one of zero length, one under row 0
    (astride), a wall beside the pedestrian; THIN_WALL: one wall across row 0's heading 6 m ahead; RING: 150 half-metre segments
    on three circles around row 0, all within its reach (more than the kernel's list holds); WALLED: walls a centimetre outside row 0's
    box (beyond the margin) on all four sides and, in front and behind, every 1.5 m out to its reach: every token ends on a wall,
    the fallback fires."""
    k = CASES[name]
    rng = np.random.default_rng(k['seed'])
    A, K, copies, margin = k['A'], k['token_size'], k['copies'], k['margin']
    S0, T, c = len(N_RECORDS), T_CASE, C_CASE
    S = S0 * copies
    pos = (ORIGIN + rng.uniform(0.0, SIDE, (S, T, A, 2))).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, (S, T, A)).astype(np.float32)
    state = np.ones((S, T, A), np.int32)
    n_agents = np.full(S, min(A, 8), np.int32)
    n_agents[MIXED * copies] = A
    state[MIXED * copies, c, 3] = INVALID
    atype = np.broadcast_to((np.arange(A) % 3).astype(np.int32), (S, A)).copy()
    shape = np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1).astype(np.float32)
    shape[atype == 1, :2] = [0.8, 0.8]
    shape[:, 0, :2] = [4.5, 2.0]
    E = max(N_RECORDS.values())
    seg = np.zeros((S0, E, 4), np.float64)
    for ms, nrec in N_RECORDS.items():
        a = ORIGIN + rng.uniform(0.0, SIDE, (nrec, 2))
        th, ln = rng.uniform(-np.pi, np.pi, nrec), rng.uniform(0.5, 8.0, nrec)
        seg[ms, :nrec] = np.concatenate([a, a + ln[:, None] * np.stack([np.cos(th), np.sin(th)], -1)], -1)
        p0, h0 = pos[ms * copies, c, 0].astype(np.float64), float(head[ms * copies, c, 0])
        at = _frame(p0, h0)
        if ms == MIXED:
            seg[ms, 0] = np.concatenate([at(-3.0, 0.3), at(3.0, -0.2)])                     # under row 0
            pp, ph = pos[ms * copies, c, PED_ROW].astype(np.float64), float(head[ms * copies, c, PED_ROW])
            seg[ms, 1] = np.concatenate([_frame(pp, ph)(-2.0, 1.2 + margin), _frame(pp, ph)(2.0, 1.2 + margin)])
            seg[ms, ZERO_LENGTH, 2:] = seg[ms, ZERO_LENGTH, :2]
        elif ms == THIN_WALL:
            seg[ms, 0] = np.concatenate([at(6.0, -4.0), at(6.0, 4.0)])
        elif ms == RING:
            for q, radius in enumerate((3.2 + margin, 3.8 + margin, 4.4 + margin)):
                for j in range(50):
                    phi = 2 * np.pi * (j + 0.37 * q) / 50
                    mid, tang = at(radius * np.cos(phi), radius * np.sin(phi)), np.array([-np.sin(phi + h0), np.cos(phi + h0)])
                    seg[ms, 50 * q + j] = np.concatenate([mid - 0.25 * tang, mid + 0.25 * tang])
        elif ms == WALLED:
            seg[ms, :22] = walls_around(p0, h0, 2.25, 1.0, margin)
    segments = seg.astype(np.float32)
    n_segments = np.array([N_RECORDS[ms] for ms in range(S0)], np.int32)
    out = dict(k, pos=pos, head=head, state=state, n_agents=n_agents, atype=atype, shape=shape, c=c, S0=S0,
               segments=segments, n_segments=n_segments, types=(1, 0, 1),
               vocab=np.stack([vocab[t] for t in ('veh', 'ped', 'cyc')]).astype(np.float32))
    if k['base']:
        sets = rng.random((3, K)) < 0.6
        sets[:, 0] = True
        mask_row = rng.choice(np.array([-1, -1, -1, 0, 2], np.int32), S * A).astype(np.int32)
        out.update(sets=sets, mask_row=mask_row, mask_type=[0, 1, 2])
        sel = np.where(mask_row >= 0, mask_row, atype.reshape(-1))
        out['base_rows'] = sets[sel]
    else:
        out['base_rows'] = None
    return out


def case_reference(case, first_new=None):
    rec = records_from_segments(case['segments'], case['n_segments'])
    return reference(case['pos'], case['head'], case['state'], case['n_agents'], case['atype'], case['shape'], case['vocab'], case['c'],
                     rec, case['copies'], case['sweep'], case['margin'], case['types'], case['base_rows'], first_new)
