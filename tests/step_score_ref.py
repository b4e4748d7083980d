"""float64 restatement of the step scores ("step scores" of include/infgen_hip.h) from the same fp32 inputs, a numpy
restatement of ``branching.score_log_weight``, and the operator-level cases the CPU and GPU tests share.  numpy only."""
from __future__ import annotations

import numpy as np

from collision_ref import box_corners, polygons_overlap_brute, sat_sep      # noqa: F401  (re-exported for the tests)
from road_ref import records_from_segments

INVALID = 0
BAND = 1e-4          # metres: a decision whose |sep| is below this may fall either way in fp32
N_LIVE, N_OVERLAP, MIN_SEP, N_OFFROAD, MAX_ACCEL, MAX_YAW_RATE = range(6)
LIVE_BIT, OVERLAP_BIT, OFFROAD_BIT = 1, 2, 4


def _wrap(x):
    return (x + np.pi) % (2 * np.pi) - np.pi


def reference(pos, head, state, n_agents, atype, shape, c1, records=None, copies=1, sweep=1, margin=0.0, types=(1, 0, 1), dt=0.5):
    """the definition, slot by slot and row by row, in float64.  pos [S][T][A][2], head / state [S][T][A], n_agents [S], atype [S][A],
    shape [S][A][3]; records: None or the per-map-scene arrays [R][8] of road_ref.records_from_*.
    -> dict: score [S][8], row [S][A] uint8, pair_sep: slot -> [n][n] (inf where either row is not live, and on the diagonal),
    box_sep / path_sep: (slot, row) -> [R] (inf: record never used / no path rectangle), band: the smallest |sep| of any decision"""
    pos, head, shape = (np.asarray(x, np.float64) for x in (pos, head, shape))
    state, atype = np.asarray(state), np.asarray(atype)
    S, T, A = state.shape
    score, row = np.zeros((S, 8)), np.zeros((S, A), np.uint8)
    pair_sep, box_sep, path_sep, band = {}, {}, {}, np.inf
    for s in range(S):
        n = min(max(int(n_agents[s]), 0), A)
        live = np.zeros(A, bool)
        live[:n] = state[s, c1, :n] != INVALID
        live1 = live & (state[s, c1 - 1] != INVALID) if c1 >= 1 else np.zeros(A, bool)
        live2 = live1 & (state[s, c1 - 2] != INVALID) if c1 >= 2 else np.zeros(A, bool)
        own = 0.5 * shape[s, :, :2]
        idx = np.flatnonzero(live)
        sep = np.full((A, A), np.inf)
        if idx.size >= 2:
            sub = sat_sep(pos[s, c1, idx][:, None], head[s, c1, idx][:, None], own[idx][:, None], pos[s, c1, idx][None],
                          head[s, c1, idx][None], own[idx][None])
            sub[np.arange(idx.size), np.arange(idx.size)] = np.inf
            sep[np.ix_(idx, idx)] = sub
        pair_sep[s] = sep
        overlap = (sep < 0).any(axis=1)
        if np.isfinite(sep).any():
            band = min(band, float(np.abs(sep[np.isfinite(sep)]).min()))
        off = np.zeros(A, bool)
        rec = None if records is None else records[s // copies]
        if rec is not None and len(rec):
            ok = rec[:, 7] >= 0
            oh = np.arctan2(rec[:, 5], rec[:, 4])
            oe = np.stack([rec[:, 6] + margin, np.full(len(rec), float(margin))], -1)
            for i in idx:
                ty = int(atype[s, i]) if 0 <= int(atype[s, i]) <= 2 else 0
                if not types[ty]:
                    continue
                rel = (rec[:, 0:2] - pos[s, c1, i]) + rec[:, 2:4]
                sb = np.where(ok, sat_sep(np.zeros(2), head[s, c1, i], own[i], rel, oh, oe), np.inf)
                sp = np.full(len(rec), np.inf)
                d = pos[s, c1, i] - pos[s, c1 - 1, i] if (sweep and live1[i]) else np.zeros(2)
                if np.hypot(*d) > 0:
                    sp = np.where(ok, sat_sep(-0.5 * d, np.arctan2(d[1], d[0]), np.array([0.5 * np.hypot(*d), own[i, 1]]), rel, oh, oe), np.inf)
                box_sep[s, i], path_sep[s, i] = sb, sp
                off[i] = bool((sb < 0).any() or (sp < 0).any())
                both = np.concatenate([sb, sp])
                if np.isfinite(both).any():
                    band = min(band, float(np.abs(both[np.isfinite(both)]).min()))
        acc = yaw = 0.0
        if live2.any():
            d1 = np.linalg.norm(pos[s, c1, live2] - pos[s, c1 - 1, live2], axis=-1)
            d0 = np.linalg.norm(pos[s, c1 - 1, live2] - pos[s, c1 - 2, live2], axis=-1)
            acc = float(np.abs(d1 - d0).max() / dt ** 2)
        if live1.any():
            yaw = float(np.abs(_wrap(head[s, c1, live1] - head[s, c1 - 1, live1])).max() / dt)
        finite = sep[np.isfinite(sep)]
        score[s, :6] = [live.sum(), overlap.sum(), finite.min() if finite.size else np.inf, off.sum(), acc, yaw]
        row[s] = live * LIVE_BIT + (live & overlap) * OVERLAP_BIT + (live & off) * OFFROAD_BIT
    return dict(score=score, row=row, pair_sep=pair_sep, box_sep=box_sep, path_sep=path_sep, band=band)


WEIGHT_DEFAULTS = dict(w_overlap=1.0, w_offroad=1.0, w_accel=0.0, w_yaw=0.0, w_gap=0.0, accel_limit=4.0, yaw_limit=1.0, gap_limit=0.5)


def log_weight(step_score, t0, t1, weights=None, copies=1):
    """numpy restatement of branching.score_log_weight: step_score [S0 * copies][steps][8] -> [S0][copies] float64"""
    w = dict(WEIGHT_DEFAULTS, **(weights or {}))
    x = np.asarray(step_score, np.float64)[:, t0:t1]
    relu = lambda v: np.maximum(v, 0.0)
    gap = np.where(np.isinf(x[..., MIN_SEP]), 0.0, relu(w['gap_limit'] - np.where(np.isinf(x[..., MIN_SEP]), 0.0, x[..., MIN_SEP])))
    cost = (w['w_overlap'] * x[..., N_OVERLAP] + w['w_offroad'] * x[..., N_OFFROAD] + w['w_accel'] * relu(x[..., MAX_ACCEL] - w['accel_limit'])
            + w['w_yaw'] * relu(x[..., MAX_YAW_RATE] - w['yaw_limit']) + w['w_gap'] * gap)
    return -cost.sum(axis=1).reshape(-1, copies)


# ------------------------------------------------------------------------------------------ the shared operator-level cases
# A_cap 8 (below a wave), 33 (across a 32-bit boundary), 70 (more rows than one wave) and 300 (one lane per row, two rounds: a
# scene of 300 live rows in a 60 m square, most of them overlapping), copies 1 and 2, sweep 0 / 1, both type
# switches, c1 = 3 and 2, record counts 0, 1, 63, 64, 65, 150.  Seeds chosen so the band condition holds
# (tests/test_step_scores_cpu.py asserts it)
CASES = {
    'a8_c1_s1_m0': dict(A=8, copies=1, sweep=1, margin=0.0, types=(1, 0, 1), c1=3, counts=(150, 0, 63, 64, 1, 65), seed=31),
    'a33_c2_s1_m05': dict(A=33, copies=2, sweep=1, margin=0.5, types=(1, 1, 1), c1=3, counts=(65, 64, 150), seed=32),
    'a70_c1_s0_m0': dict(A=70, copies=1, sweep=0, margin=0.0, types=(1, 1, 1), c1=2, counts=(150, 0, 63, 64, 1, 65), seed=33),
    'a33_c2_s0_m05': dict(A=33, copies=2, sweep=0, margin=0.5, types=(1, 0, 1), c1=2, counts=(0, 63, 1), seed=34),
    'a70_c2_s1_m0': dict(A=70, copies=2, sweep=1, margin=0.0, types=(1, 0, 1), c1=3, counts=(1, 63, 65), seed=35),
    'a300_c1_s1_m0': dict(A=300, copies=1, sweep=1, margin=0.0, types=(1, 1, 1), c1=3, counts=(65, 0, 63, 64, 1, 150), seed=36),
}
T_CASE, S_CASE = 4, 6
ORIGIN = np.array([5000.0, -5000.0])      # the square lies 5 km from the origin: the exact-difference rule matters
SIDE = 60.0
# the scene slots: FULL every row of the layout (row 1 invalid at c1 - 1, row 2 at c1 - 2, row 3 at c1; row 5 parked on row 4), ONE a
# single live row, NONE no live row, ASTRIDE row 0 sits across segment 0 of its map scene, JUMP row 0 jumps a thin wall between
# c1 - 1 and c1 (segment 0 of its map scene; only the path rectangle meets it), FEW at most 8 random rows.  ASTRIDE and JUMP lie
# 300 m and 600 m east of the square, out of reach of the random segments
FULL, ONE, NONE, ASTRIDE, JUMP, FEW = range(S_CASE)
FAR = {ASTRIDE: 300.0, JUMP: 600.0}
ZERO_LENGTH = 5      # this segment of every map scene with more than five has length 0: a record that is never used


def _frame(p, h):
    u, v = np.array([np.cos(h), np.sin(h)]), np.array([-np.sin(h), np.cos(h)])
    return lambda x, y: p + x * u + y * v


def make_case(name):
    k = CASES[name]
    rng = np.random.default_rng(k['seed'])
    A, copies, c1, margin = k['A'], k['copies'], k['c1'], k['margin']
    S, T = S_CASE, T_CASE
    S0 = S // copies
    end = ORIGIN + rng.uniform(0.0, SIDE, (S, A, 2))
    vel = rng.uniform(0.0, 12.0, (S, A, 1)) * np.stack([np.cos(th := rng.uniform(-np.pi, np.pi, (S, A))), np.sin(th)], -1)
    pos = np.stack([end - (T - 1 - t) * vel + rng.normal(0.0, 0.4, (S, A, 2)) for t in range(T)], 1)
    head = (th[:, None, :] + rng.normal(0.0, 0.15, (S, T, A)) + np.pi) % (2 * np.pi) - np.pi
    for s, dx in FAR.items():
        pos[s, :, :, 0] += dx
    state = np.ones((S, T, A), np.int32)
    n_agents = np.full(S, min(A, 8), np.int32)
    n_agents[FULL], n_agents[ONE] = A, 1
    state[FULL, c1 - 1, 1] = state[FULL, c1 - 2, 2] = state[FULL, c1, 3] = INVALID
    state[NONE, c1] = INVALID
    atype = np.broadcast_to((np.arange(A) % 3).astype(np.int32), (S, A)).copy()
    shape = np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1)
    shape[atype == 1, :2] = [0.8, 0.8]
    shape[:, 0, :2] = [4.5, 2.0]
    # two boxes overlapping on purpose: row 5 a metre beside row 4
    pos[FULL, c1, 5] = _frame(pos[FULL, c1, 4], head[FULL, c1, 4])(1.0, 0.3)
    # the jump: 10 m straight ahead between c1 - 1 and c1
    head[JUMP, c1, 0] = 0.3
    pos[JUMP, c1 - 1, 0] = _frame(pos[JUMP, c1, 0], 0.3)(-10.0, 0.0)
    pos, head, shape = pos.astype(np.float32), head.astype(np.float32), shape.astype(np.float32)
    E = max(max(k['counts']), 1)
    seg = np.zeros((S0, E, 4), np.float64)
    for ms, nrec in enumerate(k['counts']):
        a = ORIGIN + rng.uniform(0.0, SIDE, (nrec, 2))
        ph, ln = rng.uniform(-np.pi, np.pi, nrec), rng.uniform(0.5, 8.0, nrec)
        seg[ms, :nrec] = np.concatenate([a, a + ln[:, None] * np.stack([np.cos(ph), np.sin(ph)], -1)], -1)
        if nrec > ZERO_LENGTH:
            seg[ms, ZERO_LENGTH, 2:] = seg[ms, ZERO_LENGTH, :2]
        if nrec and ms == ASTRIDE // copies:
            at = _frame(pos[ASTRIDE, c1, 0].astype(np.float64), float(head[ASTRIDE, c1, 0]))
            seg[ms, 0] = np.concatenate([at(-3.0, 0.3), at(3.0, -0.2)])
        if nrec and ms == JUMP // copies:
            at = _frame(pos[JUMP, c1, 0].astype(np.float64), float(head[JUMP, c1, 0]))
            seg[ms, 1 if (ms == ASTRIDE // copies and nrec > 1) else 0] = np.concatenate([at(-5.0, -4.0), at(-5.0, 4.0)])
    return dict(k, pos=pos, head=head, state=state, n_agents=n_agents, atype=atype, shape=shape, S0=S0,
                segments=seg.astype(np.float32), n_segments=np.array(k['counts'], np.int32))


def case_reference(case, sweep=None):
    rec = records_from_segments(case['segments'], case['n_segments'])
    return reference(case['pos'], case['head'], case['state'], case['n_agents'], case['atype'], case['shape'], case['c1'], rec,
                     case['copies'], case['sweep'] if sweep is None else sweep, case['margin'], case['types'])
