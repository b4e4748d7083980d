"""float64 restatement of collision-aware decoding's allowed-token sets ("collision masks" of include/infgen_hip.h) and the
operator-level cases the CPU and GPU tests share.  numpy only."""
from __future__ import annotations

import numpy as np

INVALID = 0
BAND = 1e-4          # metres: a (row, token) whose smallest |sep| is below this may fall either way in fp32


def token_end_poses(vocab):
    """vocab [3][token_size][6][4][2] -> centre [3][token_size][2], heading [3][token_size] of every token's last contour"""
    last = np.asarray(vocab, np.float64)[:, :, -1]
    centre = last.mean(axis=2)
    heading = np.arctan2(last[:, :, 0, 1] - last[:, :, 3, 1], last[:, :, 0, 0] - last[:, :, 3, 0])
    return centre, heading


def sat_sep(ca, ha, ea, cb, hb, eb):
    """separating-axis test of two oriented rectangles: centres c* [..., 2], headings h* [...], half extents e* [..., 2] (half length,
    half width) -> sep [...], the largest gap over the four axes; the boxes overlap iff sep < 0"""
    ca, cb, ea, eb = (np.asarray(x, np.float64) for x in (ca, cb, ea, eb))
    ha, hb = np.asarray(ha, np.float64), np.asarray(hb, np.float64)
    ua = np.stack([np.cos(ha), np.sin(ha)], -1)
    va = np.stack([-np.sin(ha), np.cos(ha)], -1)
    ub = np.stack([np.cos(hb), np.sin(hb)], -1)
    vb = np.stack([-np.sin(hb), np.cos(hb)], -1)
    d = cb - ca
    dot = lambda x, y: (x * y).sum(-1)
    sep = None
    for ax in (ua, va, ub, vb):
        r = (ea[..., 0] * np.abs(dot(ua, ax)) + ea[..., 1] * np.abs(dot(va, ax)) +
             eb[..., 0] * np.abs(dot(ub, ax)) + eb[..., 1] * np.abs(dot(vb, ax)))
        g = np.abs(dot(d, ax)) - r
        sep = g if sep is None else np.maximum(sep, g)
    return sep


def box_corners(c, h, e):
    c, e = np.asarray(c, np.float64), np.asarray(e, np.float64)
    u = np.array([np.cos(h), np.sin(h)])
    v = np.array([-np.sin(h), np.cos(h)])
    return np.stack([c + e[0] * u + e[1] * v, c + e[0] * u - e[1] * v, c - e[0] * u - e[1] * v, c - e[0] * u + e[1] * v])


def polygons_overlap_brute(pa, pb):
    """do two convex polygons (corner lists in order) share interior points?  Brute force, independent of the axis test: a proper
    crossing of two edges, or a corner, an edge midpoint or the centroid of one strictly inside the other"""
    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    def inside(p, poly):
        s = [cross(poly[i], poly[(i + 1) % len(poly)], p) for i in range(len(poly))]
        return all(x > 0 for x in s) or all(x < 0 for x in s)
    for i in range(len(pa)):
        a0, a1 = pa[i], pa[(i + 1) % len(pa)]
        for j in range(len(pb)):
            b0, b1 = pb[j], pb[(j + 1) % len(pb)]
            if cross(a0, a1, b0) * cross(a0, a1, b1) < 0 and cross(b0, b1, a0) * cross(b0, b1, a1) < 0:
                return True
    mids = lambda poly: [(np.asarray(poly[i]) + np.asarray(poly[(i + 1) % len(poly)])) / 2 for i in range(len(poly))]
    pts_a, pts_b = list(pa) + mids(pa) + [np.mean(pa, axis=0)], list(pb) + mids(pb) + [np.mean(pb, axis=0)]
    return any(inside(p, pb) for p in pts_a) or any(inside(p, pa) for p in pts_b)


def unpack(words, token_size):
    """int32 / uint32 words [rows][token_size / 32] -> bool [rows][token_size]"""
    w = np.asarray(words).view(np.uint32).reshape(-1, token_size // 32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[0], token_size)


def reference(pos, head, state, n_agents, atype, shape, vocab, c, predict=1, margin=0.0, base=None, first_new=None):
    """the definition, scene by scene and row by row, in float64.  pos [S][T][A][2], head / state [S][T][A], n_agents [S], atype [S][A],
    shape [S][A][3] (length, width, height), vocab [3][token_size][6][4][2]; base: bool [S * A][token_size] (None: all tokens).
    -> dict: allowed (after the empty-set fallback) / pre (before it) bool [S * A][token_size], count [S * A] (of pre), live [S * A],
    sep [S * A][token_size][A] (inf where j is no obstacle of the row), min_abs_sep [S * A][token_size]"""
    pos, head, shape = (np.asarray(x, np.float64) for x in (pos, head, shape))
    state, atype = np.asarray(state), np.asarray(atype)
    S, T, A = state.shape
    centre, dth = token_end_poses(vocab)
    K = centre.shape[1]
    base = np.ones((S * A, K), bool) if base is None else np.asarray(base, bool)
    pre, live = base.copy(), np.zeros(S * A, bool)
    sep_all = np.full((S * A, K, A), np.inf)
    for s in range(S):
        n = min(int(n_agents[s]), A)
        if first_new is not None:
            n = min(n, int(first_new[s]))
        here = np.zeros(A, bool)
        here[:n] = state[s, c, :n] != INVALID
        # obstacle poses
        op, oh = pos[s, c].copy(), head[s, c].copy()
        if predict and c > 0:
            vel = here & (state[s, c - 1] != INVALID)
            op[vel] = pos[s, c][vel] + (pos[s, c][vel] - pos[s, c - 1][vel])
            dh = head[s, c][vel] - head[s, c - 1][vel]
            oh[vel] = head[s, c][vel] + (dh + np.pi) % (2 * np.pi) - np.pi
        oe = 0.5 * shape[s, :, :2] + margin
        for i in np.flatnonzero(here):
            row = s * A + i
            live[row] = True
            obs = here.copy()
            obs[i] = False
            js = np.flatnonzero(obs)
            if js.size == 0:
                continue
            ty = int(atype[s, i])
            ci, si = np.cos(head[s, c, i]), np.sin(head[s, c, i])
            # the row's frame: pos[c][i] is subtracted from everything first
            cc = np.stack([centre[ty, :, 0] * ci - centre[ty, :, 1] * si, centre[ty, :, 0] * si + centre[ty, :, 1] * ci], -1)   # [K][2]
            ch = head[s, c, i] + dth[ty]
            ce = np.broadcast_to(0.5 * shape[s, i, :2], (K, 1, 2))
            rel = op[js] - pos[s, c, i]
            sp = sat_sep(cc[:, None, :], ch[:, None], ce, rel[None], oh[js][None], oe[js][None])      # [K][len(js)]
            sep_all[row][:, js] = sp
            pre[row] &= ~(sp < 0).any(axis=1)
    count = pre.sum(axis=1)
    allowed = np.where((count == 0)[:, None], base, pre)
    return dict(allowed=allowed, pre=pre, count=count, live=live, sep=sep_all, min_abs_sep=np.abs(sep_all).min(axis=2), base=base)


# ------------------------------------------------------------------------------------------ the shared operator-level cases
# token_size 2048 and 64 (lanes without a word), A_cap 8 and 33 (the compaction crosses a 32-bit boundary), predict 0 / 1,
# margin 0 / 0.5, with and without a base table.  Seeds chosen so the band holds at most 0.1 % of a case's (row, token) pairs
# (tests/test_collision_masks_cpu.py checks that).  The dense case: 160 small boxes in a 16 m square, so that rows have more than LIST
# obstacles within reach and the kernel's list overflows into further passes over the tokens (seed: the first from 33 on that the CPU
# test accepts; with 33 a row's fallback decision hangs on a pair inside the band)
LIST = 128           # RIDER_LIST of infgen_amd/csrc/kernels.h
CASES = {
    'k2048_a8_p1_m0': dict(token_size=2048, A=8, predict=1, margin=0.0, base=False, seed=11),
    'k2048_a33_p1_m05_base': dict(token_size=2048, A=33, predict=1, margin=0.5, base=True, seed=12),
    'k64_a33_p0_m0_base': dict(token_size=64, A=33, predict=0, margin=0.0, base=True, seed=13),
    'k64_a8_p1_m05': dict(token_size=64, A=8, predict=1, margin=0.5, base=False, seed=14),
    'k2048_a33_p0_m0': dict(token_size=2048, A=33, predict=0, margin=0.0, base=False, seed=15),
    'k2048_a8_p0_m05_base': dict(token_size=2048, A=8, predict=0, margin=0.5, base=True, seed=16),
    'k64_a160_p1_m0_dense': dict(token_size=64, A=160, predict=1, margin=0.0, base=False, seed=34, dense=True),
}
T_CASE, C_CASE = 4, 2
ORIGIN = np.array([5000.0, -5000.0])      # the 64 m square lies 5 km from the origin: the relative-frame rule matters
BOXED_SCENE, BOXED_ROW = 3, 0


def thin_vocab(vocab, token_size):
    """a fixed random subset of a vocabulary dict's tokens, in order: the small vocabularies of the operator-level cases"""
    keep = np.sort(np.random.default_rng(0).choice(next(iter(vocab.values())).shape[0], token_size, replace=False))
    return {k: np.ascontiguousarray(v[keep]) for k, v in vocab.items()}


def make_case(name, vocab):
    """-> the arrays of an operator-level case.  Four scenes: 0 full (A rows; row 1 absent at c - 1, row 2 invalid at c, rows 3 and 6 in line), 1 one agent,
    2 every row invalid, 3 a row boxed in on purpose (a 60 m box sits on it: every token collides, the fallback fires).
    dense: the square is 16 m wide, column c - 1 at most 1 m behind, and every row of scene 0 is live with a 0.8 x 0.8 m box."""
    k = CASES[name]
    dense = k.get('dense', False)
    rng = np.random.default_rng(k['seed'])
    A, K, S, T, c = k['A'], k['token_size'], 4, T_CASE, C_CASE
    side, step = (16.0, 1.0) if dense else (64.0, 3.0)
    pos = (ORIGIN + rng.uniform(0.0, side, (S, T, A, 2))).astype(np.float32)
    # column c - 1 a short step behind column c, so the extrapolation stays inside the square's scale
    pos[:, c - 1] = pos[:, c] - rng.uniform(-step, step, (S, A, 2)).astype(np.float32)
    head = rng.uniform(-np.pi, np.pi, (S, T, A)).astype(np.float32)
    head[:, c - 1] = head[:, c] + rng.uniform(-0.3, 0.3, (S, A)).astype(np.float32)
    # rows 3 and 6 of scene 0 (both vehicles) drive in line, 7 m apart: some of their tokens end inside the other's box, most do not
    ahead = 7.0 * np.stack([np.cos(head[0, c, 3]), np.sin(head[0, c, 3])])
    pos[0, c, 6] = pos[0, c, 3] + ahead.astype(np.float32)
    pos[0, c - 1, 6] = pos[0, c, 6] - np.float32(0.5)
    head[0, c - 1:c + 1, 6] = head[0, c, 3]
    state = np.ones((S, T, A), np.int32)
    n_agents = np.array([A, 1, min(A, 5), 2], np.int32)
    state[0, c - 1, 1] = INVALID
    state[0, c, 2] = 1 if dense else INVALID
    state[2] = INVALID
    atype = (np.arange(S * A).reshape(S, A) % 3).astype(np.int32)
    shape = np.stack([rng.uniform(3.5, 5.5, (S, A)), rng.uniform(1.6, 2.2, (S, A)), rng.uniform(1.4, 1.9, (S, A))], -1).astype(np.float32)
    shape[atype == 1, :2] = [0.8, 0.8]
    if dense:
        shape[0, :, :2] = [0.8, 0.8]
    pos[BOXED_SCENE, :, 1] = pos[BOXED_SCENE, :, 0]
    shape[BOXED_SCENE, 1, :2] = [60.0, 60.0]
    out = dict(k, pos=pos, head=head, state=state, n_agents=n_agents, atype=atype, shape=shape, c=c,
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


def reachable(case):
    """-> [A] obstacles within reach of every row of scene 0: centre distance <= own radius + the type's largest token displacement +
    the obstacle's radius, obstacles at their extrapolated centres (what k_collision_mask puts on a row's list)"""
    c, A = case['c'], case['A']
    far = np.linalg.norm(token_end_poses(case['vocab'])[0], axis=-1).max(axis=1)
    p = case['pos'][0].astype(np.float64)
    here = case['state'][0, c] != INVALID
    vel = here & (case['state'][0, c - 1] != INVALID) & bool(case['predict'])
    q = p[c] + np.where(vel[:, None], p[c] - p[c - 1], 0.0)
    rad = np.linalg.norm(0.5 * case['shape'][0, :, :2].astype(np.float64) + case['margin'], axis=-1)
    own = np.linalg.norm(0.5 * case['shape'][0, :, :2].astype(np.float64), axis=-1)
    dist = np.linalg.norm(q[None] - p[c][:, None], axis=-1)
    near = (dist <= (own + far[case['atype'][0]])[:, None] + rad[None]) & here[None] & here[:, None] & ~np.eye(A, dtype=bool)
    return near.sum(axis=1)


def case_reference(case):
    return reference(case['pos'], case['head'], case['state'], case['n_agents'], case['atype'], case['shape'], case['vocab'],
                     case['c'], case['predict'], case['margin'], case['base_rows'])
