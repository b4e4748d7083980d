"""Plain float64 reference of the edge-attention operators (infgen_edge_attn*, include/infgen_hip.h), written from the reference
semantics - AttentionLayer's message / propagate (infgen/modules/layers.py:78-92,109) with torch_geometric's softmax
exp(s - max) / (sum + 1e-16) - and not from the kernels: per destination row and head h (16 columns)

    s_e,h = q_h . k_src(e),h + u_h . rhat_e          a_e,h = softmax over the row's list
    AGG[16h:16h+16] = sum_e a_e,h v_src(e),h          Z[h] = sum_e a_e,h rhat_e          SIG[h] = sum_e a_e,h

Lists are addressed through off / cnt only (off need not be contiguous or monotone); rows without edges give exact zeros.  The
same formula in float32 (edge_attn_fp32: true maximum, natural exp, edges summed in list order) gives the FP32_ERR_EDGE_* figures
below, and a device kernel is held to BAR = 4 x that figure per output and score regime: summation order and one-ulp
transcendentals, not algorithmic error.  `mutate` switches on one deliberately wrong variant (MUTANTS);
tests/test_edge_attn_ref_cpu.py shows that compare_edge - the comparison tests/test_edge_attn_gpu.py applies - tells each of them
apart at the bars.  Not a test module."""
import functools
import math

import numpy as np

H, DH, D = 8, 16, 128
PREFIX = 'agent_encoder.a2a_attn_layers.1'      # the layer whose W_kr / W_vr the fused cases use
WEIGHT_SEED = 3

MUTANTS = ('swap_h4',             # heads h and h + 4 exchanged in the u . rhat part of the score
           'swap_h2',             # heads h and h + 2 exchanged there
           'stale_z',             # Z not rescaled when a deferred softmax reference moves
           'last_twice',          # the last edge of a list counted twice
           'drop_64',             # edge 64 of a list dropped
           'z_norm_neighbour',    # Z normalised with the neighbouring head's sum
           'sig1_empty',          # SIG = 1 on rows without edges
           'wide_avg',            # the eight interleaved sub-lists normalised separately and averaged
           'eps_nan')             # the 1e-16 placed so that a row without edges gives 0 / 0
R24_MUTANT = 'r16'                # (a switch of unpack_r24: the low plane ignored)

# ---- the fp32 figures: error of edge_attn_fp32 / the fp32 fused formula against float64, relative to max |ref| of the output in
# the case, largest over the cases of a score regime (with and without rhat); measured and pinned by
# tests/test_edge_attn_ref_cpu.py::test_fp32_figures_are_pinned.  BAR = 4 x the figure (bar()).
# regimes: A ordinary, B queries x 8, C equal scores, D staircases (steps 7.5 / 8.5 in the log2 domain), E one dominant edge,
# F descending beyond 130 in the log2 domain, G all scores around -90
FP32_ERR_EDGE_AGG_A = 1.60e-06
FP32_ERR_EDGE_AGG_B = 1.68e-06
FP32_ERR_EDGE_AGG_C = 7.95e-07
FP32_ERR_EDGE_AGG_D = 1.28e-06
FP32_ERR_EDGE_AGG_E = 0.0
FP32_ERR_EDGE_AGG_F = 1.24e-06
FP32_ERR_EDGE_AGG_G = 2.95e-06
FP32_ERR_EDGE_Z_A = 1.23e-06
FP32_ERR_EDGE_Z_B = 1.35e-06
FP32_ERR_EDGE_Z_C = 7.85e-07
FP32_ERR_EDGE_Z_D = 1.98e-06
FP32_ERR_EDGE_Z_E = 0.0
FP32_ERR_EDGE_Z_F = 1.34e-06
FP32_ERR_EDGE_Z_G = 3.62e-06
FP32_ERR_EDGE_SIG_A = 1.67e-06
FP32_ERR_EDGE_SIG_B = 5.37e-07
FP32_ERR_EDGE_SIG_C = 1.26e-06
FP32_ERR_EDGE_SIG_D = 3.58e-07
FP32_ERR_EDGE_SIG_E = 0.0
FP32_ERR_EDGE_SIG_F = 2.39e-07
FP32_ERR_EDGE_SIG_G = 7.16e-07
FP32_ERR_EDGE_FUSED_A = 7.32e-07
FP32_ERR_EDGE_FUSED_B = 3.80e-06
FP32_ERR_EDGE_FUSED_C = 1.02e-06
FP32_ERR_EDGE_FUSED_D = 1.43e-06
FP32_ERR_EDGE_FUSED_E = 4.68e-08
FP32_ERR_EDGE_FUSED_F = 1.36e-06
FP32_ERR_EDGE_FUSED_G = 2.89e-06
REGIMES = 'ABCDEFG'
OUTPUTS = ('AGG', 'Z', 'SIG', 'FUSED')


def fp32_err(output, regime):
    return globals()[f'FP32_ERR_EDGE_{output}_{regime}']


def bar(output, regime):
    return 4 * fp32_err(output, regime)


# ------------------------------------------------------------------------------------------------ the reference
def _seq_sum(x):
    """sum over axis 0 in list order (one running sum: what 'summed in list order' means in float32)"""
    return np.add.accumulate(x, axis=0)[-1]


def _row_scores(q, u, kj, rj, mutate):
    s = np.einsum('hc,nhc->nh', q.reshape(H, DH), kj.reshape(-1, H, DH))
    if u is not None:
        ur = np.einsum('hd,nd->nh', u, rj)
        if mutate == 'swap_h4':
            ur = ur[:, [4, 5, 6, 7, 0, 1, 2, 3]]
        if mutate == 'swap_h2':
            ur = ur[:, [2, 3, 0, 1, 6, 7, 4, 5]]
        s = s + ur
    return s


def _row_softmax(s, vj, rj, f, mutate=None):
    """one list: scores s [n][8] (n >= 1), values vj [n][128], rhat rows rj [n][128] or None -> AGG [128], Z [8][128] or None, SIG [8]"""
    n = len(s)
    p = np.exp(s - s.max(0))
    den = _seq_sum(p) + f(1e-16)
    a = p / den
    agg = _seq_sum(np.repeat(a, DH, axis=1) * vj)
    sig = _seq_sum(a)
    z = None
    if rj is not None:
        az = a
        if mutate == 'z_norm_neighbour':
            az = p / den[[1, 0, 3, 2, 5, 4, 7, 6]]
        z = _seq_sum(az[:, :, None] * rj[:, None, :])
        if mutate == 'stale_z':
            z = _stale_z(s, rj, den)
    return agg, z, sig


MOVE_LOG2 = 8.0          # a deferred softmax reference of this module's own (stale_z, count_moves): it moves when a score exceeds it
                         # by more than this many units of the log2 domain


def _deferred(s):
    """the references a deferred-rescale rule visits, per head: -> (m [n][8] the reference in force at edge e, moved [n][8])"""
    tau = MOVE_LOG2 * math.log(2.0)
    m = np.full(s.shape[1], -np.inf)
    ms, moved = np.empty_like(s), np.zeros(s.shape, bool)
    for e in range(len(s)):
        grow = s[e] > m + tau
        m = np.where(grow, s[e], m)
        ms[e], moved[e] = m, grow
    return ms, moved


def count_moves(s):
    """how often such a rule moves its reference on the float64 scores s [n][8], per head (the first edge counts).  For
    information: it says which lists exercise a rescale, it is not a model of any kernel."""
    return _deferred(np.asarray(s, np.float64))[1].sum(0)


def _stale_z(s, rj, den):
    """Z accumulated against a deferred reference and NOT rescaled when the reference moves, normalised as if it had been"""
    ms, _ = _deferred(s)
    z = ((np.exp(s - ms))[:, :, None] * rj[:, None, :]).sum(0)
    return z * np.exp(ms[-1] - s.max(0))[:, None] / den[:, None]


def edge_attn_ref(q, u, k, v, off, cnt, src, rhat, f=np.float64, mutate=None, want_scores=False):
    """-> (AGG [rows][128], Z [rows][8][128] or None, SIG [rows][8]) in precision f.  u / rhat None: no positional part (Z is None)."""
    rows = len(off)
    q, k, v = (np.asarray(a, f) for a in (q, k, v))
    has_r = u is not None and rhat is not None
    u = np.asarray(u, f).reshape(rows, H, D) if has_r else None
    rhat = np.asarray(rhat, f) if has_r else None
    AGG, SIG = np.zeros((rows, D), f), np.zeros((rows, H), f)
    Z = np.zeros((rows, H, D), f) if has_r else None
    scores = []
    for i in range(rows):
        e = np.arange(off[i], off[i] + cnt[i])
        if mutate == 'last_twice' and len(e):
            e = np.append(e, e[-1])
        if mutate == 'drop_64' and len(e) > 64:
            e = np.delete(e, 64)
        if len(e) == 0:
            scores.append(np.zeros((0, H)))
            if mutate == 'sig1_empty':
                SIG[i] = 1
            if mutate == 'eps_nan':                       # 0 / 0 + 1e-16
                AGG[i], SIG[i] = np.nan, np.nan
                if has_r:
                    Z[i] = np.nan
            continue
        kj, vj = k[src[e]], v[src[e]]
        rj = rhat[e] if has_r else None
        s = _row_scores(q[i], u[i] if has_r else None, kj, rj, mutate)
        scores.append(s)
        if mutate == 'wide_avg':
            parts = [_row_softmax(s[w::8], vj[w::8], None if rj is None else rj[w::8], f) for w in range(8) if len(s[w::8])]
            agg = sum(p[0] for p in parts) / len(parts)
            z = sum(p[1] for p in parts) / len(parts) if has_r else None
            sig = sum(p[2] for p in parts) / len(parts)
        else:
            agg, z, sig = _row_softmax(s, vj, rj, f, mutate)
        AGG[i], SIG[i] = agg, sig
        if has_r:
            Z[i] = z
    if want_scores:
        return AGG, Z, SIG, scores
    return AGG, Z, SIG


def edge_attn_fp32(q, u, k, v, off, cnt, src, rhat):
    """the same straightforward formula in float32: the true maximum of the list, numpy's exp, every sum one running sum in list order"""
    return edge_attn_ref(q, u, k, v, off, cnt, src, rhat, f=np.float32)


def fused_weights(sd, prefix, f=np.float64):
    """W'_kr = to_k_r.weight gamma_r, W'_vr = to_v_r.weight gamma_r, b' = to_v_r.weight beta_r + to_v_r.bias from the state dict: the
    affine part of attn_prenorm_r folded into the two projections of the normalised rows (the k-side constant to_k_r.weight beta_r
    is the same for every edge of a row and drops out of the softmax) - the algebra packing.pack_attention_layer documents"""
    g = lambda name: np.asarray(sd[f'{prefix}.{name}'], f)
    gam, bet = g('attn_prenorm_r.weight'), g('attn_prenorm_r.bias')
    return g('to_k_r.weight') * gam[None, :], g('to_v_r.weight') * gam[None, :], g('to_v_r.weight') @ bet + g('to_v_r.bias')


def absorbed_query(sd, prefix, q, f=np.float64):
    """u_h = q_h . W'_kr[16h:16h+16, :] -> [rows][8][128]"""
    wkr = fused_weights(sd, prefix, f)[0]
    return np.einsum('rhc,hcd->rhd', np.asarray(q, f).reshape(-1, H, DH), wkr.reshape(H, DH, D))


def edge_attn_fused_ref(sd, prefix, q, k, v, off, cnt, src, rhat, f=np.float64, mutate=None):
    """AGG of infgen_edge_attn_fused from the state dict: the edge operator with the absorbed query, then
    AGG_h += W'_vr[16h:16h+16, :] . Z_h + b'_h SIG_h"""
    _, wvr, bvr = fused_weights(sd, prefix, f)
    agg, z, sig = edge_attn_ref(q, absorbed_query(sd, prefix, q, f), k, v, off, cnt, src, rhat, f, mutate)
    out = agg.reshape(-1, H, DH) + (np.einsum('hcd,rhd->rhc', wvr.reshape(H, DH, D), z) + bvr.reshape(H, DH)[None] * sig[:, :, None])
    return out.reshape(-1, D)


# ------------------------------------------------------------------------------------------------ packed 24-bit rows
R24_ROW_BYTES = 384


def pack_r24(rhat):
    """include/infgen_hip.h: per row 128 x 16 bit (bits 31..16 of the fp32 values) followed by 128 x 8 bit (bits 15..8), 384 bytes,
    the values rounded to nearest even at bit 8 -> uint8 [rows][384]"""
    u = np.ascontiguousarray(rhat, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7f + ((u >> 8) & 1)) >> 8) & 0xffffff
    out = np.empty((u.shape[0], R24_ROW_BYTES), np.uint8)
    out[:, :256] = (r >> 8).astype('<u2').view(np.uint8).reshape(u.shape[0], 256)
    out[:, 256:] = (r & 0xff).astype(np.uint8)
    return out


def unpack_r24(b, low=True):
    """the fp32 rows a packed buffer stands for; low = False: the 8-bit plane ignored (R24_MUTANT)"""
    b = np.ascontiguousarray(b, np.uint8).reshape(-1, R24_ROW_BYTES)
    bits = np.ascontiguousarray(b[:, :256]).view('<u2').astype(np.uint32) << 16
    if low:
        bits |= b[:, 256:].astype(np.uint32) << 8
    return bits.view(np.float32)


# ------------------------------------------------------------------------------------------------ the comparison
def compare_edge(regime, got, ref, cnt):
    """what the GPU tests assert of one launch's outputs: got / ref map 'AGG', 'Z', 'SIG' or 'FUSED' to arrays of `rows` rows.
    Every value finite, rows without edges exactly zero, the error relative to max |ref| within bar(output, regime).
    -> {output: error}"""
    empty = np.asarray(cnt) == 0
    errs = {}
    for name, r in ref.items():
        g = np.asarray(got[name], np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), f'{name}: a row below `rows` is not finite'
        assert (g[empty] == 0).all(), f'{name}: a row without edges is not exactly zero'
        errs[name] = float(np.abs(g - r).max() / np.abs(r).max())
    for name, e in errs.items():
        assert e <= bar(name, regime), f'{name} regime {regime}: error {e:.3g} beyond the bar {bar(name, regime):.3g}'
    return errs


# ------------------------------------------------------------------------------------------------ cases
DEGREES = [0, 1, 2, 3, 5, 7, 9, 63, 64, 65, 127, 128, 129, 300]      # tails of trips of 4, 6, 8; odd lengths; the 64-edge chunks; the cap
STEP_75, STEP_85 = 7.5, 8.5          # staircase steps in the log2 domain: on either side of the kernels' documented rescale threshold


@functools.lru_cache(maxsize=None)
def _weights():
    from conftest import make_weights
    return make_weights(seed=WEIGHT_SEED)


weights = _weights


def _normalised_rows(rng, n):
    """layer-normalised rows (no affine part) of inputs with per-row scales 0.2 .. 5"""
    x = rng.standard_normal((n, D)) * rng.uniform(0.2, 5.0, (n, 1))
    x = (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5)
    return x.astype(np.float32)


def _layout(rng, degs):
    """lists stored in reverse row order with gaps of 0 .. 3 unused edges in front of each: -> off, cnt, e_cap"""
    rows = len(degs)
    off, e = np.zeros(rows, np.int32), 0
    for i in range(rows - 1, -1, -1):
        e += int(rng.integers(0, 4))
        off[i] = e
        e += degs[i]
    return off, np.asarray(degs, np.int32), e + int(rng.integers(1, 4))


def _targets(regime, name, rng, i, n):
    """the wanted float64 scores [n][8] of row i's list in a constructed regime"""
    ho = rng.uniform(0.0, 3.0, H)
    pos = np.arange(n)
    if regime == 'C':
        return np.broadcast_to(rng.uniform(-20.0, 20.0, H), (n, H)).copy()
    if regime == 'D':
        levels = min(n, 16)
        step = (STEP_85 if name.endswith('85') else STEP_75) * math.log(2.0)
        return -45.0 + ho[None, :] + step * ((pos * levels) // n)[:, None]
    if regime == 'E':
        t = rng.normal(-35.0, 1.0, (n, H))
        t[min([0, n - 1, 63, 64][i % 4], n - 1)] = 30.0 + ho
        return t
    if regime == 'F':
        return np.linspace(54.0, -54.0, n)[:, None] - ho[None, :] if n > 1 else 54.0 - ho[None, :]
    if regime == 'G':
        return rng.normal(-90.0, 1.5, (n, H))
    raise ValueError(regime)


def _make_case(name, regime, seed, degs, n_src=None, q_scale=1.0, ties=False):
    """q, k, k_nor (the K rows of the launches without rhat / u: k itself in the regimes A / B, in a constructed regime solved
    for the same target scores without the positional part), v, the absorbed query u of PREFIX's weights (the fused entries compute their own from q), CSR lists and normalised
    rhat rows (NaN in the rows no list names).  Regimes A / B: random sources out of n_src with repeats inside a list, sources 0 and
    n_src - 1 present.  Constructed regimes (C .. G): every edge has a source of its own whose k row is solved, head by head, so
    that the float64 score of the edge is the regime's target (up to the float32 rounding of k: ~1e-6 of the score)."""
    sd = _weights()
    rng = np.random.default_rng(seed)
    rows = len(degs)
    off, cnt, e_cap = _layout(rng, degs)
    constructed = regime not in 'AB'
    if constructed:
        n_src = e_cap
    q = (rng.standard_normal((rows, D)) * q_scale).astype(np.float32)
    k = rng.standard_normal((n_src, D)).astype(np.float32)
    v = (rng.standard_normal((n_src, D)) * 3.0).astype(np.float32)
    rhat = np.full((e_cap, D), np.nan, np.float32)
    src = np.zeros(e_cap, np.int32)
    perm = rng.permutation(e_cap)
    for i in range(rows):
        e = np.arange(off[i], off[i] + cnt[i])
        r = _normalised_rows(rng, len(e))
        if ties and len(e):
            # every value exactly half-way between two 24-bit neighbours, odd and even ones: bits 7..0 = 0x80
            r = ((r.view(np.uint32) & np.uint32(0xffffff00)) | np.uint32(0x80)).view(np.float32)
        rhat[e] = r
        if constructed:
            src[e] = perm[e]
        else:
            s = rng.integers(0, n_src, len(e))
            if len(e) >= 2:
                s[1] = s[0]                                  # the same source twice inside the list
            if len(e) >= 4:
                s[-1], s[2] = n_src - 1, 0
            src[e] = s
    if regime == 'B':
        # queries x 8, then a row whose largest |score| would pass 95 is scaled back (scores are linear in q)
        u = absorbed_query(sd, PREFIX, q)
        sc = edge_attn_ref(q, u, k, v, off, cnt, src, rhat, want_scores=True)[3]
        nor = edge_attn_ref(q, None, k, v, off, cnt, src, None, want_scores=True)[3]
        for i in range(rows):
            top = max(np.abs(sc[i]).max(), np.abs(nor[i]).max()) if len(sc[i]) else 0.0
            if top > 95.0:
                q[i] *= np.float32(95.0 / top)
    u = absorbed_query(sd, PREFIX, q)
    k_nor = k
    if constructed:
        k_nor = k.copy()
        q64 = q.astype(np.float64).reshape(rows, H, DH)
        for i in range(rows):
            e = np.arange(off[i], off[i] + cnt[i])
            if len(e) == 0:
                continue
            t = _targets(regime, name, rng, i, len(e))
            for kd, tt in ((k, t - np.einsum('hd,nd->nh', u[i], rhat[e].astype(np.float64))), (k_nor, t)):
                kk = q64[i][None] * (tt / (q64[i] ** 2).sum(-1)[None])[:, :, None]
                kd[src[e]] = kk.reshape(len(e), D).astype(np.float32)
    return dict(name=name, regime=regime, rows=rows, n_src=n_src, e_cap=e_cap, q=q, u=u.astype(np.float32).reshape(rows, H * D),
                k=k, k_nor=k_nor, v=v, off=off, cnt=cnt, src=src, rhat=rhat)


def _cycle(base, n):
    return [base[i % len(base)] for i in range(n)]


_SMALL_DEGS = [3, 0, 65, 1, 9, 2, 64, 5, 7, 0, 129, 4, 6, 8, 63, 11, 1]
_CONSTRUCTED = DEGREES + [4, 6, 8]                         # 17 rows: a partial second group
_SPECS = {
    # name: (regime, seed, degrees, n_src, q_scale, ties)
    'mixed45': ('A', 1, DEGREES + [4, 6, 8] + _cycle([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], 28), 45, 1.0, False),
    'rows1': ('A', 2, [65], 70, 1.0, False),
    'rows15': ('A', 3, _cycle(_SMALL_DEGS, 15), 15, 1.0, False),
    'rows16': ('A', 4, _cycle(_SMALL_DEGS, 16), 40, 1.0, False),
    'rows17': ('A', 5, _cycle(_SMALL_DEGS, 17), 17, 1.0, False),
    'wide12': ('A', 6, [1, 2, 3, 4, 5, 6, 7, 8, 9, 2348, 0, 300], 2400, 1.0, False),     # waves without an edge; 300 + 2048: the seed node
    'r24tie': ('A', 7, [2, 7, 64, 0, 9], 12, 1.0, True),
    'x8_bip33': ('B', 8, DEGREES + _cycle([4, 6, 8, 0, 1, 2, 3, 5, 10, 11], 19), 60, 8.0, False),
    'equal17': ('C', 9, _CONSTRUCTED, None, 1.0, False),
    'stair75': ('D', 10, _CONSTRUCTED, None, 1.0, False),
    'stair85': ('D', 11, _CONSTRUCTED, None, 1.0, False),
    'dominant17': ('E', 12, _CONSTRUCTED, None, 1.0, False),
    'descending17': ('F', 13, _CONSTRUCTED, None, 1.0, False),
    'negative17': ('G', 14, _CONSTRUCTED, None, 1.0, False),
    # the switches between kernels: degrees 0 .. 9 / 0 .. 3 so that the launches stay tiny
    'rows256': ('A', 15, 256, 300, 1.0, False),
    'rows257': ('A', 16, 257, 257, 1.0, False),
    'rows4096': ('A', 17, 4096, 500, 1.0, False),
    'rows4112': ('A', 18, 4112, 500, 1.0, False),
}
SMALL_CASES = [n for n, s in _SPECS.items() if not isinstance(s[2], int)]
AUTO_CASES = ['rows256', 'rows257']
SIZE_CASES = ['rows4096', 'rows4112']
ALL_CASES = list(_SPECS)


@functools.lru_cache(maxsize=None)
def gen_case(name):
    """the case of that name (cached: callers must leave the arrays unchanged)"""
    regime, seed, degs, n_src, q_scale, ties = _SPECS[name]
    if isinstance(degs, int):
        degs = list(np.random.default_rng(1000 + seed).integers(0, 10 if degs < 1000 else 4, degs))
        degs[0], degs[7], degs[-1] = 0, 0, 3
    c = _make_case(name, regime, seed, degs, n_src, q_scale, ties)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """float64 outputs of a case, computed once: kind 'r' (AGG, Z, SIG with rhat and u), 'nor' (AGG, SIG without), 'fused',
    'fused_r24' (the fused operator on unpack_r24(pack_r24(rhat)): exactly the rows the packed buffer stands for)"""
    c = gen_case(name)
    lists = (c['off'], c['cnt'], c['src'])
    if kind == 'r':
        agg, z, sig = edge_attn_ref(c['q'], c['u'], c['k'], c['v'], *lists, c['rhat'])
        return dict(AGG=agg, Z=z, SIG=sig)
    if kind == 'nor':
        agg, _, sig = edge_attn_ref(c['q'], None, c['k_nor'], c['v'], *lists, None)
        return dict(AGG=agg, SIG=sig)
    rhat = c['rhat'] if kind == 'fused' else unpack_r24(pack_r24(c['rhat']))
    return dict(FUSED=edge_attn_fused_ref(_weights(), PREFIX, c['q'], c['k'], c['v'], *lists, rhat))
