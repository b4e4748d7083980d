"""Plain float64 reference of the NODE side of an AttentionLayer (infgen_attn_pre / infgen_attn_post / infgen_attn_post_pre,
include/infgen_hip.h) and of infgen_mlp_embedding, written from the reference model - AttentionLayer.forward / update / _attn_block /
_ff_block (infgen/modules/layers.py:61-113), MLPEmbedding (layers.py:163-192) - and the state dict, not from packing.py or a kernel:

    post (layer p):  agg' = AGG + W'_vr,h z_h + b'_h sigma_h        W'_vr = to_v_r.weight gamma_r,  b' = to_v_r.weight beta_r + to_v_r.bias
                     g = sigmoid(to_g [agg' ; LN_dst(x)]);  upd = agg' + g (to_s LN_dst(x) - agg')
                     x1 = x + LN_post(to_out upd);  x2 = x1 + LN_ffpost(ff_mlp.3 relu(ff_mlp.0 LN_ffpre(x1)))
    pre (layer n):   xn = LN_src|dst(x);  Q = dh^-0.5 to_q xn;  U_h = Q_h W'_kr,h (W'_kr = to_k_r.weight gamma_r);  K = to_k xn;  V = to_v xn

The same formulas in float32 with every dot product one running sum in ascending k (_dot) give the FP32_ERR_NODE_* figures below;
a device kernel is held to bar = 4 x that figure per output and input regime (the project's margin for a kernel whose summation
order differs from the fp32 evaluation's).  The error of a row is max |got - ref| / max(1, max |ref row|) (compare_node), so rows
of large magnitude are judged relative to themselves.  `mutate` switches on one deliberately wrong variant (MUTANTS);
tests/test_node_attn_ref_cpu.py shows that compare_node - the comparison tests/test_node_attn_gpu.py applies - tells each of them
apart at the bars.  Weight VARIANTS transform a copy of make_weights(seed=3); the reference uses the transformed dict.
Not a test module."""
import functools
import math

import numpy as np

H, DH, D = 8, 16, 128
POST_PREFIX = 'agent_encoder.a2a_attn_layers.1'       # the layer whose post part runs
PRE_PREFIX = 'agent_encoder.t_attn_layers.2'          # the NEXT layer, whose pre part runs
MLP_PREFIX = 'agent_encoder.fusion_emb'
WEIGHT_SEED = 3

OUTPUTS = ('X', 'Q', 'U', 'K', 'V')
REGIMES = 'ABC'
MLP_REGIMES = 'AB'
# ---- the fp32 figures: largest row error (compare_node's measure) of the float32 evaluation against float64 over the weight variants
# and entry forms of a regime, the cyclic base block included; measured and pinned by
# tests/test_node_attn_ref_cpu.py::test_fp32_figures_are_pinned.  bar = 4 x the figure.
# regimes: A nominal, B row magnitudes 2^-20 .. 2^20 (x) and 2^-10 .. 2^10 (AGG), C degenerate rows
FP32_ERR_NODE_X_A = 8.06e-07
FP32_ERR_NODE_X_B = 2.54e-06
FP32_ERR_NODE_X_C = 1.02e-06
FP32_ERR_NODE_Q_A = 8.61e-07
FP32_ERR_NODE_Q_B = 1.92e-06
FP32_ERR_NODE_Q_C = 8.43e-07
FP32_ERR_NODE_U_A = 9.58e-07
FP32_ERR_NODE_U_B = 3.07e-06
FP32_ERR_NODE_U_C = 1.07e-06
FP32_ERR_NODE_K_A = 1.02e-06
FP32_ERR_NODE_K_B = 3.73e-06
FP32_ERR_NODE_K_C = 1.15e-06
FP32_ERR_NODE_V_A = 9.73e-07
FP32_ERR_NODE_V_B = 2.77e-06
FP32_ERR_NODE_V_C = 1.10e-06
FP32_ERR_NODE_MLPEMB_A = 9.94e-07
FP32_ERR_NODE_MLPEMB_B = 6.82e-07


def fp32_err(output, regime):
    return globals()[f'FP32_ERR_NODE_{output}_{regime}']


def bar(output, regime):
    return 4 * fp32_err(output, regime)


# ------------------------------------------------------------------------------------------------ operand scales (AH_HDR)
# slot -> the matrix it descales (csrc/layout.h: AH_HDR): the pre part reads 0 .. 3, the post part 4 .. 9
SLOTS = ('wq', 'wkr', 'wk', 'wv', 'wvr', 'wg', 'ws', 'wo', 'w1', 'w2')
PRE_SLOTS, POST_SLOTS, MLP_SLOTS = (0, 1, 2, 3), (4, 5, 6, 7, 8, 9), (0, 1, 2)
SCALE_TARGET, SCALE_CAP = 32000.0, 2.0 ** 14


def prescale(w):
    """the documented power-of-two prescale of a split matrix: min(2^floor(log2(32000 / max |w|)), 2^14)"""
    return float(min(2.0 ** math.floor(math.log2(SCALE_TARGET / max(float(np.abs(np.asarray(w, np.float32)).max()), 1e-30))), SCALE_CAP))


def slot_matrices(sd, prefix):
    """the ten matrices of a layer as the split section stores them (fp32: what the packer rounds), in slot order; a layer
    without to_k_r / to_v_r gives None in slots 1 and 4"""
    g = lambda name: np.asarray(sd[f'{prefix}.{name}'], np.float32)
    has_r = f'{prefix}.to_k_r.weight' in sd
    gam = g('attn_prenorm_r.weight') if has_r else None
    return [g('to_q.weight') * np.float32(DH ** -0.5), g('to_k_r.weight') * gam[None, :] if has_r else None, g('to_k.weight'),
            g('to_v.weight'), g('to_v_r.weight') * gam[None, :] if has_r else None, g('to_g.weight'), g('to_s.weight'),
            g('to_out.weight'), g('ff_mlp.0.weight'), g('ff_mlp.3.weight')]


def prescales(sd, prefix):
    return [1.0 if m is None else prescale(m) for m in slot_matrices(sd, prefix)]


def mlp_prescales(sd, prefix=MLP_PREFIX):
    return [prescale(sd[f'{prefix}.mlp.{i}.weight']) for i in (0, 3, 6)]


def _pairs(slots):
    return [(i, j) for i in slots for j in slots if i != j]


# projection of slot i descaled with slot j's factor, one per ordered pair of slots that the same kernel part reads; the gate reads
# slot 5 twice (agg' half, x half), so each half has a variant of its own against slot 6
SLOT_MUTANTS = tuple(f'scale_{i}_as_{j}' for i, j in _pairs(PRE_SLOTS) + _pairs(POST_SLOTS)) + ('scale_5a_as_6', 'scale_5x_as_6')
MLP_SLOT_MUTANTS = tuple(f'mlp_scale_{i}_as_{j}' for i, j in _pairs(MLP_SLOTS))
MUTANTS = SLOT_MUTANTS + (
    'ln_src_for_dst',        # attn_prenorm_x_src where attn_prenorm_x_dst belongs (post part, pre part with use_src_ln = 0)
    'ln_dst_for_src',        # the reverse (pre part with use_src_ln = 1)
    'post_for_ffpre',        # attn_postnorm's parameters in ff_prenorm
    'bprime_no_beta',        # b' without the to_v_r.weight beta_r term
    'gate_swapped',          # g agg' + (1 - g) s
    'drop_ffn_chunk',        # hidden units 128 .. 255 dropped
    'bv_on_k',               # to_v.bias added to K
    'u_no_scale',            # the dh^-0.5 factor missing from u
    'u_swap_h4',             # heads h and h + 4 exchanged in U
    'z_stride64',            # Z of head h read at stride 64
    'skip_z_sig0',           # W'_vr z skipped where SIG = 0
)


def _slot_factor(pres, slot, mutate, half=None):
    """the factor a slot mutant leaves on the projection of `slot`: prescale_slot / prescale_other (1 without a matching mutant)"""
    if not mutate or not mutate.startswith('scale_'):
        return 1.0
    i, j = mutate[len('scale_'):].split('_as_')
    if i[-1] in 'ax':                      # one half of the gate only
        if half != i[-1]:
            return 1.0
        i = i[:-1]
    return pres[int(i)] / pres[int(j)] if int(i) == slot else 1.0


# ------------------------------------------------------------------------------------------------ the reference
def _dot(x, wt, f):
    """x [rows][K] @ wt [K][N]; in float32 one running sum per output in ascending k (product rounded, then added)"""
    if f is np.float64:
        return x @ wt
    acc = np.zeros((x.shape[0], wt.shape[1]), f)
    for k in range(wt.shape[0]):
        acc += x[:, k:k + 1] * wt[k][None, :]
    return acc


def _seq_sum_cols(x):
    """sum over the columns of x [rows][n] in column order"""
    return np.add.accumulate(x, axis=1)[:, -1]


def _ln(x, gam, bet, f):
    """torch.nn.LayerNorm (biased variance, eps 1e-5); gam None: affine-free"""
    n = f(x.shape[1])
    xc = x - (_seq_sum_cols(x) / n)[:, None]
    y = xc / np.sqrt(_seq_sum_cols(xc * xc) / n + f(1e-5))[:, None]
    return y if gam is None else y * gam[None, :] + bet[None, :]


def _sigmoid(p, f):
    with np.errstate(over='ignore'):
        return f(1) / (f(1) + np.exp(-p))


def post_ref(sd, prefix, x, AGG, Z, SIG, has_pos, f=np.float64, mutate=None, want='x2'):
    """-> x2 [rows][128]: the post part of layer `prefix` on rows x with the edge side's AGG [rows][128], Z [rows][8][128],
    SIG [rows][8] (Z / SIG unused without has_pos); want = 'hidden': the FFN's hidden layer [rows][512] instead"""
    g = lambda name: np.asarray(sd[f'{prefix}.{name}'], f)
    ln = lambda name: (g(name + '.weight'), g(name + '.bias'))
    pres = prescales(sd, prefix) if mutate and mutate.startswith('scale_') else None
    c = lambda slot, half=None: f(_slot_factor(pres, slot, mutate, half))
    x, agg = np.asarray(x, f), np.array(AGG, f)
    rows = len(x)
    if has_pos:
        Z, SIG = np.asarray(Z, f).reshape(rows, H, D), np.asarray(SIG, f).reshape(rows, H)
        gam, bet = ln('attn_prenorm_r')
        wvr = g('to_v_r.weight') * gam[None, :]
        bvr = g('to_v_r.bias') if mutate == 'bprime_no_beta' else _dot(bet[None, :], g('to_v_r.weight').T.copy(), f)[0] + g('to_v_r.bias')
        zflat = Z.reshape(rows, H * D)
        for h in range(H):
            zh = zflat[:, 64 * h:64 * h + D] if mutate == 'z_stride64' else Z[:, h, :]
            pz = _dot(zh, wvr[DH * h:DH * (h + 1), :].T.copy(), f) * c(4)
            if mutate == 'skip_z_sig0':
                pz = pz * (SIG[:, h:h + 1] != 0)
            agg[:, DH * h:DH * (h + 1)] += pz + bvr[None, DH * h:DH * (h + 1)] * SIG[:, h:h + 1]
    xn = _ln(x, *ln('attn_prenorm_x_src' if mutate == 'ln_src_for_dst' else 'attn_prenorm_x_dst'), f)
    wg = g('to_g.weight')
    if (mutate or '').startswith('scale_5'):
        pg = _dot(agg, wg[:, :D].T.copy(), f) * c(5, 'a') + _dot(xn, wg[:, D:].T.copy(), f) * c(5, 'x')
    else:
        pg = _dot(np.concatenate([agg, xn], axis=1), wg.T.copy(), f)
    gate = _sigmoid(pg + g('to_g.bias')[None, :], f)
    s = _dot(xn, g('to_s.weight').T.copy(), f) * c(6) + g('to_s.bias')[None, :]
    upd = gate * agg + (f(1) - gate) * s if mutate == 'gate_swapped' else agg + gate * (s - agg)
    o = _dot(upd, g('to_out.weight').T.copy(), f) * c(7) + g('to_out.bias')[None, :]
    x1 = x + _ln(o, *ln('attn_postnorm'), f)
    xf = _ln(x1, *ln('attn_postnorm' if mutate == 'post_for_ffpre' else 'ff_prenorm'), f)
    hdn = np.maximum(_dot(xf, g('ff_mlp.0.weight').T.copy(), f) * c(8) + g('ff_mlp.0.bias')[None, :], f(0))
    if mutate == 'drop_ffn_chunk':
        hdn[:, 128:256] = 0
    if want == 'hidden':
        return hdn
    ffn = _dot(hdn, g('ff_mlp.3.weight').T.copy(), f) * c(9) + g('ff_mlp.3.bias')[None, :]
    return x1 + _ln(ffn, *ln('ff_postnorm'), f)


def pre_ref(sd, prefix, x, use_src_ln, f=np.float64, mutate=None):
    """-> Q [rows][128] (with the dh^-0.5 factor), U [rows][8][128] (None for a layer without to_k_r), K, V [rows][128]"""
    g = lambda name: np.asarray(sd[f'{prefix}.{name}'], f)
    pres = prescales(sd, prefix) if mutate and mutate.startswith('scale_') else None
    c = lambda slot: f(_slot_factor(pres, slot, mutate))
    src = bool(use_src_ln)
    if (mutate == 'ln_src_for_dst' and not src) or (mutate == 'ln_dst_for_src' and src):
        src = not src
    name = 'attn_prenorm_x_src' if src else 'attn_prenorm_x_dst'
    xn = _ln(np.asarray(x, f), g(name + '.weight'), g(name + '.bias'), f)
    q = (_dot(xn, g('to_q.weight').T.copy(), f) * c(0) + g('to_q.bias')[None, :]) * f(DH ** -0.5)
    U = None
    if f'{prefix}.to_k_r.weight' in sd:
        wkr = g('to_k_r.weight') * g('attn_prenorm_r.weight')[None, :]
        qu = q * f(DH ** 0.5) if mutate == 'u_no_scale' else q
        U = np.stack([_dot(qu[:, DH * h:DH * (h + 1)], wkr[DH * h:DH * (h + 1), :], f) * c(1) for h in range(H)], axis=1)
        if mutate == 'u_swap_h4':
            U = U[:, [4, 5, 6, 7, 0, 1, 2, 3], :]
    K = _dot(xn, g('to_k.weight').T.copy(), f) * c(2)
    if mutate == 'bv_on_k':
        K = K + g('to_v.bias')[None, :]
    V = _dot(xn, g('to_v.weight').T.copy(), f) * c(3) + g('to_v.bias')[None, :]
    return q, U, K, V


def mlp_embedding_ref(sd, prefix, x, f=np.float64, mutate=None):
    """MLPEmbedding.forward on continuous inputs x [rows][K0]: Linear LN ReLU Linear LN ReLU Linear -> [rows][128]"""
    g = lambda name: np.asarray(sd[f'{prefix}.mlp.{name}'], f)
    cf = [1.0, 1.0, 1.0]
    if mutate and mutate.startswith('mlp_scale_'):
        i, j = (int(v) for v in mutate[len('mlp_scale_'):].split('_as_'))
        pres = mlp_prescales(sd, prefix)
        cf[i] = pres[i] / pres[j]
    h = np.asarray(x, f)
    h = np.maximum(_ln(_dot(h, g('0.weight').T.copy(), f) * f(cf[0]) + g('0.bias')[None, :], g('1.weight'), g('1.bias'), f), f(0))
    h = np.maximum(_ln(_dot(h, g('3.weight').T.copy(), f) * f(cf[1]) + g('3.bias')[None, :], g('4.weight'), g('4.bias'), f), f(0))
    return _dot(h, g('6.weight').T.copy(), f) * f(cf[2]) + g('6.bias')[None, :]


# ------------------------------------------------------------------------------------------------ the comparison
def row_error(got, ref):
    """max over rows of max |got - ref| / max(1, max |ref row|)"""
    r = np.asarray(ref, np.float64).reshape(len(ref), -1)
    g = np.asarray(got, np.float64).reshape(r.shape)
    return float((np.abs(g - r).max(1) / np.maximum(1.0, np.abs(r).max(1))).max())


def compare_node(regime, got, ref):
    """what the GPU tests assert of one launch's outputs: got / ref map 'X', 'Q', 'U', 'K', 'V' or 'MLPEMB' to arrays of the same rows.
    Every value finite, every output's row error within bar(output, regime).  -> {output: error}"""
    errs = {}
    for name, r in ref.items():
        g = np.asarray(got[name], np.float64).reshape(np.shape(r))
        assert np.isfinite(g).all(), f'{name}: a row below `rows` is not finite'
        errs[name] = row_error(g, r)
    for name, e in errs.items():
        assert e <= bar(name, regime), f'{name} regime {regime}: error {e:.3g} beyond the bar {bar(name, regime):.3g}'
    return errs


# ------------------------------------------------------------------------------------------------ weight variants
@functools.lru_cache(maxsize=None)
def _weights():
    from conftest import make_weights
    return make_weights(seed=WEIGHT_SEED)


LN_NAMES = ('attn_prenorm_x_dst', 'attn_prenorm_x_src', 'attn_postnorm', 'ff_prenorm', 'ff_postnorm', 'attn_prenorm_r')
# wanted prescale exponents per slot in the two `scales` variants (14: the cap).  Every pair of slots of a kernel part differs in at
# least one of the two, each variant has three distinct exponents and a capped slot per part; the factors stay <= 64 so that a
# bias behind a scaled chain (to_out.bias behind to_s / to_v_r x to_out, ff_mlp.3.bias behind ff_mlp.0 x ff_mlp.3) keeps a
# share of its LayerNorm's input far above the bars - a wrong descale of such a product shows only through that share
SCALE_EXPONENTS = {
    'scales_a': dict(wq=13, wkr=12, wk=14, wv=11, wvr=13, wg=14, ws=12, wo=14, w1=13, w2=14),
    'scales_b': dict(wq=14, wkr=13, wk=12, wv=13, wvr=12, wg=14, ws=13, wo=12, w1=14, w2=13),
}
MLP_SCALE_EXPONENTS = {'scales_a': (13, 14, 12), 'scales_b': (14, 12, 13)}
_SLOT_KEY = dict(wq='to_q.weight', wkr='to_k_r.weight', wk='to_k.weight', wv='to_v.weight', wvr='to_v_r.weight', wg='to_g.weight',
                 ws='to_s.weight', wo='to_out.weight', w1='ff_mlp.0.weight', w2='ff_mlp.3.weight')
DEAD_FFN_BIAS = -200.0       # |ff_mlp.0 LN_ffpre(x1)| <= 128 x 0.097 x (1.2 sqrt(127) + 0.1) = 169 for any row


def _factor_for(w, exponent):
    """the power of two that brings matrix w (as the split section stores it) to the wanted prescale exponent"""
    fac = 1.0
    while prescale(np.asarray(w, np.float32) * np.float32(fac)) > 2.0 ** exponent:
        fac *= 2.0
    assert prescale(np.asarray(w, np.float32) * np.float32(fac)) == 2.0 ** exponent
    return np.float32(fac)


def _v_plain(sd):
    return sd


def _v_scales(which):
    def f(sd):
        for prefix in (POST_PREFIX, PRE_PREFIX):
            mats = slot_matrices(sd, prefix)
            for slot, name in enumerate(SLOTS):
                key = f'{prefix}.{_SLOT_KEY[name]}'
                sd[key] = sd[key] * _factor_for(mats[slot], SCALE_EXPONENTS[which][name])
        for i, e in zip((0, 3, 6), MLP_SCALE_EXPONENTS[which]):
            key = f'{MLP_PREFIX}.mlp.{i}.weight'
            sd[key] = sd[key] * _factor_for(sd[key], e)
        return sd
    return f


def _v_ln(sd):
    """per feature: gamma x 2^U(-2, 2) (0.25 .. 4), beta + U(-2, 2); attn_prenorm_x_dst gets parameters of its own in every layer"""
    for li, prefix in enumerate((POST_PREFIX, PRE_PREFIX)):
        for ni, name in enumerate(LN_NAMES):
            rng = np.random.default_rng(7000 + 10 * li + ni)
            sd[f'{prefix}.{name}.weight'] = (sd[f'{prefix}.{name}.weight'] * 2.0 ** rng.uniform(-2.0, 2.0, D)).astype(np.float32)
            sd[f'{prefix}.{name}.bias'] = (sd[f'{prefix}.{name}.bias'] + rng.uniform(-2.0, 2.0, D)).astype(np.float32)
    return sd


def _v_dead_ffn(sd):
    sd[f'{POST_PREFIX}.ff_mlp.0.bias'] = np.full(4 * D, DEAD_FFN_BIAS, np.float32)
    return sd


_VARIANT_FN = dict(plain=_v_plain, scales_a=_v_scales('scales_a'), scales_b=_v_scales('scales_b'), ln=_v_ln, dead_ffn=_v_dead_ffn)
VARIANTS = tuple(_VARIANT_FN)
SCALES_VARIANTS = ('scales_a', 'scales_b')
MLP_VARIANTS = ('plain', 'scales_a', 'scales_b')


@functools.lru_cache(maxsize=None)
def weights(variant='plain'):
    """the state dict of a variant (cached: callers must leave the arrays unchanged)"""
    sd = _VARIANT_FN[variant](dict(_weights()))
    for k in sd:
        if k.startswith((POST_PREFIX, PRE_PREFIX, MLP_PREFIX)):
            sd[k].setflags(write=False)
    return sd


@functools.lru_cache(maxsize=None)
def mlp_weights(variant, k0):
    """the variant's dict with fusion_emb's first Linear cut to its first k0 input columns (an MLPEmbedding of k0 inputs)"""
    sd = dict(weights(variant))
    key = f'{MLP_PREFIX}.mlp.0.weight'
    sd[key] = np.ascontiguousarray(sd[key][:, :k0])
    return sd


# ------------------------------------------------------------------------------------------------ inputs
SMALL_ROWS = 129                        # the small base block: every small case takes its first n rows
GPU_ROWS = 65                           # the row count at which the GPU tests run every (variant, regime, form)
ROW_COUNTS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129]
CYCLE_ROWS = 997                        # the base block the large cases repeat cyclically
PERSISTENT_ROWS = 32768 + 69            # 512 workgroups x 64 rows, then two more tiles: one full, one of 5 rows
SWITCH_ROWS = [6144, 6145, 10240, 10241]
X_EXP, AGG_EXP = 20, 10                 # regime B: rows of x times 2^e, |e| <= 20; rows of AGG times 2^e, |e| <= 10
CONST_ROWS = (1.5, -0.75)               # constant x rows: every partial sum of 128 such values is exact in fp32, in any order -
                                        # the row tests (x - mean) = 0 under 1 / sqrt(eps), not the rounding of a mean
C_BLOCKS = (0, 60, 120)                 # regime C: the nine degenerate rows start here (three tiles of 64, every 16-row group kind)
Z_BOUND = math.sqrt(127.0)


def _normalised_rows(rng, n):
    """layer-normalised rows (no affine part) of inputs with per-row scales 0.2 .. 5 (as tests/edge_attn_ref.py)"""
    x = rng.standard_normal((n, D)) * rng.uniform(0.2, 5.0, (n, 1))
    return (x - x.mean(1, keepdims=True)) / np.sqrt(x.var(1, keepdims=True) + 1e-5)


def _one_hot_normalised(k):
    v = np.zeros(D)
    v[k] = 1000.0
    return (v - v.mean()) / np.sqrt(v.var() + 1e-5)


def x_exponent(i):
    return (7 * i) % (2 * X_EXP + 1) - X_EXP


def agg_exponent(i):
    return (11 * i + 5) % (2 * AGG_EXP + 1) - AGG_EXP


@functools.lru_cache(maxsize=None)
def gen_inputs(regime, rows=SMALL_ROWS):
    """x [rows][128], AGG [rows][128], Z [rows][8][128], SIG [rows][8] in float32 (cached: callers must leave them unchanged).
    A: x ~ N(0, 1), AGG ~ 0.5 N(0, 1), Z convex combinations of six affine-free LayerNorm rows per (row, head), SIG 0 or 1 and a
    quarter fractional.  B: A with the rows of x / AGG scaled by 2^x_exponent(i) / 2^agg_exponent(i).  C: A with nine
    degenerate rows at each of C_BLOCKS (see the code)."""
    rng = np.random.default_rng({'A': 11, 'B': 12, 'C': 13}[regime] + 100 * rows)
    x = rng.standard_normal((rows, D))
    agg = 0.5 * rng.standard_normal((rows, D))
    rh = _normalised_rows(rng, rows * H * 6).reshape(rows, H, 6, D)
    a = rng.dirichlet(np.ones(6), size=(rows, H))
    z = np.einsum('rhe,rhed->rhd', a, rh)
    sig = rng.integers(0, 2, (rows, H)).astype(np.float64)
    frac = rng.random((rows, H)) < 0.25
    sig[frac] = rng.random((rows, H))[frac]
    if regime == 'B':
        i = np.arange(rows)
        x *= 2.0 ** x_exponent(i)[:, None]
        agg *= 2.0 ** agg_exponent(i)[:, None]
    if regime == 'C':
        for b in C_BLOCKS:
            if b + 9 > rows:
                continue
            x[b] = 0.0                                                   # an all-zero x row
            x[b + 1], x[b + 2] = CONST_ROWS                              # constant x rows
            agg[b + 3:b + 5], z[b + 3:b + 5], sig[b + 3:b + 5] = 0.0, 0.0, 0.0      # edgeless rows
            for r in (b + 5, b + 6):                                     # Z at its bound: the LayerNorm of a one-hot vector, SIG = 1
                for h in range(H):
                    z[r, h] = _one_hot_normalised((17 * h + 5 * r) % D) * (1 if (h + r) % 2 else -1)
                sig[r] = 1.0
            agg[b + 7] = 0.0                                             # an AGG row of zeros next to a non-zero Z
            x[b + 8], agg[b + 8], z[b + 8], sig[b + 8] = 0.0, 0.0, 0.0, 0.0       # everything zero
    out = tuple(np.ascontiguousarray(v, np.float32) for v in (x, agg, z, sig))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gen_mlp_inputs(regime, rows):
    """x [rows][512] float32: A N(0, 1); B the rows times 2^x_exponent(i) and, independently, each 128-column chunk c times 2^(3 c - 4)"""
    rng = np.random.default_rng({'A': 21, 'B': 22}[regime] + 100 * rows)
    x = rng.standard_normal((rows, 4 * D))
    if regime == 'B':
        x *= 2.0 ** x_exponent(np.arange(rows))[:, None]
        x *= np.repeat(2.0 ** (3.0 * np.arange(4) - 4.0), D)[None, :]
    x = np.ascontiguousarray(x, np.float32)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------------------------------------ entry forms and references
# form -> (has a post part, has_pos, pre part: None / 'next' (on x2, dst LayerNorm) / 'src' / 'dst' (on x), the outputs written):
# the pointer combinations infgen_decode_layers and infgen_insert_seed issue (csrc/api.hip)
FORMS = {
    'post0': (True, 0, None, ('X',)),                            # infgen_attn_post, fused-edge flow: Z = SIG = NULL
    'post1': (True, 1, None, ('X',)),                            # infgen_attn_post, unfused flow
    'post_pre4': (True, 1, 'next', ('X', 'Q', 'U', 'K', 'V')),    # infgen_attn_post_pre, unfused flow (map -> agent sublayers)
    'post_pre_fused': (True, 0, 'next', ('X', 'Q', 'K', 'V')),    # infgen_attn_post_pre with nU = NULL
    'pre_src_kv': (False, 0, 'src', ('K', 'V')),                 # infgen_attn_pre, use_src_ln = 1, K and V only (a bipartite source)
    'pre_dst4': (False, 0, 'dst', ('Q', 'U', 'K', 'V')),          # infgen_attn_pre, use_src_ln = 0
}


@functools.lru_cache(maxsize=64)
def _post(variant, regime, rows, has_pos, fname, mutate):
    x, agg, z, sig = gen_inputs(regime, rows)
    return post_ref(weights(variant), POST_PREFIX, x, agg, z, sig, has_pos, f=getattr(np, fname), mutate=mutate)


def evaluate(variant, regime, form, f=np.float64, mutate=None, rows=SMALL_ROWS):
    """the outputs of an entry form on the base block of `rows` rows in precision f -> {output: array}; the pre part of a
    post + pre form runs on the x2 of the same precision"""
    has_post, has_pos, pre, outs = FORMS[form]
    fname = np.dtype(f).name
    x = gen_inputs(regime, rows)[0]
    res = {}
    if has_post:
        x = res['X'] = _post(variant, regime, rows, has_pos, fname, mutate)
    if pre:
        q, u, k, v = pre_ref(weights(variant), PRE_PREFIX, x, pre == 'src', f=f, mutate=mutate)
        res.update(Q=q, U=u.reshape(len(q), H * D), K=k, V=v)
    return {o: res[o] for o in outs}


@functools.lru_cache(maxsize=None)
def reference(variant, regime, form, rows=SMALL_ROWS):
    """float64 outputs of an entry form, computed once (callers must leave them unchanged)"""
    return evaluate(variant, regime, form, rows=rows)


@functools.lru_cache(maxsize=None)
def mlp_reference(variant, regime, k0, rows):
    return mlp_embedding_ref(mlp_weights(variant, k0), MLP_PREFIX, gen_mlp_inputs(regime, rows)[:, :k0])


MLP_K0 = (128, 256, 384, 512)
MLP_ROW_COUNTS = [1, 17, 63, 64, 65, 300]
MLP_ROWS = 300                          # the small base block of the embedding cases
MLP_PERSISTENT_ROWS = 32768 + 69
