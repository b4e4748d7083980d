"""Plain float64 reference of FourierEmbedding.forward (infgen_fourier_embed / _tab / _r24 and infgen_fourier_last_dim_table,
include/infgen_hip.h), written from the reference model's definition as oracle/rollout_oracle.fourier_embedding restates it and from
the state dict, not from packing.py or a kernel; n = 2, 3 and 4 continuous inputs:

    z_i = ((x_i f_i) 2) pi  in FLOAT32, rounded after each product, left to right        (f_i = freqs.weight[i], 64 frequencies)
    e_i = mlps.i.3 relu(LN_i(mlps.i.0 [cos z_i ; sin z_i ; x_i]))
    out = to_out.2 relu(LN_out(sum_i e_i [+ categorical addends]))                       [+ an affine-free LayerNorm: normalize]

The operator is DEFINED on the float32 argument z: the reference model and both kernels form it with those three roundings, so the
float64 reference forms z in float32 and takes cos / sin of that float32 value in float64; everything after is float64.  n = 1 is
left out: the ABI accepts it, no pack size exists for it.  Non-finite inputs are left out: the header does not define them.

Table mode (infgen_fourier_last_dim_table / infgen_fourier_embed_tab): table row k = mlps.(n-1) at the input -k without its second
bias (table_ref); the embedding evaluates dims 0 .. n-2 per row and adds row min(max(int(-g), 0), 31) for the last input g - for
integer g in 0 .. -31 the plain operator, for any other g the clamp of fourier_h_body.inc / fourier_ap_body.inc.

The same formulas in float32 with every dot product one running sum in ascending k give the FP32_ERR_FOURIER_* figures; the split
kernels take sin / cos from the hardware with a measured 2.6e-7 absolute error per feature (csrc/fourier_h.hip,
tools/hw_sincos_probe.hip), which no float32 evaluation holds, so the float64 evaluation with every feature moved by +-2.6e-7 gives
the PERT_ERR_FOURIER_* figures and the split kernels' figure is the larger of the two.  bar = 4 x the figure, per output (PLAIN,
NORM) and input regime; the error of a row is node_attn_ref.row_error's.  No figure comes from a device.  `mutate` switches on one
deliberately wrong evaluation (MUTANTS); tests/test_fourier_ref_cpu.py shows that the bars see each of them on a case of CASES,
the list tests/test_fourier_gpu.py runs.  Weight VARIANTS transform a copy of make_weights(seed=3).  Not a test module."""
import functools
import math

import numpy as np

from node_attn_ref import _dot, row_error

D, NF = 128, 64
WEIGHT_SEED = 3
PREFIXES = {'agent_encoder.x_a_emb': 2, 'agent_encoder.r_a2a_emb': 3, 'agent_encoder.r_pt2a_emb': 3, 'agent_encoder.r_t_emb': 4}
CAT_PREFIX = 'agent_encoder.x_a_emb'                  # the embedding the rollout gives categorical addends
PREFIX_OF_N = {2: 'agent_encoder.x_a_emb', 3: 'agent_encoder.r_a2a_emb', 4: 'agent_encoder.r_t_emb'}
OUTPUTS = ('PLAIN', 'NORM')
REGIMES = 'ABC'
SPLIT_KERNELS = ('k_fourier_h', 'k_fourier_h12', 'k_fourier_h_multi')
KERNELS = ('k_fourier',) + SPLIT_KERNELS
HW_SINCOS_ERR = 2.6e-7                                # csrc/fourier_h.hip: max |error| of sincos_hw against fp64
PERT_SEEDS = (0, 1, 2)
TAB_ROWS = 32                                         # csrc/kernels.h: DT_TAB_ROWS

# ---- the figures: largest row error over the variants, prefixes and forms of a regime (tests/test_fourier_ref_cpu.py measures and
# pins them: each within [0.5, 1.0] x its constant).  FP32: the float32 evaluation against float64.  PERT: the float64 evaluation
# with every feature moved by +-HW_SINCOS_ERR (fixed random signs, the worst of PERT_SEEDS) against float64.
FP32_ERR_FOURIER_PLAIN_A = 8.2e-07
FP32_ERR_FOURIER_PLAIN_B = 8.9e-07
FP32_ERR_FOURIER_PLAIN_C = 8.3e-07
FP32_ERR_FOURIER_NORM_A = 8.3e-07
FP32_ERR_FOURIER_NORM_B = 7.2e-07
FP32_ERR_FOURIER_NORM_C = 8.2e-07
PERT_ERR_FOURIER_PLAIN_A = 8.4e-07
PERT_ERR_FOURIER_PLAIN_B = 8.1e-07
PERT_ERR_FOURIER_PLAIN_C = 7.9e-07
PERT_ERR_FOURIER_NORM_A = 8.4e-07
PERT_ERR_FOURIER_NORM_B = 7.3e-07
PERT_ERR_FOURIER_NORM_C = 7.9e-07


def fp32_err(output, regime):
    return globals()[f'FP32_ERR_FOURIER_{output}_{regime}']


def pert_err(output, regime):
    return globals()[f'PERT_ERR_FOURIER_{output}_{regime}']


def figure(output, regime, kernel):
    """k_fourier: the float32 figure; the split kernels: the larger of it and the hardware-sine figure"""
    assert kernel in KERNELS, kernel
    return fp32_err(output, regime) if kernel == 'k_fourier' else max(fp32_err(output, regime), pert_err(output, regime))


def bar(output, regime, kernel):
    return 4 * figure(output, regime, kernel)


# ------------------------------------------------------------------------------------------------ operand scales (FH_HDR)
# the prescale rule of packing.pack_fourier, restated: sw1[i] / sw2 / sw3 scale the feature columns of mlps.i.0.weight, every
# mlps.i.3.weight (one factor: the smallest) and to_out.2.weight; sa1 / sa2 scale the LayerNorm outputs that feed mlps.i.3 / to_out.2
# (bound 11.3 max |gamma| + max |beta|; one sa1 for all dims); sf scales the features.  hdr[i] = 1 / (sw1[i] sf),
# hdr[4] = 1 / (sw2 sa1), hdr[5] = 1 / (sw3 sa2)
SCALE_TARGET, SCALE_CAP, ACT_CAP, SF, LN_MAX = 32000.0, 2.0 ** 14, 4096.0, 1024.0, 11.3


def pow2(bound):
    return float(2.0 ** math.floor(math.log2(SCALE_TARGET / max(float(bound), 1e-30))))


def _absmax(a):
    return float(np.abs(np.asarray(a, np.float32)).max())


def prescales(sd, prefix):
    """-> dict(sw1=[n], sw2, sw3, sa1, sa2, sf) of the documented rule"""
    n = PREFIXES.get(prefix) or sd[f'{prefix}.freqs.weight'].shape[0]
    g = lambda k: np.asarray(sd[f'{prefix}.{k}'], np.float32)
    ln_bound = lambda name: LN_MAX * _absmax(g(name + '.weight')) + _absmax(g(name + '.bias'))
    return dict(sw1=[min(pow2(_absmax(g(f'mlps.{i}.0.weight')[:, :D])), SCALE_CAP) for i in range(n)],
                sw2=min(min(pow2(_absmax(g(f'mlps.{i}.3.weight'))) for i in range(n)), SCALE_CAP),
                sw3=min(pow2(_absmax(g('to_out.2.weight'))), SCALE_CAP),
                sa1=min(min(pow2(ln_bound(f'mlps.{i}.1')) for i in range(n)), ACT_CAP),
                sa2=min(pow2(ln_bound('to_out.0')), ACT_CAP), sf=SF)


def header(sd, prefix):
    """slots 0 .. 5 of the split section's header as the rule gives them (slots n .. 3 are zero)"""
    p = prescales(sd, prefix)
    hdr = [0.0] * 6
    for i, s in enumerate(p['sw1']):
        hdr[i] = 1.0 / (s * p['sf'])
    hdr[4], hdr[5] = 1.0 / (p['sw2'] * p['sa1']), 1.0 / (p['sw3'] * p['sa2'])
    return hdr


HDR_MUTANTS = tuple(f'hdr_{i}_as_{j}' for i in range(4) for j in range(4) if i != j)      # needs n > max(i, j)
TAB_MUTANTS = ('tab_row_plus_one', 'tab_no_clamp', 'tab_last_dim_twice', 'gap_from_wrong_column')
MUTANTS = (
    'sin_cos_swapped',       # cos where sin belongs and the reverse
    'z_in_float64',          # the argument not rounded to float32
    'x_column_dropped',      # the rank-1 term w1x x missing
    'b2_once',               # the second bias of dim 0 only instead of the sum over the dims
    'cat_after_ln',          # the categorical addends added behind to_out.0
    'ln_no_eps',             # every LayerNorm without its 1e-5
    'relu_missing_out',      # no ReLU between to_out.0 and to_out.2
    'norm_with_affine',      # `normalize` with to_out.0's gamma and beta
) + HDR_MUTANTS + ('hdr_4_as_5',) + TAB_MUTANTS


def mutant_applies(mutate, n, cat, normalize, tab):
    """whether a case reaches the code a mutant changes"""
    if mutate in HDR_MUTANTS:
        i, j = int(mutate[4]), int(mutate[9])
        return max(i, j) < (n - 1 if tab else n)
    if mutate in TAB_MUTANTS:
        return tab and (mutate != 'gap_from_wrong_column' or n == 3)
    return dict(cat_after_ln=cat, norm_with_affine=normalize).get(mutate, True)


# ------------------------------------------------------------------------------------------------ the reference
def _ln(x, gam, bet, f, eps=1e-5):
    """torch.nn.LayerNorm (biased variance); gam None: affine-free"""
    n = f(x.shape[1])
    xc = x - (np.add.accumulate(x, axis=1)[:, -1] / n)[:, None]
    y = xc / np.sqrt(np.add.accumulate(xc * xc, axis=1)[:, -1] / n + f(eps))[:, None]
    return y if gam is None else y * gam[None, :] + bet[None, :]


def argument(sd, prefix, i, x32):
    """z [rows][64] float32: ((x f) 2) pi, rounded after each product"""
    fr = np.asarray(sd[f'{prefix}.freqs.weight'], np.float32)[i]
    with np.errstate(over='ignore'):
        return ((np.asarray(x32, np.float32)[:, None] * fr[None, :]) * np.float32(2)) * np.float32(math.pi)


def features(sd, prefix, i, x32, f=np.float64, mutate=None, perturb=None):
    """[cos z ; sin z] [rows][128] in precision f; perturb: a seed - every feature moved by +-HW_SINCOS_ERR"""
    if mutate == 'z_in_float64':
        z = np.asarray(x32, np.float64)[:, None] * np.asarray(sd[f'{prefix}.freqs.weight'], np.float64)[i][None, :] * 2 * math.pi
    else:
        z = argument(sd, prefix, i, x32).astype(f)
    c, s = np.cos(z), np.sin(z)
    if mutate == 'sin_cos_swapped':
        c, s = s, c
    feat = np.concatenate([c, s], axis=1).astype(f)
    if perturb is not None:
        sign = np.random.default_rng(1000 * perturb + i).integers(0, 2, feat.shape) * 2.0 - 1.0
        feat = feat + f(HW_SINCOS_ERR) * sign.astype(f)
    return feat


def branch(sd, prefix, i, x32, f=np.float64, mutate=None, perturb=None, c1=1.0):
    """mlps.i on inputs x32 [rows] WITHOUT its second bias -> [rows][128]; c1: a factor on the feature product (HDR_MUTANTS)"""
    g = lambda name: np.asarray(sd[f'{prefix}.mlps.{i}.{name}'], f)
    eps = 0.0 if mutate == 'ln_no_eps' else 1e-5
    w1 = g('0.weight')
    h = _dot(features(sd, prefix, i, x32, f, mutate, perturb), w1[:, :D].T.copy(), f) * f(c1)
    if mutate != 'x_column_dropped':
        h = h + np.asarray(x32, np.float32).astype(f)[:, None] * w1[:, D][None, :]
    h = np.maximum(_ln(h + g('0.bias')[None, :], g('1.weight'), g('1.bias'), f, eps), f(0))
    return _dot(h, g('3.weight').T.copy(), f)


def table_of(sd, prefix, f=np.float64, mutate=None, perturb=None):
    """[32][128]: the last dim's branch at the inputs 0, -1, .., -31, without its second bias"""
    n = sd[f'{prefix}.freqs.weight'].shape[0]
    return branch(sd, prefix, n - 1, -np.arange(TAB_ROWS, dtype=np.float32), f, mutate, perturb)


def table_row(g):
    """the row fourier_h_body.inc / fourier_ap_body.inc read for a last input g: min(max(int(-g), 0), 31), int() truncating"""
    return np.clip(np.trunc(-np.asarray(g, np.float64)), 0, TAB_ROWS - 1).astype(np.int64)


def fourier_ref(sd, prefix, raw, cat=None, normalize=False, f=np.float64, mutate=None, tab=False, perturb=None):
    """the operator on raw [rows][4] float32 (components n .. 3 unused) -> [rows][128] in precision f"""
    n = sd[f'{prefix}.freqs.weight'].shape[0]
    assert n in (2, 3, 4), 'n = 1 has no pack size'
    g = lambda name: np.asarray(sd[f'{prefix}.{name}'], f)
    raw = np.asarray(raw, np.float32)
    eps = 0.0 if mutate == 'ln_no_eps' else 1e-5
    c1 = [1.0] * n
    if mutate in HDR_MUTANTS:
        i, j = int(mutate[4]), int(mutate[9])
        sw1 = prescales(sd, prefix)['sw1']
        c1[i] = sw1[i] / sw1[j]                    # hdr[j] where hdr[i] belongs
    per_row = n if (not tab or mutate == 'tab_last_dim_twice') else n - 1
    acc = np.zeros((len(raw), D), f)
    for i in range(per_row):
        acc = acc + branch(sd, prefix, i, raw[:, i], f, mutate, perturb, c1[i])
    if mutate == 'hdr_4_as_5':
        p = prescales(sd, prefix)
        acc = acc * f((p['sw2'] * p['sa1']) / (p['sw3'] * p['sa2']))
    if tab:
        gap = raw[:, 3 if (mutate == 'gap_from_wrong_column' and n == 3) else n - 1]
        bad = ~np.isfinite(gap)
        gap = np.where(bad, np.float32(0), gap)
        if mutate == 'tab_no_clamp':               # a table without an end: the branch at the unclamped -int(-g)
            last = branch(sd, prefix, n - 1, (-np.trunc(-gap.astype(np.float64))).astype(np.float32), f, None, perturb)
        else:
            k = table_row(gap)
            if mutate == 'tab_row_plus_one':
                k = np.minimum(k + 1, TAB_ROWS - 1)
            last = table_of(sd, prefix, f, mutate, perturb)[k]
        acc = acc + last
        acc[bad] = np.nan                          # (a gap that is not finite selects no row)
    b2 = [g(f'mlps.{i}.3.bias') for i in range(n)]
    acc = acc + (b2[0] if mutate == 'b2_once' else functools.reduce(lambda a, b: a + b, b2))[None, :]
    if cat is not None and mutate != 'cat_after_ln':
        acc = acc + np.asarray(cat, np.float32).astype(f)
    h = _ln(acc, g('to_out.0.weight'), g('to_out.0.bias'), f, eps)
    if cat is not None and mutate == 'cat_after_ln':
        h = h + np.asarray(cat, np.float32).astype(f)
    if mutate != 'relu_missing_out':
        h = np.maximum(h, f(0))
    out = _dot(h, g('to_out.2.weight').T.copy(), f) + g('to_out.2.bias')[None, :]
    if normalize:
        out = _ln(out, g('to_out.0.weight'), g('to_out.0.bias'), f, eps) if mutate == 'norm_with_affine' else _ln(out, None, None, f, eps)
    return out


# ------------------------------------------------------------------------------------------------ the comparison
def compare_fourier(regime, kernel, got, ref):
    """what the GPU tests assert of one launch: got / ref map 'PLAIN' / 'NORM' to arrays of the same rows.  Every value finite,
    every output's row error within bar(output, regime, kernel).  -> {output: error}"""
    errs = {}
    for name, r in ref.items():
        g = np.asarray(got[name], np.float64).reshape(np.shape(r))
        assert np.isfinite(g).all(), f'{name}: a row below the count is not finite'
        errs[name] = row_error(g, r)
    for name, e in errs.items():
        b = bar(name, regime, kernel)
        assert e <= b, f'{kernel} {name} regime {regime}: error {e:.3g} beyond the bar {b:.3g}'
    return errs


# ------------------------------------------------------------------------------------------------ weight variants
@functools.lru_cache(maxsize=None)
def _weights():
    from conftest import make_weights
    return make_weights(seed=WEIGHT_SEED)


# wanted prescale exponents in the two `scales` variants (14: the cap): sw1 per dim, sw2, sw3.  The dims' exponents are pairwise
# distinct in each variant (what hdr_i_as_j needs), no slot holds the same exponent in both, sw1[0] (a) and sw1[1] / sw3 (b) sit
# at the cap, and hdr[4] != hdr[5] in both (sa1 = sa2 = 2048 with these LayerNorms).  The factors stay <= 64 (plain max |w| = 0.153),
# so that b1 and the rank-1 term keep a share of LN_i's input, and b2sum of LN_out's, far above the bars: a wrong descale of a
# product shows only through the share of what is added to it unscaled (tests/node_attn_ref.py)
SCALE_EXPONENTS = {'scales_a': dict(sw1=(14, 13, 12, 11), sw2=13, sw3=12), 'scales_b': dict(sw1=(12, 14, 11, 13), sw2=12, sw3=14)}
FREQ_TARGET_RAD, A_MAX_DIST, A_MAX_GAP = 1.0e3, 60.0, 12.0


def _factor_for(w, exponent):
    """the power of two that brings matrix w to the wanted prescale exponent"""
    fac = 1.0
    scale = lambda: min(pow2(_absmax(np.asarray(w, np.float32) * np.float32(fac))), SCALE_CAP)
    while scale() > 2.0 ** exponent:
        fac *= 2.0
    assert scale() == 2.0 ** exponent
    return np.float32(fac)


def _v_plain(sd):
    return sd


def _v_scales(which):
    def fn(sd):
        want = SCALE_EXPONENTS[which]
        for prefix, n in PREFIXES.items():
            for i in range(n):
                w = np.array(sd[f'{prefix}.mlps.{i}.0.weight'])
                w[:, :D] *= _factor_for(w[:, :D], want['sw1'][i])          # the feature columns: what sw1[i] is taken from
                sd[f'{prefix}.mlps.{i}.0.weight'] = w
            fac = _factor_for(np.stack([sd[f'{prefix}.mlps.{i}.3.weight'] for i in range(n)]), want['sw2'])
            for i in range(n):
                sd[f'{prefix}.mlps.{i}.3.weight'] = sd[f'{prefix}.mlps.{i}.3.weight'] * fac
            sd[f'{prefix}.to_out.2.weight'] = sd[f'{prefix}.to_out.2.weight'] * _factor_for(sd[f'{prefix}.to_out.2.weight'], want['sw3'])
        return sd
    return fn


def _v_ln(sd):
    """per feature: the dims' LayerNorms gamma x 2^U(-3.3, 3.3) (0.1 .. 10), beta + U(-2, 2): sa1 drops to 2^8; to_out.0 gamma x
    2^U(-6.6, -1.3) (0.01 .. 0.4), beta + U(-1, 1): sa2 at its cap of 4096"""
    for pi, (prefix, n) in enumerate(PREFIXES.items()):
        for i in range(n):
            rng = np.random.default_rng(8100 + 10 * pi + i)
            key = f'{prefix}.mlps.{i}.1'
            sd[key + '.weight'] = (sd[key + '.weight'] * 2.0 ** rng.uniform(-3.3, 3.3, D)).astype(np.float32)
            sd[key + '.bias'] = (sd[key + '.bias'] + rng.uniform(-2.0, 2.0, D)).astype(np.float32)
        rng = np.random.default_rng(8100 + 10 * pi + 9)
        key = f'{prefix}.to_out.0'
        sd[key + '.weight'] = (sd[key + '.weight'] * 2.0 ** rng.uniform(-6.6, -1.3, D)).astype(np.float32)
        sd[key + '.bias'] = (sd[key + '.bias'] + rng.uniform(-1.0, 1.0, D)).astype(np.float32)
    return sd


def _v_freq(sd):
    """freqs.weight x one factor per embedding and dim: the largest |z| of regime A's inputs - distances up to 60, angles up to pi,
    gaps down to -12 - becomes 1e3 rad in every dim (at a small x the rounding of z is then far above the bars: z_in_float64)"""
    for prefix, n in PREFIXES.items():
        key = f'{prefix}.freqs.weight'
        w = np.array(sd[key], np.float32)
        for i in range(n):
            xmax = A_MAX_DIST if i == 0 else A_MAX_GAP if (n == 4 and i == 3) else math.pi
            w[i] *= np.float32(FREQ_TARGET_RAD / (2 * math.pi * xmax * _absmax(w[i])))
        sd[key] = w
    return sd


_VARIANT_FN = dict(plain=_v_plain, scales_a=_v_scales('scales_a'), scales_b=_v_scales('scales_b'), ln=_v_ln, freq=_v_freq)
VARIANTS = tuple(_VARIANT_FN)
SCALES_VARIANTS = ('scales_a', 'scales_b')


@functools.lru_cache(maxsize=None)
def weights(variant='plain'):
    """the state dict of a variant (cached: callers must leave the arrays unchanged)"""
    sd = _VARIANT_FN[variant](dict(_weights()))
    for k in sd:
        if k.startswith(tuple(PREFIXES)):
            sd[k] = np.ascontiguousarray(sd[k])
            sd[k].setflags(write=False)
    return sd


# ------------------------------------------------------------------------------------------------ inputs
BASE_ROWS = 385                         # the base block: every small case takes its first rows, every large one repeats it
GPU_ROWS = 257                          # the row count at which the GPU tests run every (variant, regime, prefix, form)
ROW_COUNTS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 385]
# csrc/api.hip and csrc/kernels.h: k_fourier takes 32-row tiles on at most 2048 workgroups (launch_fourier); the split kernels
# 128-row tiles (k_fourier_h: 8 waves x 16 rows), k_fourier_h12 192-row tiles, on at most 256 x FH_WG_PER_CU = 256 workgroups
# (fourier_h_grid); k_fourier_h12 runs from a capacity of 150000 (knob fh12_min)
TILE = {'k_fourier': 32, 'k_fourier_h': 128, 'k_fourier_h12': 192}
GRID_CAP = {'k_fourier': 2048, 'k_fourier_h': 256, 'k_fourier_h12': 256}
WAVE_ROWS = 16
H12_MIN_CAP = 150000
# a workgroup takes a second tile, then one more full tile and one of 5 rows
PERSISTENT_ROWS = {k: GRID_CAP[k] * TILE[k] + TILE[k] + 5 for k in TILE}
C_BLOCKS = (0, 133, 251)                # regime C: the six special rows start at a tile start, in the middle of a wave's 16 rows
                                        # (row 5 of the wave at 128), and are the last rows of the partial tile of GPU_ROWS rows
C_GAPS = (0.0, -31.0, -32.0, -40.0, 3.0, -2.5)      # the special rows' last input where it is a time gap
BIG_Z = 1.0e5                           # sincos_group's slow path
B_EXP_LO, B_EXP_HI = -20, 10


def b_exponent(i):
    return (7 * i) % (B_EXP_HI - B_EXP_LO + 1) + B_EXP_LO


def _special_x(prefix):
    """x of the six special rows, from the PLAIN freqs of dim 0: x3 puts exactly one frequency at |z| >= 1e5, x4 all 64"""
    fr = np.sort(np.abs(np.asarray(_weights()[f'{prefix}.freqs.weight'], np.float64)[0]))
    x3 = BIG_Z / (2 * math.pi * math.sqrt(fr[-1] * fr[-2]))
    x4 = 2 * BIG_Z / (2 * math.pi * fr[0])
    return (0.0, -0.0, 1e-30, x3, x4, -1500.0)


@functools.lru_cache(maxsize=None)
def gen_inputs(regime, prefix, gaps=None):
    """raw [BASE_ROWS][4] float32 of an embedding (cached, read-only; seeded per (regime, n)); the unused components n .. 3 are NaN
    - the kernels load a float4 and must use the first n only.  gaps: the last input is a time gap (default: n = 4).
    A: distances 0 .. 60, angles in [-pi, pi], gaps -1 .. -12.  B: x_0 = U(1, 1.95) 2^b_exponent(i) (2^-20 .. 2^10: up to 2000),
    angles with exactly +-pi and +-0 in every fourth row, gaps 0 .. -31.  C: A with the six special rows (see _special_x; the
    first is all zero) at each of C_BLOCKS, their gaps C_GAPS."""
    n = PREFIXES[prefix]
    gaps = n == 4 if gaps is None else gaps
    rng = np.random.default_rng({'A': 31, 'B': 32, 'C': 33}[regime] + 100 * n)
    raw = np.full((BASE_ROWS, 4), np.nan, np.float64)
    raw[:, 0] = rng.uniform(0.0, A_MAX_DIST, BASE_ROWS)
    raw[:, 1:n] = rng.uniform(-math.pi, math.pi, (BASE_ROWS, n - 1))
    gap = -rng.integers(1, 13, BASE_ROWS).astype(np.float64)
    if regime == 'B':
        i = np.arange(BASE_ROWS)
        raw[:, 0] = rng.uniform(1.0, 1.95, BASE_ROWS) * 2.0 ** b_exponent(i)
        edge = np.array([np.float32(math.pi), -np.float32(math.pi), 0.0, -0.0])
        for c in range(1, n):
            raw[c::4, c] = edge[(np.arange(len(raw[c::4])) + c) % 4]
        gap = -rng.integers(0, TAB_ROWS, BASE_ROWS).astype(np.float64)
    if gaps:
        raw[:, n - 1] = gap
    if regime == 'C':
        xs = _special_x(prefix)
        for b in C_BLOCKS:
            raw[b:b + 6, 0] = xs
            raw[b, :n] = 0.0
            if gaps:
                raw[b:b + 6, n - 1] = C_GAPS
    out = np.ascontiguousarray(raw, np.float32)
    assert np.isfinite(out[:, :n]).all()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gen_cat():
    """the categorical addends [BASE_ROWS][128] float32 of CAT_PREFIX: the sum of two embedding rows of N(0, 0.5)"""
    rng = np.random.default_rng(41)
    out = np.ascontiguousarray(0.5 * (rng.standard_normal((BASE_ROWS, D)) + rng.standard_normal((BASE_ROWS, D))), np.float32)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ cases and references
def evaluate(variant, regime, prefix, cat=False, normalize=False, tab=False, gaps=None, dtype=np.float64, mutate=None, perturb=None,
             rows=BASE_ROWS):
    """the operator on the first `rows` rows of the base block in precision dtype"""
    raw = gen_inputs(regime, prefix, gaps)[:rows]
    return fourier_ref(weights(variant), prefix, raw, gen_cat()[:rows] if cat else None, normalize, dtype, mutate, tab, perturb)


@functools.lru_cache(maxsize=None)
def reference(variant, regime, prefix, cat=False, normalize=False, tab=False, gaps=None):
    """float64 rows of the whole base block, computed once (callers must leave them unchanged)"""
    out = evaluate(variant, regime, prefix, cat, normalize, tab, gaps)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table_ref(variant, prefix):
    out = table_of(weights(variant), prefix)
    out.setflags(write=False)
    return out


def _cases():
    """(variant, regime, prefix, cat, normalize, tab, gaps): what tests/test_fourier_gpu.py runs at GPU_ROWS rows.  Per-row forms:
    every variant x regime x prefix, plain and normalised, the n = 2 embedding with its categorical addends as well; table forms:
    regimes A and C, n = 4, and n = 3 with an integer-valued last input"""
    out = []
    for variant in VARIANTS:
        for regime in REGIMES:
            for prefix in PREFIXES:
                for normalize in (False, True):
                    out.append((variant, regime, prefix, False, normalize, False, None))
                    if prefix == CAT_PREFIX:
                        out.append((variant, regime, prefix, True, normalize, False, None))
            if regime != 'B':
                for prefix in (PREFIX_OF_N[4], PREFIX_OF_N[3], 'agent_encoder.r_pt2a_emb'):
                    for normalize in (False, True):
                        out.append((variant, regime, prefix, False, normalize, True, True))
    return tuple(out)


CASES = _cases()
VALUE_CASES = tuple(c for c in CASES if not c[5])
TAB_CASES = tuple(c for c in CASES if c[5])


def case_id(case):
    variant, regime, prefix, cat, normalize, tab, gaps = case
    return '-'.join([variant, regime, prefix.split('.')[-1], 'norm' if normalize else 'plain'] + (['cat'] if cat else []) + (['tab'] if tab else []))
