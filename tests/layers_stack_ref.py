"""Plain numpy reference of infgen_decode_layers (include/infgen_hip.h) for ONE column: the 6 x (temporal, map -> agent,
agent <-> agent) AttentionLayers of a decode step (infgen/modules/agent_decoder.py:2123-2158 over infgen/modules/layers.py:61-113)
with the temporal keys / values of earlier columns taken from a ring of cached projections, written from the reference model and the
state dict - composed of tests/edge_attn_ref.py (the edge operator) and tests/node_attn_ref.py (pre_ref / post_ref), not of a kernel:

    layer i:  q, K_t, V_t = pre(t_i, x);  ring slot c % ring of layer i <- K_t, V_t;  x = post(t_i, x, edge(q, ring, temporal set))
              q = pre(pt2a_i, x) (destination LayerNorm);  x = post(pt2a_i, x, edge(q, map K / V of layer i, map set))
              q, K_a, V_a = pre(a2a_i, x);  x = post(a2a_i, x, edge(q, K_a, V_a, agent set))

Outputs (OUTPUTS): the final X; RK / RV [6][rows][128], the rows the temporal sublayers write into ring slot c % ring (they tap
the residual stream entering every triple); KA / VA [2][rows][128], the agent-set rows of the last two layers.  In float64 the
edge side is edge_attn_ref.edge_attn_fused_ref; in float32 (and under a slot mutant) it is the unfused composition pre_ref's U ->
edge_attn_ref -> post_ref(has_pos = 1), every dot product of the node side one running sum in ascending k (node_attn_ref._dot) -
the two are the same algebra (tests/test_layers_stack_ref_cpu.py).  The float32 evaluation against float64 gives the
FP32_ERR_STACK_* figures below; a device kernel is held to bar = 4 x the figure per output and input regime (node_attn_ref.bar's
margin), row error max |got - ref| / max(1, max |ref row|).  `mutate` switches on one deliberately wrong variant (MUTANTS);
tests/test_layers_stack_ref_cpu.py shows that compare_stack - the comparison tests/test_layers_stack_gpu.py applies - rejects
each.  Weight VARIANTS transform a copy of make_weights(seed=3) in all 18 layers.  Not a test module."""
import functools

import numpy as np

import edge_attn_ref as ea
import node_attn_ref as na

H, DH, D = na.H, na.DH, na.D
L = 6
KINDS = 'tma'
_KIND_NAME = dict(t='t_attn_layers', m='pt2a_attn_layers', a='a2a_attn_layers')
SUBLAYERS = [(i, kind) for i in range(L) for kind in KINDS]          # chain order: sublayer k = 3 i + kind
OUTPUTS = ('X', 'RK', 'RV', 'KA', 'VA')
REGIMES = 'ABC'
# ---- the fp32 figures: largest row error of the float32 evaluation of this chain against float64 over the weight variants and
# the cases (CASES) of a regime; measured and pinned by tests/test_layers_stack_ref_cpu.py::test_fp32_figures_are_pinned.
# bar = 4 x the figure.  regimes: A nominal, B rows of X times 2^-20 .. 2^20 and ring / map rows times 2^-10 .. 2^10, C degenerate rows
FP32_ERR_STACK_X_A = 4.10e-06
FP32_ERR_STACK_X_B = 1.90e-04
FP32_ERR_STACK_X_C = 7.36e-06
FP32_ERR_STACK_RK_A = 5.45e-06
FP32_ERR_STACK_RK_B = 2.06e-04
FP32_ERR_STACK_RK_C = 5.64e-06
FP32_ERR_STACK_RV_A = 3.70e-06
FP32_ERR_STACK_RV_B = 2.46e-04
FP32_ERR_STACK_RV_C = 4.62e-06
FP32_ERR_STACK_KA_A = 4.39e-06
FP32_ERR_STACK_KA_B = 1.91e-04
FP32_ERR_STACK_KA_C = 5.94e-06
FP32_ERR_STACK_VA_A = 4.18e-06
FP32_ERR_STACK_VA_B = 1.75e-04
FP32_ERR_STACK_VA_C = 4.47e-06


def fp32_err(output, regime):
    return globals()[f'FP32_ERR_STACK_{output}_{regime}']


def bar(output, regime):
    return 4 * fp32_err(output, regime)


def prefix(i, kind):
    return f'agent_encoder.{_KIND_NAME[kind]}.{i}'


PREFIXES = [prefix(i, kind) for i, kind in SUBLAYERS]
MUTANT_AT = SUBLAYERS.index((3, 'm'))      # the slot mutants' site: the post part of pt2a_attn_layers.3 and the pre part that follows
                                           # it in the chain (a2a_attn_layers.3: q, u, k, v) - node_attn_ref's post + pre pair
MUTANTS = na.SLOT_MUTANTS + (
    'hdr_of_previous_layer',   # every pre part but the first descaled with slots 0 .. 3 of the sublayer before it in the chain
    'stale_agent_kv',          # the agent sublayer of layer l >= 1 reads the K / V rows of layer l - 1 (the parity buffers mixed up)
    'half_list_dropped',       # the second half (the last cnt // 2 edges) of every list of the agent set ignored
    'empty_half_poisons',      # a row with exactly one edge is merged with an empty second half that counts as one phantom edge of
                               # score 0 with zero value and zero rhat row: a = e^s / (e^s + 1) instead of 1 (the "empty partial
                               # state" of a two-way softmax merge entered with running maximum 0 and sum 1 instead of -inf and 0)
    'ring_slot_off_by_one',    # the column's K / V rows written to ring slot (c + 1) % ring
    'map_src_ln_dst',          # the query of the map -> agent sublayers normalised with attn_prenorm_x_src
    'skip_last_ffn',           # the last sublayer ends at x1 = x + LN_post(out)
)


# ------------------------------------------------------------------------------------------------ the reference
def _scaled_pre(sd, p, prev):
    """the dict whose pre-part matrices of `p` carry the factor a descale with `prev`'s header slots 0 .. 3 leaves"""
    mine, other = na.prescales(sd, p), na.prescales(sd, prev)
    out = dict(sd)
    for slot, key in ((0, 'to_q.weight'), (1, 'to_k_r.weight'), (2, 'to_k.weight'), (3, 'to_v.weight')):
        out[f'{p}.{key}'] = np.asarray(sd[f'{p}.{key}'], np.float64) * (mine[slot] / other[slot])
    return out


def _no_ffn(sd, p):
    out = dict(sd)
    out[f'{p}.ff_postnorm.weight'] = np.zeros(D, np.float32)
    out[f'{p}.ff_postnorm.bias'] = np.zeros(D, np.float32)
    return out


def _phantom(q, u, k, v, off, cnt, src, rhat, agg, z, sig, f):
    """empty_half_poisons on the rows with exactly one edge (see MUTANTS)"""
    for i in np.nonzero(np.asarray(cnt) == 1)[0]:
        e = int(off[i])
        s = ea._row_scores(q[i], u[i].reshape(H, D), k[src[e:e + 1]], rhat[e:e + 1], None)[0]
        mx = np.maximum(s, 0)
        a = np.exp(s - mx) / (np.exp(s - mx) + np.exp(-mx))
        agg[i] = np.repeat(a, DH) * v[src[e]]
        z[i] = a[:, None] * rhat[e][None, :]
        sig[i] = a
    return agg, z, sig


def stack_ref(sd, X, ringK, ringV, slot, mapK, mapV, edges, f=np.float64, mutate=None, first=0, last=3 * L, state=None, fused=None):
    """X [rows][128]; ringK / ringV: per layer [ring * rows][128] (slot s holds rows s * rows ..); slot = c % ring, the slot of the
    current column; mapK / mapV: per layer [n_map][128]; edges: {'t' | 'm' | 'a': (off, cnt, src, rhat)} with src indexing the
    ring / the map rows / the rows, rhat [e_cap][128] the layer-normalised relative-position rows (None with every cnt = 0).
    fused: the edge side as edge_attn_fused_ref (default: in float64 without a mutant), else as the unfused composition.
    Runs sublayers first .. last - 1 (`state`: the dict a run up to `first` returned under 'state'), then - unless it was the
    last one - the temporal pre part that follows a triple, so that RK / RV of the next layer are out.  -> {'X', 'RK': {i: rows},
    'RV', 'KA', 'VA', 'state'}"""
    rows = len(X)
    ring = len(ringK[0]) // rows
    if fused is None:
        fused = f is np.float64 and mutate is None
    assert not fused or (f is np.float64 and mutate is None)
    st = dict(x=np.asarray(X, f), ka={}, va={}) if state is None else dict(x=state['x'].astype(f), ka=dict(state['ka']), va=dict(state['va']))
    out = dict(RK={}, RV={}, KA={}, VA={})
    x = st['x']

    def pre(k, x, use_src):
        p, m, s = PREFIXES[k], None, sd
        if mutate in na.SLOT_MUTANTS and k == MUTANT_AT + 1:
            m = mutate
        if mutate == 'hdr_of_previous_layer' and k > 0:
            s = _scaled_pre(sd, p, PREFIXES[k - 1])
        if mutate == 'map_src_ln_dst' and SUBLAYERS[k][1] == 'm':
            use_src = 1
        return na.pre_ref(s, p, x, use_src, f=f, mutate=m)

    def edge_post(k, x, q, U, Ks, Vs, es):
        p = PREFIXES[k]
        off, cnt, src, rhat = es
        cnt = np.asarray(cnt)
        if mutate == 'half_list_dropped' and SUBLAYERS[k][1] == 'a':
            cnt = cnt - cnt // 2
        if rhat is None:
            rhat = np.zeros((1, D), np.float32)
        m = mutate if mutate in na.SLOT_MUTANTS and k == MUTANT_AT else None
        s = _no_ffn(sd, p) if mutate == 'skip_last_ffn' and k == 3 * L - 1 else sd
        if fused:
            agg = ea.edge_attn_fused_ref(sd, p, q, Ks, Vs, off, cnt, src, rhat)
            return na.post_ref(s, p, x, agg, None, None, 0)
        agg, z, sig = ea.edge_attn_ref(q, U.reshape(rows, -1), Ks, Vs, off, cnt, src, rhat, f=f)
        if mutate == 'empty_half_poisons':
            agg, z, sig = _phantom(np.asarray(q, f), U, np.asarray(Ks, f), np.asarray(Vs, f), off, cnt, src, np.asarray(rhat, f), agg, z, sig, f)
        return na.post_ref(s, p, x, agg, z, sig, 1, f=f, mutate=m)

    def temporal_pre(i, x):
        q, U, K, V = pre(3 * i, x, 1)
        out['RK'][i], out['RV'][i] = K, V
        return q, U, K, V

    for k in range(first, last):
        i, kind = SUBLAYERS[k]
        if kind == 't':
            q, U, K, V = temporal_pre(i, x)
            rk, rv = np.array(ringK[i], f), np.array(ringV[i], f)
            w = ((slot + 1) % ring if mutate == 'ring_slot_off_by_one' else slot) * rows
            rk[w:w + rows], rv[w:w + rows] = K, V
            if mutate == 'ring_slot_off_by_one':                 # what the observed slot then holds: the rows it held before
                out['RK'][i], out['RV'][i] = rk[slot * rows:(slot + 1) * rows], rv[slot * rows:(slot + 1) * rows]
            x = edge_post(k, x, q, U, rk, rv, edges['t'])
        elif kind == 'm':
            q, U, _, _ = pre(k, x, 0)
            x = edge_post(k, x, q, U, mapK[i], mapV[i], edges['m'])
        else:
            q, U, K, V = pre(k, x, 1)
            st['ka'][i], st['va'][i] = K, V
            if i >= L - 2:
                out['KA'][i], out['VA'][i] = K, V
            if mutate == 'stale_agent_kv' and i >= 1:
                K, V = st['ka'][i - 1], st['va'][i - 1]
            x = edge_post(k, x, q, U, K, V, edges['a'])
    if last < 3 * L and SUBLAYERS[last][1] == 't':
        temporal_pre(last // 3, x)
    st['x'] = x
    out['X'], out['state'] = x, st
    return out


# ------------------------------------------------------------------------------------------------ the comparison
def flatten(res):
    """the per-output arrays a comparison takes: X, and RK / RV / KA / VA stacked over the layers present"""
    out = {}
    for o in OUTPUTS:
        v = res.get(o)
        if v is None or (isinstance(v, dict) and not v):
            continue
        out[o] = np.asarray(v) if o == 'X' else np.concatenate([np.asarray(v[i]) for i in sorted(v)])
    return out


def compare_stack(regime, got, ref):
    """what the GPU tests assert of one call's observables: got / ref map OUTPUTS to arrays of the same rows (flatten).  Every
    value finite, every output's row error within bar(output, regime).  -> {output: error}"""
    errs = {}
    for name, r in ref.items():
        g = np.asarray(got[name], np.float64).reshape(np.shape(r))
        assert np.isfinite(g).all(), f'{name}: a value is not finite'
        errs[name] = na.row_error(g, r)
    for name, e in errs.items():
        assert e <= bar(name, regime), f'{name} regime {regime}: error {e:.3g} beyond the bar {bar(name, regime):.3g}'
    return errs


# ------------------------------------------------------------------------------------------------ weight variants
LN_NAMES = na.LN_NAMES
# The prescale exponents.  A matrix of the synthetic weights has a natural exponent of 17 .. 19 (capped to 14), so exponent e costs a
# factor 2^(17 - e) .. 2^(19 - e) on the matrix; the tables stay within 12 .. 14 to keep those factors small.  Per slot a pair
# (scales_a, scales_b); the pairs of the slots one kernel part reads (0 .. 3 / 4 .. 9) are distinct, so every two of them differ in
# at least one variant.  Sublayer k rotates both by (k + k // 3) % 3 within 12 .. 14 - a bijection, so the pairs stay distinct in
# every sublayer, the same slot differs between a sublayer and the next one in the chain in BOTH variants (a header taken from P
# where NP belongs leaves a factor 2 or 4) and between layer i and layer i + 1 of the same kind.
SCALE_CODES = dict(wq=(13, 14), wkr=(12, 13), wk=(14, 12), wv=(12, 14), wvr=(13, 12), wg=(14, 14), ws=(12, 13), wo=(14, 12),
                   w1=(13, 14), w2=(14, 13))
# ... and shrink both pre-norms of x (gamma and beta): to_q, to_k and to_k_r grow by up to 128, 32 and 32, and scores thousands of
# times the nominal ones turn every softmax of the chain into a hard maximum whose near-ties no float32 evaluation reproduces
# (measured: row errors of 0.3 through 18 sublayers).  With the factor below the scores stay within a few times the nominal ones.
SCALES_LN_FACTOR = 2.0 ** -10


def scale_exponents(which, k):
    v = SCALES_VARIANTS.index(which)
    return {s: 12 + (c[v] - 12 + k + k // 3) % 3 for s, c in SCALE_CODES.items()}


def _v_scales(which):
    def fn(sd):
        for k, p in enumerate(PREFIXES):
            mats, want = na.slot_matrices(sd, p), scale_exponents(which, k)
            for slot, name in enumerate(na.SLOTS):
                key = f'{p}.{na._SLOT_KEY[name]}'
                sd[key] = sd[key] * na._factor_for(mats[slot], want[name])
            for name in ('attn_prenorm_x_src', 'attn_prenorm_x_dst'):
                for leaf in ('weight', 'bias'):
                    sd[f'{p}.{name}.{leaf}'] = sd[f'{p}.{name}.{leaf}'] * np.float32(SCALES_LN_FACTOR)
        return sd
    return fn


def _bipartite(p):
    return '.pt2a_attn_layers.' in p


def _v_ln(sd):
    """per feature: gamma x 2^U(-2, 2), beta + U(-2, 2), every LayerNorm of every layer with draws of its own; the non-bipartite
    layers register ONE LayerNorm as attn_prenorm_x_src and attn_prenorm_x_dst (layers.py:52-53): dst is a copy of src there"""
    for k, p in enumerate(PREFIXES):
        for ni, name in enumerate(LN_NAMES):
            rng = np.random.default_rng(9000 + 10 * k + ni)
            sd[f'{p}.{name}.weight'] = (sd[f'{p}.{name}.weight'] * 2.0 ** rng.uniform(-2.0, 2.0, D)).astype(np.float32)
            sd[f'{p}.{name}.bias'] = (sd[f'{p}.{name}.bias'] + rng.uniform(-2.0, 2.0, D)).astype(np.float32)
        if not _bipartite(p):
            for leaf in ('weight', 'bias'):
                sd[f'{p}.attn_prenorm_x_dst.{leaf}'] = sd[f'{p}.attn_prenorm_x_src.{leaf}'].copy()
    return sd


PEAKS = (32.0, 4.0, 16.0, 2.0, 8.0)        # neighbours differ by factors of 2 or more, cyclically too


def peak_of(name, k):
    """(feature, gamma) of the peaked feature of LayerNorm `name` in sublayer k"""
    o = 0 if name == 'ff_prenorm' else 2
    return (37 * k + 11 + 50 * o) % D, PEAKS[(k + o) % len(PEAKS)]


def _v_ln_peaked(sd):
    """ff_prenorm and attn_prenorm_x_dst (with its twin attn_prenorm_x_src in the non-bipartite layers): gamma x 0.8 (<= 0.96),
    one feature at the sublayer's peak"""
    for k, p in enumerate(PREFIXES):
        for name in ('ff_prenorm', 'attn_prenorm_x_dst'):
            g = (sd[f'{p}.{name}.weight'] * np.float32(0.8)).astype(np.float32)
            feat, peak = peak_of(name, k)
            g[feat] = peak
            sd[f'{p}.{name}.weight'] = g
            if name == 'attn_prenorm_x_dst' and not _bipartite(p):
                sd[f'{p}.attn_prenorm_x_src.weight'] = g.copy()
    return sd


def _v_dead_ffn(sd):
    for p in PREFIXES:
        sd[f'{p}.ff_mlp.0.bias'] = np.full(4 * D, na.DEAD_FFN_BIAS, np.float32)
    return sd


_VARIANT_FN = dict(plain=lambda sd: sd, scales_a=_v_scales('scales_a'), scales_b=_v_scales('scales_b'), ln=_v_ln,
                   ln_peaked=_v_ln_peaked, dead_ffn=_v_dead_ffn)
VARIANTS = tuple(_VARIANT_FN)
SCALES_VARIANTS = ('scales_a', 'scales_b')


@functools.lru_cache(maxsize=None)
def weights(variant='plain'):
    """the state dict of a variant (cached: callers must leave the arrays unchanged)"""
    sd = _VARIANT_FN[variant](dict(na._weights()))
    for k in sd:
        if k.startswith('agent_encoder.') and '_attn_layers.' in k:
            sd[k].setflags(write=False)
    return sd


# ------------------------------------------------------------------------------------------------ inputs
RING = 13                                # cfg.window + 1 of the standard configuration
SLOT = 1                                 # the first decode column: c = 1
X_EXP, KV_EXP = 20, 10
CONST_ROWS = na.CONST_ROWS
# the base scenes: (agents, map tokens) per row capacity; a batch of more scenes repeats them cyclically
BASE_SCENES = {32: ((32, 32), (1, 8), (9, 20), (21, 32)), 64: ((64, 32), (1, 8), (33, 24), (50, 32))}      # (the scene of one agent second:
                                         # a batch of two scenes has it)
M_CAP = 32


def x_exponent(i):
    return (7 * i) % (2 * X_EXP + 1) - X_EXP


def kv_exponent(i):
    return (11 * i + 5) % (2 * KV_EXP + 1) - KV_EXP


def degenerate_rows(a_cap):
    """regime C: {row of the base block: kind} - zero and constant rows of X among the agents of the first scene, the one agent of
    the second scene, and that scene's padding rows: all inside the first two scenes, the whole batch of the smallest case"""
    n0 = BASE_SCENES[a_cap][0][0]
    assert BASE_SCENES[a_cap][1][0] == 1
    return {0: 'zero', 3: CONST_ROWS[0], 5: CONST_ROWS[1], n0 - 1: 'zero', a_cap: CONST_ROWS[0], a_cap + 1: 'zero', a_cap + 2: CONST_ROWS[1],
            a_cap + 7: 'zero', 2 * a_cap - 1: CONST_ROWS[0]}


@functools.lru_cache(maxsize=None)
def gen_values(regime, a_cap=32):
    """the values a case overwrites the context's arrays with, for the base block of len(BASE_SCENES[a_cap]) scenes: X [rows][128],
    ringK / ringV [6][RING][rows][128], mapK / mapV [6][scenes * M_CAP][128] in float32 (cached: leave them unchanged).
    A: N(0, 1).  B: A with row i of X times 2^x_exponent(i) and row i of every ring slot / of the map rows times 2^kv_exponent(i + slot).
    C: A with the degenerate rows of degenerate_rows (the scene of one agent, the padding rows without edges and rows whose three
    lists are all empty come with the scenes)."""
    nb = len(BASE_SCENES[a_cap])
    rows = nb * a_cap
    rng = np.random.default_rng({'A': 31, 'B': 32, 'C': 33}[regime] + 100 * a_cap)
    X = rng.standard_normal((rows, D))
    rk, rv = rng.standard_normal((L, RING, rows, D)), rng.standard_normal((L, RING, rows, D))
    mk, mv = rng.standard_normal((L, nb * M_CAP, D)), rng.standard_normal((L, nb * M_CAP, D))
    if regime == 'B':
        X *= 2.0 ** x_exponent(np.arange(rows))[:, None]
        e = 2.0 ** kv_exponent(np.arange(rows)[None, :] + np.arange(RING)[:, None])
        rk *= e[None, :, :, None]
        rv *= e[None, :, ::-1, None]
        em = 2.0 ** kv_exponent(np.arange(nb * M_CAP))
        mk *= em[None, :, None]
        mv *= em[None, ::-1, None]
    if regime == 'C':
        for r, kind in degenerate_rows(a_cap).items():
            X[r] = 0.0 if kind == 'zero' else kind
    out = tuple(np.ascontiguousarray(v, np.float32) for v in (X, rk, rv, mk, mv))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gen_edges(a_cap=32):
    """synthetic edge sets of the base block for the CPU measurements (the GPU tests read the device's own lists back): temporal
    lists of 0 .. 3 edges into ring slots other than SLOT, map lists of 0 .. 5 tokens of the row's scene, agent lists of 0 .. n - 1
    other agents of the scene (the first agent of a scene names all of them); rows beyond a scene's agents have no edges; rhat rows
    are affine-free LayerNorm rows"""
    rng = np.random.default_rng(500 + a_cap)
    scenes = BASE_SCENES[a_cap]
    rows = len(scenes) * a_cap
    deg = dict(t=np.zeros(rows, int), m=np.zeros(rows, int), a=np.zeros(rows, int))
    for s, (n, m) in enumerate(scenes):
        for a in range(n):
            r = s * a_cap + a
            deg['t'][r], deg['m'][r] = (a + s) % 4, (2 * a + s) % 6
            deg['a'][r] = n - 1 if a == 0 else int(rng.integers(0, n)) if n > 1 else 0
            if (s, a) == (2, 4):                          # an agent none of whose lists has an edge
                deg['t'][r] = deg['m'][r] = deg['a'][r] = 0
    out = {}
    for kind in KINDS:
        off, cnt, e_cap = ea._layout(rng, list(deg[kind]))
        src = np.zeros(e_cap, np.int32)
        for r in range(rows):
            s, a = divmod(r, a_cap)
            n, m = scenes[s]
            c = cnt[r]
            if kind == 't':
                slots = rng.permutation([x for x in range(RING) if x != SLOT])[:c]
                src[off[r]:off[r] + c] = slots * rows + r
            elif kind == 'm':
                src[off[r]:off[r] + c] = s * M_CAP + rng.permutation(m)[:c]
            else:
                src[off[r]:off[r] + c] = s * a_cap + rng.permutation([x for x in range(n) if x != a])[:c]
        rhat = ea._normalised_rows(rng, e_cap)
        for v in (off, cnt, src, rhat):
            v.setflags(write=False)
        out[kind] = (off, cnt, src, rhat)
    return out


CASES = ((32,), (64,))                   # the cases of a regime: the base block of either row capacity


def run(variant, regime, a_cap=32, f=np.float64, mutate=None, edges=None, edgeless=False, slot=SLOT, scenes=None, **kw):
    """the chain on the base block of (regime, a_cap) with the synthetic edge sets, or the ones given (edgeless: every list empty);
    scenes = n: on the first n scenes of the block only (with lists given for those)"""
    X, rk, rv, mk, mv = gen_values(regime, a_cap)
    if scenes is not None:
        n = scenes * a_cap
        X, rk, rv, mk, mv = X[:n], rk[:, :, :n], rv[:, :, :n], mk[:, :scenes * M_CAP], mv[:, :scenes * M_CAP]
    rows = len(X)
    edges = edges or gen_edges(a_cap)
    if edgeless:
        z = np.zeros(rows, np.int32)
        edges = {kind: (z, z, np.zeros(1, np.int32), None) for kind in KINDS}
    return stack_ref(weights(variant), X, rk.reshape(L, RING * rows, D), rv.reshape(L, RING * rows, D), slot, mk, mv, edges, f=f,
                     mutate=mutate, **kw)


@functools.lru_cache(maxsize=None)
def reference(variant, regime, a_cap=32):
    """float64 outputs on the synthetic edge sets, computed once (callers must leave them unchanged)"""
    return run(variant, regime, a_cap)


@functools.lru_cache(maxsize=None)
def state_at(variant, regime, a_cap, k):
    """the float64 chain's state in front of sublayer k (for runs that start there)"""
    return run(variant, regime, a_cap, last=k)['state']


def run_part(variant, regime, first, last, a_cap=32, mutate=None):
    """sublayers first .. last - 1 in float64 from the reference's state -> (got, ref) flattened to the outputs such a run has"""
    st = state_at(variant, regime, a_cap, first) if first else None
    got = flatten(run(variant, regime, a_cap, mutate=mutate, first=first, last=last, state=st))
    ref = flatten(run(variant, regime, a_cap, fused=False, first=first, last=last, state=st))
    return got, ref
