"""Anchors of tests/node_attn_ref.py (the plain float64 reference of the node side of an AttentionLayer and of MLPEmbedding) and of
its cases: together with edge_attn_ref's unfused edge operator the reference equals oracle.rollout_oracle.attention_layer in
float64; every weight variant and input regime reaches the path it is named for; the fp32 figures the device bars are four times of
still hold; every deliberately wrong variant fails compare_node - the comparison tests/test_node_attn_gpu.py applies - at those bars
on a (variant, regime, form) the GPU tests run, every slot mix-up on a `scales` variant; and the packer's split section holds the
matrices and scales the reference assumes."""
import math

import numpy as np
import pytest
import torch

import edge_attn_ref as ea
import node_attn_ref as na

GPU_ROWS = na.GPU_ROWS


class _f64:
    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)
        return False


def _tsd64(sd):
    return {k: torch.from_numpy(np.array(v)).double() if np.asarray(v).dtype.kind == 'f' else torch.from_numpy(np.array(v))
            for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('prefix,bip,with_r', [('agent_encoder.a2a_attn_layers.1', False, True), ('agent_encoder.a2a_attn_layers.1', False, False),
                                               ('agent_encoder.pt2a_attn_layers.0', True, True), ('agent_encoder.occ2sa_attn_layers.0', True, False)])
def test_reference_equals_the_oracle_layer(prefix, bip, with_r):
    """pre_ref -> edge_attn_ref (the unfused float64 edge operator on the affine-free LayerNorm of r) -> post_ref against the
    oracle's AttentionLayer on the raw r, in float64"""
    from oracle import rollout_oracle as ro
    sd = na.weights('plain')
    rng = np.random.default_rng(3)
    degs = [0, 3, 1, 7, 0, 12, 2, 5, 4, 1, 6]
    rows, n_src = len(degs), 14 if bip else len(degs)
    off, cnt, e_cap = ea._layout(rng, degs)
    src = rng.integers(0, n_src, e_cap).astype(np.int32)
    x = rng.standard_normal((rows, 128))
    xs = rng.standard_normal((n_src, 128)) if bip else None
    r = rng.standard_normal((e_cap, 128)) * rng.uniform(0.2, 5.0, (e_cap, 1))
    rhat = torch.nn.functional.layer_norm(torch.from_numpy(r), (128,)).numpy()
    q, u, _, _ = na.pre_ref(sd, prefix, x, 0)
    _, _, k, v = na.pre_ref(sd, prefix, xs if bip else x, 1)
    assert (u is not None) == ('occ2sa' not in prefix)
    if with_r:
        agg, z, sig = ea.edge_attn_ref(q, u.reshape(rows, -1), k, v, off, cnt, src, rhat)
    else:
        agg, z, sig = ea.edge_attn_ref(q, None, k, v, off, cnt, src, None)
    mine = na.post_ref(sd, prefix, x, agg, z, sig, 1 if with_r else 0)
    e_idx = np.concatenate([np.arange(off[i], off[i] + cnt[i]) for i in range(rows)])
    dst = torch.from_numpy(np.concatenate([np.full(cnt[i], i) for i in range(rows)])).long()
    with _f64(), torch.no_grad():
        ref = ro.attention_layer(_tsd64(sd), prefix, torch.from_numpy(x), torch.from_numpy(r[e_idx]) if with_r else None,
                                 torch.from_numpy(src[e_idx]).long(), dst, x_src_raw=torch.from_numpy(xs) if bip else None).numpy()
    assert np.abs(mine - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize('k0', na.MLP_K0)
def test_mlp_reference_equals_the_oracle(k0):
    from oracle import rollout_oracle as ro
    sd = na.mlp_weights('plain', k0)
    x = np.random.default_rng(k0).standard_normal((9, k0))
    with _f64(), torch.no_grad():
        ref = ro.mlp_embedding(_tsd64(sd), na.MLP_PREFIX, torch.from_numpy(x)).numpy()
    assert np.abs(na.mlp_embedding_ref(sd, na.MLP_PREFIX, x) - ref).max() <= 1e-12 * np.abs(ref).max()


def test_float32_evaluation_sums_in_ascending_k():
    """_dot in float32 is the running sum a plain loop gives, not a blocked product"""
    rng = np.random.default_rng(0)
    x, w = rng.standard_normal((3, 128)).astype(np.float32), rng.standard_normal((128, 5)).astype(np.float32)
    acc = np.zeros((3, 5), np.float32)
    for k in range(128):
        for i in range(3):
            for j in range(5):
                acc[i, j] = np.float32(acc[i, j] + np.float32(x[i, k] * w[k, j]))
    assert np.array_equal(na._dot(x, w, np.float32), acc)


# ------------------------------------------------------------------------------------------------ the cases reach their paths
def _exponents(sd, prefix):
    return [int(math.log2(p)) for p in na.prescales(sd, prefix)]


def test_plain_weights_hit_the_cap_in_every_slot():
    """the gap these tests close: with make_weights(seed=3) every operand scale is 2^-14"""
    for prefix in (na.POST_PREFIX, na.PRE_PREFIX):
        assert _exponents(na.weights('plain'), prefix) == [14] * 10
        assert _exponents(na.weights('ln'), prefix) == [14] * 10
    assert na.mlp_prescales(na.weights('plain')) == [2.0 ** 14] * 3


def test_scales_variants_spread_the_prescale_exponents():
    exps = {}
    for v in na.SCALES_VARIANTS:
        for prefix in (na.POST_PREFIX, na.PRE_PREFIX):
            e = _exponents(na.weights(v), prefix)
            assert e == [na.SCALE_EXPONENTS[v][s] for s in na.SLOTS]
            for part in (na.PRE_SLOTS, na.POST_SLOTS):
                pe = [e[i] for i in part]
                assert len(set(pe)) >= 3 and 14 in pe and min(pe) < 14
        exps[v] = _exponents(na.weights(v), na.POST_PREFIX)
        me = [int(math.log2(p)) for p in na.mlp_prescales(na.weights(v))]
        assert tuple(me) == na.MLP_SCALE_EXPONENTS[v] and len(set(me)) == 3 and 14 in me
    # every pair of slots of a part differs in at least one of the variants
    for part in (na.PRE_SLOTS, na.POST_SLOTS):
        for i, j in na._pairs(part):
            assert any(exps[v][i] != exps[v][j] for v in na.SCALES_VARIANTS), (i, j)
    for i, j in na._pairs(na.MLP_SLOTS):
        assert any(na.MLP_SCALE_EXPONENTS[v][i] != na.MLP_SCALE_EXPONENTS[v][j] for v in na.SCALES_VARIANTS)


def test_ln_variant_separates_the_layernorms():
    sd, plain = na.weights('ln'), na.weights('plain')
    for prefix in (na.POST_PREFIX, na.PRE_PREFIX):
        ratio = np.concatenate([sd[f'{prefix}.{n}.weight'] / plain[f'{prefix}.{n}.weight'] for n in na.LN_NAMES])
        assert ratio.min() < 0.3 and ratio.max() > 3.3 and ratio.min() >= 0.25 and ratio.max() <= 4.0
        assert max(np.abs(sd[f'{prefix}.{n}.bias']).max() for n in na.LN_NAMES) > 1.8
        assert np.array_equal(plain[f'{prefix}.attn_prenorm_x_dst.weight'], plain[f'{prefix}.attn_prenorm_x_src.weight'])
        for a in range(len(na.LN_NAMES)):
            for b in range(a + 1, len(na.LN_NAMES)):
                for p in ('weight', 'bias'):
                    d = np.abs(sd[f'{prefix}.{na.LN_NAMES[a]}.{p}'] - sd[f'{prefix}.{na.LN_NAMES[b]}.{p}'])
                    assert np.median(d) > 0.2, (prefix, a, b, p)


@pytest.mark.parametrize('regime', na.REGIMES)
def test_dead_ffn_zeroes_the_hidden_layer(regime):
    """exactly zero on every case row, in float64 and in the float32 evaluation; then ffn = b2"""
    sd = na.weights('dead_ffn')
    for rows in (na.SMALL_ROWS,):
        x, agg, z, sig = na.gen_inputs(regime, rows)
        for has_pos in (0, 1):
            for f in (np.float64, np.float32):
                assert (na.post_ref(sd, na.POST_PREFIX, x, agg, z, sig, has_pos, f=f, want='hidden') == 0).all()
            live = na.post_ref(na.weights('plain'), na.POST_PREFIX, x, agg, z, sig, has_pos, want='hidden')
            assert (live > 0).mean() > 0.2
    w1 = np.abs(na.weights('plain')[f'{na.POST_PREFIX}.ff_mlp.0.weight']).sum(1).max()
    g, b = (np.abs(na.weights('plain')[f'{na.POST_PREFIX}.ff_prenorm.{p}']).max() for p in ('weight', 'bias'))
    assert w1 * (g * math.sqrt(127.0) + b) < -na.DEAD_FFN_BIAS


def test_regime_b_covers_the_exponent_ranges():
    x, agg, _, _ = na.gen_inputs('B')
    xa = na.gen_inputs('A')[0]
    ex = np.array([na.x_exponent(i) for i in range(na.SMALL_ROWS)])
    eg = np.array([na.agg_exponent(i) for i in range(na.SMALL_ROWS)])
    for n in (GPU_ROWS, na.SMALL_ROWS):
        assert set(ex[:n]) == set(range(-20, 21)) and set(eg[:n]) == set(range(-10, 11))
    assert abs(np.corrcoef(ex, eg)[0, 1]) < 0.5                         # the two exponents are independent of each other
    top = np.abs(x).max(1)
    assert top.max() > 2.0 ** 20 and top.min() < 2.0 ** -18 and np.abs(agg).max(1).max() > 2.0 ** 9 and np.abs(agg).max(1).min() < 2.0 ** -9
    # after the residual: the large rows keep their magnitude, the small ones are carried by the two post-norm terms
    x2 = na.reference('plain', 'B', 'post1')['X']
    t2 = np.abs(x2).max(1)
    assert (t2[ex == 20] > 2.0 ** 20).all() and (t2[ex == -20] < 16.0).all() and (t2[ex == -20] > 0.5).all()
    assert int(np.log2(t2.max())) - int(np.log2(t2.min())) >= 20
    assert xa.shape == x.shape


def test_regime_c_has_its_degenerate_rows():
    x, agg, z, sig = na.gen_inputs('C')
    for b in na.C_BLOCKS:
        assert (x[b] == 0).all() and (x[b + 1] == 1.5).all() and (x[b + 2] == -0.75).all()
        for c in na.CONST_ROWS:                     # the partial sums of a constant row are exact in float32
            assert np.float32(c) * 128 == np.add.accumulate(np.full(128, c, np.float32))[-1]
        assert (agg[b + 3:b + 5] == 0).all() and (z[b + 3:b + 5] == 0).all() and (sig[b + 3:b + 5] == 0).all() and np.abs(x[b + 3]).max() > 0
        for r in (b + 5, b + 6):
            top = np.abs(z[r]).max(1)
            assert (top <= na.Z_BOUND).all() and (top >= 0.99 * na.Z_BOUND).all() and (sig[r] == 1).all()
            assert (z[r].max(1) > 11).any() and (z[r].min(1) < -11).any()
        assert (agg[b + 7] == 0).all() and np.abs(z[b + 7]).max() > 0.1
        assert not x[b + 8].any() and not agg[b + 8].any() and not z[b + 8].any() and not sig[b + 8].any()
    assert na.C_BLOCKS[0] + 9 <= 15 and na.C_BLOCKS[1] + 9 > 64 > na.C_BLOCKS[1] and na.C_BLOCKS[2] + 9 == na.SMALL_ROWS
    # the nominal Z stays well inside its bound, SIG has zeros, ones and fractions
    za, sa = na.gen_inputs('A')[2:]
    assert np.abs(za).max() < 0.6 * na.Z_BOUND and (sa == 0).any() and (sa == 1).any() and ((sa > 0) & (sa < 1)).any()
    # a row with SIG = 0 next to a non-zero Z exists (what skip_z_sig0 needs)
    assert ((sa == 0) & (np.abs(za).max(2) > 0.1)).any()


def test_row_counts_and_large_shapes():
    assert na.ROW_COUNTS == [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129] and max(na.ROW_COUNTS) == na.SMALL_ROWS
    assert na.PERSISTENT_ROWS == 32768 + 69 and na.SWITCH_ROWS == [6144, 6145, 10240, 10241]
    tiles = -(-na.PERSISTENT_ROWS // 64)
    assert tiles == 512 + 2 and na.PERSISTENT_ROWS % 64 == 5            # two workgroups take a second tile, the last one is partial
    assert na.CYCLE_ROWS % 64 and na.CYCLE_ROWS % 16 and math.gcd(na.CYCLE_ROWS, 64) == 1


# ------------------------------------------------------------------------------------------------ the fp32 figures
def fp32_figures():
    """{(output, regime): largest row error of the float32 evaluation against float64 over variants and forms, the cyclic block included}"""
    fig = {}

    def note(out, regime, got, ref):
        fig[out, regime] = max(fig.get((out, regime), 0.0), na.row_error(got, ref))

    for regime in na.REGIMES:
        for variant in na.VARIANTS:
            for form in na.FORMS:
                got, ref = na.evaluate(variant, regime, form, f=np.float32), na.reference(variant, regime, form)
                for o in ref:
                    note(o, regime, got[o], ref[o])
    for form in ('post_pre4', 'post_pre_fused'):
        got, ref = na.evaluate('plain', 'A', form, f=np.float32, rows=na.CYCLE_ROWS), na.reference('plain', 'A', form, na.CYCLE_ROWS)
        for o in ref:
            note(o, 'A', got[o], ref[o])
    for regime in na.MLP_REGIMES:
        for variant in na.MLP_VARIANTS:
            for k0 in na.MLP_K0:
                x = na.gen_mlp_inputs(regime, na.MLP_ROWS)[:, :k0]
                note('MLPEMB', regime, na.mlp_embedding_ref(na.mlp_weights(variant, k0), na.MLP_PREFIX, x, f=np.float32),
                     na.mlp_reference(variant, regime, k0, na.MLP_ROWS))
    x = na.gen_mlp_inputs('A', na.CYCLE_ROWS)
    note('MLPEMB', 'A', na.mlp_embedding_ref(na.mlp_weights('plain', 512), na.MLP_PREFIX, x, f=np.float32),
         na.mlp_reference('plain', 'A', 512, na.CYCLE_ROWS))
    return fig


def test_fp32_figures_are_pinned():
    """the pinned FP32_ERR_NODE_* reproduce: none is exceeded, none has drifted below 0.7 of its pin (the tolerance of the edge
    figures: numpy's float32 exp may differ in the last place between builds; the pins are the measured figures rounded up)"""
    fig = fp32_figures()
    assert set(fig) == {(o, g) for o in na.OUTPUTS for g in na.REGIMES} | {('MLPEMB', g) for g in na.MLP_REGIMES}
    bad = []
    for (o, g), e in sorted(fig.items()):
        pin = na.fp32_err(o, g)
        print(f'FP32_ERR_NODE_{o}_{g} = {e:.3e} (pinned {pin:.3e}, bar {na.bar(o, g):.3e})')
        if not 0.7 * pin <= e <= pin:
            bad.append((o, g, e, pin))
        assert na.bar(o, g) == 4 * pin
    assert not bad, bad


def test_float32_evaluation_passes_the_comparison():
    for regime in na.REGIMES:
        for variant in na.VARIANTS:
            for form in na.FORMS:
                na.compare_node(regime, na.evaluate(variant, regime, form, f=np.float32), na.reference(variant, regime, form))


# ------------------------------------------------------------------------------------------------ the wrong variants are caught
# variant -> (weight variant, regime, form) of the GPU tests (first GPU_ROWS rows) on which compare_node fails at the bars
CAUGHT_ON = {
    'ln_src_for_dst': ('ln', 'A', 'post1'), 'ln_dst_for_src': ('ln', 'A', 'pre_src_kv'), 'post_for_ffpre': ('ln', 'A', 'post0'),
    'bprime_no_beta': ('ln', 'A', 'post1'), 'gate_swapped': ('plain', 'A', 'post0'), 'drop_ffn_chunk': ('plain', 'A', 'post0'),
    'bv_on_k': ('plain', 'A', 'pre_src_kv'), 'u_no_scale': ('plain', 'A', 'pre_dst4'), 'u_swap_h4': ('plain', 'A', 'post_pre4'),
    'z_stride64': ('plain', 'A', 'post1'), 'skip_z_sig0': ('plain', 'A', 'post1'),
}


def _slot_forms(mutate):
    i = int(mutate[len('scale_')])
    return ('post_pre4', 'pre_dst4') if i in na.PRE_SLOTS else ('post1', 'post_pre4') if i == 4 else ('post0', 'post1', 'post_pre4', 'post_pre_fused')


def _fails(mutate, variant, regime, form):
    ref = {o: r[:GPU_ROWS] for o, r in na.reference(variant, regime, form).items()}
    got = {o: r[:GPU_ROWS] for o, r in na.evaluate(variant, regime, form, mutate=mutate).items()}
    na.compare_node(regime, ref, ref)
    try:
        na.compare_node(regime, got, ref)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize('mutate', [m for m in na.MUTANTS if m not in na.SLOT_MUTANTS])
def test_wrong_variant_fails_the_comparison(mutate):
    assert _fails(mutate, *CAUGHT_ON[mutate])


@pytest.mark.parametrize('mutate', na.SLOT_MUTANTS)
def test_slot_mix_up_fails_on_a_scales_variant(mutate):
    """on every form that reads the slot, in at least one of the two scales variants (in both where the two exponents differ in
    both) - and on no form with the plain weights, where every slot holds 2^-14: the gap"""
    i, j = mutate[len('scale_'):].split('_as_')
    i, j = int(i.rstrip('ax')), int(j)
    for form in _slot_forms(mutate):
        caught = {v: _fails(mutate, v, 'A', form) for v in na.SCALES_VARIANTS}
        differ = {v: na.SCALE_EXPONENTS[v][na.SLOTS[i]] != na.SCALE_EXPONENTS[v][na.SLOTS[j]] for v in na.SCALES_VARIANTS}
        assert caught == differ and any(caught.values()), (mutate, form, caught, differ)
        assert not _fails(mutate, 'plain', 'A', form)


@pytest.mark.parametrize('mutate', na.MLP_SLOT_MUTANTS)
def test_mlp_slot_mix_up_fails_on_a_scales_variant(mutate):
    i, j = (int(v) for v in mutate[len('mlp_scale_'):].split('_as_'))
    hit = False
    for v in na.SCALES_VARIANTS:
        x = na.gen_mlp_inputs('A', na.MLP_ROWS)
        ref = dict(MLPEMB=na.mlp_reference(v, 'A', 512, na.MLP_ROWS))
        got = dict(MLPEMB=na.mlp_embedding_ref(na.mlp_weights(v, 512), na.MLP_PREFIX, x, mutate=mutate))
        differ = na.MLP_SCALE_EXPONENTS[v][i] != na.MLP_SCALE_EXPONENTS[v][j]
        if differ:
            with pytest.raises(AssertionError):
                na.compare_node('A', got, ref)
            hit = True
        else:
            na.compare_node('A', got, ref)
    assert hit


# ------------------------------------------------------------------------------------------------ the packer
def _unpack_matrix_h(halfs):
    """inverse of packing.pack_matrix_h(natural_k=False): [k-step 4][tile 8][hi, lo][lane 64][slot 8] fp16 -> hi + lo [128][128]"""
    v = np.asarray(halfs, np.uint16).view(np.float16).astype(np.float64).reshape(4, 8, 2, 64, 8).sum(2)
    s_, t_, l_, p_ = np.meshgrid(np.arange(4), np.arange(8), np.arange(64), np.arange(8), indexing='ij')
    w = np.zeros((128, 128))
    w[16 * t_ + (l_ & 15), 32 * s_ + 16 * (p_ >> 2) + 4 * (l_ >> 4) + (p_ & 3)] = v
    return w


def _unpack_wvr_h(halfs):
    v = np.asarray(halfs, np.uint16).view(np.float16).astype(np.float64).reshape(8, 4, 2, 64, 8).sum(2)
    h_, s_, l_, p_ = np.meshgrid(np.arange(8), np.arange(4), np.arange(64), np.arange(8), indexing='ij')
    w = np.zeros((128, 128))
    w[16 * h_ + (l_ & 15), 32 * s_ + 8 * (l_ >> 4) + p_] = v
    return w


def _unpack_wkr_h(halfs):
    v = np.asarray(halfs, np.uint16).view(np.float16).astype(np.float64).reshape(8, 8, 2, 64, 4).sum(2)
    h_, c_, l_, p_ = np.meshgrid(np.arange(8), np.arange(8), np.arange(64), np.arange(4), indexing='ij')
    w = np.zeros((128, 128))
    w[16 * h_ + 4 * (l_ >> 4) + p_, 16 * c_ + (l_ & 15)] = v
    return w


def _close(got, want):
    return np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()


@pytest.mark.parametrize('variant', na.VARIANTS)
def test_packer_scales_match_the_matrices_they_were_applied_to(variant):
    """hdr[i] x prescale_i = 1 with the prescale of the documented rule on the matrix of slot i, and the hi + lo planes of every
    split matrix give that matrix times its prescale back to 2^-22 of its largest entry"""
    from infgen_amd import _lib, packing
    lib = _lib.load()
    sd = na.weights(variant)
    M = 32768                                                          # fp16 values per split matrix (four quarters)
    for prefix in (na.POST_PREFIX, na.PRE_PREFIX):
        pack = packing.pack_attention_layer(sd, prefix)
        hdr = pack[lib.infgen_attn_pack_offset(b'h_hdr'):][:16]
        pres, mats = na.prescales(sd, prefix), na.slot_matrices(sd, prefix)
        assert [float(h) * p for h, p in zip(hdr[:10], pres)] == [1.0] * 10
        o = lib.infgen_attn_pack_offset(b'h_pre')
        halfs = pack[o:o + 17 * M // 2].view(np.uint16)
        m = lambda n: halfs[n * M:(n + 1) * M]
        w = [a.astype(np.float64) * p for a, p in zip(mats, pres)]
        assert _close(_unpack_matrix_h(m(0)), w[0]) and _close(_unpack_wkr_h(m(1)), w[1])
        assert _close(_unpack_matrix_h(m(2)), w[2]) and _close(_unpack_matrix_h(m(3)), w[3])
        assert _close(_unpack_wvr_h(m(4)), w[4])
        assert _close(_unpack_matrix_h(m(5)), w[5][:, :128]) and _close(_unpack_matrix_h(m(6)), w[5][:, 128:])
        assert _close(_unpack_matrix_h(m(7)), w[6]) and _close(_unpack_matrix_h(m(8)), w[7])
        for c in range(4):
            assert _close(_unpack_matrix_h(m(9 + 2 * c)), w[8][128 * c:128 * (c + 1), :])
            assert _close(_unpack_matrix_h(m(10 + 2 * c)), w[9][:, 128 * c:128 * (c + 1)])
    if variant in na.MLP_VARIANTS:
        for k0 in na.MLP_K0:
            msd = na.mlp_weights(variant, k0)
            pack = packing.pack_mlp_embedding(msd, na.MLP_PREFIX)
            oh = (k0 * 128 + 3 * 128) + (16384 + 3 * 128) + (16384 + 128)          # the three fp32 stages, then the split section
            pres = na.mlp_prescales(msd)
            assert [float(h) * p for h, p in zip(pack[oh:oh + 3], pres)] == [1.0] * 3
            halfs = pack[oh + 16:].view(np.uint16)
            ws = [np.asarray(msd[f'{na.MLP_PREFIX}.mlp.{i}.weight'], np.float64) * p for i, p in zip((0, 3, 6), pres)]
            n0 = k0 // 128
            assert halfs.size == (n0 + 2) * M
            for c in range(n0):
                assert _close(_unpack_matrix_h(halfs[c * M:(c + 1) * M]), ws[0][:, 128 * c:128 * (c + 1)])
            assert _close(_unpack_matrix_h(halfs[n0 * M:(n0 + 1) * M]), ws[1]) and _close(_unpack_matrix_h(halfs[(n0 + 1) * M:]), ws[2])
