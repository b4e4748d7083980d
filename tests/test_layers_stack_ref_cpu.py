"""Anchors of tests/layers_stack_ref.py (the plain float64 reference of the 18 sublayers of a decode step) and of its cases: the
chain equals 18 chained calls of oracle.rollout_oracle.attention_layer in float64 on the raw relative-position rows; the fused and
the unfused composition of the edge side agree; the fp32 figures the device bars are four times of still hold and the float32
evaluation passes the comparison; every deliberately wrong variant fails compare_stack - the comparison
tests/test_layers_stack_gpu.py applies - at those bars, every slot mix-up and the header of the neighbouring layer on a `scales`
variant; the weight variants show in the packer's headers of all 18 layers; the input regimes hold the rows they are named for."""
import functools
import math

import numpy as np
import pytest
import torch

import edge_attn_ref as ea
import layers_stack_ref as ls
import node_attn_ref as na
from test_node_attn_ref_cpu import _f64, _tsd64


# ------------------------------------------------------------------------------------------------ anchors
def test_chain_equals_eighteen_oracle_layers():
    """a scene of 11 agents (rows 9 and 10 without any edge) and 14 map tokens, a ring of 4 columns whose cached K / V rows are the
    projections of raw feature rows: the chain on the affine-free LayerNorm of r against the oracle's AttentionLayer on the raw r,
    the temporal layers over all ring * rows nodes, the map layers bipartite"""
    from oracle import rollout_oracle as ro
    sd = ls.weights('plain')
    rng = np.random.default_rng(5)
    rows, n_map, ring, slot = 11, 14, 4, 1
    degs = dict(t=[2, 1, 0, 3, 1, 0, 2, 1, 3, 0, 0], m=[5, 0, 3, 1, 4, 2, 0, 5, 1, 0, 0], a=[8, 3, 0, 1, 7, 2, 5, 0, 4, 0, 0])
    edges, raw = {}, {}
    for kind in ls.KINDS:
        off, cnt, e_cap = ea._layout(rng, degs[kind])
        src = np.zeros(e_cap, np.int32)
        for r in range(rows):
            c = cnt[r]
            if kind == 't':
                src[off[r]:off[r] + c] = rng.permutation([s for s in range(ring) if s != slot])[:c] * rows + r
            else:
                src[off[r]:off[r] + c] = rng.permutation(n_map if kind == 'm' else 9)[:c]
        raw[kind] = rng.standard_normal((e_cap, 128)) * rng.uniform(0.2, 5.0, (e_cap, 1))
        rhat = torch.nn.functional.layer_norm(torch.from_numpy(raw[kind]), (128,)).numpy()
        edges[kind] = (off, cnt, src, rhat)
    x = rng.standard_normal((rows, 128))
    hist = rng.standard_normal((ls.L, ring * rows, 128))           # the residual stream of the ring's columns entering each triple
    x_pt = rng.standard_normal((n_map, 128))
    ringK, ringV, mapK, mapV = [], [], [], []
    for i in range(ls.L):
        _, _, k, v = na.pre_ref(sd, ls.prefix(i, 't'), hist[i], 1)
        ringK.append(k), ringV.append(v)
        _, _, k, v = na.pre_ref(sd, ls.prefix(i, 'm'), x_pt, 1)
        mapK.append(k), mapV.append(v)
    mine = ls.stack_ref(sd, x, ringK, ringV, slot, mapK, mapV, edges)

    def lists(kind):
        off, cnt, src, _ = edges[kind]
        e = np.concatenate([np.arange(off[i], off[i] + cnt[i]) for i in range(rows)])
        dst = np.concatenate([np.full(cnt[i], i) for i in range(rows)])
        return torch.from_numpy(raw[kind][e]), torch.from_numpy(src[e]).long(), torch.from_numpy(dst).long()

    tsd = _tsd64(sd)
    taps = dict(RK={}, RV={}, KA={}, VA={})

    def kv(p, xin):            # the oracle's own key / value projections of the rows entering layer p (attention_layer's first lines)
        xs = ro._ln(tsd, p + '.attn_prenorm_x_src', xin)
        return ro._lin(tsd, p + '.to_k', xs, bias=False).numpy(), ro._lin(tsd, p + '.to_v', xs).numpy()

    with _f64(), torch.no_grad():
        xo = torch.from_numpy(x)
        for i in range(ls.L):
            taps['RK'][i], taps['RV'][i] = kv(ls.prefix(i, 't'), xo)
            nodes = torch.from_numpy(hist[i]).clone()
            nodes[slot * rows:(slot + 1) * rows] = xo
            r, s, d = lists('t')
            xo = ro.attention_layer(tsd, ls.prefix(i, 't'), nodes, r, s, d + slot * rows)[slot * rows:(slot + 1) * rows]
            r, s, d = lists('m')
            xo = ro.attention_layer(tsd, ls.prefix(i, 'm'), xo, r, s, d, x_src_raw=torch.from_numpy(x_pt))
            r, s, d = lists('a')
            if i >= ls.L - 2:
                taps['KA'][i], taps['VA'][i] = kv(ls.prefix(i, 'a'), xo)
            xo = ro.attention_layer(tsd, ls.prefix(i, 'a'), xo, r, s, d)
    ref = xo.numpy()
    assert np.abs(mine['X'] - ref).max() <= 1e-11 * np.abs(ref).max()
    # the other observables: the oracle's projections of ITS residual stream entering every triple / the last two agent layers
    for o, want in taps.items():
        assert sorted(mine[o]) == sorted(want) and len(want) == (ls.L if o[0] == 'R' else 2)
        for i, w in want.items():
            assert np.abs(mine[o][i] - w).max() <= 1e-11 * np.abs(w).max(), (o, i)


def test_fused_and_unfused_compositions_agree():
    """float64: edge_attn_fused_ref -> post_ref(has_pos = 0) against pre_ref's U -> edge_attn_ref -> post_ref(has_pos = 1), the form
    the float32 evaluation and the mutants take"""
    a, b = ls.flatten(ls.reference('scales_a', 'A')), ls.flatten(ls.run('scales_a', 'A', fused=False))
    for o in ls.OUTPUTS:
        assert np.abs(a[o] - b[o]).max() <= 1e-9 * np.abs(a[o]).max(), o      # (float64 rounding through 18 sublayers)


# ------------------------------------------------------------------------------------------------ the variants do what they claim
def _header(variant, p):
    from infgen_amd import _lib, packing
    lib = _lib.load()
    pack = packing.pack_attention_layer(ls.weights(variant), p)
    return pack[lib.infgen_attn_pack_offset(b'h_hdr'):][:16]


@functools.lru_cache(maxsize=None)
def _headers(variant):
    return [_header(variant, p) for p in ls.PREFIXES]


def test_plain_weights_hit_the_cap_in_all_18_layers():
    for v in ('plain', 'ln', 'ln_peaked', 'dead_ffn'):
        for h in _headers(v):
            assert [float(x) for x in h[:10]] == [2.0 ** -14] * 10


def test_scales_variants_spread_the_exponents_in_every_layer():
    exps = {v: [[-int(math.log2(float(x))) for x in h[:10]] for h in _headers(v)] for v in ls.SCALES_VARIANTS}
    for v in ls.SCALES_VARIANTS:
        for k in range(18):
            assert exps[v][k] == [ls.scale_exponents(v, k)[s] for s in na.SLOTS], (v, k)
            assert exps[v][k] == [int(math.log2(p)) for p in na.prescales(ls.weights(v), ls.PREFIXES[k])]
    for k in range(18):
        for part in (na.PRE_SLOTS, na.POST_SLOTS):          # the slots one kernel part reads differ pairwise in a variant
            for i, j in na._pairs(part):
                assert any(exps[v][k][i] != exps[v][k][j] for v in ls.SCALES_VARIANTS), (k, i, j)
        if k + 1 < 18:                                       # the same slot differs from sublayer to sublayer in BOTH variants,
            for v in ls.SCALES_VARIANTS:                    # so a header taken from P where NP belongs cancels nowhere
                assert all(a != b for a, b in zip(exps[v][k], exps[v][k + 1])), (v, k)
        if k + 3 < 18:                                       # and from layer i to layer i + 1 of the same kind
            for v in ls.SCALES_VARIANTS:
                assert all(a != b for a, b in zip(exps[v][k], exps[v][k + 3])), (v, k)


def test_ln_variant_gives_every_layernorm_parameters_of_its_own():
    sd, plain = ls.weights('ln'), ls.weights('plain')
    seen = []
    for p in ls.PREFIXES:
        ratio = np.concatenate([sd[f'{p}.{n}.weight'] / plain[f'{p}.{n}.weight'] for n in ls.LN_NAMES if 'x_dst' not in n])
        assert 0.25 <= ratio.min() < 0.3 and 3.3 < ratio.max() <= 4.0
        assert max(np.abs(sd[f'{p}.{n}.bias']).max() for n in ls.LN_NAMES) > 1.8
        same = all(np.array_equal(sd[f'{p}.attn_prenorm_x_dst.{q}'], sd[f'{p}.attn_prenorm_x_src.{q}']) for q in ('weight', 'bias'))
        assert same == ('pt2a' not in p), p              # equal in the non-bipartite layers (layers.py:52-53), apart in the map layers
        for n in ls.LN_NAMES:
            if n == 'attn_prenorm_x_dst' and same:
                continue
            seen.append(sd[f'{p}.{n}.weight'])
    for a in range(len(seen)):
        for b in range(a + 1, len(seen)):
            assert np.median(np.abs(seen[a] - seen[b])) > 0.2
    for k, h in enumerate(_headers('ln')):
        p = ls.PREFIXES[k]
        want = [np.abs(sd[f'{p}.{n}']).max() for n in ('ff_prenorm.weight', 'ff_prenorm.bias', 'attn_prenorm_x_dst.weight', 'attn_prenorm_x_dst.bias')]
        assert [float(x) for x in h[10:14]] == [float(np.float32(w)) for w in want]


def test_ln_peaked_moves_the_bounds_from_layer_to_layer():
    sd = ls.weights('ln_peaked')
    hd = _headers('ln_peaked')
    feats = set()
    for k, h in enumerate(hd):
        p = ls.PREFIXES[k]
        for slot, name in ((10, 'ff_prenorm'), (12, 'attn_prenorm_x_dst')):
            g = sd[f'{p}.{name}.weight']
            feat, peak = ls.peak_of(name, k)
            assert g[feat] == peak == float(h[slot]) == np.abs(g).max() and np.delete(g, feat).max() <= 1.0
            feats.add((name, feat))
        assert float(h[11]) == np.abs(sd[f'{p}.ff_prenorm.bias']).max() and float(h[13]) == np.abs(sd[f'{p}.attn_prenorm_x_dst.bias']).max()
        if 'pt2a' not in p:
            assert np.array_equal(sd[f'{p}.attn_prenorm_x_dst.weight'], sd[f'{p}.attn_prenorm_x_src.weight'])
        if k:
            for slot in (10, 12):
                r = float(h[slot]) / float(hd[k - 1][slot])
                assert r >= 2 or r <= 0.5, (k, slot, r)
        assert float(h[10]) / float(h[12]) >= 2 or float(h[10]) / float(h[12]) <= 0.5       # (the two bounds of one header too)
    assert len(feats) == 36
    assert {float(h[10]) for h in hd} == set(ls.PEAKS) == {float(h[12]) for h in hd}


def test_dead_ffn_zeroes_every_hidden_layer():
    sd = ls.weights('dead_ffn')
    x = ls.gen_values('B')[0]
    for p in (ls.PREFIXES[0], ls.PREFIXES[10], ls.PREFIXES[17]):
        z = np.zeros((len(x), 128))
        assert (na.post_ref(sd, p, x, z, None, None, 0, want='hidden') == 0).all()
        w1 = np.abs(ls.weights('plain')[f'{p}.ff_mlp.0.weight']).sum(1).max()
        g, b = (np.abs(ls.weights('plain')[f'{p}.ff_prenorm.{q}']).max() for q in ('weight', 'bias'))
        assert w1 * (g * math.sqrt(127.0) + b) < -na.DEAD_FFN_BIAS


# ------------------------------------------------------------------------------------------------ the regimes hold their rows
@pytest.mark.parametrize('a_cap', [32, 64])
def test_regime_b_covers_the_exponent_ranges(a_cap):
    X, rk, rv, mk, mv = ls.gen_values('B', a_cap)
    XA = ls.gen_values('A', a_cap)[0]
    rows = len(X)
    assert {ls.x_exponent(i) for i in range(rows)} == set(range(-20, 21))
    top = np.abs(X).max(1)
    assert top.max() > 2.0 ** 20 and top.min() < 2.0 ** -18 and np.abs(XA).max() < 8
    for a in (rk, rv, mk, mv):
        t = np.abs(a).max(-1)
        assert t.max() > 2.0 ** 10 and t.min() < 2.0 ** -8
    for s in range(ls.RING):                               # every ring slot, and the map rows, see the whole exponent range
        assert {ls.kv_exponent(i + s) for i in range(rows)} == set(range(-10, 11))
    assert {ls.kv_exponent(i) for i in range(len(ls.BASE_SCENES[a_cap]) * ls.M_CAP)} == set(range(-10, 11))


@pytest.mark.parametrize('a_cap', [32, 64])
def test_regime_c_has_its_degenerate_rows(a_cap):
    X = ls.gen_values('C', a_cap)[0]
    scenes = ls.BASE_SCENES[a_cap]
    deg = ls.degenerate_rows(a_cap)
    kinds = {('zero' if k == 'zero' else 'const', (r % a_cap) < scenes[r // a_cap][0]) for r, k in deg.items()}
    assert kinds == {('zero', True), ('zero', False), ('const', True), ('const', False)}      # among agents and among padding rows
    for r, k in deg.items():
        assert (X[r] == (0.0 if k == 'zero' else k)).all()
    for c in ls.CONST_ROWS:
        assert np.float32(c) * 128 == np.add.accumulate(np.full(128, c, np.float32))[-1]
    assert any(n == 1 for n, _ in scenes) and all(n <= a_cap for n, _ in scenes) and max(n for n, _ in scenes) == a_cap
    e = ls.gen_edges(a_cap)
    allempty = (e['t'][1] == 0) & (e['m'][1] == 0) & (e['a'][1] == 0)
    agent = np.array([(r % a_cap) < scenes[r // a_cap][0] for r in range(len(X))])
    assert allempty[~agent].all() and allempty[agent].any()           # padding rows, and an agent, without any edge
    counts = np.concatenate([e[k][1] for k in ls.KINDS])
    assert {0, 1, 2, 3} <= set(counts) and e['a'][1].max() == a_cap - 1
    one = scenes.index(next(s for s in scenes if s[0] == 1))
    assert e['a'][1][one * a_cap] == 0                                    # the agent that is alone in its scene


# ------------------------------------------------------------------------------------------------ the fp32 figures
FIGURE_CASES = [(v, g, 32) for g in ls.REGIMES for v in ls.VARIANTS] + [('scales_a', 'A', 64), ('ln_peaked', 'A', 64)]


@functools.lru_cache(maxsize=None)
def _fp32(variant, regime, a_cap):
    return ls.flatten(ls.run(variant, regime, a_cap, f=np.float32))


def fp32_figures():
    """{(output, regime): largest row error of the float32 evaluation against float64 over FIGURE_CASES: every (variant, regime)
    on the base block of 32-row scenes, the two variants the GPU tests run on the 64-row scenes}"""
    fig = {}
    for v, g, a_cap in FIGURE_CASES:
        got, ref = _fp32(v, g, a_cap), ls.flatten(ls.reference(v, g, a_cap))
        for o in ls.OUTPUTS:
            fig[o, g] = max(fig.get((o, g), 0.0), na.row_error(got[o], ref[o]))
    return fig


def test_fp32_figures_are_pinned():
    """the pinned FP32_ERR_STACK_* reproduce: none is exceeded, none has drifted below 0.7 of its pin (numpy's float32 exp may
    differ in the last place between builds; the pins are the measured figures rounded up)"""
    fig = fp32_figures()
    assert set(fig) == {(o, g) for o in ls.OUTPUTS for g in ls.REGIMES}
    bad = []
    for (o, g), e in sorted(fig.items()):
        pin = ls.fp32_err(o, g)
        print(f'FP32_ERR_STACK_{o}_{g} = {e:.3e} (pinned {pin:.3e}, bar {ls.bar(o, g):.3e})')
        if not 0.7 * pin <= e <= pin:
            bad.append((o, g, e, pin))
        assert ls.bar(o, g) == 4 * pin
    assert not bad, bad


def test_float32_evaluation_passes_the_comparison():
    for v, g, a_cap in FIGURE_CASES:
        ls.compare_stack(g, _fp32(v, g, a_cap), ls.flatten(ls.reference(v, g, a_cap)))


# ------------------------------------------------------------------------------------------------ the wrong variants are caught
def _fails(mutate, variant, regime, first, last):
    got, ref = ls.run_part(variant, regime, first, last, mutate=mutate)
    ls.compare_stack(regime, ref, ref)
    try:
        ls.compare_stack(regime, got, ref)
    except AssertionError:
        return True
    return False


def _fails_full(mutate, variant, regime):
    """the whole 18-sublayer chain with the mutant against the reference, on exactly the outputs the GPU tests compare"""
    ref = ls.flatten(ls.reference(variant, regime))
    got = ls.flatten(ls.run(variant, regime, mutate=mutate))
    assert set(got) == set(ref) == set(ls.OUTPUTS)
    try:
        ls.compare_stack(regime, got, ref)
    except AssertionError:
        return True
    return False


# mutant -> (weight variant, regime) of the GPU tests on which compare_stack fails at the bars, over the full chain
CAUGHT_ON = {
    'stale_agent_kv': ('plain', 'A'), 'half_list_dropped': ('plain', 'A'), 'empty_half_poisons': ('plain', 'C'),
    'ring_slot_off_by_one': ('plain', 'A'), 'map_src_ln_dst': ('ln', 'A'), 'skip_last_ffn': ('plain', 'A'),
}


@pytest.mark.parametrize('mutate', list(CAUGHT_ON))
def test_wrong_variant_fails_the_comparison(mutate):
    assert _fails_full(mutate, *CAUGHT_ON[mutate])


@pytest.mark.parametrize('variant', ls.SCALES_VARIANTS)
def test_header_of_the_previous_layer_fails_on_a_scales_variant(variant):
    assert _fails_full('hdr_of_previous_layer', variant, 'A')
    assert not _fails('hdr_of_previous_layer', 'plain', 'A', 0, 3)          # every slot 2^-14: the gap


@pytest.mark.parametrize('mutate', na.SLOT_MUTANTS)
def test_slot_mix_up_deep_in_the_stack_fails_on_a_scales_variant(mutate):
    """at layer 3's map -> agent sublayer (post part of pt2a_attn_layers.3, pre part of a2a_attn_layers.3), judged by the ring rows
    of layer 4 and the X two sublayers on: caught in exactly the variants whose two exponents differ there, in at least one"""
    i, j = mutate[len('scale_'):].split('_as_')
    i, j = int(i.rstrip('ax')), int(j)
    k = ls.MUTANT_AT + (1 if i in na.PRE_SLOTS else 0)
    caught = {v: _fails(mutate, v, 'A', ls.MUTANT_AT, ls.MUTANT_AT + 2) for v in ls.SCALES_VARIANTS}
    differ = {v: ls.scale_exponents(v, k)[na.SLOTS[i]] != ls.scale_exponents(v, k)[na.SLOTS[j]] for v in ls.SCALES_VARIANTS}
    assert caught == differ and any(caught.values()), (mutate, caught, differ)
    assert not _fails(mutate, 'plain', 'A', ls.MUTANT_AT, ls.MUTANT_AT + 2)


def test_every_mutant_has_a_test():
    assert set(ls.MUTANTS) == set(na.SLOT_MUTANTS) | set(CAUGHT_ON) | {'hdr_of_previous_layer'}
