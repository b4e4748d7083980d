"""Anchors of tests/fourier_ref.py (the plain float64 reference of FourierEmbedding and of its last-dim table) and of its cases: the
reference equals oracle.rollout_oracle.fourier_embedding in float64 once both take the same float32-rounded arguments; the table
form equals the plain operator on integer gaps 0 .. -31; the float32 and hardware-sine figures the device bars are four times of
still hold; the `scales` variants reach the prescale exponents they are named for and packing.pack_fourier's header holds their
reciprocals; every deliberately wrong evaluation is at least 4 x the bar away on a case of fourier_ref.CASES - the list
tests/test_fourier_gpu.py runs; and the input regimes and row counts reach the paths they are named for.  n = 1, non-finite
inputs and k_fourier_h12_multi are outside these tests (fourier_ref.py, test_fourier_gpu.py say why)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import fourier_ref as fr
from conftest import REPO

GPU_ROWS = fr.GPU_ROWS


class _f64:
    """oracle operators evaluated in float64 (the oracle allocates with torch's default dtype)"""

    def __enter__(self):
        self.old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *exc):
        torch.set_default_dtype(self.old)
        return False


# ------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize('variant', ['plain', 'freq'])
@pytest.mark.parametrize('prefix', list(fr.PREFIXES))
def test_reference_equals_the_oracle(prefix, variant):
    """regime A.  The oracle forms z in the dtype it is given, the operator is defined on the float32 z: so (1) the float32
    argument is the oracle's own expression on float32 tensors, bit for bit, and (2) everything behind the features is compared
    by handing the oracle the same features - its cos / sin / concatenation replaced by the reference's float32-argument
    features - to 1e-12 relative"""
    from oracle import rollout_oracle as ro
    sd = fr.weights(variant)
    n = fr.PREFIXES[prefix]
    raw = fr.gen_inputs('A', prefix)
    x32 = torch.from_numpy(np.array(raw[:, :n]))
    z_oracle = (x32.unsqueeze(-1) * torch.from_numpy(np.array(sd[f'{prefix}.freqs.weight'])) * 2 * math.pi).numpy()
    z = np.stack([fr.argument(sd, prefix, i, raw[:, i]) for i in range(n)], axis=1)
    assert z.dtype == np.float32 and np.array_equal(z.view(np.int32), z_oracle.view(np.int32))
    assert np.abs(z).max() > (900.0 if variant == 'freq' else 10.0)

    tsd = {k: torch.from_numpy(np.array(v)).double() for k, v in sd.items() if k.startswith(prefix + '.')}
    feats = torch.from_numpy(np.stack([fr.features(sd, prefix, i, raw[:, i]) for i in range(n)], axis=1))       # [rows][n][128]
    cat = fr.gen_cat() if prefix == fr.CAT_PREFIX else None

    def oracle_behind_the_features():
        # rollout_oracle.fourier_embedding from its `for i in range(n)` on, fed f = [features ; x]
        f = torch.cat([feats, x32.double().unsqueeze(-1)], dim=-1)
        embs = []
        for i in range(n):
            h = ro._lin(tsd, f'{prefix}.mlps.{i}.0', f[:, i])
            h = torch.nn.functional.relu(ro._ln(tsd, f'{prefix}.mlps.{i}.1', h))
            embs.append(ro._lin(tsd, f'{prefix}.mlps.{i}.3', h))
        out = torch.stack(embs).sum(dim=0)
        if cat is not None:
            out = out + torch.stack([torch.from_numpy(np.array(cat)).double()]).sum(dim=0)
        out = torch.nn.functional.relu(ro._ln(tsd, prefix + '.to_out.0', out))
        return ro._lin(tsd, prefix + '.to_out.2', out)

    with _f64(), torch.no_grad():
        want = oracle_behind_the_features()
        want_n = torch.nn.functional.layer_norm(want, (128,))
        # the oracle itself, whole, in float64: equal up to the rounding of z (|z| 2^-24 per argument), a sanity bound only
        whole = ro.fourier_embedding(tsd, prefix, x32.double(), None if cat is None else [torch.from_numpy(np.array(cat)).double()])
    got = fr.reference(variant, 'A', prefix, cat is not None, False)
    got_n = fr.reference(variant, 'A', prefix, cat is not None, True)
    assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max()
    assert np.abs(got_n - want_n.numpy()).max() <= 1e-12 * np.abs(want_n.numpy()).max()
    assert np.abs(got - whole.numpy()).max() <= 1e-2 * np.abs(want.numpy()).max()
    # and z_in_float64 IS the whole oracle in float64
    mut = fr.evaluate(variant, 'A', prefix, cat is not None, False, mutate='z_in_float64')
    assert np.abs(mut - whole.numpy()).max() <= 1e-12 * np.abs(whole.numpy()).max()


@pytest.mark.parametrize('prefix', [fr.PREFIX_OF_N[4], fr.PREFIX_OF_N[3]])
def test_table_form_is_the_operator_on_integer_gaps(prefix):
    """regime B's gaps are integers in 0 .. -31; regime C's special gaps take the clamped row"""
    for variant in ('plain', 'ln'):
        a, b = fr.reference(variant, 'B', prefix, gaps=True), fr.reference(variant, 'B', prefix, tab=True, gaps=True)
        assert set(np.unique(fr.gen_inputs('B', prefix, True)[:, fr.PREFIXES[prefix] - 1])) == set(-np.arange(32.0))
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    assert list(fr.table_row(np.array(fr.C_GAPS, np.float32))) == [0, 31, 31, 31, 0, 2]
    raw = np.array(fr.gen_inputs('C', prefix, True))
    n = fr.PREFIXES[prefix]
    clamped = raw.copy()
    clamped[:, n - 1] = -fr.table_row(raw[:, n - 1])
    want = fr.fourier_ref(fr.weights('plain'), prefix, clamped)
    assert np.abs(fr.reference('plain', 'C', prefix, tab=True, gaps=True) - want).max() <= 1e-12 * np.abs(want).max()
    b = fr.C_BLOCKS[1]
    per_edge = fr.reference('plain', 'C', prefix, gaps=True)
    assert np.abs(per_edge[b + 2:b + 6] - want[b + 2:b + 6]).max() > 1e-3          # -32, -40, +3, -2.5: as they are


def test_table_ref_is_the_last_branch_without_its_bias():
    for prefix in (fr.PREFIX_OF_N[4], fr.PREFIX_OF_N[3]):
        sd, n = fr.weights('plain'), fr.PREFIXES[prefix]
        t = fr.table_ref('plain', prefix)
        assert t.shape == (32, 128)
        raw = np.zeros((32, 4), np.float32)
        raw[:, n - 1] = -np.arange(32)
        # the whole sum minus the other dims at 0 and minus every second bias
        full = sum(fr.branch(sd, prefix, i, raw[:, i]) for i in range(n))
        rest = sum(fr.branch(sd, prefix, i, raw[:, i]) for i in range(n - 1))
        assert np.abs((full - rest) - t).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ the figures
@pytest.fixture(scope='module')
def figures():
    """{('FP32' | 'PERT', output, regime): largest row error over fourier_ref.CASES on the base block}"""
    fig = {}
    for case in fr.CASES:
        variant, regime, prefix, cat, normalize, tab, gaps = case
        out = 'NORM' if normalize else 'PLAIN'
        ref = fr.reference(*case)
        e32 = fr.row_error(fr.evaluate(*case, dtype=np.float32), ref)
        fig['FP32', out, regime] = max(fig.get(('FP32', out, regime), 0.0), e32)
        for seed in fr.PERT_SEEDS:
            ep = fr.row_error(fr.evaluate(*case, perturb=seed), ref)
            fig['PERT', out, regime] = max(fig.get(('PERT', out, regime), 0.0), ep)
    return fig


def test_figures_are_pinned(figures):
    """every FP32_ERR_FOURIER_* and PERT_ERR_FOURIER_* reproduces within [0.5, 1.0] x its pinned constant (numpy's float32 cos / sin
    may differ in the last place between builds; the pins are the measured figures rounded up)"""
    assert set(figures) == {(k, o, g) for k in ('FP32', 'PERT') for o in fr.OUTPUTS for g in fr.REGIMES}
    bad = []
    for (kind, o, g), e in sorted(figures.items()):
        pin = fr.fp32_err(o, g) if kind == 'FP32' else fr.pert_err(o, g)
        print(f'{kind}_ERR_FOURIER_{o}_{g} = {e:.3e} (pinned {pin:.3e})')
        if not 0.5 * pin <= e <= pin:
            bad.append((kind, o, g, e, pin))
    for o in fr.OUTPUTS:
        for g in fr.REGIMES:
            assert fr.bar(o, g, 'k_fourier') == 4 * fr.fp32_err(o, g)
            for k in fr.SPLIT_KERNELS:
                assert fr.bar(o, g, k) == 4 * max(fr.fp32_err(o, g), fr.pert_err(o, g))
    assert not bad, bad


def test_float32_evaluation_passes_the_comparison():
    for case in fr.CASES[::7]:
        out = 'NORM' if case[4] else 'PLAIN'
        fr.compare_fourier(case[1], 'k_fourier', {out: fr.evaluate(*case, dtype=np.float32)}, {out: fr.reference(*case)})


# ------------------------------------------------------------------------------------------------ prescale coverage
def _exp(v):
    e = math.log2(v)
    assert e == int(e)
    return int(e)


def test_plain_weights_hit_the_cap_in_every_slot():
    """the gap these tests close: with make_weights(seed=3) every matrix prescale is 2^14 and both activation scales are 2^11"""
    for prefix, n in fr.PREFIXES.items():
        p = fr.prescales(fr.weights('plain'), prefix)
        assert [_exp(v) for v in p['sw1'] + [p['sw2'], p['sw3']]] == [14] * (n + 2) and (p['sa1'], p['sa2']) == (2048.0, 2048.0)


def test_scales_variants_spread_the_prescale_exponents():
    seen = {}
    for v in fr.SCALES_VARIANTS:
        want = fr.SCALE_EXPONENTS[v]
        for prefix, n in fr.PREFIXES.items():
            p = fr.prescales(fr.weights(v), prefix)
            e1 = [_exp(s) for s in p['sw1']]
            assert e1 == list(want['sw1'][:n]) and _exp(p['sw2']) == want['sw2'] and _exp(p['sw3']) == want['sw3']
            assert len(set(e1)) == n, 'the descales of two dims could be exchanged unseen'
            hdr = fr.header(fr.weights(v), prefix)
            assert len(set(hdr[:n])) == n and hdr[4] != hdr[5]
            assert 14 in e1 + [_exp(p['sw2']), _exp(p['sw3'])], 'no slot at the cap'
            seen[v, prefix] = hdr
    for prefix, n in fr.PREFIXES.items():
        a, b = seen['scales_a', prefix], seen['scales_b', prefix]
        assert all(a[s] != b[s] for s in list(range(n)) + [4, 5]), 'a slot holds the same value in both variants'


def test_ln_variant_moves_the_activation_scales():
    for prefix in fr.PREFIXES:
        p, sd = fr.prescales(fr.weights('ln'), prefix), fr.weights('ln')
        assert p['sa1'] < 2048.0 and p['sa2'] == 4096.0
        g, b = sd[f'{prefix}.to_out.0.weight'], sd[f'{prefix}.to_out.0.bias']
        assert fr.pow2(fr.LN_MAX * np.abs(g).max() + np.abs(b).max()) >= 4096.0         # the cap binds (or is met exactly)
        for i in range(fr.PREFIXES[prefix]):
            gam = np.abs(sd[f'{prefix}.mlps.{i}.1.weight'])
            assert gam.max() / gam.min() >= 50.0          # (128 draws of 2^U(-3.3, 3.3) on gammas of 0.8 .. 1.2)


def test_freq_variant_reaches_1e3_rad():
    for prefix, n in fr.PREFIXES.items():
        raw = fr.gen_inputs('A', prefix)
        z = np.abs(fr.argument(fr.weights('freq'), prefix, 0, raw[:, 0])).max()
        zp = max(np.abs(fr.argument(fr.weights('plain'), prefix, i, raw[:, i])).max() for i in range(n))
        assert 900.0 <= z <= 1000.5 and zp < 25.0, (prefix, z, zp)


@pytest.mark.parametrize('variant', fr.VARIANTS)
def test_packer_header_holds_the_reciprocals_of_the_rule(variant):
    from infgen_amd import _lib, packing
    try:
        lib = _lib.load()
    except (OSError, _lib.InfgenHipError) as e:
        pytest.skip(f'the library cannot be loaded here: {e}')
    sd = fr.weights(variant)
    for prefix, n in fr.PREFIXES.items():
        pack = packing.pack_fourier(sd, prefix, n)
        hdr = pack[lib.infgen_fourier_pack_offset(b'h_hdr', n, 0):][:16]
        want = fr.header(sd, prefix)
        assert [float(h) for h in hdr[:6]] == want and float(hdr[6]) == fr.SF, (prefix, list(hdr[:7]), want)
        p = fr.prescales(sd, prefix)
        for i in range(n):
            o = lib.infgen_fourier_pack_offset(b'h_g1', n, i)
            assert np.array_equal(pack[o:o + 128], np.asarray(sd[f'{prefix}.mlps.{i}.1.weight'], np.float32) * np.float32(p['sa1']))
        o = lib.infgen_fourier_pack_offset(b'h_g2', n, 0)
        assert np.array_equal(pack[o:o + 128], np.asarray(sd[f'{prefix}.to_out.0.weight'], np.float32) * np.float32(p['sa2']))


# ------------------------------------------------------------------------------------------------ the wrong evaluations are seen
def _worst_ratio(mutate, cases):
    """the largest (row error of the mutant on the first GPU_ROWS rows) / (the widest bar of the case) over the cases it applies to"""
    worst, where = 0.0, None
    for case in cases:
        variant, regime, prefix, cat, normalize, tab, gaps = case
        if not fr.mutant_applies(mutate, fr.PREFIXES[prefix], cat, normalize, tab):
            continue
        got = fr.evaluate(*case, mutate=mutate, rows=GPU_ROWS)
        out = 'NORM' if normalize else 'PLAIN'
        b = max(fr.bar(out, regime, k) for k in fr.KERNELS)
        r = math.inf if not np.isfinite(got).all() else fr.row_error(got, fr.reference(*case)[:GPU_ROWS]) / b
        if r > worst:
            worst, where = r, case
    return worst, where


@pytest.mark.parametrize('mutate', [m for m in fr.MUTANTS if m not in fr.HDR_MUTANTS and m != 'hdr_4_as_5'])
def test_wrong_evaluation_is_seen(mutate):
    """at least 4 x the (widest) bar on a case of the list the GPU module runs (a value that is not finite fails compare_fourier
    outright and counts as seen)"""
    r, where = _worst_ratio(mutate, fr.CASES)
    print(f'{mutate}: {r:.3g} x the bar on {where and fr.case_id(where)}')
    assert r >= 4.0, (mutate, r, where)


@pytest.mark.parametrize('mutate', fr.HDR_MUTANTS + ('hdr_4_as_5',))
def test_header_mix_up_is_seen_on_a_scales_variant(mutate):
    """per prefix that has both dims: seen under a `scales` variant - and not at all with the plain weights, where the slots of the
    dims hold one value: the gap"""
    for prefix, n in fr.PREFIXES.items():
        if not fr.mutant_applies(mutate, n, False, False, False):
            continue
        r, where = _worst_ratio(mutate, [c for c in fr.CASES if c[0] in fr.SCALES_VARIANTS and c[2] == prefix])
        assert r >= 4.0, (mutate, prefix, r, where)
        if mutate != 'hdr_4_as_5':
            assert _worst_ratio(mutate, [c for c in fr.CASES if c[0] == 'plain' and c[2] == prefix])[0] == 0.0


def test_comparison_fails_a_mutant_and_a_value_that_is_not_finite():
    case = ('plain', 'A', fr.PREFIX_OF_N[3], False, True, False, None)
    ref = {'NORM': fr.reference(*case)}
    with pytest.raises(AssertionError, match='beyond the bar'):
        fr.compare_fourier('A', 'k_fourier_h', {'NORM': fr.evaluate(*case, mutate='sin_cos_swapped')}, ref)
    bad = np.array(ref['NORM'])
    bad[7, 3] = np.nan
    with pytest.raises(AssertionError, match='not finite'):
        fr.compare_fourier('A', 'k_fourier_h', {'NORM': bad}, ref)


# ------------------------------------------------------------------------------------------------ regime and row-count coverage
def test_regime_a_leaves_the_unused_components_nan():
    for regime in fr.REGIMES:
        for prefix, n in fr.PREFIXES.items():
            raw = fr.gen_inputs(regime, prefix)
            assert raw.shape == (fr.BASE_ROWS, 4) and raw.dtype == np.float32 and not raw.flags.writeable
            assert np.isnan(raw[:, n:]).all() and np.isfinite(raw[:, :n]).all()
    raw = fr.gen_inputs('A', fr.PREFIX_OF_N[4])
    assert raw[:, 0].min() >= 0 and raw[:, 0].max() <= 60 and np.abs(raw[:, 1:3]).max() <= math.pi
    assert set(np.unique(raw[:, 3])) == set(-np.arange(1.0, 13.0))


def test_regime_b_covers_the_magnitudes_and_the_angle_edges():
    for prefix, n in fr.PREFIXES.items():
        raw = fr.gen_inputs('B', prefix)
        e = np.floor(np.log2(raw[:, 0]))
        assert e.min() == -20 and e.max() == 10 and 1000.0 < raw[:, 0].max() < 2048.0
        ang = raw[:, 1:(n if n < 4 else 3)]
        pi32 = np.float32(math.pi)
        assert (ang == pi32).any() and (ang == -pi32).any()
        assert ((ang == 0) & ~np.signbit(ang)).any() and ((ang == 0) & np.signbit(ang)).any()


def test_regime_c_has_its_special_rows():
    """per block: the all-zero row, -0.0, 1e-30, a row with exactly one |z| >= 1e5 - in one group of the eight frequencies
    32 s + 8 rg .. + 7 a lane evaluates together -, a row with all 64, a large negative x; at a tile start of every kernel, in the
    middle of a wave's 16 rows, and as the last rows of the GPU case's partial tile"""
    assert fr.C_BLOCKS[0] % 192 == 0 and fr.C_BLOCKS[0] % 128 == 0
    assert 0 < fr.C_BLOCKS[1] % fr.WAVE_ROWS and fr.C_BLOCKS[1] % fr.WAVE_ROWS + 6 < fr.WAVE_ROWS
    assert fr.C_BLOCKS[2] + 6 == GPU_ROWS and all(GPU_ROWS % t for t in fr.TILE.values())
    for prefix, n in fr.PREFIXES.items():
        raw, sd = fr.gen_inputs('C', prefix), fr.weights('plain')
        for b in fr.C_BLOCKS:
            assert (raw[b, :n] == 0).all() and raw[b + 1, 0] == 0 and np.signbit(raw[b + 1, 0]) and raw[b + 2, 0] == np.float32(1e-30)
            assert raw[b + 5, 0] == -1500.0
            big = np.abs(fr.argument(sd, prefix, 0, raw[b:b + 6, 0])) >= fr.BIG_Z
            groups = big.reshape(6, 8, 8).sum(2)                     # frequencies 8 g .. 8 g + 7
            assert sorted(groups[3]) == [0] * 7 + [1] and (groups[4] == 8).all() and not big[[0, 1, 2, 5]].any()
            assert np.isfinite(fr.argument(sd, prefix, 0, raw[b:b + 6, 0])).all()
        assert np.abs(fr.argument(sd, prefix, 0, raw[:, 0])).max() < 2.0 ** 40         # sincos_big's range
        if n == 4:
            for b in fr.C_BLOCKS:
                assert tuple(raw[b:b + 6, 3]) == fr.C_GAPS
    g3 = fr.gen_inputs('C', fr.PREFIX_OF_N[3], True)
    assert tuple(g3[fr.C_BLOCKS[1]:fr.C_BLOCKS[1] + 6, 2]) == fr.C_GAPS and (g3[:, 2] == np.trunc(g3[:, 2])).sum() >= fr.BASE_ROWS - 3


def test_row_counts_hit_every_tile_edge():
    assert fr.ROW_COUNTS == [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257, 385]
    assert max(fr.ROW_COUNTS) == fr.BASE_ROWS and GPU_ROWS in fr.ROW_COUNTS
    for t in list(fr.TILE.values()) + [fr.WAVE_ROWS]:
        assert {t - 1, t, t + 1} <= set(fr.ROW_COUNTS), t
    assert fr.PERSISTENT_ROWS == {'k_fourier': 2048 * 32 + 32 + 5, 'k_fourier_h': 256 * 128 + 128 + 5, 'k_fourier_h12': 256 * 192 + 192 + 5}
    for k, rows in fr.PERSISTENT_ROWS.items():
        tiles = -(-rows // fr.TILE[k])
        assert tiles == fr.GRID_CAP[k] + 2 and rows % fr.TILE[k] == 5       # workgroups 0 and 1 take a second tile, the last of 5 rows
        assert math.gcd(fr.BASE_ROWS, fr.TILE[k]) == 1                      # a base row meets every position of a tile
    assert fr.PERSISTENT_ROWS['k_fourier_h12'] < fr.H12_MIN_CAP


def test_tiles_and_grid_caps_are_the_sources():
    """the constants the persistent counts are derived from, read in csrc/api.hip, kernels.h and tile.cuh"""
    src = lambda name: open(os.path.join(REPO, 'infgen_amd', 'csrc', name)).read()
    api, kh, tile = src('api.hip'), src('kernels.h'), src('tile.cuh')
    assert re.search(r'int grid = ceil_div\(a\.e_cap, TR\);\s*if \(grid > 2048\) grid = 2048;', api)
    assert re.search(r'constexpr int TR = 32;', tile)
    assert re.search(r'return grid > 256 \* FH_WG_PER_CU \? 256 \* FH_WG_PER_CU : grid;', api)
    assert re.search(r'#define IG_FH_WAVES 8\b', kh) and re.search(r'constexpr int FH_TILE = 16 \* FH_WAVES;', kh)
    assert re.search(r'constexpr int FH_WG_PER_CU = FH_WAVES == 8 \? 1 : 2;', kh) and re.search(r'FH12_TILE = 192\b', kh)
    assert re.search(r'env_int\("INFGEN_FH12_MIN", 150000\)', api) and re.search(r'constexpr int DT_TAB_ROWS = 32;', kh)
