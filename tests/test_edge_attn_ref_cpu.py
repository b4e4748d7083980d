"""Anchors of tests/edge_attn_ref.py (the plain float64 reference of the edge-attention operators) and of its case generators:
the reference agrees with a direct torch float64 scatter-softmax restatement of AttentionLayer's message / propagate
(infgen/modules/layers.py:78-92,109) from the UNFOLDED weights; the packed 24-bit rows round-trip; every case reaches the path it
is named for; the fp32 figures the device bars are four times of still hold; and every deliberately wrong variant fails
compare_edge - the comparison tests/test_edge_attn_gpu.py applies - at those bars on a named case."""
import math

import numpy as np
import pytest
import torch

import edge_attn_ref as ea


def _lists(c):
    return c['off'], c['cnt'], c['src']


# ------------------------------------------------------------------------------------------------ anchors
def test_reference_equals_a_torch_scatter_softmax_of_the_unfolded_layer():
    """k_j + to_k_r(LN(r)), v_j + to_v_r(LN(r)) with the affine LayerNorm, softmax by scatter amax / scatter add over the
    destinations, index_add of the messages - in float64, from raw (not normalised) rows r and the state dict's own matrices.  The
    reference works on the normalised rows with gamma / beta folded into W'_kr, W'_vr, b': the same AGG to float64 round-off, and
    its plain operator the same attention-weighted sums."""
    sd = ea.weights()
    p = ea.PREFIX
    rng = np.random.default_rng(0)
    rows, n_src = 9, 14
    degs = [0, 3, 1, 7, 0, 12, 2, 5, 4]
    off, cnt, e_cap = ea._layout(rng, degs)
    src = rng.integers(0, n_src, e_cap).astype(np.int32)
    r = rng.standard_normal((e_cap, 128)) * rng.uniform(0.2, 5.0, (e_cap, 1))
    q, k, v = rng.standard_normal((rows, 128)), rng.standard_normal((n_src, 128)), rng.standard_normal((n_src, 128))
    t = lambda name: torch.from_numpy(np.asarray(sd[f'{p}.{name}'], np.float64))
    tr = torch.from_numpy(r)
    rhat = torch.nn.functional.layer_norm(tr, (128,))
    mine = ea.edge_attn_fused_ref(sd, p, q, k, v, off, cnt, src, rhat.numpy())
    # the restatement, on (src, dst) endpoint lists in list order
    e_idx = np.concatenate([np.arange(off[i], off[i] + cnt[i]) for i in range(rows)])
    dst = torch.from_numpy(np.concatenate([np.full(cnt[i], i) for i in range(rows)])).long()
    sj = torch.from_numpy(src[e_idx]).long()
    rn = torch.nn.functional.layer_norm(tr[e_idx], (128,), t('attn_prenorm_r.weight'), t('attn_prenorm_r.bias'))
    kj = (torch.from_numpy(k)[sj] + rn @ t('to_k_r.weight').T).view(-1, 8, 16)
    vj = (torch.from_numpy(v)[sj] + rn @ t('to_v_r.weight').T + t('to_v_r.bias')).view(-1, 8, 16)
    sim = (torch.from_numpy(q).view(-1, 8, 16)[dst] * kj).sum(-1)
    idx = dst.view(-1, 1).expand_as(sim)
    mx = torch.full((rows, 8), float('-inf'), dtype=torch.float64).scatter_reduce(0, idx, sim, reduce='amax', include_self=True)
    ex = (sim - mx[dst]).exp()
    den = torch.zeros(rows, 8, dtype=torch.float64).scatter_add(0, idx, ex)
    attn = ex / (den[dst] + 1e-16)
    agg = torch.zeros(rows, 8, 16, dtype=torch.float64).index_add_(0, dst, vj * attn.unsqueeze(-1)).view(rows, 128).numpy()
    assert np.abs(mine - agg).max() <= 1e-12 * np.abs(agg).max()
    assert (mine[[0, 4]] == 0).all() and (agg[[0, 4]] == 0).all()
    # the plain operator: Z and SIG are the attention-weighted sums of the normalised rows / of ones
    u = ea.absorbed_query(sd, p, q)
    AGG, Z, SIG = ea.edge_attn_ref(q, u, k, v, off, cnt, src, rhat.numpy())
    zt = torch.zeros(rows, 8, 128, dtype=torch.float64).index_add_(0, dst, attn.unsqueeze(-1) * rhat[e_idx].unsqueeze(1)).numpy()
    st = torch.zeros(rows, 8, dtype=torch.float64).index_add_(0, dst, attn).numpy()
    at = torch.zeros(rows, 8, 16, dtype=torch.float64).index_add_(0, dst, torch.from_numpy(v)[sj].view(-1, 8, 16) * attn.unsqueeze(-1))
    assert np.abs(Z - zt).max() <= 1e-12 and np.abs(SIG - st).max() <= 1e-12 and np.abs(AGG - at.view(rows, 128).numpy()).max() <= 1e-12


def test_packed_rows_round_trip_within_half_a_24_bit_step():
    rng = np.random.default_rng(1)
    x = ea._normalised_rows(rng, 300)
    x[0, :4] = [0.0, -0.0, 1.0, -1.9999999]
    b = ea.pack_r24(x)
    assert b.shape == (300, 384) and b.dtype == np.uint8
    y = ea.unpack_r24(b)
    nz = x != 0
    # sign + exponent + 15 mantissa bits: neighbours are 2^-15 of the binade apart, so rounding to nearest is within 2^-16 of a
    # value at the binade's lower end and 2^-17 at its upper end (the header's "2^-17" is the latter; no 24-bit format does better)
    rel = np.abs(y.astype(np.float64) - x)[nz] / np.abs(x.astype(np.float64))[nz]
    assert rel.max() <= 2.0 ** -16 and 2.0 ** -17 < rel.max() and np.sqrt((rel ** 2).mean()) <= 2.0 ** -17
    assert (y[~nz] == 0).all()
    assert np.array_equal(ea.pack_r24(y), b), 'values of 24 bits are kept exactly'
    assert (y.view(np.uint32) & 0xff == 0).all()
    # layout: column c of a row - bits 31..16 little-endian at bytes 2c, 2c + 1; bits 15..8 at byte 256 + c
    one = np.zeros((1, 128), np.float32)
    one[0, 5] = np.uint32(0x40123480).view(np.float32)           # a tie above an even 24-bit value: rounds down
    one[0, 6] = np.uint32(0x40123580).view(np.float32)           # a tie above an odd one: rounds up
    one[0, 7] = np.uint32(0x40ffff80).view(np.float32)           # the carry runs into bits 31..16
    pb = ea.pack_r24(one)[0]
    assert (pb[10], pb[11], pb[256 + 5]) == (0x12, 0x40, 0x34)
    assert (pb[12], pb[13], pb[256 + 6]) == (0x12, 0x40, 0x36)
    assert (pb[14], pb[15], pb[256 + 7]) == (0x00, 0x41, 0x00)
    # the low plane ignored: 16-bit rows
    assert (ea.unpack_r24(b, low=False).view(np.uint32) & 0xffff == 0).all()


# ------------------------------------------------------------------------------------------------ the cases reach their paths
def _scores(name):
    c = ea.gen_case(name)
    return c, ea.edge_attn_ref(c['q'], c['u'], c['k'], c['v'], *_lists(c), c['rhat'], want_scores=True)[3]


@pytest.mark.parametrize('name', ea.ALL_CASES)
def test_case_is_well_formed(name):
    """lists inside the buffers and disjoint, sources in range, rhat rows normalised where a list names them and NaN elsewhere,
    every |score| <= 100 natural units with and without the positional part"""
    c, sc = _scores(name)
    rows = c['rows']
    assert c['q'].shape == (rows, 128) and c['u'].shape == (rows, 1024) and c['k'].shape == c['v'].shape == (c['n_src'], 128)
    used = np.zeros(c['e_cap'], int)
    for i in range(rows):
        assert 0 <= c['off'][i] and c['off'][i] + c['cnt'][i] <= c['e_cap']
        used[c['off'][i]:c['off'][i] + c['cnt'][i]] += 1
    assert used.max() == 1 and used.min() == 0                          # disjoint lists, gaps between them
    live = used == 1
    assert (c['src'][live] >= 0).all() and (c['src'][live] < c['n_src']).all() and (c['src'][~live] == 0).all()
    assert np.isnan(c['rhat'][~live]).all() and np.isfinite(c['rhat'][live]).all()
    r = c['rhat'][live].astype(np.float64)
    assert np.abs(r.mean(1)).max() < 1e-3 and np.abs(r.var(1) - 1).max() < 1e-2 and np.abs(r).max() <= math.sqrt(127)
    assert max(np.abs(s).max() for s in sc if len(s)) <= 100.0
    nor = ea.edge_attn_ref(c['q'], None, c['k_nor'], c['v'], *_lists(c), None, want_scores=True)[3]
    assert max(np.abs(s).max() for s in nor if len(s)) <= 100.0
    assert (c['cnt'] == 0).any() or rows == 1


def test_cases_cover_the_degrees_and_lists():
    c = ea.gen_case('mixed45')
    assert c['rows'] == 45 == c['n_src'] and set(ea.DEGREES) <= set(c['cnt'].tolist())
    assert ea.DEGREES == [0, 1, 2, 3, 5, 7, 9, 63, 64, 65, 127, 128, 129, 300]
    live = [i for i in range(45) if c['cnt'][i] > 0]
    assert all(c['off'][a] > c['off'][b] for a, b in zip(live, live[1:])), 'lists are stored in reverse row order'
    ends = sorted((c['off'][i], c['off'][i] + c['cnt'][i]) for i in live)
    assert any(b[0] > a[1] for a, b in zip(ends, ends[1:])), 'gaps between lists'
    for i in live:
        s = c['src'][c['off'][i]:c['off'][i] + c['cnt'][i]]
        if len(s) >= 2:
            assert s[0] == s[1], 'a source repeated inside the list'
        if len(s) >= 4:
            assert 0 in s and c['n_src'] - 1 in s
    b = ea.gen_case('x8_bip33')
    assert b['rows'] == 33 and b['n_src'] == 60 and set(ea.DEGREES) <= set(b['cnt'].tolist())
    w = ea.gen_case('wide12')
    assert set(range(1, 10)) <= set(w['cnt'].tolist()) and 2348 in w['cnt'] and 0 in w['cnt']
    assert [ea.gen_case(n)['rows'] for n in ('rows1', 'rows15', 'rows16', 'rows17', 'rows256', 'rows257', 'rows4096', 'rows4112')] == \
        [1, 15, 16, 17, 256, 257, 4096, 4112]
    for n in ea.SIZE_CASES:
        assert ea.gen_case(n)['cnt'].max() == 3 and ea.gen_case(n)['cnt'].min() == 0
    for n in ('equal17', 'stair75', 'stair85', 'dominant17', 'descending17', 'negative17'):
        assert ea.gen_case(n)['cnt'].tolist() == ea.DEGREES + [4, 6, 8]
    t = ea.gen_case('r24tie')
    live = np.isfinite(t['rhat']).all(1)
    bits = t['rhat'][live].view(np.uint32)
    assert (bits & 0xff == 0x80).all() and ((bits >> 8) & 1 == 0).any() and ((bits >> 8) & 1 == 1).any()
    back = ea.unpack_r24(ea.pack_r24(t['rhat'][live])).view(np.uint32)
    assert ((back >> 8) & 1 == 0).all() and (np.abs(back.astype(np.int64) - bits) == 0x80).all(), 'every tie went to the even neighbour'


def test_score_regimes_have_the_wanted_shape():
    """on the float64 scores of the float32 inputs.  The staircase steps are stated in the log2 domain as numbers: 7.5 and 8.5, on
    either side of 8; count_moves is this module's own deferred-reference rule with that threshold, for information."""
    ln2 = math.log(2.0)
    c, sc = _scores('equal17')
    assert all(np.ptp(s, axis=0).max() <= 1e-4 for s in sc if len(s))
    for name, step, per_level in (('stair75', 7.5, 2), ('stair85', 8.5, 1)):
        c, sc = _scores(name)
        for s in sc:
            if len(s) == 0:
                continue
            levels = min(len(s), 16)
            d = np.diff(s, axis=0) / ln2
            rises = d[np.abs(d) > 1e-3]
            assert np.abs(rises - step).max() <= 1e-4 if len(rises) else levels == 1
            assert len(rises) == 8 * (levels - 1)
            # the reference moves at every level for 8.5, at every second one for 7.5 (two steps make 15 > 8)
            assert (ea.count_moves(s) == (levels + per_level - 1) // per_level).all(), (name, len(s))
    c, sc = _scores('dominant17')
    seen = set()
    for i, s in enumerate(sc):
        if len(s) > 1:
            top = s.argmax(0)
            assert (top == top[0]).all() and (s[top[0]] - np.delete(s, top[0], axis=0).max(0) >= 60.0).all()
            seen.add((int(top[0]), len(s)))
    assert {p for p, n in seen} >= {0, 63, 64} and any(p == n - 1 for p, n in seen)
    c, sc = _scores('descending17')
    long = [s for s in sc if len(s) >= 9]
    assert all((np.diff(s, axis=0) < 0).all() and (np.ptp(s, axis=0) / ln2 > 150.0).all() for s in long)
    assert all((ea.count_moves(s) == 1).all() for s in long)
    # ... so that an interleaved sub-list's rescale to the list's maximum underflows: 0 in float32, denormals included
    assert np.float32(2.0) ** np.float32(-(long[-1][0] - long[-1][-8:]).min() / ln2) == 0
    c, sc = _scores('negative17')
    allsc = np.concatenate([s for s in sc if len(s)])
    assert allsc.max() < -80.0 and allsc.min() > -100.0
    c, sc = _scores('x8_bip33')
    assert max(np.abs(s).max() for s in sc if len(s)) > 60.0                        # (ordinary scores stay below ~25)
    assert max(ea.count_moves(s).max() for s in sc if len(s)) >= 3
    c, sc = _scores('mixed45')
    assert max(np.abs(s).max() for s in sc if len(s)) < 40.0


# ------------------------------------------------------------------------------------------------ the fp32 figures
def fp32_figures():
    """{(output, regime): error of the float32 evaluation against float64, relative to max |ref|, largest over the regime's cases}"""
    fig = {}

    def note(out, regime, got, ref):
        e = float(np.abs(got.astype(np.float64) - ref).max() / np.abs(ref).max())
        fig[out, regime] = max(fig.get((out, regime), 0.0), e)

    sd = ea.weights()
    for name in ea.ALL_CASES:
        c = ea.gen_case(name)
        g = c['regime']
        agg, z, sig = ea.edge_attn_fp32(c['q'], c['u'], c['k'], c['v'], *_lists(c), c['rhat'])
        ref = ea.reference(name, 'r')
        note('AGG', g, agg, ref['AGG']); note('Z', g, z, ref['Z']); note('SIG', g, sig, ref['SIG'])
        agg, _, sig = ea.edge_attn_fp32(c['q'], None, c['k_nor'], c['v'], *_lists(c), None)
        ref = ea.reference(name, 'nor')
        note('AGG', g, agg, ref['AGG']); note('SIG', g, sig, ref['SIG'])
        fused = ea.edge_attn_fused_ref(sd, ea.PREFIX, c['q'], c['k'], c['v'], *_lists(c), c['rhat'], f=np.float32)
        note('FUSED', g, fused, ea.reference(name, 'fused')['FUSED'])
    return fig


def test_fp32_figures_are_pinned():
    """the pinned FP32_ERR_EDGE_* reproduce: none is exceeded, none has drifted below 0.7 of its pin (numpy's float32 exp may differ
    in the last place between builds; the pins are the measured figures rounded up to three digits)"""
    fig = fp32_figures()
    assert set(fig) == {(o, g) for o in ea.OUTPUTS for g in ea.REGIMES}
    for (o, g), e in sorted(fig.items()):
        pin = ea.fp32_err(o, g)
        print(f'FP32_ERR_EDGE_{o}_{g} = {e:.3e} (pinned {pin:.3e}, bar {ea.bar(o, g):.3e})')
        assert 0.7 * pin <= e <= pin, (o, g, e, pin)
        assert ea.bar(o, g) == 4 * pin


# ------------------------------------------------------------------------------------------------ the wrong variants are caught
# variant -> (case, which outputs) on which compare_edge fails at the bars
CAUGHT_ON = {
    'swap_h4': ('mixed45', 'r'), 'swap_h2': ('mixed45', 'r'), 'stale_z': ('stair85', 'r'), 'last_twice': ('mixed45', 'r'),
    'drop_64': ('mixed45', 'r'), 'z_norm_neighbour': ('mixed45', 'r'), 'sig1_empty': ('rows16', 'r'), 'wide_avg': ('wide12', 'r'),
    'eps_nan': ('rows17', 'r'),
}


def _mutant(name, kind, mutate):
    c = ea.gen_case(name)
    if kind == 'r':
        agg, z, sig = ea.edge_attn_ref(c['q'], c['u'], c['k'], c['v'], *_lists(c), c['rhat'], mutate=mutate)
        return dict(AGG=agg, Z=z, SIG=sig)
    return dict(FUSED=ea.edge_attn_fused_ref(ea.weights(), ea.PREFIX, c['q'], c['k'], c['v'], *_lists(c), c['rhat'], mutate=mutate))


@pytest.mark.parametrize('mutate', ea.MUTANTS)
def test_wrong_variant_fails_the_comparison(mutate):
    name, kind = CAUGHT_ON[mutate]
    c = ea.gen_case(name)
    ea.compare_edge(c['regime'], ea.reference(name, kind), ea.reference(name, kind), c['cnt'])        # (the reference itself passes)
    for k in (kind, 'fused'):
        with pytest.raises(AssertionError):
            ea.compare_edge(c['regime'], _mutant(name, k, mutate), ea.reference(name, k), c['cnt'])


def test_stale_accumulator_shows_only_where_the_reference_moves():
    """steps of 7.5 move a deferred reference too (every second level), equal scores never do: there the stale variant IS the reference"""
    c = ea.gen_case('equal17')
    ea.compare_edge('C', _mutant('equal17', 'r', 'stale_z'), ea.reference('equal17', 'r'), c['cnt'])
    with pytest.raises(AssertionError):
        ea.compare_edge('D', _mutant('stair75', 'r', 'stale_z'), ea.reference('stair75', 'r'), ea.gen_case('stair75')['cnt'])


@pytest.mark.parametrize('name', ['mixed45', 'r24tie'])
def test_sixteen_bit_rows_fail_the_packed_comparison(name):
    """the low plane ignored: 2^-9 of every rhat value, far beyond four times float32 round-off"""
    c = ea.gen_case(name)
    rows16 = ea.unpack_r24(ea.pack_r24(c['rhat']), low=False)
    got = dict(FUSED=ea.edge_attn_fused_ref(ea.weights(), ea.PREFIX, c['q'], c['k'], c['v'], *_lists(c), rows16))
    with pytest.raises(AssertionError):
        ea.compare_edge(c['regime'], got, ea.reference(name, 'fused_r24'), c['cnt'])
    # and the packed reference differs from the fp32-row one by more than the bar: a kernel that read fp32 rows would not pass either
    with pytest.raises(AssertionError):
        ea.compare_edge(c['regime'], ea.reference(name, 'fused'), ea.reference(name, 'fused_r24'), c['cnt'])
