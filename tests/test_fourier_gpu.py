"""Operator-level tests of the Fourier embedding kernels through the C ABI - k_fourier (fourier_mode 0), k_fourier_h<3> (the
default), k_fourier_h12<3> (a capacity of 150,000 rows and more, the row count given through count_dev), k_fourier_h<1>
(gemm_terms 1), k_fourier_h_b16<1> (gemm_terms 2 with packs of packing.operand_bits(8)) and k_fourier_h_multi<3> (inside
infgen_decode_layers) - behind infgen_fourier_embed, infgen_fourier_embed_r24, infgen_fourier_last_dim_table / infgen_fourier_embed_tab:
each against the plain float64 reference of tests/fourier_ref.py, never against another kernel.  Every output's row error (max
|got - ref| / max(1, max |ref row|)) within fourier_ref.bar - four times the error of a float32 numpy evaluation of the same
formulas, for the split kernels four times the larger of that and of the float64 evaluation under the hardware sine's documented
2.6e-7 per feature; no bar comes from a device.  Outputs are NaN-filled allocations of the full capacity with a guard tail: every
word a launch must not write keeps its bits.  The reduced-precision kernels (gemm_terms 1 and 2) are judged by the structural
checks only (a row's bits do not depend on its position) and by their existing emulation tests.  Options go through
infgen_thread_options; no process-wide setter is called.  tests/test_fourier_ref_cpu.py shows that these comparisons see the
reference's deliberately wrong evaluations on the same case list (fourier_ref.CASES).  The largest device error / bar per kernel,
output and regime is printed at the end of the module and written as JSON to the file INFGEN_FOURIER_RECORD names, if it is set.

Left out: n = 1 (the ABI accepts it, no pack size exists), non-finite inputs (the header does not define them) and
k_fourier_h12_multi (reachable only with INFGEN_FH12_MULTI_ROWS set)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import edge_attn_ref as ea
import fourier_ref as fr
import layers_stack_ref as ls

pytestmark = pytest.mark.gpu

D = 128
GUARD_ROWS = 64
CANARY = 0x7fc00000                     # the bits torch.full(..., nan) writes
BYTE_CANARY = 0xa5
VALUE_KERNELS = ('k_fourier', 'k_fourier_h', 'k_fourier_h12')
# kernel -> (option block, significand bits of the packs)
SELECT = {'k_fourier': (dict(fourier_mode=0), 11), 'k_fourier_h': ({}, 11), 'k_fourier_h12': ({}, 11),
          'k_fourier_h<1>': (dict(gemm_terms=1), 11), 'k_fourier_h_b16<1>': (dict(gemm_terms=2), 8)}
ALL_KERNELS = tuple(SELECT)


def _r24_excess(got, ref, bar):
    """packed rows against float64: the largest |got - ref| / (bar x max(1, max |ref row|) + half a 24-bit step of the value).  The
    header's "2^-17 relative" of the packed format is relative to the upper end of a value's binade (sign + exponent + 15 mantissa
    bits: tests/test_edge_attn_ref_cpu.py::test_packed_rows_round_trip_within_half_a_24_bit_step) - the allowance is that half step,
    2^-17 x 2^(floor(log2 |v|) + 1), per element, of the larger of the two values compared"""
    g, r = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    m = np.maximum(np.abs(g), np.abs(r))
    half = np.where(m > 0, 2.0 ** -17 * 2.0 ** (np.floor(np.log2(np.maximum(m, 1e-300))) + 1), 0.0)
    allow = bar * np.maximum(1.0, np.abs(r).max(1))[:, None] + half
    return float((np.abs(g - r) / allow).max())


class _gpu_call:
    """a failed launch or synchronisation ends the session: nothing more is started on a device that reported an error"""

    def __enter__(self):
        return self

    def __exit__(self, kind, exc, tb):
        if kind is not None and not issubclass(kind, AssertionError):
            pytest.exit(f'device error, session stopped: {exc}', returncode=3)
        return False


@pytest.fixture(scope='module')
def env():
    from infgen_amd import _lib
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    e = dict(lib=_lib.load(), dev=torch.device('cuda:0'), packs={}, inputs={}, ratios={}, ran=set())
    o = _lib.Options()
    _lib.check(e['lib'].infgen_get_options(C.byref(o)))
    assert (o.fourier_mode, o.gemm_terms) == (1, 3), 'the defaults k_fourier_h<3> and k_fourier_h12<3> are selected by'
    yield e
    print('fourier kernels that ran: ' + ', '.join(sorted(e['ran'])))
    for k, (r, err, b) in sorted(e['ratios'].items()):
        print(f'fourier worst {k}: error {err:.3g} / bar {b:.3g} = {r:.2f}')
    if os.environ.get('INFGEN_FOURIER_RECORD'):
        with open(os.environ['INFGEN_FOURIER_RECORD'], 'w') as f:
            json.dump({k: dict(ratio=r, error=err, bar=b) for k, (r, err, b) in e['ratios'].items()}, f, indent=1, sort_keys=True)
            f.write('\n')


def _modes(env, **kw):
    """the calling thread's option block for the operator-level entries (no process-wide state is edited)"""
    from infgen_amd import _lib
    o = _lib.Options()
    _lib.check(env['lib'].infgen_get_options(C.byref(o)))
    for k, v in kw.items():
        setattr(o, k, int(v))
    o.use = 0
    return _lib.thread_options(o)


def _pack(env, variant, prefix, bits=11):
    from infgen_amd import packing
    key = (variant, prefix, bits)
    if key not in env['packs']:
        with packing.operand_bits(bits):
            p = packing.pack_fourier(fr.weights(variant), prefix, fr.PREFIXES[prefix])
        env['packs'][key] = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(env['dev'])
    return env['packs'][key]


def _dev(env, a):
    return torch.from_numpy(np.array(a)).to(env['dev'])


def _raw(env, regime, prefix, gaps=None):
    key = (regime, prefix, gaps)
    if key not in env['inputs']:
        env['inputs'][key] = _dev(env, fr.gen_inputs(regime, prefix, gaps))
    return env['inputs'][key]


def _rows_of(base, rows):
    """the first `rows` rows of a base block, or (rows > base) the block repeated cyclically"""
    return base[torch.arange(rows, device=base.device) % base.shape[0]].contiguous()


def _launch(env, kernel, variant, prefix, raw, *, count=None, e_cap=None, cat=None, ldcat=D, normalize=False, ldo=D, col0=0,
            table=None, r24=False, expect_fail=False, extra_opts=None):
    """one launch into a fresh sentinel-filled output of the FULL capacity plus a guard tail.  raw: device rows [rows][4] (padded
    with zeros to the capacity); count: the value behind count_dev (None: a NULL count_dev); k_fourier_h12 is selected by the capacity
    alone.  -> (out [cap + GUARD_ROWS][ldo] fp32, or [cap + GUARD_ROWS][384] uint8 for packed rows; capacity; rc)"""
    from infgen_amd import _lib
    lib, dev = env['lib'], env['dev']
    opts, bits = SELECT[kernel]
    rows = raw.shape[0]
    if e_cap is None:
        e_cap = fr.H12_MIN_CAP if kernel == 'k_fourier_h12' else rows
    if kernel == 'k_fourier_h12':
        assert e_cap >= fr.H12_MIN_CAP and count is not None
    else:
        assert e_cap < fr.H12_MIN_CAP
    n = fr.PREFIXES[prefix]
    rawc = torch.zeros(max(e_cap, 1) + GUARD_ROWS, 4, device=dev)
    rawc[:rows] = raw
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev)
    catc = None
    if cat is not None:
        catc = torch.full((max(e_cap, 1) + GUARD_ROWS, ldcat), float('nan'), device=dev)
        catc[:rows, :D] = cat
    if r24:
        out = torch.full((e_cap + GUARD_ROWS, ea.R24_ROW_BYTES), BYTE_CANARY, dtype=torch.uint8, device=dev)
    else:
        out = torch.full((e_cap + GUARD_ROWS, ldo), float('nan'), device=dev)
    pack = _pack(env, variant, prefix, bits)
    p = lambda t: None if t is None else t.data_ptr()
    with _gpu_call(), _modes(env, **dict(opts, **(extra_opts or {}))):
        if r24:
            rc = lib.infgen_fourier_embed_r24(p(rawc), n, p(cnt), e_cap, p(pack), p(out), None)
        elif table is not None:
            rc = lib.infgen_fourier_embed_tab(p(rawc), n, p(cnt), e_cap, p(pack), p(table) if table is not False else None,
                                              out.data_ptr() + 4 * col0, ldo, int(normalize), None)
        else:
            rc = lib.infgen_fourier_embed(p(rawc), n, p(cnt), e_cap, p(pack), p(catc), ldcat, out.data_ptr() + 4 * col0, ldo,
                                          int(normalize), None)
        if not expect_fail:
            _lib.check(rc, f'{kernel} launch')
        torch.cuda.synchronize()
    if rc == 0 and e_cap > 0 and (count is None or count > 0):
        env['ran'].add(kernel + (' (table)' if table is not None else '') + (' (r24)' if r24 else ''))
    return out, e_cap, rc


def _untouched(out, written_rows, col0=0, r24=False):
    """every word outside rows < written_rows x columns [col0, col0 + 128) keeps its sentinel bits"""
    if r24:
        return bool((out[written_rows:] == BYTE_CANARY).all())
    v = out.view(torch.int32)
    return (bool((v[written_rows:] == CANARY).all()) and bool((v[:written_rows, :col0] == CANARY).all())
            and bool((v[:written_rows, col0 + D:] == CANARY).all()))


def _note(env, kernel, regime, errs):
    bk = kernel.split(' ')[0]
    for o, e in errs.items():
        k = f'{kernel} {o} {regime}'
        b = fr.bar(o, regime, bk)
        if e / b >= env['ratios'].get(k, (-1.0,))[0]:
            env['ratios'][k] = (e / b, e, b)


def _judge(env, kernel, what, regime, normalize, got, ref, label=None):
    """compare_fourier on one launch's rows, the error printed first and noted for the module's summary; names the worst row"""
    out = 'NORM' if normalize else 'PLAIN'
    bk = kernel.split(' ')[0]
    g = np.asarray(got, np.float64)
    r = np.asarray(ref, np.float64)
    per_row = np.abs(g - r).max(1) / np.maximum(1.0, np.abs(r).max(1))
    finite = np.isfinite(g).all()
    worst = int(np.nanargmax(per_row)) if finite else int(np.argmax(~np.isfinite(g).all(1)))
    err = float(per_row.max()) if finite else float('nan')
    print(f'{kernel} {what}: {out} regime {regime} device error {err:.3g} (bar {fr.bar(out, regime, bk):.3g}) worst row {worst}')
    if finite:
        _note(env, label or kernel, regime, {out: err})
    try:
        fr.compare_fourier(regime, bk, {out: g}, {out: r})
    except AssertionError as e:
        t = fr.TILE.get(bk, 128)
        raise AssertionError(f'{kernel} {what}: {e} - worst row {worst} (tile {worst // t}, wave {worst % t // 16}, row {worst % 16} of the wave)')


def _run_case(env, kernel, case, rows=fr.GPU_ROWS, ldcat=D):
    """a case of fourier_ref.CASES on the first `rows` rows of its base block -> the rows written"""
    variant, regime, prefix, cat, normalize, tab, gaps = case
    raw = _raw(env, regime, prefix, gaps)[:rows]
    h12 = kernel == 'k_fourier_h12'
    out, cap, _ = _launch(env, kernel, variant, prefix, raw, count=rows if h12 else None, cat=_dev(env, fr.gen_cat()[:rows]) if cat else None,
                          ldcat=ldcat, normalize=normalize, table=_table(env, variant, prefix) if tab else None)
    what = f'{fr.case_id(case)} rows={rows}' + (f' ldcat={ldcat}' if cat else '')
    assert _untouched(out, rows), f'{kernel} {what}: written beyond row {rows}'
    got = out[:rows].cpu().numpy()
    _judge(env, kernel + (' (table)' if tab else ''), what, regime, normalize, got, fr.reference(*case)[:rows])
    return out[:rows]


# ------------------------------------------------------------------------------------------------ a. values
@pytest.mark.parametrize('regime', fr.REGIMES)
@pytest.mark.parametrize('variant', fr.VARIANTS)
@pytest.mark.parametrize('kernel', VALUE_KERNELS)
def test_fourier_values(env, kernel, variant, regime):
    """every prefix, plain and normalised, at 257 rows (two tiles of 128 and one row; one of 192 and 65 rows; eight of 32 and one
    row); the n = 2 embedding with its categorical addends at ldcat 128 and 256 (NaN between the rows' 128 addends)"""
    failures = []
    for case in fr.VALUE_CASES:
        if case[:2] != (variant, regime):
            continue
        for ldcat in ((128, 256) if case[3] else (128,)):
            try:
                _run_case(env, kernel, case, ldcat=ldcat)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('n', [2, 3, 4])
@pytest.mark.parametrize('kernel', VALUE_KERNELS)
def test_fourier_row_counts(env, kernel, n):
    """one prefix per n at every small row count around the 16 rows of a wave and the 32-, 128- and 192-row tiles, regime A:
    partial waves, absent waves, a tile of one row"""
    failures = []
    for rows in fr.ROW_COUNTS:
        case = ('scales_a', 'A', fr.PREFIX_OF_N[n], n == 2, n != 2, False, None)
        assert case in fr.CASES
        try:
            _run_case(env, kernel, case, rows=rows)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)


def _copies_equal(out, rows, base, what):
    """every cyclic copy of the base block bit-equal to the first: a row's arithmetic does not depend on its position"""
    v = out[:rows].view(torch.int32)
    full = rows // base
    blocks = v[:full * base].view(full, base, -1)
    same = (blocks == blocks[:1]).all(2)
    if not bool(same.all()):
        c, r = [int(x[0]) for x in torch.nonzero(~same, as_tuple=True)]
        raise AssertionError(f'{what}: row {c * base + r} (copy {c} of base row {r}) differs from the first copy')
    rest = v[full * base:rows]
    assert torch.equal(rest, v[:rows - full * base]), f'{what}: the last, partial copy differs from the first'


@pytest.mark.parametrize('kernel', VALUE_KERNELS)
def test_fourier_persistent_tiles(env, kernel):
    """cap x tile + tile + 5 rows: workgroups 0 and 1 take a second tile (the last of 5 rows), so the weight stream runs across a tile
    boundary.  The inputs repeat the base block of 385 rows (coprime to every tile); the first copy is compared with float64, every
    other copy with the first, bit for bit"""
    case = ('plain', 'A', fr.PREFIX_OF_N[3], False, True, False, None)
    rows = fr.PERSISTENT_ROWS[kernel]
    raw = _rows_of(_raw(env, 'A', case[2]), rows)
    out, cap, _ = _launch(env, kernel, 'plain', case[2], raw, count=rows if kernel == 'k_fourier_h12' else None, normalize=True)
    assert _untouched(out, rows), f'{kernel}: written beyond row {rows}'
    _judge(env, kernel, f'persistent rows={rows}', 'A', True, out[:fr.BASE_ROWS].cpu().numpy(), fr.reference(*case))
    _copies_equal(out, rows, fr.BASE_ROWS, f'{kernel} rows={rows}')


# ------------------------------------------------------------------------------------------------ b. position independence
def _plain_launch(env, kernel, prefix, raw, normalize=True, variant='scales_b'):
    rows = raw.shape[0]
    out, _, _ = _launch(env, kernel, variant, prefix, raw, count=rows if kernel == 'k_fourier_h12' else None, normalize=normalize)
    assert _untouched(out, rows), f'{kernel}: written beyond row {rows}'
    assert bool(torch.isfinite(out[:rows]).all()), f'{kernel}: a row below the count is not finite'
    return out[:rows].view(torch.int32)


def _first_diff(a, b):
    rows = torch.nonzero((a != b).any(1))[:, 0]
    return [int(r) for r in rows[:8]]


@pytest.mark.parametrize('prefix', [fr.PREFIX_OF_N[2], fr.PREFIX_OF_N[4]])
@pytest.mark.parametrize('kernel', ALL_KERNELS)
def test_rows_do_not_depend_on_their_position(env, kernel, prefix):
    """regime C (the slow sine path is a wave-uniform branch: its rows sit next to ordinary ones).  The rows of a launch in
    reversed order give the reversed outputs, and row i of an n-row launch is row i of the 385-row launch, bit for bit"""
    raw = _raw(env, 'C', prefix)
    full = _plain_launch(env, kernel, prefix, raw)
    rev = _plain_launch(env, kernel, prefix, raw.flip(0).contiguous())
    assert torch.equal(rev.flip(0), full), f'{kernel}: rows {_first_diff(rev.flip(0), full)} change with the order of the rows'
    for n in fr.ROW_COUNTS[:-1]:
        part = _plain_launch(env, kernel, prefix, raw[:n])
        assert torch.equal(part, full[:n]), f'{kernel}: rows {_first_diff(part, full[:n])} of a launch of {n} rows differ from the 385-row launch'


@pytest.mark.parametrize('prefix', list(fr.PREFIXES))
def test_h_and_h12_give_the_same_bits_at_small_counts(env, prefix):
    """(the existing suite requires this at 90,001 rows only)"""
    raw = _raw(env, 'B', prefix)
    for n in fr.ROW_COUNTS:
        for normalize in (False, True):
            a = _plain_launch(env, 'k_fourier_h', prefix, raw[:n], normalize)
            b = _plain_launch(env, 'k_fourier_h12', prefix, raw[:n], normalize)
            assert torch.equal(a, b), f'rows {_first_diff(a, b)} of {n} differ between k_fourier_h and k_fourier_h12'


# ------------------------------------------------------------------------------------------------ c. bounds
@pytest.mark.parametrize('kernel,e_cap,counts', [('k_fourier', 257, (0, 1, 127, 128, 129, 257, 264)), ('k_fourier_h', 257, (0, 1, 127, 128, 129, 257, 264)),
                                                 ('k_fourier_h12', fr.H12_MIN_CAP, (0, 191, 192, 193))])
def test_count_dev_bounds_the_rows_written(env, kernel, e_cap, counts):
    """rows < min(count, e_cap) are written and within the bar, every other word of the allocation keeps its bits"""
    case = ('scales_a', 'A', fr.PREFIX_OF_N[4], False, True, False, None)
    raw = _raw(env, 'A', case[2])[:min(e_cap, fr.BASE_ROWS)]
    for count in counts:
        out, cap, _ = _launch(env, kernel, case[0], case[2], raw, count=count, e_cap=e_cap, normalize=True)
        E = min(count, e_cap)
        assert _untouched(out, E), f'{kernel} count {count} e_cap {e_cap}: a word outside rows < {E} changed'
        if E:
            _judge(env, kernel, f'count={count} e_cap={e_cap}', 'A', True, out[:E].cpu().numpy(), fr.reference(*case)[:E])


@pytest.mark.parametrize('kernel', ['k_fourier', 'k_fourier_h'])
def test_e_cap_0_returns_0(env, kernel):
    out, _, rc = _launch(env, kernel, 'plain', fr.PREFIX_OF_N[3], _raw(env, 'A', fr.PREFIX_OF_N[3])[:0], e_cap=0)
    assert rc == 0 and _untouched(out, 0)


@pytest.mark.parametrize('kernel', VALUE_KERNELS)
def test_rows_of_stride_512_keep_their_other_columns(env, kernel):
    """the rollout's fus_in + 128 with stride 512: columns 0 .. 127 and 256 .. 511 of every row keep their bits"""
    case = ('plain', 'A', fr.CAT_PREFIX, True, False, False, None)
    rows = fr.GPU_ROWS
    out, _, _ = _launch(env, kernel, case[0], case[2], _raw(env, 'A', case[2])[:rows], count=rows if kernel == 'k_fourier_h12' else None,
                        cat=_dev(env, fr.gen_cat()[:rows]), ldo=512, col0=128)
    assert _untouched(out, rows, col0=128), f'{kernel}: a column outside [128, 256) or a row beyond {rows} changed'
    _judge(env, kernel, 'ldo=512', 'A', False, out[:rows, 128:256].cpu().numpy(), fr.reference(*case)[:rows])


# ------------------------------------------------------------------------------------------------ d. packed rows
@pytest.mark.parametrize('prefix', [fr.PREFIX_OF_N[3], fr.PREFIX_OF_N[4]])
@pytest.mark.parametrize('kernel', ['k_fourier_h', 'k_fourier_h12'])
def test_packed_rows(env, kernel, prefix):
    """infgen_fourier_embed_r24: the bytes of rows < E are pack_r24 of the fp32 rows the same kernel writes for the same inputs
    (it packs the same registers), the bytes of rows >= E are untouched (store_rows_r24's guard inside a wave's 16 rows), and the
    values they stand for are within the bar plus half a 24-bit step (_r24_excess) of float64"""
    case = ('scales_a', 'C', prefix, False, True, False, None)
    e_cap = fr.H12_MIN_CAP if kernel == 'k_fourier_h12' else fr.GPU_ROWS
    for rows in (1, 15, 16, 17, 127, 129, 193):
        raw = _raw(env, 'C', prefix)[:rows]
        packed, _, _ = _launch(env, kernel, case[0], prefix, raw, count=rows, e_cap=e_cap, r24=True)
        plain, _, _ = _launch(env, kernel, case[0], prefix, raw, count=rows, e_cap=e_cap, normalize=True)
        assert _untouched(packed, rows, r24=True), f'{kernel} rows={rows}: packed bytes beyond row {rows} changed'
        got = packed[:rows].cpu().numpy()
        want = ea.pack_r24(plain[:rows].cpu().numpy())
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, f'{kernel} rows={rows}: packed rows {bad[:8]} are not the packed fp32 rows'
        val = ea.unpack_r24(got).astype(np.float64)
        assert np.isfinite(val).all()
        x = _r24_excess(val, fr.reference(*case)[:rows], fr.bar('NORM', 'C', kernel))
        print(f'{kernel} (r24) rows={rows}: error / (bar + half a 24-bit step) = {x:.3g}')
        assert x <= 1.0, f'{kernel} rows={rows}: packed rows off by {x:.3g} x (bar + half a 24-bit step)'


def test_packed_rows_are_refused_by_the_fp32_kernel(env):
    prefix = fr.PREFIX_OF_N[3]
    out, _, rc = _launch(env, 'k_fourier', 'plain', prefix, _raw(env, 'A', prefix)[:33], count=33, r24=True, expect_fail=True)
    assert rc != 0 and _untouched(out, 0, r24=True)


# ------------------------------------------------------------------------------------------------ e. table mode
def _table(env, variant, prefix, check=True):
    """the last-dim table of a pack by infgen_fourier_last_dim_table (gemm_terms 3), checked against table_ref once"""
    from infgen_amd import _lib
    key = ('table', variant, prefix)
    if key not in env['packs']:
        t = torch.full((fr.TAB_ROWS + GUARD_ROWS, D), float('nan'), device=env['dev'])
        with _gpu_call(), _modes(env):
            _lib.check(env['lib'].infgen_fourier_last_dim_table(_pack(env, variant, prefix).data_ptr(), fr.PREFIXES[prefix], t.data_ptr(), None),
                       'infgen_fourier_last_dim_table')
            torch.cuda.synchronize()
        assert _untouched(t, fr.TAB_ROWS), 'the table launch wrote beyond its 32 rows'
        got = t[:fr.TAB_ROWS].cpu().numpy()
        assert np.isfinite(got).all()
        err = fr.row_error(got, fr.table_ref(variant, prefix))
        b = fr.bar('PLAIN', 'A', 'k_fourier_h')
        print(f'table {variant} {prefix}: error {err:.3g} (bar {b:.3g})')
        _note(env, 'k_fourier_h (the table)', 'A', dict(PLAIN=err))
        assert err <= b, f'table {variant} {prefix}: error {err:.3g} beyond the bar {b:.3g}'
        env['ran'].add('k_fourier_h (dt_mode 2)')
        env['packs'][key] = t[:fr.TAB_ROWS].contiguous()
    return env['packs'][key]


@pytest.mark.parametrize('regime', ['A', 'C'])
@pytest.mark.parametrize('variant', fr.VARIANTS)
def test_table_mode_values(env, variant, regime):
    """n = 4, and n = 3 with an integer-valued last input; regime C carries the gaps 0, -31, -32, -40, +3 and -2.5: the reference
    takes the clamped row, nothing outside the table is read"""
    failures = []
    for case in fr.TAB_CASES:
        if case[:2] != (variant, regime):
            continue
        try:
            _run_case(env, 'k_fourier_h', case)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)


def test_table_mode_row_counts_and_persistent_tiles(env):
    """the weight stream has one more unit per tile in this mode (the dims' units, then to_out.2's from a second segment): the
    small row counts, and the count at which two workgroups take a second tile"""
    case = ('scales_b', 'C', fr.PREFIX_OF_N[4], False, True, True, True)
    assert case in fr.CASES
    failures = []
    for rows in fr.ROW_COUNTS:
        try:
            _run_case(env, 'k_fourier_h', case, rows=rows)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)
    for prefix in (fr.PREFIX_OF_N[4], fr.PREFIX_OF_N[3]):
        case = ('plain', 'C', prefix, False, True, True, True)
        rows = fr.PERSISTENT_ROWS['k_fourier_h']
        out, _, _ = _launch(env, 'k_fourier_h', 'plain', prefix, _rows_of(_raw(env, 'C', prefix, True), rows), normalize=True,
                            table=_table(env, 'plain', prefix))
        assert _untouched(out, rows)
        _judge(env, 'k_fourier_h (table)', f'persistent rows={rows}', 'C', True, out[:fr.BASE_ROWS].cpu().numpy(), fr.reference(*case))
        _copies_equal(out, rows, fr.BASE_ROWS, f'k_fourier_h (table) rows={rows}')


def test_table_mode_refusals(env):
    """fourier_embed_impl: the table needs the split kernel and a table"""
    prefix = fr.PREFIX_OF_N[4]
    raw = _raw(env, 'A', prefix)[:33]
    tab = _table(env, 'plain', prefix)
    out, _, rc = _launch(env, 'k_fourier', 'plain', prefix, raw, table=tab, expect_fail=True)
    assert rc != 0 and _untouched(out, 0)
    out, _, rc = _launch(env, 'k_fourier_h', 'plain', prefix, raw, table=False, expect_fail=True)
    assert rc != 0 and _untouched(out, 0)
    t = torch.full((fr.TAB_ROWS, D), float('nan'), device=env['dev'])
    with _modes(env, fourier_mode=0):
        assert env['lib'].infgen_fourier_last_dim_table(_pack(env, 'plain', prefix).data_ptr(), 4, t.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert bool((t.view(torch.int32) == CANARY).all())


# ------------------------------------------------------------------------------------------------ f. in-step: k_fourier_h_multi
SCENE_SEEDS = ((7301, 60.0), (7302, 40.0))          # tests/test_layers_stack_gpu.py: the first two base scenes of 32 rows
SETS = (('t', 'agent_encoder.r_t_emb', 4), ('m', 'agent_encoder.r_pt2a_emb', 3), ('a', 'agent_encoder.r_a2a_emb', 3))


@pytest.fixture(scope='module')
def engine(env):
    """a two-scene, 32-row context as tests/test_layers_stack_gpu.py builds it: RolloutEngine + prologue(), no graph"""
    from infgen_amd import engine as eng, synth
    cfg = synth.standard_config()
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scenes = [synth.make_scene(seed, n, m, cfg, half_extent=ext, ego_last=(k % 2 == 0), vocab=vocab, grid=grid, slip=0.3)
              for k, ((seed, ext), (n, m)) in enumerate(zip(SCENE_SEEDS, ls.BASE_SCENES[32]))]
    with _gpu_call():
        w = eng.PackedWeights(fr.weights('plain'), cfg, env['dev'])
        e = eng.RolloutEngine(w, scenes, vocab, map_vocab, grid, a_cap=32, store_logits=False, use_graph=False, options=dict(layers_p=1))
        e.prologue()
        torch.cuda.synchronize()
    assert e.rows == 64
    return e


@pytest.mark.parametrize('rhat_format', [0, 1], ids=['fp32', 'r24'])
@pytest.mark.parametrize('layers_p', [1, 0])
def test_in_step_fourier_sets(env, engine, layers_p, rhat_format):
    """infgen_decode_layers(ctx, 1, 0): the step's three sets in ONE launch of k_fourier_h_multi (gridDim.y = the sets, counts from
    the device totals, the temporal set through the engine's time-gap table, rows fp32 or packed).  Each set's rhat rows against
    the normalised float64 reference of the raw rows read back, with the engine's own state dict; rows at or beyond the total
    keep the sentinel they held before the call"""
    from infgen_amd import _lib
    e = engine
    e.options = dict(layers_p=layers_p, rhat_format=rhat_format)
    e._refresh_opts()
    assert e._ctx.four_t_dt is not None, 'the time-gap table is the path a rollout takes'
    for k, _, _ in SETS:
        e.edges[k]['rhat'].view(torch.int32).fill_(CANARY)
    with _gpu_call():
        _lib.prof_enable((1 << len(_lib.KERNEL_IDS)) - 1)
        try:
            _lib.check(env['lib'].infgen_decode_layers(C.byref(e._ctx), 1, 0, e.ops.stream), 'infgen_decode_layers')
            torch.cuda.synchronize()
            counts = _lib.prof_collect()
        finally:
            _lib.prof_enable(0)
    # fourier_multi_ok (csrc/api.hip): 64 rows, edges, the split kernel, no overlap -> one multi-set launch, not three
    assert counts['k_fourier']['calls'] == 1, counts['k_fourier']
    env['ran'].add('k_fourier_h_multi' + (' (r24)' if rhat_format else ''))
    sd = e.w.sd
    # step_mode (csrc/api.hip): the packed rows need the fused edge side, which 64 rows take inside k_layers_p only - under the
    # per-sublayer launches rhat_format 1 leaves fp32 rows
    assert env['lib'].infgen_layers_p_capacity() > 0
    r24 = bool(rhat_format) and bool(layers_p)
    for k, prefix, n in SETS:
        ed = e.edges[k]
        total, cap = int(ed['total'].item()), ed['cap']
        assert 0 < total <= cap, (k, total, cap)
        assert counts['k_fourier']['rows'].get(n, 0) >= total
        raw = ed['raw'][:total].cpu().numpy()
        assert np.isfinite(raw[:, :n]).all()
        words = ed['rhat'].view(torch.int32).view(-1)
        row_words = ea.R24_ROW_BYTES // 4 if r24 else D
        assert bool((words[total * row_words:] == CANARY).all()), f'set {k}: a word at or beyond row {total} changed'
        if r24:
            got = ea.unpack_r24(ed['rhat'].view(torch.uint8).view(-1)[:total * ea.R24_ROW_BYTES].view(total, ea.R24_ROW_BYTES).cpu().numpy())
        else:
            got = ed['rhat'][:total].cpu().numpy()
        if k == 't':
            gap = raw[:, 3]
            assert (gap == np.trunc(gap)).all() and gap.max() <= 0 and gap.min() > -fr.TAB_ROWS
        ref = fr.fourier_ref(sd, prefix, raw, normalize=True, tab=(k == 't'))
        assert np.isfinite(got).all(), f'set {k}: a row below the total is not finite'
        b = fr.bar('NORM', 'A', 'k_fourier_h_multi')
        what = f'k_fourier_h_multi layers_p={layers_p} {"r24" if r24 else "fp32"} set {k} ({total} rows)'
        if r24:
            x = _r24_excess(got, ref, b)
            print(f'{what}: error / (bar + half a 24-bit step) = {x:.3g}')
            assert x <= 1.0, f'{what}: packed rows off by {x:.3g} x (bar + half a 24-bit step)'
        else:
            err = fr.row_error(got, ref)
            print(f'{what}: error {err:.3g} (bar {b:.3g})')
            _note(env, 'k_fourier_h_multi', 'A', dict(NORM=err))
            assert err <= b, f'{what}: error {err:.3g} beyond the bar {b:.3g}'
