"""Operator-level tests of the edge-attention kernels through the C ABI - k_edge_attn / k_edge_attn_wide with and without rhat
(infgen_edge_attn_mode), the switch of infgen_edge_attn at 256 rows, every k_edge_fused / k_edge_fused3 instantiation an option
reaches (infgen_edge_attn_fused under InfgenOptions.edge_kernel / edge_loop), the switch of edge_kernel = 1 at 4096 rows and the
four packed-row instantiations (infgen_edge_attn_fused_r24) - each against the plain float64 reference of tests/edge_attn_ref.py,
never against another kernel: error relative to max |ref| within edge_attn_ref.bar (four times the error of a float32 numpy
evaluation of the same formula, per output and score regime), rows without edges exactly zero, a NaN-filled guard tail of rows
behind every output untouched, every row below `rows` finite, and the same bits from a second launch.
tests/test_edge_attn_ref_cpu.py shows that this comparison tells the reference's deliberately wrong variants apart."""
import ctypes as C

import numpy as np
import pytest
import torch

import edge_attn_ref as ea

pytestmark = pytest.mark.gpu

GUARD_ROWS = 5
CANARY = 0x7fc00000                     # the bits torch.full(..., nan) writes
FUSED_SELECTIONS = [(0, 6), (0, 4), (0, 8), (2, 4), (2, 6), (2, 8)]      # (edge_kernel, edge_loop)


@pytest.fixture(scope='module')
def env():
    from infgen_amd import _lib, packing
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    dev = torch.device('cuda:0')
    pack = torch.from_numpy(packing.pack_attention_layer(ea.weights(), ea.PREFIX)).to(dev)
    return dict(lib=_lib.load(), dev=dev, pack=pack, cases={})


def _device_case(env, name):
    """device copies of a case's inputs (cached per module: the kernels only read them), the packed 24-bit rows among them"""
    if name not in env['cases']:
        c = ea.gen_case(name)
        d = {k: torch.from_numpy(np.array(c[k])).to(env['dev']) for k in ('q', 'u', 'k', 'k_nor', 'v', 'off', 'cnt', 'src', 'rhat')}
        d['rhat24'] = torch.from_numpy(ea.pack_r24(c['rhat'])).to(env['dev'])
        env['cases'][name] = d
    return env['cases'][name]


def _out(env, rows, width):
    return torch.full(((rows + GUARD_ROWS) * width,), float('nan'), device=env['dev'])


def _launch(env, name, entry, wide=None, hasr=True, kernel=None, loop=None):
    """one launch of `entry` ('mode', 'auto', 'fused', 'r24') into fresh NaN-filled outputs with guard tails -> {output: tensor}"""
    from infgen_amd import _lib
    lib, c, d = env['lib'], ea.gen_case(name), _device_case(env, name)
    rows = c['rows']
    p = lambda t: t.data_ptr()
    lists = (p(d['off']), p(d['cnt']), p(d['src']))
    o = _lib.Options()
    _lib.check(lib.infgen_get_options(C.byref(o)))
    if kernel is not None:
        o.edge_kernel, o.use = kernel, 0
    if loop is not None:
        o.edge_loop, o.use = loop, 0
    with _lib.thread_options(o):
        if entry in ('mode', 'auto'):
            out = dict(AGG=_out(env, rows, 128), SIG=_out(env, rows, 8))
            if hasr:
                out['Z'] = _out(env, rows, 1024)
            args = (rows, p(d['q']), p(d['u']) if hasr else None, p(d['k'] if hasr else d['k_nor']), p(d['v']), *lists,
                    p(d['rhat']) if hasr else None, p(out['AGG']), p(out['Z']) if hasr else None, p(out['SIG']))
            if entry == 'mode':
                _lib.check(lib.infgen_edge_attn_mode(*args, int(wide), None), 'infgen_edge_attn_mode')
            else:
                _lib.check(lib.infgen_edge_attn(*args, None), 'infgen_edge_attn')
        else:
            out = dict(FUSED=_out(env, rows, 128))
            args = (rows, p(d['q']), p(env['pack']), p(d['k']), p(d['v']), *lists)
            if entry == 'fused':
                _lib.check(lib.infgen_edge_attn_fused(*args, p(d['rhat']), p(out['FUSED']), None), 'infgen_edge_attn_fused')
            else:
                _lib.check(lib.infgen_edge_attn_fused_r24(*args, p(d['rhat24']), p(out['FUSED']), None), 'infgen_edge_attn_fused_r24')
    torch.cuda.synchronize()
    return out


WIDTH = dict(AGG=128, Z=1024, SIG=8, FUSED=128)


def _same_bits(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a) and set(a) == set(b)


def _check(env, name, kind, what, **launch):
    """the checks of one launch: the comparison with float64 (edge_attn_ref.compare_edge: bars, finite rows, exact zeros on rows
    without edges), the guard tails, a second launch's bits -> the first launch's outputs"""
    c = ea.gen_case(name)
    rows = c['rows']
    out = _launch(env, name, **launch)
    for k, t in out.items():
        tail = t[rows * WIDTH[k]:].view(torch.int32)
        assert tail.numel() == GUARD_ROWS * WIDTH[k] and bool((tail == CANARY).all()), f'{what}: {k} written beyond row {rows}'
    got = {k: t[:rows * WIDTH[k]].cpu().numpy() for k, t in out.items()}
    ref = ea.reference(name, kind)
    try:
        errs = ea.compare_edge(c['regime'], got, ref, c['cnt'])
    finally:
        fig = {k: float(np.nanmax(np.abs(got[k].astype(np.float64).reshape(ref[k].shape) - ref[k])) / np.abs(ref[k]).max()) for k in ref}
        print(f'{what} {name} regime {c["regime"]}: device errors ' +
              ' '.join(f'{k} {fig[k]:.3g} (bar {ea.bar(k, c["regime"]):.3g})' for k in fig))
    assert _same_bits(out, _launch(env, name, **launch)), f'{what}: a second launch gave other bits'
    return out


@pytest.mark.parametrize('hasr', [True, False], ids=['rhat', 'norhat'])
@pytest.mark.parametrize('wide', [0, 1], ids=['wave', 'wide'])
@pytest.mark.parametrize('name', ea.SMALL_CASES)
def test_edge_attn_mode(env, name, wide, hasr):
    """k_edge_attn (wide = 0) and k_edge_attn_wide (wide = 1): AGG, Z, SIG with rhat and U; AGG, SIG of the loops without
    (rhat = U = Z = NULL)"""
    _check(env, name, 'r' if hasr else 'nor', f'edge_attn_mode wide={wide} hasr={hasr}', entry='mode', wide=wide, hasr=hasr)


@pytest.mark.parametrize('name,wide', [('rows256', 1), ('rows257', 0)])
def test_edge_attn_picks_by_row_count(env, name, wide):
    """infgen_edge_attn: the wide kernel up to 256 rows, one wave per destination from 257 - both sides of the switch against
    float64 and bit-equal to the mode it should have picked (and not to the other)"""
    auto = _check(env, name, 'r', 'edge_attn auto', entry='auto')
    assert _same_bits(auto, _check(env, name, 'r', f'edge_attn_mode wide={wide}', entry='mode', wide=wide))
    assert not _same_bits(auto, _launch(env, name, entry='mode', wide=1 - wide))


@pytest.mark.parametrize('kernel,loop', FUSED_SELECTIONS)
@pytest.mark.parametrize('name', ea.SMALL_CASES)
def test_edge_attn_fused(env, name, kernel, loop):
    """edge_kernel 0: k_edge_fused<6, false, 1, 16> / <4, false, 2, 16> / <8, false, 2, 16> (at most 4096 rows); edge_kernel 2:
    k_edge_fused3<4 / 6 / 8>"""
    _check(env, name, 'fused', f'edge_attn_fused kernel={kernel} loop={loop}', entry='fused', kernel=kernel, loop=loop)


def test_edge_attn_fused_beyond_4096_rows(env):
    """edge_kernel 0, edge_loop 6, 4112 rows: k_edge_fused<6, false, 1, 8>"""
    _check(env, 'rows4112', 'fused', 'edge_attn_fused kernel=0 loop=6', entry='fused', kernel=0, loop=6)


@pytest.mark.parametrize('name,forced', [('rows4096', 0), ('rows4112', 2)])
def test_edge_attn_fused_picks_by_row_count(env, name, forced):
    """edge_kernel 1 (the default): k_edge_fused up to 4096 rows, k_edge_fused3 beyond - both sides of the switch against float64
    and bit-equal to the forced kernel (and not to the other)"""
    from infgen_amd import _lib
    o = _lib.Options()
    _lib.check(env['lib'].infgen_get_options(C.byref(o)))
    assert (o.edge_kernel, o.edge_loop) == (1, 6), 'the defaults this test is about'
    auto = _check(env, name, 'fused', 'edge_attn_fused default', entry='fused')
    assert _same_bits(auto, _check(env, name, 'fused', f'edge_attn_fused kernel={forced}', entry='fused', kernel=forced, loop=6))
    assert not _same_bits(auto, _launch(env, name, entry='fused', kernel=2 - forced, loop=6))


@pytest.mark.parametrize('loop', [6, 4, 8])
@pytest.mark.parametrize('name', ea.SMALL_CASES)
def test_edge_attn_fused_r24(env, name, loop):
    """k_edge_fused<6, true, 1, 16> / <4, true, 2, 16> / <8, true, 2, 16> on pack_r24's rows against the reference on
    unpack_r24(pack_r24(rhat)): exactly known inputs, so the bars are those of the fp32 rows (r24tie: every value a tie)"""
    _check(env, name, 'fused_r24', f'edge_attn_fused_r24 loop={loop}', entry='r24', loop=loop)


def test_edge_attn_fused_r24_beyond_4096_rows(env):
    """4112 rows: k_edge_fused<6, true, 1, 8>; edge_kernel 2 does not apply to packed rows (the same bits as edge_kernel 0)"""
    a = _check(env, 'rows4112', 'fused_r24', 'edge_attn_fused_r24 loop=6', entry='r24', kernel=0, loop=6)
    assert _same_bits(a, _launch(env, 'rows4112', entry='r24', kernel=2, loop=6))
