"""Operator-level tests of the node-side attention kernels through the C ABI - k_attn_pre / k_attn_post (attn_mode 0), k_attn_h<4, 3>
(attn_mode 1) and k_attn_hs<3> (attn_mode 3) behind infgen_attn_pre, infgen_attn_post and infgen_attn_post_pre, in the pointer
combinations the rollout issues (node_attn_ref.FORMS), the by-size switch of attn_mode 2, the persistent tiles of k_attn_h beyond
32,768 rows, and k_mlpemb_h / the fp32 chain behind infgen_mlp_embedding - each against the plain float64 reference of
tests/node_attn_ref.py, never against another kernel: every output's row error (max |got - ref| / max(1, max |ref row|)) within
node_attn_ref.bar (four times the error of a float32 numpy evaluation of the same formulas, per output and input regime), a
NaN-filled guard tail of 64 rows behind every output untouched, the inputs unchanged, every row below `rows` finite, and the same
bits from a second launch.  Weight variants spread the operand scales AH_HDR[0..9], separate the LayerNorms and kill the FFN's hidden
layer; input regimes scale rows by 2^-20 .. 2^20 and add degenerate rows.  tests/test_node_attn_ref_cpu.py shows that this
comparison tells the reference's deliberately wrong variants apart.  The largest device error / bar per output, regime and kernel
family is printed at the end of the module and written as JSON to the file INFGEN_NODE_ATTN_RECORD names, if it is set.

Out of scope here: gemm_terms 1 and 2, k_attn_h<8, 3> (an environment knob read at load time) and the row-group list path; k_layers_p
has its own operator-level tests in tests/test_layers_stack_gpu.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import node_attn_ref as na

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
CANARY = 0x7fc00000                     # the bits torch.full(..., nan) writes
KERNELS = {0: 'fp32-mfma', 1: 'k_attn_h', 3: 'k_attn_hs'}
WIDTH = dict(X=128, Q=128, U=1024, K=128, V=128)
CHUNK = 8192                            # rows per comparison of the large cases


@pytest.fixture(scope='module')
def env():
    from infgen_amd import _lib
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    e = dict(lib=_lib.load(), dev=torch.device('cuda:0'), packs={}, inputs={}, ratios={})
    yield e
    for k, (r, err, b) in sorted(e['ratios'].items()):
        print(f'node attn worst {k}: error {err:.3g} / bar {b:.3g} = {r:.2f}')
    if os.environ.get('INFGEN_NODE_ATTN_RECORD'):
        with open(os.environ['INFGEN_NODE_ATTN_RECORD'], 'w') as f:
            json.dump({k: dict(ratio=r, error=err, bar=b) for k, (r, err, b) in e['ratios'].items()}, f, indent=1, sort_keys=True)


def _modes(env, attn_mode):
    """the calling thread's option block for the operator-level entries (no process-wide state is edited)"""
    from infgen_amd import _lib
    o = _lib.Options()
    _lib.check(env['lib'].infgen_get_options(C.byref(o)))
    if attn_mode is not None:
        o.attn_mode = int(attn_mode)
    o.use = 0
    return _lib.thread_options(o)


class _gpu_call:
    """a failed launch or synchronisation ends the session: nothing more is started on a device that reported an error"""

    def __enter__(self):
        return self

    def __exit__(self, kind, exc, tb):
        if kind is not None and not issubclass(kind, AssertionError):
            pytest.exit(f'device error, session stopped: {exc}', returncode=3)
        return False


def _pack(env, variant, prefix):
    from infgen_amd import packing
    if (variant, prefix) not in env['packs']:
        env['packs'][variant, prefix] = torch.from_numpy(packing.pack_attention_layer(na.weights(variant), prefix)).to(env['dev'])
    return env['packs'][variant, prefix]


def _inputs(env, regime, base, rows):
    """device copies of the first `rows` rows of a base block, or (rows > base) of the block repeated cyclically"""
    key = (regime, base, rows)
    if key not in env['inputs']:
        idx = torch.arange(rows, device=env['dev']) % base
        env['inputs'][key] = tuple(torch.from_numpy(np.array(a)).to(env['dev'])[idx].contiguous() for a in na.gen_inputs(regime, base))
    return env['inputs'][key]


def _out(env, rows, width):
    return torch.full(((rows + GUARD_ROWS) * width,), float('nan'), device=env['dev'])


def _launch(env, mode, variant, regime, form, rows, base):
    """one launch of an entry form into fresh NaN-filled outputs with guard tails (X: the input rows in front of its tail)
    -> ({output: tensor}, the inputs' device tensors)"""
    from infgen_amd import _lib
    lib = env['lib']
    has_post, has_pos, pre, outs = na.FORMS[form]
    x0, agg, z, sig = _inputs(env, regime, base, rows)
    p = lambda t: None if t is None else t.data_ptr()
    out = {o: _out(env, rows, WIDTH[o]) for o in outs if o != 'X'}
    X = _out(env, rows, 128)
    X[:rows * 128] = x0.reshape(-1)
    o_ = lambda n: p(out.get(n))
    with _gpu_call(), _modes(env, mode):
        if not has_post:
            _lib.check(lib.infgen_attn_pre(p(X), rows, p(_pack(env, variant, na.PRE_PREFIX)), int(pre == 'src'), o_('Q'), o_('U'), o_('K'),
                                           o_('V'), None), 'infgen_attn_pre')
        else:
            zs = (p(z), p(sig)) if has_pos else (None, None)
            post = _pack(env, variant, na.POST_PREFIX)
            if pre:
                _lib.check(lib.infgen_attn_post_pre(p(X), rows, p(post), p(agg), *zs, has_pos, p(_pack(env, variant, na.PRE_PREFIX)),
                                                    o_('Q'), o_('U'), o_('K'), o_('V'), None), 'infgen_attn_post_pre')
            else:
                _lib.check(lib.infgen_attn_post(p(X), rows, p(post), p(agg), *zs, has_pos, None), 'infgen_attn_post')
        torch.cuda.synchronize()
    out['X'] = X
    return out


def _same_bits(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def _note(env, what, regime, errs):
    for o, e in errs.items():
        k = f'{what} {o} {regime}'
        r = e / na.bar(o, regime)
        if r >= env['ratios'].get(k, (-1.0,))[0]:
            env['ratios'][k] = (r, e, na.bar(o, regime))


def _check(env, mode, variant, regime, form, rows, base=na.SMALL_ROWS):
    """the checks of one launch: guard tails, inputs unchanged, the comparison with float64 (node_attn_ref.compare_node: finite
    rows, bars), a second launch's bits -> the first launch's outputs"""
    what = f'{KERNELS.get(mode, "default")} {variant} {form} rows={rows}'
    outs = na.FORMS[form][3]
    out = _launch(env, mode, variant, regime, form, rows, base)
    for k, t in out.items():
        tail = t[rows * WIDTH[k]:].view(torch.int32)
        assert tail.numel() == GUARD_ROWS * WIDTH[k] and bool((tail == CANARY).all()), f'{what}: {k} written beyond row {rows}'
    idx = torch.arange(rows, device=env['dev']) % base
    for name, t, host in zip(('X', 'AGG', 'Z', 'SIG'), _inputs(env, regime, base, rows), na.gen_inputs(regime, base)):
        if name == 'X':
            if 'X' not in outs:          # a pre-only entry must not write X
                assert torch.equal(out['X'][:rows * 128].view(torch.int32), t.reshape(-1).view(torch.int32)), f'{what}: X changed'
            continue
        fresh = torch.from_numpy(np.array(host)).to(env['dev'])[idx]
        assert torch.equal(t.view(torch.int32), fresh.view(torch.int32)), f'{what}: input {name} changed'
    ref = na.reference(variant, regime, form, base)
    worst, failure = {}, None
    for r0 in range(0, rows, CHUNK):
        r1 = min(rows, r0 + CHUNK)
        src = np.arange(r0, r1) % base
        got = {o: out[o][r0 * WIDTH[o]:r1 * WIDTH[o]].cpu().numpy().reshape(r1 - r0, WIDTH[o]) for o in outs}
        want = {o: ref[o][src] for o in outs}
        for o in outs:
            if np.isfinite(got[o]).all():
                worst[o] = max(worst.get(o, 0.0), na.row_error(got[o], want[o]))
        try:
            na.compare_node(regime, got, want)
        except AssertionError as e:
            failure = failure or e
    print(f'{what} regime {regime}: device errors ' + ' '.join(f'{o} {worst.get(o, float("nan")):.3g} (bar {na.bar(o, regime):.3g})' for o in outs))
    _note(env, KERNELS.get(mode, 'default'), regime, worst)
    if failure:
        raise AssertionError(f'{what}: {failure}')
    assert _same_bits(out, _launch(env, mode, variant, regime, form, rows, base)), f'{what}: a second launch gave other bits'
    return out


@pytest.mark.parametrize('form', list(na.FORMS))
@pytest.mark.parametrize('regime', na.REGIMES)
@pytest.mark.parametrize('variant', na.VARIANTS)
@pytest.mark.parametrize('mode', list(KERNELS), ids=list(KERNELS.values()))
def test_node_attn_forms(env, mode, variant, regime, form):
    """every kernel, weight variant, input regime and entry form at 65 rows: a full 64-row tile (two 32-row tiles, four 16-row
    groups) and one more row"""
    _check(env, mode, variant, regime, form, na.GPU_ROWS)


@pytest.mark.parametrize('rows', na.ROW_COUNTS)
@pytest.mark.parametrize('variant', ['scales_a', 'scales_b', 'ln'])
@pytest.mark.parametrize('mode', list(KERNELS), ids=list(KERNELS.values()))
def test_node_attn_row_counts(env, mode, variant, rows):
    """infgen_attn_post_pre with all four outputs around the 16-row group, the fp32 kernels' 32-row tile and the 64-row tile: a
    partial last group, absent waves, rows beyond the end that reload the last row"""
    _check(env, mode, variant, 'A', 'post_pre4', rows)


@pytest.mark.parametrize('regime', ['B', 'C'])
@pytest.mark.parametrize('rows', [1, 17, 63, 129])
@pytest.mark.parametrize('mode', list(KERNELS), ids=list(KERNELS.values()))
def test_node_attn_pre_row_counts(env, mode, regime, rows):
    """the pre part alone (X read-only) at partial tiles, on scaled and degenerate rows"""
    _check(env, mode, 'ln', regime, 'pre_dst4', rows)
    _check(env, mode, 'ln', regime, 'pre_src_kv', rows)


@pytest.mark.parametrize('form', ['post_pre4', 'post_pre_fused'], ids=['has_pos1', 'has_pos0'])
def test_attn_h_persistent_tiles(env, form):
    """k_attn_h at 32,768 + 69 rows: 514 tiles on 512 workgroups, so two workgroups take a second tile (one of them of 5 rows) and
    their weight ring carries over from one tile's quarter stream into the next.  The inputs repeat a base block of 997 rows
    cyclically; every device row is compared with the float64 reference of its base row."""
    _check(env, 1, 'plain', 'A', form, na.PERSISTENT_ROWS, base=na.CYCLE_ROWS)


@pytest.mark.parametrize('rows,forced,other', [(6144, 3, 0), (6145, 0, 3), (10240, 0, 1), (10241, 1, 0)])
def test_attn_mode_2_picks_by_row_count(env, rows, forced, other):
    """the default mode: k_attn_hs up to 6,144 rows, the fp32-MFMA kernels from 6,145 to 10,240, k_attn_h from 10,241 - both sides of
    each switch against float64, bit-equal to the forced kernel and not to its neighbour"""
    if 'INFGEN_ATTN_HS_MAX' in os.environ:
        pytest.skip('INFGEN_ATTN_HS_MAX moves the switch')
    from infgen_amd import _lib
    o = _lib.Options()
    _lib.check(env['lib'].infgen_get_options(C.byref(o)))
    assert o.attn_mode == 2, 'the default this test is about'
    assert rows in na.SWITCH_ROWS
    args = ('plain', 'A', 'post_pre4', rows, na.CYCLE_ROWS)
    auto = _check(env, None, *args)
    assert _same_bits(auto, _check(env, forced, *args))
    # (k_attn_hs and k_attn_h issue the same products in the same order and give the same bits here, U included: only the
    # switches to and from the fp32-MFMA kernels show in the bits)
    assert not _same_bits(auto, _launch(env, other, *args))


# ------------------------------------------------------------------------------------------------ infgen_mlp_embedding
LDX_PAD, LDY_PAD = 12, 8                # columns behind K0 / behind the 128 outputs (rows stay 16-byte aligned)


def _mlp_pack(env, variant, k0):
    from infgen_amd import packing
    key = ('mlp', variant, k0)
    if key not in env['packs']:
        env['packs'][key] = torch.from_numpy(packing.pack_mlp_embedding(na.mlp_weights(variant, k0), na.MLP_PREFIX)).to(env['dev'])
    return env['packs'][key]


def _mlp_launch(env, mode, variant, x, k0, rows):
    from infgen_amd import _lib
    dev = env['dev']
    ldx, ldy = k0 + LDX_PAD, 128 + LDY_PAD
    X = torch.full((rows, ldx), float('nan'), device=dev)
    X[:, :k0] = x
    Y = torch.full((rows + GUARD_ROWS, ldy), float('nan'), device=dev)
    t1, t2 = torch.zeros(rows, 128, device=dev), torch.zeros(rows, 128, device=dev)
    pack = _mlp_pack(env, variant, k0)
    with _gpu_call(), _modes(env, mode):
        _lib.check(env['lib'].infgen_mlp_embedding(X.data_ptr(), ldx, rows, k0, pack.data_ptr(), t1.data_ptr(), t2.data_ptr(),
                                                   Y.data_ptr(), ldy, None), 'infgen_mlp_embedding')
        torch.cuda.synchronize()
    return X, Y


def _mlp_check(env, mode, variant, regime, k0, rows, base):
    what = f'mlp_embedding {"k_mlpemb_h" if mode else "fp32-mfma"} {variant} K0={k0} rows={rows}'
    idx = torch.arange(rows, device=env['dev']) % base
    x = torch.from_numpy(np.array(na.gen_mlp_inputs(regime, base)[:, :k0])).to(env['dev'])[idx].contiguous()
    X, Y = _mlp_launch(env, mode, variant, x, k0, rows)
    Yi = Y.view(torch.int32)
    assert bool((Yi[rows:] == CANARY).all()), f'{what}: written beyond row {rows}'
    assert bool((Yi[:rows, 128:] == CANARY).all()), f'{what}: written beyond column 128'
    assert torch.equal(X[:, :k0].view(torch.int32), x.view(torch.int32)) and bool((X[:, k0:].view(torch.int32) == CANARY).all()), f'{what}: X changed'
    got = Y[:rows, :128].cpu().numpy()
    ref = na.mlp_reference(variant, regime, k0, base)[np.arange(rows) % base]
    err = na.row_error(got, ref) if np.isfinite(got).all() else float('nan')
    print(f'{what} regime {regime}: device error {err:.3g} (bar {na.bar("MLPEMB", regime):.3g})')
    if err == err:
        _note(env, 'k_mlpemb_h' if mode else 'fp32-mfma', regime, dict(MLPEMB=err))
    na.compare_node(regime, dict(MLPEMB=got), dict(MLPEMB=ref))
    assert torch.equal(Yi, _mlp_launch(env, mode, variant, x, k0, rows)[1].view(torch.int32)), f'{what}: a second launch gave other bits'


@pytest.mark.parametrize('rows', na.MLP_ROW_COUNTS)
@pytest.mark.parametrize('k0', na.MLP_K0)
@pytest.mark.parametrize('regime', na.MLP_REGIMES)
@pytest.mark.parametrize('variant', na.MLP_VARIANTS)
@pytest.mark.parametrize('mode', [1, 0], ids=['k_mlpemb_h', 'fp32-mfma'])
def test_mlp_embedding(env, mode, variant, regime, k0, rows):
    """MLPEmbedding of K0 = 128 .. 512 inputs with ldx > K0 and ldy > 128: NaN in the columns behind the inputs (never read), the
    canary in the columns behind the outputs and in the guard rows (never written)"""
    _mlp_check(env, mode, variant, regime, k0, rows, na.MLP_ROWS)


def test_mlp_embedding_persistent_tiles(env):
    """k_mlpemb_h at 32,768 + 69 rows: two workgroups take a second tile of the one weight stream"""
    _mlp_check(env, 1, 'plain', 'A', 512, na.MLP_PERSISTENT_ROWS, na.CYCLE_ROWS)
