"""Operator-level tests of infgen_decode_layers through k_layers_p (csrc/layers_p.hip: the 18 sublayers of a decode step in one
launch) against the plain float64 reference of tests/layers_stack_ref.py, never against another kernel; the per-sublayer launches
(layers_p = 0) run through the same checks as the control.

A context is built by engine.RolloutEngine + prologue(); then X, the temporal ring and the map K / V rows are overwritten with the
values of an input regime (layers_stack_ref.gen_values: copies of a base scene get copies of the values) and
infgen_decode_layers(ctx, 1, 0) runs the first decode column.  The three edge sets and their rhat rows are read back and are INPUTS
of the reference (the edge builder and the Fourier kernel have operator tests of their own).  Observables, all present without tap_x:
X, ring slot c % ring of the six layers, the agent-set K / V rows of the last two layers (k_layers_p double-buffers them by layer
parity: layer 4 in Ka / Va, layer 5 in the first 2 * rows * 128 floats of U; the per-sublayer launches keep ONE buffer, so the
control and the fallback are compared on layer 5's rows in Ka / Va only).  Every case: row errors within layers_stack_ref.bar
(four times the float32 evaluation's error, per output and regime), every value finite, every copy of a base scene bit-equal to
it (row0, the tile order and the scene counters leak nothing between scenes), a second call on restored inputs bit-equal, the
other ring slots, the map rows and the edge lists unchanged, and the launch counts of the profiler proving which path ran.  Rows
beyond a scene's agents are edgeless rows of the same operator and are compared like the rest.  Shapes follow layers_p_launch's rule
from infgen_layers_p_capacity(); no INFGEN_LP_* variable is set.  The 32-row scenes have agent lists of at most 31 edges, so the odd
count >= 33 of the degree coverage is asserted on the 64-row case of ROWS = 4.  The largest device error / bar per output, regime
and path is printed at the end of the module and written as JSON to the file INFGEN_LAYERS_STACK_RECORD names, if it is set."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import edge_attn_ref as ea
import layers_stack_ref as ls
import node_attn_ref as na

pytestmark = pytest.mark.gpu

COL = 1                                  # the first decode column
D = 128
# (scenes, seed, half_extent) of the base scenes per row capacity: agents / map tokens are layers_stack_ref.BASE_SCENES
SCENE_SEEDS = {32: ((7301, 60.0), (7302, 40.0), (7303, 60.0), (7304, 150.0)), 64: ((7401, 20.0), (7402, 45.0), (7403, 60.0), (7404, 120.0))}
SHAPES_32 = [2, 8, 16, 17, 64, 65, 128, 129, 256, 257]
SHAPES_64 = [4, 9, 33]


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
    from infgen_amd import _lib, synth
    assert torch.cuda.is_available(), 'these tests need the GPU box'
    cfg = synth.standard_config()
    e = dict(lib=_lib.load(), dev=torch.device('cuda:0'), cfg=cfg, vocab=synth.make_agent_vocab(cfg.token_size),
             map_vocab=synth.make_map_vocab(), grid=synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius),
             weights={}, engines={}, values={}, refs={}, ratios={}, rows_seen=set())
    e['cap'] = e['lib'].infgen_layers_p_capacity()
    assert e['cap'] > 0, 'k_layers_p would never run on this device'
    yield e
    for k, (r, err, b) in sorted(e['ratios'].items()):
        print(f'layers stack worst {k}: error {err:.3g} / bar {b:.3g} = {r:.2f}')
    if os.environ.get('INFGEN_LAYERS_STACK_RECORD'):
        with open(os.environ['INFGEN_LAYERS_STACK_RECORD'], 'w') as f:
            json.dump({k: dict(ratio=r, error=err, bar=b) for k, (r, err, b) in e['ratios'].items()}, f, indent=1, sort_keys=True)
            f.write('\n')


def expected_launch(S, a_cap, cap):
    """layers_p_launch's rule (csrc/api.hip) -> (rows per workgroup, launches); (0, 0): the batch takes the per-sublayer launches"""
    limit, rows, gps16 = min(cap, 256), S * a_cap, a_cap // 16
    if gps16 > limit or -(-S // (limit // gps16)) > 2:
        return 0, 0
    rpw = 16
    for rr in (8, 4):
        if a_cap % rr == 0 and rows // rr <= (limit // 2 if rr == 4 else limit):
            rpw = rr
    return rpw, 1 if rows // rpw <= limit else -(-S // (limit // gps16))


def _weights(env, variant):
    """PackedWeights of a variant: only the 18 attention packs differ from the plain pack, the rest is shared"""
    from infgen_amd import engine, packing
    if 'plain' not in env['weights']:
        env['weights']['plain'] = engine.PackedWeights(ls.weights('plain'), env['cfg'], env['dev'])
    if variant not in env['weights']:
        w = copy.copy(env['weights']['plain'])
        sd = ls.weights(variant)
        put = lambda kind: [torch.from_numpy(np.ascontiguousarray(packing.pack_attention_layer(sd, ls.prefix(i, kind)), np.float32)).to(env['dev'])
                            for i in range(ls.L)]
        w.attn_t, w.attn_m, w.attn_a, w.sd = put('t'), put('m'), put('a'), sd
        env['weights'][variant] = w
    return env['weights'][variant]


def _scenes(env, a_cap):
    from infgen_amd import synth
    return [synth.make_scene(seed, n, m, env['cfg'], half_extent=ext, ego_last=(k % 2 == 0), vocab=env['vocab'], grid=env['grid'], slip=0.3)
            for k, ((seed, ext), (n, m)) in enumerate(zip(SCENE_SEEDS[a_cap], ls.BASE_SCENES[a_cap]))]


def _engine(env, S, a_cap):
    from infgen_amd import engine
    if (S, a_cap) not in env['engines']:
        base = _scenes(env, a_cap)
        with _gpu_call():
            e = engine.RolloutEngine(_weights(env, 'plain'), [base[s % len(base)] for s in range(S)], env['vocab'], env['map_vocab'],
                                     env['grid'], a_cap=a_cap, store_logits=False, use_graph=False, options=dict(layers_p=1))
            e.prologue()
            torch.cuda.synchronize()
        assert (e.A_cap, e.M_cap, e.ring, e.rows) == (a_cap, ls.M_CAP, ls.RING, S * a_cap)
        assert [h['A'] for h in e.hosts[:len(base)]] == [n for n, _ in ls.BASE_SCENES[a_cap]][:S]
        e._variant = 'plain'
        env['engines'] = {(S, a_cap): e}                 # one engine at a time: the large batches hold hundreds of MB
    return env['engines'][S, a_cap]


def _values(env, regime, a_cap):
    if (regime, a_cap) not in env['values']:
        env['values'][regime, a_cap] = tuple(torch.from_numpy(np.array(a)).to(env['dev']) for a in ls.gen_values(regime, a_cap))
    return env['values'][regime, a_cap]


def _fill(env, e, regime):
    """X, ring and map rows of the context <- the regime's values, scene s taking base scene s % nb's"""
    X, rk, rv, mk, mv = _values(env, regime, e.A_cap)
    nb = len(ls.BASE_SCENES[e.A_cap])
    idx = torch.arange(e.S, device=env['dev']) % nb
    e.X.copy_(X.view(nb, e.A_cap, D)[idx].reshape(e.rows, D))
    for i in range(ls.L):
        e.ringK[i].copy_(rk[i].view(ls.RING, nb, e.A_cap, D)[:, idx].reshape(ls.RING, e.rows, D))
        e.ringV[i].copy_(rv[i].view(ls.RING, nb, e.A_cap, D)[:, idx].reshape(ls.RING, e.rows, D))
        e.mapK[i].copy_(mk[i].view(nb, ls.M_CAP, D)[idx].reshape(e.S * ls.M_CAP, D))
        e.mapV[i].copy_(mv[i].view(nb, ls.M_CAP, D)[idx].reshape(e.S * ls.M_CAP, D))
    for t in (e.Ka, e.Va, e.U):
        t.fill_(float('nan'))                            # (outputs of the call, or scratch it must overwrite before reading)


def _call(env, e, col, edgeless):
    """one infgen_decode_layers under the profiler -> {kernel: launches}"""
    from infgen_amd import _lib
    with _gpu_call():
        _lib.prof_enable((1 << len(_lib.KERNEL_IDS)) - 1)
        try:
            _lib.check(env['lib'].infgen_decode_layers(C.byref(e._ctx), col, edgeless, e.ops.stream), 'infgen_decode_layers')
            torch.cuda.synchronize()
            counts = _lib.prof_collect()
        finally:
            _lib.prof_enable(0)
    return {k: v['calls'] for k, v in counts.items()}


def _observe(e, col, lp):
    """device tensors of the observables: X, ring slot col % ring of the six layers, the agent-set K / V rows (see the module docstring)"""
    slot, n = col % e.ring, e.rows * D
    obs = dict(X=e.X.clone()[None], RK=torch.stack([e.ringK[i][slot] for i in range(ls.L)]), RV=torch.stack([e.ringV[i][slot] for i in range(ls.L)]))
    if lp:
        u = e.U.view(-1)
        obs['KA'] = torch.stack([e.Ka, u[:n].view(e.rows, D)])
        obs['VA'] = torch.stack([e.Va, u[n:2 * n].view(e.rows, D)])
    else:
        obs['KA'], obs['VA'] = e.Ka.clone()[None], e.Va.clone()[None]
    return obs


def _untouched(e, col):
    slot = col % e.ring
    keep = [s for s in range(e.ring) if s != slot]
    return [t[keep].clone() for t in e.ringK + e.ringV] + [t.clone() for t in e.mapK + e.mapV]


def _lists(e, r24=0):
    """the three sets as the kernels read them: counts, and the sources / rhat rows of every list in row order (the offsets are the
    builder's allocation and may differ from call to call; entries no list names are not part of the sets)"""
    out = []
    for k in ls.KINDS:
        ed = e.edges[k]
        off, cnt = ed['off'].long(), ed['cnt'].long()
        start = torch.cumsum(cnt, 0) - cnt
        idx = torch.repeat_interleave(off - start, cnt) + torch.arange(int(cnt.sum()), device=cnt.device)
        w = ea.R24_ROW_BYTES // 4 if r24 else D                      # int32 words per rhat row (packed rows: 384 bytes)
        out += [ed['cnt'].clone(), ed['src'][idx], ed['rhat'].view(torch.int32).view(-1)[:ed['cap'] * w].view(ed['cap'], w)[idx]]
    return out


def _base_edges(e, r24):
    """the three edge sets of the base block read back as compact lists with sources renumbered to the block: temporal
    slot * rows + row -> slot * block rows + row, map scene * M_cap + token and agent scene * A_cap + agent as they are (the block
    is the first scenes); every list must name rows of its own scene only"""
    nb = min(len(ls.BASE_SCENES[e.A_cap]), e.S)
    br = nb * e.A_cap
    out = {}
    for kind in ls.KINDS:
        ed = e.edges[kind]
        off, cnt = ed['off'][:br].cpu().numpy().astype(np.int64), ed['cnt'][:br].cpu().numpy().astype(np.int64)
        idx = np.concatenate([np.arange(o, o + c) for o, c in zip(off, cnt)] + [np.zeros(0, np.int64)])
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < ed['cap'])
        ti = torch.from_numpy(idx).to(ed['src'].device)
        src = ed['src'][ti].cpu().numpy().astype(np.int64)
        if r24:
            rh = ea.unpack_r24(ed['rhat'].view(torch.uint8).view(-1)[:ed['cap'] * ea.R24_ROW_BYTES].view(ed['cap'], ea.R24_ROW_BYTES)[ti].cpu().numpy())
        else:
            rh = ed['rhat'][ti].cpu().numpy()
        dst = np.repeat(np.arange(br), cnt)
        if kind == 't':
            assert np.array_equal(src % e.rows, dst) and (src // e.rows != COL % e.ring).all()
            src = (src // e.rows) * br + src % e.rows
        elif kind == 'm':
            assert np.array_equal(src // e.M_cap, dst // e.A_cap)
        else:
            assert np.array_equal(src // e.A_cap, dst // e.A_cap)
        noff = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
        out[kind] = (noff, cnt, src, rh.reshape(-1, D) if idx.size else None)
    return out


def _reference(env, variant, regime, a_cap, edges, key, **kw):
    k = (variant, regime, a_cap, key)
    if k not in env['refs']:
        env['refs'][k] = ls.flatten(ls.run(variant, regime, a_cap, edges=edges, **kw))
    return env['refs'][k]


def _note(env, what, regime, errs):
    for o, err in errs.items():
        k = f'{what} {o} {regime}'
        r = err / ls.bar(o, regime)
        if r >= env['ratios'].get(k, (-1.0,))[0]:
            env['ratios'][k] = (r, err, ls.bar(o, regime))


def _check(env, S, a_cap, variant, regime, mode=1, edgeless=0, rhat_format=0):
    """the checks of one case -> the first call's observables (device tensors)"""
    from infgen_amd import _lib
    e = _engine(env, S, a_cap)
    what = f'layers_p={mode} S={S} A_cap={a_cap} {variant} regime {regime}' + (' edgeless' if edgeless else '') + (' r24' if rhat_format else '')
    if e._variant != variant:
        e.w = _weights(env, variant)
        e._build_ctx()
        e._variant = variant
    e.options = dict(layers_p=mode, rhat_format=rhat_format)
    e._refresh_opts()
    col = 0 if edgeless else COL
    rpw, launches = expected_launch(S, a_cap, env['cap'])
    lp = mode != 0 and rpw != 0
    nb = min(len(ls.BASE_SCENES[a_cap]), S)          # (S = 2: the first two base scenes are the block)
    br = nb * a_cap

    _fill(env, e, regime)
    keep = _untouched(e, col)
    counts = _call(env, e, col, edgeless)
    obs = _observe(e, col, lp)
    # ---- which path ran
    if lp:
        assert counts['k_edge_attn'] == launches and counts['k_attn_post'] == 0 and counts['k_attn_pre'] == 0, (what, counts)
        env['rows_seen'].add(rpw)
    elif not edgeless:
        assert counts['k_edge_attn'] == 18 and counts['k_attn_post'] == 18, (what, counts)
    # ---- nothing else written, nothing but finite values, copies bit-equal to their base scene
    for a, b in zip(keep, _untouched(e, col)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: a ring slot or a map row the call must not touch changed'
    for o, t in obs.items():
        assert bool(torch.isfinite(t).all()), f'{what}: {o} holds a value that is not finite'
        v = t.view(t.shape[0], S, a_cap, D).view(torch.int32)
        if S > nb:
            idx = torch.arange(nb, S, device=t.device) % nb
            assert torch.equal(v[:, nb:], v[:, idx]), f'{what}: {o} of a copy differs from its base scene'
    # ---- the reference on the base block, fed the device's own lists
    if edgeless:
        for k in ls.KINDS:
            assert int(e.edges[k]['cnt'].abs().sum()) == 0
        ref = _reference(env, variant, regime, a_cap, None, ('edgeless', nb), edgeless=True, slot=0, scenes=nb)
    else:
        ekey = ('edges', S, a_cap, rhat_format)
        if ekey not in env['refs']:
            env['refs'][ekey] = _base_edges(e, rhat_format)
        edges = env['refs'][ekey]
        first = env['refs'].setdefault(('edges0', a_cap, rhat_format, nb), edges)          # the same lists at every batch size
        for k in ls.KINDS:
            assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(edges[k][:3], first[k][:3])), (what, k)
            if not rhat_format and edges[k][3] is not None:
                assert np.array_equal(edges[k][3].view(np.int32), first[k][3].view(np.int32)), (what, k)
        ref = _reference(env, variant, regime, a_cap, first, ('lists', rhat_format, nb), scenes=nb)
    got = {o: t.view(t.shape[0], S, a_cap, D)[:, :nb].reshape(-1, D).cpu().numpy() for o, t in obs.items()}
    if not lp:                                         # one K / V buffer: layer 5's rows
        ref = dict(ref, KA=ref['KA'][br:], VA=ref['VA'][br:])
    errs = {o: na.row_error(got[o], ref[o]) for o in ref}
    path = f'k_layers_p ROWS={rpw}' if lp else 'per-sublayer'
    print(f'{what} [{path}]: device errors ' + ' '.join(f'{o} {errs[o]:.3g} (bar {ls.bar(o, regime):.3g})' for o in ref))
    _note(env, path + (' r24' if rhat_format else ''), regime, errs)
    ls.compare_stack(regime, got, ref)
    # ---- a second call on restored inputs repeats every bit, and rebuilds the same lists
    lists = None if edgeless else _lists(e, rhat_format)
    _fill(env, e, regime)
    _call(env, e, col, edgeless)
    again = _observe(e, col, lp)
    for o in obs:
        assert torch.equal(obs[o].view(torch.int32), again[o].view(torch.int32)), f'{what}: {o} of a second call has other bits'
    if lists is not None:
        for a, b in zip(lists, _lists(e, rhat_format)):
            assert torch.equal(a, b), f'{what}: an edge list changed between two calls'
    return obs, e


def _degrees(e, a_cap):
    nb = min(len(ls.BASE_SCENES[a_cap]), e.S)
    return np.concatenate([e.edges[k]['cnt'][:nb * a_cap].cpu().numpy() for k in ls.KINDS])


def test_case_list_covers_every_variant_of_the_launch(env):
    """the expected rows per workgroup of every shape below, from the capacity of this device (256 on the full device)"""
    cap = env['cap']
    got32 = [expected_launch(S, 32, cap) for S in SHAPES_32]
    got64 = [expected_launch(S, 64, cap) for S in SHAPES_64]
    assert {r for r, _ in got32} == {0, 4, 8, 16} and 2 in {n for _, n in got32}, got32
    assert {r for r, _ in got64} == {4, 8, 16}, got64
    if cap == 256:
        assert got32 == [(4, 1), (4, 1), (4, 1), (8, 1), (8, 1), (16, 1), (16, 1), (16, 2), (16, 2), (0, 0)]
        assert got64 == [(4, 1), (8, 1), (16, 1)]


@pytest.mark.parametrize('regime', ls.REGIMES)
@pytest.mark.parametrize('variant', ls.VARIANTS)
@pytest.mark.parametrize('S', [2, 17])
def test_layers_p_variants_and_regimes(env, S, variant, regime):
    """every weight variant and input regime through ROWS = 4 (S = 2: 16 workgroups, lists halved between two waves) and ROWS = 8
    (S = 17); under ROWS = 4 the lists read back hold 0, 1, 2 and 3 edges: an empty half, a half of one, unequal halves.  The first
    two base scenes - the whole batch at S = 2 - hold the scene of one agent and the degenerate rows of regime C"""
    _, e = _check(env, S, 32, variant, regime)
    if expected_launch(S, 32, env['cap'])[0] == 4:
        assert {0, 1, 2, 3} <= set(_degrees(e, 32)), sorted(set(_degrees(e, 32)))


@pytest.mark.parametrize('variant', ['scales_a', 'ln_peaked'])
@pytest.mark.parametrize('S', SHAPES_32)
def test_layers_p_shapes(env, S, variant):
    """both sides of every switch of the launch rule: the last / first sizes of ROWS = 4, 8 and 16, the tile order on and off, two
    chunks (the second with one scene at row0 = 4096, and full), and the first size that takes the per-sublayer launches"""
    _check(env, S, 32, variant, 'A')


@pytest.mark.parametrize('variant', ['scales_a', 'ln_peaked'])
@pytest.mark.parametrize('S', SHAPES_64)
def test_layers_p_scenes_of_64_agents(env, S, variant):
    """four workgroups per scene and agent lists of up to 63 edges: under ROWS = 4 an odd count >= 33 (halves of 32 and 31)"""
    _, e = _check(env, S, 64, variant, 'A')
    deg = _degrees(e, 64)
    assert deg.max() == 63
    if expected_launch(S, 64, env['cap'])[0] == 4:
        assert any(d >= 33 and d % 2 for d in deg) and {0, 1, 2, 3} <= set(deg), sorted(set(deg))


@pytest.mark.parametrize('regime', ls.REGIMES)
@pytest.mark.parametrize('variant', ls.VARIANTS)
@pytest.mark.parametrize('S', [2, 17, 65])
def test_per_sublayer_control(env, S, variant, regime):
    """the per-sublayer launches (unfused edge kernels at 64 rows, k_edge_fused + k_attn_hs above 256) judged by the same bars"""
    _check(env, S, 32, variant, regime, mode=0)


@pytest.mark.parametrize('variant', ls.VARIANTS)
@pytest.mark.parametrize('S', [2, 65])
def test_layers_p_edgeless_column(env, S, variant):
    """the edgeless column-0 chain of the prologue: every list empty, ring slot 0 written"""
    _check(env, S, 32, variant, 'A', edgeless=1)


HIP_ATTR_COOPERATIVE_LAUNCH, HIP_ATTR_MULTIPROCESSOR_COUNT = 10, 63      # hipDeviceAttribute_t (hip_runtime_api.h, ROCm 6 / 7)


def _device_reports_cooperative_launch(env):
    """hipDeviceAttributeCooperativeLaunch of device 0, asked of the HIP runtime this process has mapped - what lp_device() reads;
    the enum values are checked against the one attribute torch also reports"""
    hip = C.CDLL('libamdhip64.so')
    v = C.c_int(-1)
    assert hip.hipDeviceGetAttribute(C.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0
    assert v.value == torch.cuda.get_device_properties(0).multi_processor_count, 'hipDeviceAttribute_t differs from the values above'
    assert hip.hipDeviceGetAttribute(C.byref(v), HIP_ATTR_COOPERATIVE_LAUNCH, 0) == 0
    return bool(v.value)


@pytest.mark.parametrize('S', [2, 65])
def test_cooperative_launch_is_bitwise_the_plain_launch(env, S):
    """layers_p = 2: the same kernel through hipLaunchCooperativeKernel; on a device that reports cooperative launch a fall-back to
    the per-sublayer launches (a refused launch) is a failure"""
    if not _device_reports_cooperative_launch(env):
        pytest.skip('the device reports no cooperative launch')
    e = _engine(env, S, 32)
    e.w, e._variant = _weights(env, 'scales_a'), 'scales_a'
    e._build_ctx()
    e.options = dict(layers_p=2)
    e._refresh_opts()
    _fill(env, e, 'A')
    counts = _call(env, e, COL, 0)
    assert counts['k_edge_attn'] == expected_launch(S, 32, env['cap'])[1] and counts['k_attn_post'] == 0 and counts['k_attn_pre'] == 0, counts
    coop = _observe(e, COL, True)
    plain, _ = _check(env, S, 32, 'scales_a', 'A', mode=1)
    for o in plain:
        assert torch.equal(plain[o].view(torch.int32), coop[o].view(torch.int32)), o


@pytest.mark.parametrize('S', [2, 17, 65])
def test_layers_p_packed_rhat_rows(env, S):
    """rhat_format = 1: k_layers_p<true, .> on packed 24-bit rows; the reference consumes edge_attn_ref.unpack_r24 of the rows read
    back (their rounding belongs to the inputs), the bars are the fp32 bars"""
    _check(env, S, 32, 'scales_a', 'A', rhat_format=1)


def test_every_row_variant_was_launched(env):
    """ROWS = 4, 8 and 16 each through the profiled one-launch path (the three sizes here, next to whatever ran before)"""
    for S in (2, 17, 65):
        _check(env, S, 32, 'scales_b', 'C')
    assert env['rows_seen'] >= ({4, 8, 16} if env['cap'] == 256 else {16}), env['rows_seen']
