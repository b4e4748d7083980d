"""CPU: the ABI, field layout and switches of top-k sampling inside the split heads kernel (infgen_heads_sample,
InfgenRollout.sample_logprob, RolloutEngine(sample_logprob=True), InfGenDecoder.sample_logprob)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_struct_carries_sample_logprob():
    """the new pointer is the newest member the struct may hold: three older members' places at the end are pinned by older tests
    (token_logprob, then the two ablation switches), so it sits directly in front of them; library and binding agree on the size"""
    from infgen_amd import _lib
    names = [f[0] for f in _lib.Rollout._fields_]
    assert names[-4:] == ['sample_logprob', 'token_logprob', 'no_grid_token', 'no_state_token']
    assert dict(_lib.Rollout._fields_)['sample_logprob'] is _lib._p
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT) == _lib.C.sizeof(_lib.Rollout)
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    body = hdr[hdr.index('typedef struct InfgenRollout'):hdr.index('} InfgenRollout;')]
    assert body.index('float* sample_logprob;') < body.index('float* token_logprob;') < body.index('int no_grid_token;')


def test_new_entries_are_declared_and_exported():
    from infgen_amd import _lib
    lib = _lib.load()
    _i, _p = _lib._i, _lib._p
    assert _lib.SYMBOLS['infgen_heads_sample'] == (_i, [_p, _i, _p, _p, _i, _i, _p, _p, _p, _p, _p, _p, _p])
    assert _lib.SYMBOLS['infgen_sample_topk_logprob'] == (_i, [_p, _i, _i, _i, _p, _p, _p, _p])
    assert _lib.SYMBOLS['infgen_heads_sample_fused'] == (_i, [_i, _i, _i])
    for sym in ('infgen_heads_sample', 'infgen_sample_topk_logprob', 'infgen_heads_sample_fused', 'infgen_sample_topk'):
        assert hasattr(lib, sym)
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    assert re.search(r'int infgen_heads_sample\(const float\* X, int rows, const float\* tok_pack, const float\* st_pack, '
                     r'int token_size, int k,\s+const float\* uniform, float\* logits, int\* next_token, int\* next_state, '
                     r'float\* token_logprob,\s+float\* sample_logprob, void\* stream\);', hdr)


def test_by_size_rule_is_one_library_query():
    """infgen_heads_sample_fused: the split kernel (attn_mode 1, or >= 2 beyond the row threshold) and 2 <= k <= the kernel's width"""
    from infgen_amd import _lib
    lib = _lib.load()
    ks, split = lib.infgen_layout_query(_lib.Q_HEADS_SAMPLE_K), lib.infgen_layout_query(_lib.Q_ATTN_SPLIT_ROWS)
    assert ks in (8, 16)
    f = lib.infgen_heads_sample_fused
    assert [f(1, 16, k) for k in (1, 2, 5, ks, ks + 1)] == [0, 1, 1, 1, 0]
    assert f(0, 10 ** 6, 5) == 0
    assert f(2, split, 5) == 0 and f(2, split + 1, 5) == 1
    # the engine asks the library and does not restate the threshold for sampled rollouts
    from infgen_amd import engine
    assert 'infgen_heads_sample_fused' in inspect.getsource(engine.RolloutEngine._refresh_opts)
    # ... nor for greedy rollouts with token_logprob: the same rule without the beam
    g = lib.infgen_heads_logprob_fused
    assert [g(0, 10 ** 6), g(1, 16), g(2, split), g(2, split + 1)] == [0, 1, 0, 1]
    assert 'Q_ATTN_SPLIT_ROWS' not in inspect.getsource(engine.RolloutEngine._refresh_opts)


def test_torch_op_is_declared():
    import torch
    from infgen_amd import torch_ops  # noqa: F401
    op = torch.ops.infgen_hip.heads_sample
    schema = str(op.default._schema)
    for arg in ('Tensor x', 'Tensor tok_pack', 'Tensor st_pack', ' token_size', ' k,', 'Tensor uniform', 'bool want_logits',
                'bool want_logprob', 'bool want_sample_logprob'):
        assert arg in schema, (arg, schema)
    assert schema.count('Tensor') >= 9           # four inputs, five outputs
    x = torch.empty(7, 128, device='meta')
    out = op(x, torch.empty(1, device='meta'), torch.empty(1, device='meta'), 2048, 5, torch.empty(7, device='meta'), True, False, True)
    assert [tuple(t.shape) for t in out] == [(7,), (7,), (7, 2048), (0,), (7,)]
    assert out[0].dtype == torch.int32 and out[4].dtype == torch.float32


def test_engine_and_decoder_accept_the_flag():
    from infgen_amd import engine
    from infgen_amd.modules.infgen_decoder import InfGenDecoder
    p = inspect.signature(engine.RolloutEngine.__init__).parameters
    assert p['sample_logprob'].default is False
    assert hasattr(engine.RolloutEngine, 'rollout_sample_logprob')
    src = inspect.getsource(InfGenDecoder.__init__)
    assert 'self.sample_logprob = False' in src
    from infgen_amd.model import infgen
    assert 'rollout_sample_logprob' in inspect.getsource(infgen.InfGen.validation_step)


# ---- the refusals of the emission entries that need no device: every call returns before any launch, so the pointers are plain
# numbers (never dereferenced).  The expected texts were recorded from the library as it stood BEFORE these entries were moved onto
# one plan and one executor (EmitReq / emit_plan / emit_tokens in api.hip), and are literals on purpose: text, "<entry>: " prefix
# and the order of adjacent checks are part of the entries' behaviour.
_P, _ODD = 4096, 4100            # a 16-byte aligned "device pointer" and one that is not
_M128 = b'token_size must be a multiple of 128'             # (always under infgen_heads' name: the heads stage reports as that entry)
_K_RANGE, _K_N, _K_TS = b'k must be in 1..16', b'k must not exceed n', b'k must not exceed token_size'
_NO_U = b'uniform is NULL'
_LG_HEADS = b'this row count takes k_heads: it needs a logits buffer [rows][token_size]'
_LG_TOPK = b'this row count or beam takes k_sample_topk: it needs a logits buffer [rows][token_size]'
_TEMP = b'temperature must be finite and >= 0 (0: unset, i.e. 1)'
_DENORM = b'temperature is a denormal: 1 / T overflows'
_TOP_P = b'top_p must be in (0, 1] (0: unset, i.e. 1)'
_N_SETS = b'token mask: n_sets must be >= 0'
_TYPES = b"token mask: a per-type set needs the rows' types"
_M32 = b'token mask: token_size must be a multiple of 32'
_ALIGN = b'token mask: the table must be 16-byte aligned'


def _sampling(temperature=0.0, top_p=0.0):
    from infgen_amd import _lib
    return _lib.Sampling(temperature, top_p, None)


def _heads(ts=128, rows=16):
    return ('infgen_heads', (_P, rows, _P, _P, ts, _P, _P, _P, None))


def _heads_lp(ts=128, logits=_P, lp=_P, rows=16):
    return ('infgen_heads_logprob', (_P, rows, _P, _P, ts, logits, _P, _P, lp, None))


def _hs(entry, k=5, ts=128, u=_P, logits=_P, lp=None, sampling=None, mask=(None, 0, None, None, None), rows=16):
    """one call of infgen_heads_sample / _ex / _mask (sample_logprob stays NULL: with k == 1 it is zeroed on the device)"""
    head = (_P, rows, _P, _P, ts, k, u)
    tail = (logits, _P, _P, lp, None, None)
    if entry == 'infgen_heads_sample':
        return (entry, head + tail)
    if entry == 'infgen_heads_sample_ex':
        return (entry, head + (sampling,) + tail)
    return (entry, head + (sampling,) + tuple(mask) + tail)


def _topk(entry, n=128, k=5, sampling=None, mask=(None, 0, None, None, None), rows=16):
    head = (_P, rows, n, k, _P)
    if entry == 'infgen_sample_topk':
        return (entry, head + (_P, None))
    if entry == 'infgen_sample_topk_logprob':
        return (entry, head + (_P, None, None))
    if entry == 'infgen_sample_topk_ex':
        return (entry, head + (sampling, _P, None, None, None))
    return (entry, head + (sampling,) + tuple(mask) + (_P, None, None, None))


_BY_TYPE = (0, -1, -1)           # mask_type: vehicles take set 0 (read on the host)
_ROWSEL = (_P, 2, _P, None, None)                  # an active mask: a table and per-row selectors
_IDLE = (_P, 2, None, None, None)                  # a table no row can select: inactive
_HS3 = ('infgen_heads_sample', 'infgen_heads_sample_ex', 'infgen_heads_sample_mask')
_TK4 = ('infgen_sample_topk', 'infgen_sample_topk_logprob', 'infgen_sample_topk_ex', 'infgen_sample_topk_mask')
_EX, _MK, _TEX, _TMK = _HS3[1], _HS3[2], _TK4[2], _TK4[3]


def _refusals():
    """(id, attn_mode, (entry, args), prefix or None for the entry's own, text)"""
    t = []
    # infgen_heads: its one check, on either route (attn_mode 1: the split kernel for any row count; 2: k_heads at 16 rows)
    t += [(f'heads-ts100-m{m}', m, _heads(ts=100), 'infgen_heads', _M128) for m in (1, 2)]
    # infgen_heads_logprob
    lp = b'token_logprob is NULL (infgen_heads is the entry without it)'
    t += [('lp-null', 2, _heads_lp(lp=None), None, lp),
          ('lp-null+no-logits+ts100', 2, _heads_lp(lp=None, logits=None, ts=100), None, lp),
          ('lp-no-logits', 2, _heads_lp(logits=None), None, _LG_HEADS),
          ('lp-no-logits+ts100', 2, _heads_lp(logits=None, ts=100), None, _LG_HEADS),
          ('lp-ts100', 2, _heads_lp(ts=100), 'infgen_heads', _M128),
          ('lp-split-no-logits+ts100', 1, _heads_lp(logits=None, ts=100), 'infgen_heads', _M128)]
    # the three infgen_heads_sample*: what they share
    for e in _HS3:
        s = e[len('infgen_heads_'):]
        t += [(f'{s}-k0', 2, _hs(e, k=0), None, _K_RANGE),
              (f'{s}-k17', 2, _hs(e, k=17), None, _K_RANGE),
              (f'{s}-k17+ts8', 2, _hs(e, k=17, ts=8), None, _K_RANGE),
              (f'{s}-k9-ts8', 2, _hs(e, k=9, ts=8), None, _K_TS),
              (f'{s}-k9-ts8+no-u', 2, _hs(e, k=9, ts=8, u=None), None, _K_TS),
              (f'{s}-no-u', 2, _hs(e, u=None), None, _NO_U),
              (f'{s}-k1-no-u', 2, _hs(e, k=1, u=None), None, _NO_U),
              (f'{s}-no-u+no-logits', 2, _hs(e, u=None, logits=None), None, _NO_U),
              (f'{s}-no-logits', 2, _hs(e, logits=None), None, _LG_TOPK),
              (f'{s}-no-logits+ts100', 2, _hs(e, logits=None, ts=100), None, _LG_TOPK),
              (f'{s}-ts100', 2, _hs(e, ts=100), 'infgen_heads', _M128),
              (f'{s}-split-no-logits+ts100', 1, _hs(e, logits=None, ts=100), 'infgen_heads', _M128),
              (f'{s}-k1-ts100', 2, _hs(e, k=1, ts=100), 'infgen_heads', _M128),
              (f'{s}-k1-lp-no-logits', 2, _hs(e, k=1, lp=_P, logits=None), 'infgen_heads_logprob', _LG_HEADS),
              (f'{s}-k1-lp-no-logits+ts100', 2, _hs(e, k=1, lp=_P, logits=None, ts=100), 'infgen_heads_logprob', _LG_HEADS),
              (f'{s}-k1-lp-ts100', 2, _hs(e, k=1, lp=_P, ts=100), 'infgen_heads', _M128),
              (f'{s}-k1-lp-split-no-logits+ts100', 1, _hs(e, k=1, lp=_P, logits=None, ts=100), 'infgen_heads', _M128)]
    # ... the sampling parameters (_ex and _mask): after k and uniform, before the route; ignored by the arg-max
    for e in (_EX, _MK):
        s = e[len('infgen_heads_'):]
        t += [(f'{s}-temp', 2, _hs(e, sampling=_sampling(-1.0)), None, _TEMP),
              (f'{s}-nan', 2, _hs(e, sampling=_sampling(float('nan'))), None, _TEMP),
              (f'{s}-temp+top-p', 2, _hs(e, sampling=_sampling(-1.0, 2.0)), None, _TEMP),
              (f'{s}-denormal+top-p', 2, _hs(e, sampling=_sampling(1e-40, 2.0)), None, _DENORM),
              (f'{s}-top-p', 2, _hs(e, sampling=_sampling(1.0, 2.0)), None, _TOP_P),
              (f'{s}-no-u+temp', 2, _hs(e, u=None, sampling=_sampling(-1.0)), None, _NO_U),
              (f'{s}-top-p+no-logits', 2, _hs(e, logits=None, sampling=_sampling(1.0, 2.0)), None, _TOP_P),
              (f'{s}-k1-temp-ignored', 2, _hs(e, k=1, ts=100, sampling=_sampling(-1.0)), 'infgen_heads', _M128)]
    # ... the mask (_mask): n_sets < 0 before everything, the rest after uniform and before the sampling parameters
    t += [('mask-n-sets+rows0+k17', 2, _hs(_MK, k=17, rows=0, mask=(_P, -1, _P, None, None)), None, _N_SETS),
          ('mask-n-sets-no-table', 2, _hs(_MK, mask=(None, -1, None, None, None)), None, _N_SETS),
          ('mask-no-table-k0', 2, _hs(_MK, k=0, mask=(None, 2, _P, None, None)), None, _K_RANGE),
          ('mask-no-table-k1-no-u', 2, _hs(_MK, k=1, u=None, mask=(None, 2, _P, None, None)), None, _NO_U),
          ('mask-no-u+types', 2, _hs(_MK, u=None, mask=(_P, 2, None, _BY_TYPE, None)), None, _NO_U),
          ('mask-types', 2, _hs(_MK, mask=(_P, 2, None, _BY_TYPE, None)), None, _TYPES),
          ('mask-types+ts48', 2, _hs(_MK, ts=48, mask=(_P, 2, None, _BY_TYPE, None)), None, _TYPES),
          ('mask-ts48', 2, _hs(_MK, ts=48, mask=_ROWSEL), None, _M32),
          ('mask-ts48+odd', 2, _hs(_MK, ts=48, mask=(_ODD, 2, _P, None, None)), None, _M32),
          ('mask-odd', 2, _hs(_MK, mask=(_ODD, 2, _P, None, None)), None, _ALIGN),
          ('mask-odd+temp', 2, _hs(_MK, mask=(_ODD, 2, _P, None, None), sampling=_sampling(-1.0)), None, _ALIGN),
          ('mask-k0-is-argmax-ts64', 2, _hs(_MK, k=0, u=None, ts=64, mask=_ROWSEL), 'infgen_heads', _M128),
          ('mask-k1-lp-no-logits', 2, _hs(_MK, k=1, u=None, lp=_P, logits=None, mask=_ROWSEL), None, _LG_HEADS),
          ('mask-k1-lp-no-logits+ts64', 2, _hs(_MK, k=1, u=None, lp=_P, logits=None, ts=64, mask=_ROWSEL), None, _LG_HEADS),
          ('mask-k1-lp-split-no-logits+ts64', 1, _hs(_MK, k=1, u=None, lp=_P, logits=None, ts=64, mask=_ROWSEL), 'infgen_heads', _M128),
          ('mask-idle-k1-lp-no-logits', 2, _hs(_MK, k=1, u=None, lp=_P, logits=None, mask=_IDLE), 'infgen_heads_logprob', _LG_HEADS),
          ('mask-k5-no-logits', 2, _hs(_MK, logits=None, mask=_ROWSEL), None, _LG_TOPK),
          ('mask-k5-split-ts64', 1, _hs(_MK, logits=None, ts=64, mask=_ROWSEL), 'infgen_heads', _M128)]
    # the four infgen_sample_topk*
    for e in _TK4:
        s = e[len('infgen_sample_'):]
        t += [(f'{s}-k0', 2, _topk(e, k=0), None, _K_RANGE),
              (f'{s}-k17', 2, _topk(e, k=17), None, _K_RANGE),
              (f'{s}-k17+n8', 2, _topk(e, k=17, n=8), None, _K_RANGE),
              (f'{s}-k9-n8', 2, _topk(e, k=9, n=8), None, _K_N)]
    for e in (_TEX, _TMK):
        s = e[len('infgen_sample_'):]
        t += [(f'{s}-temp+rows0', 2, _topk(e, rows=0, sampling=_sampling(-1.0)), None, _TEMP),
              (f'{s}-temp+k17', 2, _topk(e, k=17, sampling=_sampling(-1.0)), None, _TEMP),
              (f'{s}-denormal', 2, _topk(e, sampling=_sampling(1e-40)), None, _DENORM),
              (f'{s}-top-p', 2, _topk(e, sampling=_sampling(0.5, -0.5)), None, _TOP_P),
              (f'{s}-k1-temp-ignored', 2, _topk(e, k=1, n=0, sampling=_sampling(-1.0)), None, _K_N)]
    t += [('topk_mask-temp+n-sets', 2, _topk(_TMK, sampling=_sampling(-1.0), mask=(_P, -1, _P, None, None)), None, _TEMP),
          ('topk_mask-n-sets+rows0+k17', 2, _topk(_TMK, k=17, rows=0, mask=(_P, -1, _P, None, None)), None, _N_SETS),
          ('topk_mask-n-sets-no-table', 2, _topk(_TMK, mask=(None, -1, None, None, None)), None, _N_SETS),
          ('topk_mask-types+n48', 2, _topk(_TMK, n=48, mask=(_P, 2, None, _BY_TYPE, None)), None, _TYPES),
          ('topk_mask-n48+odd', 2, _topk(_TMK, n=48, mask=(_ODD, 2, _P, None, None)), None, _M32),
          ('topk_mask-odd+k17', 2, _topk(_TMK, k=17, mask=(_ODD, 2, _P, None, None)), None, _ALIGN),
          ('topk_mask-k17', 2, _topk(_TMK, k=17, mask=_ROWSEL), None, _K_RANGE)]
    return t


_REFUSALS = _refusals()


def _call_refusal(mode, call):
    """-> (return value, infgen_last_error()) of the call under the thread's attn_mode; no device is touched"""
    import ctypes as C
    from infgen_amd import _lib
    lib = _lib.load()
    entry, args = call
    keep = []
    conv = []
    for a in args:
        if isinstance(a, tuple):                   # mask_type: three host ints
            a = (C.c_int * 3)(*a)
            keep.append(a)
        elif isinstance(a, C.Structure):
            a = C.byref(a)
        conv.append(a)
    opts = _lib.Options()
    _lib.check(lib.infgen_get_effective_options(C.byref(opts)), 'infgen_get_effective_options')
    opts.attn_mode = mode
    with _lib.thread_options(opts):
        rc = getattr(lib, entry)(*conv)
    return rc, lib.infgen_last_error()



@pytest.mark.parametrize('case', _REFUSALS, ids=[c[0] for c in _REFUSALS])
def test_refusals_that_need_no_device(case):
    _id, mode, call, prefix, text = case
    rc, err = _call_refusal(mode, call)
    assert rc != 0, 'refused'
    assert err == (prefix or call[0]).encode() + b': ' + text
