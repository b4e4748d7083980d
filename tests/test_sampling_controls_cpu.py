"""CPU: the ABI, field layout, refusals and op schema of the samplers' temperature and nucleus (top-p) controls (InfgenSampling,
infgen_sample_topk_ex / infgen_heads_sample_ex / infgen_insert_decide_topk_ex, InfgenRollout.sample_temperature / sample_top_p /
sample_temp_row, InfgenInsertion.insert_temperature / insert_top_p).  The refusals are decided on the host before any launch, so
they can be checked without a device: the pointers given are never dereferenced."""
import ctypes as C
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts():
    from infgen_amd import _lib
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT) == C.sizeof(_lib.Rollout)
    assert lib.infgen_layout_query(_lib.Q_ABI_VERSION) == 1
    names = [f[0] for f in _lib.Rollout._fields_]
    assert names[-2:] == ['no_grid_token', 'no_state_token'], 'the two ablation switches are still the last members'
    assert names[-7:-4] == ['sample_temperature', 'sample_top_p', 'sample_temp_row']
    assert C.sizeof(_lib.Sampling) == 16 and [f[0] for f in _lib.Sampling._fields_] == ['temperature', 'top_p', 'temperature_row']
    ins = [f[0] for f in _lib.Insertion._fields_]
    assert ins[-4:] == ['head_pos_xy', 'head_heading_theta', 'no_grid_token', 'no_head_token']
    assert ins[ins.index('max_new') + 1:ins.index('max_new') + 3] == ['insert_temperature', 'insert_top_p']
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    body = hdr[hdr.index('typedef struct InfgenRollout'):hdr.index('} InfgenRollout;')]
    assert body.index('float sample_temperature; float sample_top_p;') < body.index('const float* sample_temp_row;') \
        < body.index('float* sample_logprob;') < body.index('float* token_logprob;') < body.index('int no_grid_token;')
    for sym in ('infgen_sample_topk_ex', 'infgen_heads_sample_ex', 'infgen_insert_decide_topk_ex'):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym) and f'int {sym}(' in hdr


_BAD = ((-1.0, 1.0, b'temperature'), (float('nan'), 1.0, b'temperature'), (float('inf'), 1.0, b'temperature'),
        (1e-40, 1.0, b'denormal'), (1.0, 1.5, b'top_p'), (1.0, -0.25, b'top_p'), (1.0, float('nan'), b'top_p'))


@pytest.mark.parametrize('T,p,msg', _BAD)
def test_refusals(T, p, msg):
    from infgen_amd import _lib
    lib = _lib.load()
    sp = _lib.Sampling(T, p, None)
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    assert lib.infgen_sample_topk_ex(a, 4, 8, 5, a, C.byref(sp), a, None, None, None) != 0
    err = lib.infgen_last_error()
    assert err.startswith(b'infgen_sample_topk_ex: ') and msg in err, err
    assert lib.infgen_heads_sample_ex(a, 4, a, a, 128, 5, a, C.byref(sp), a, a, a, None, None, None) != 0
    assert lib.infgen_last_error().startswith(b'infgen_heads_sample_ex: ') and msg in lib.infgen_last_error()
    # the rollout context: refused by every rollout-level entry's validation, a greedy context ignores the parameters
    r = _lib.Rollout()
    r.S, r.A_cap, r.T, r.M_cap, r.W, r.ring, r.num_layers = 1, 32, 4, 32, 1, 2, 1
    r.sample_temperature, r.sample_top_p = T, p
    r.sample_k, r.sample_u = 5, a
    assert lib.infgen_decode_step(C.byref(r), -1, None) != 0 and msg in lib.infgen_last_error(), lib.infgen_last_error()
    r.sample_k = 1
    assert lib.infgen_decode_step(C.byref(r), -1, None) != 0 and b'step beyond the column range' in lib.infgen_last_error()
    # the cell draw
    r.sample_k = 0
    assert lib.infgen_insert_decide_topk_ex(C.byref(r), 0, 0, 10, a, a, a, a, a, a, a, a, a, a, a, 10, a, C.byref(sp), None) != 0
    assert msg in lib.infgen_last_error()


def test_unset_is_accepted():
    """0 means "unset" for both scalars (a zero-filled struct is the plain sampler); k == 1 ignores the parameters.  Accepted calls would
    launch, so only entries that return before a launch are used: rows == 0"""
    from infgen_amd import _lib
    lib = _lib.load()
    for T, p in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.0), (0.0, 0.9), (2.0, 1e-6)):
        sp = _lib.Sampling(T, p, None)
        assert lib.infgen_sample_topk_ex(None, 0, 8, 5, None, C.byref(sp), None, None, None, None) == 0
    r = _lib.Rollout()
    r.S, r.A_cap, r.T, r.M_cap, r.W, r.ring, r.num_layers = 1, 32, 4, 32, 1, 2, 1
    r.sample_temperature, r.sample_top_p = -1.0, 7.0          # greedy context (sample_k 0): not looked at
    assert lib.infgen_decode_step(C.byref(r), -1, None) != 0 and b'step beyond the column range' in lib.infgen_last_error()


def test_torch_ops_take_the_arguments():
    import torch
    from infgen_amd import torch_ops  # noqa: F401
    schema = str(torch.ops.infgen_hip.heads_sample.default._schema)
    for arg in ('float temperature=1.', 'float top_p=1.', 'Tensor? temperature_row=None'):
        assert arg in schema, (arg, schema)
    assert schema.index('want_sample_logprob') < schema.index('temperature')
    x = torch.empty(7, 128, device='meta')
    e = torch.empty(1, device='meta')
    out = torch.ops.infgen_hip.heads_sample(x, e, e, 2048, 5, torch.empty(7, device='meta'), True, False, True, 0.5, 0.9,
                                            torch.empty(7, device='meta'))
    assert [tuple(t.shape) for t in out] == [(7,), (7,), (7, 2048), (0,), (7,)]
    out = torch.ops.infgen_hip.heads_sample(x, e, e, 2048, 5, torch.empty(7, device='meta'))        # every existing call stays
    assert [tuple(t.shape) for t in out] == [(7,), (7,), (0, 2048), (0,), (0,)]
    tok, slp = torch.ops.infgen_hip.sample_topk(torch.empty(7, 64, device='meta'), 5, torch.empty(7, device='meta'), True,
                                                temperature=2.0, top_p=0.3, temperature_row=torch.empty(7, device='meta'))
    assert tok.shape == slp.shape == (7,) and tok.dtype == torch.int32


def test_engine_and_modules_accept_the_arguments():
    from infgen_amd import engine
    from infgen_amd.modules.infgen_decoder import InfGenDecoder
    p = inspect.signature(engine.RolloutEngine.__init__).parameters
    for k in ('sample_temperature', 'sample_top_p', 'insert_temperature', 'insert_top_p'):
        assert p[k].default == 1.0, k
        assert f'self.{k} = 1.0' in inspect.getsource(InfGenDecoder.__init__), k
    for fn in (engine.RolloutEngine.reload, engine.RolloutEngine.reload_device, engine.RolloutEngine.reload_batch,
               InfGenDecoder.inference_rollouts):
        assert 'sample_temperature' in inspect.signature(fn).parameters, fn
    with pytest.raises(ValueError):
        engine.RolloutEngine._check_top_p(1.5, 'sample_top_p')
    with pytest.raises(ValueError):
        engine.RolloutEngine._check_temperature(float('nan'), 'insert_temperature')
    # the decision to allocate logits_scratch does not look at the parameters
    src = inspect.getsource(engine.RolloutEngine._refresh_opts)
    assert 'temperature' not in src and 'top_p' not in src
