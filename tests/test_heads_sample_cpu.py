"""CPU: the ABI, field layout and switches of top-k sampling inside the split heads kernel (infgen_heads_sample,
InfgenRollout.sample_logprob, RolloutEngine(sample_logprob=True), InfGenDecoder.sample_logprob)."""
import inspect
import os
import re

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
