"""GPU: per-token log-probabilities of the rollout (k_token_logprob, k_heads_h<TERMS, true>, RolloutEngine(token_logprob=True),
InfGenDecoder.token_logprob).

Error bound of a log-probability against float64 ``log_softmax`` of the SAME fp32 logits, gathered at the same token - derived,
not measured: ``(n + 8) 2^-24 + 4 2^-24 max|logit|``.  First term: worst-case fp32 summation of n terms, a couple of ulp in exp,
log1p(d) ~ d; second term: the rounding of the maximum and of the result.  Against a fixture of the reference: 2 x 1e-3
(log-softmax moves by at most twice the largest logit difference; 1e-3 is the project's logits bar)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_case, make_weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


def _bound(logits):
    lg = np.asarray(logits)
    return (lg.shape[-1] + 8) * EPS + 4 * EPS * float(np.abs(lg).max())


def _ref(logits, token):
    """float64 log_softmax of fp32 logits [..., n] gathered at token [...] (0 where token < 0)"""
    lg = torch.as_tensor(np.asarray(logits)).double()
    tok = torch.as_tensor(np.asarray(token)).long()
    ls = torch.log_softmax(lg, dim=-1).gather(-1, tok.clamp(min=0)[..., None])[..., 0]
    return torch.where(tok >= 0, ls, torch.zeros((), dtype=torch.float64)).numpy()


def _check(lp, logits, token, what=''):
    lp, ref = np.asarray(lp, np.float64), _ref(logits, token)
    err, bound = float(np.abs(lp - ref).max()), _bound(logits)
    print(f'{what}: log-prob error {err:.3e} (bound {bound:.3e})')
    assert np.isfinite(lp).all() and err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------------------ stand-alone kernel
@pytest.mark.parametrize('n', [128, 2048])
@pytest.mark.parametrize('rows', [1, 5, 9])
def test_standalone_kernel_random_rows(rows, n):
    from infgen_amd import torch_ops  # noqa: F401
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(100 * rows + n)
    lg = (torch.randn(rows, n, generator=g) * 10).to(dev)
    tok = torch.randint(0, n, (rows,), generator=g).to(dev)
    a = torch.ops.infgen_hip.token_logprob(lg, tok)
    assert a.shape == (rows,) and a.dtype == torch.float32
    _check(a.cpu(), lg.cpu(), tok.cpu(), f'random rows={rows} n={n}')
    b = torch.ops.infgen_hip.token_logprob(lg, tok)
    assert torch.equal(a, b), 'a second launch must be bitwise equal'


@pytest.mark.parametrize('n', [128, 2048])
def test_standalone_kernel_crafted_rows(n):
    from infgen_amd import torch_ops  # noqa: F401
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(n)
    lg = torch.randn(5, n, generator=g) * 10
    lg[0] = torch.randn(n, generator=g) * 0.01
    lg[0, 37] = 80.0                           # exp(80) overflows fp32 without the max subtraction
    lg[1] = 3.25                               # all equal: -log(n)
    lg[2, n - 1] = lg[2].max() + 5.0           # the maximum in the last column
    tok = torch.tensor([37, 11, n - 1, -1, 64])
    a = torch.ops.infgen_hip.token_logprob(lg.to(dev), tok.to(dev)).cpu()
    _check(a, lg, tok, f'crafted n={n}')
    assert float(a[3]) == 0.0, 'token -1 gives 0'
    assert abs(float(a[1]) + math.log(n)) <= _bound(lg[1:2])
    # a token that is NOT the maximum of the +80 row: about -80, finite
    tok2 = tok.clone()
    tok2[0] = 5
    a2 = torch.ops.infgen_hip.token_logprob(lg.to(dev), tok2.to(dev)).cpu()
    _check(a2, lg, tok2, f'crafted n={n}, off-peak token')
    assert -81.0 < float(a2[0]) < -79.0


# ------------------------------------------------------------------------------------------ fused kernel
@pytest.fixture(scope='module')
def head_packs():
    """token / state head packs per (token_size, operand bits): the 128-token head is the first 128 outputs of the 2048-token one"""
    from infgen_amd import packing
    sd = dict(make_weights(seed=3))
    tp = 'agent_encoder.token_predict_head'
    for k in ('mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias'):
        sd[f'tok128.{k}'] = sd[f'{tp}.{k}']
    sd['tok128.mlp.3.weight'], sd['tok128.mlp.3.bias'] = sd[f'{tp}.mlp.3.weight'][:128].copy(), sd[f'{tp}.mlp.3.bias'][:128].copy()
    dev = torch.device('cuda:0')
    packs = {}
    for bits in (11, 8):
        with packing.operand_bits(bits):
            st = torch.from_numpy(packing.pack_mlp_layer(sd, 'agent_encoder.state_predict_head', row_major_out=True)).to(dev)
            for n, prefix in ((2048, tp), (128, 'tok128')):
                packs[n, bits] = (torch.from_numpy(packing.pack_mlp_layer(sd, prefix)).to(dev), st)
    return packs


@pytest.mark.parametrize('terms', [3, 1, 2], ids=['three-term', 'fp16', 'bf16'])
@pytest.mark.parametrize('token_size', [2048, 128])
@pytest.mark.parametrize('rows', [70, 16])
def test_fused_kernel_through_heads_logprob(head_packs, rows, token_size, terms):
    from infgen_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs[token_size, 8 if terms == 2 else 11]
    x = torch.from_numpy(np.random.default_rng(rows + token_size).standard_normal((rows, 128)).astype(np.float32)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    P = _lib.ptr

    def plain():
        lg, nt, ns = torch.empty(rows, token_size, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        _lib.check(lib.infgen_heads(P(x), rows, P(tokp), P(stp), token_size, P(lg), P(nt), P(ns), st), 'infgen_heads')
        return lg, nt, ns

    def with_lp(keep_logits=True):
        lg, nt, ns = torch.empty(rows, token_size, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        lp = torch.full((rows + 7,), float('nan'), device=dev)               # over-allocated: the tail must stay untouched
        _lib.check(lib.infgen_heads_logprob(P(x), rows, P(tokp), P(stp), token_size, P(lg) if keep_logits else None, P(nt), P(ns),
                                            P(lp), st), 'infgen_heads_logprob')
        return lg, nt, ns, lp
    try:
        _lib.check(lib.infgen_set_gemm_terms(terms))
        _lib.check(lib.infgen_set_attn_mode(1))                              # the split path whatever the row count
        lg0, nt0, ns0 = plain()
        lg, nt, ns, lp = with_lp()
        assert torch.equal(lg, lg0) and torch.equal(nt, nt0) and torch.equal(ns, ns0), 'the LP instantiation changes nothing else'
        assert torch.equal(nt.long(), lg.argmax(-1))
        assert torch.isnan(lp[rows:]).all(), 'entries beyond rows were written'
        _check(lp[:rows].cpu(), lg.cpu(), nt.cpu(), f'fused rows={rows} n={token_size} terms={terms}')
        _, nt_n, _, lp_n = with_lp(keep_logits=False)                        # no logits are needed on this path
        assert torch.equal(nt_n, nt) and torch.equal(lp_n[:rows], lp[:rows]) and torch.isnan(lp_n[rows:]).all()
        assert torch.equal(with_lp()[3][:rows], lp[:rows]), 'a second launch must be bitwise equal'
        # by-size rule: these row counts take k_heads (fp32 MFMA) and the stand-alone kernel over its stored logits
        _lib.check(lib.infgen_set_attn_mode(2))
        lg0, nt0, ns0 = plain()
        lg2, nt2, ns2, lp2 = with_lp()
        assert torch.equal(lg2, lg0) and torch.equal(nt2, nt0) and torch.equal(ns2, ns0)
        assert torch.isnan(lp2[rows:]).all()
        _check(lp2[:rows].cpu(), lg2.cpu(), nt2.cpu(), f'k_heads + stand-alone rows={rows} n={token_size}')
        nul = torch.zeros(rows, dtype=torch.int32, device=dev)
        assert lib.infgen_heads_logprob(P(x), rows, P(tokp), P(stp), token_size, None, P(nul), P(nul), P(lp2), st) != 0
        assert b'needs a logits buffer' in lib.infgen_last_error()
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
        _lib.check(lib.infgen_set_gemm_terms(3))


# ------------------------------------------------------------------------------------------ engine
def _engine(c, scenes=None, rollouts=1, **kw):
    from infgen_amd import engine
    w = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    eng = engine.RolloutEngine(w, scenes or [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw)
    for _ in range(rollouts):
        eng.rollout()
    return eng


def _check_scene(o, cfg, what, steps=None):
    """the scene's log-probs against its own stored logits wherever the mask holds; zeros elsewhere"""
    hc = cfg.hist_columns
    steps = steps or o['logits'].shape[0]
    lp, m, tok = o['next_token_logprob'], o['next_token_logprob_mask'], o['next_token_idx']
    assert lp.dtype == np.float32 and m.dtype == np.bool_ and lp.shape == m.shape == tok.shape
    assert not m[:, :hc].any() and not m[:, hc + steps:].any()
    assert (lp[~m] == 0).all()
    sl = slice(hc, hc + steps)
    ref = _ref(o['logits'][:steps].transpose(1, 0, 2), np.where(m[:, sl], tok[:, sl], -1))
    err, bound = float(np.abs(lp[:, sl] - ref).max()), _bound(o['logits'])
    print(f'{what}: log-prob error {err:.3e} (bound {bound:.3e}), {int(m.sum())} entries')
    assert m.any() and err <= bound, (what, err, bound)


@pytest.mark.parametrize('mode', ['by-size', 'fused', 'graph'])
def test_engine_greedy_on_the_reference_fixture(mode):
    c = load_case('c1_a8_m128')
    z, cfg = c['z'], c['cfg']
    kw = dict(store_logits=True)
    if mode == 'fused':
        kw['options'] = {'attn_mode': 1}
    plain = _engine(c, **kw).outputs()[0]
    if mode == 'graph':            # first rollout eager (kernels load), second captured, third replayed
        kw['use_graph'] = True
    eng = _engine(c, rollouts=3 if mode == 'graph' else 1, token_logprob=True, **kw)
    assert mode != 'graph' or eng._graph is not None
    o = eng.outputs()[0]
    for k in ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state', 'logits'):
        assert np.array_equal(o[k], plain[k]), (mode, k)
    assert set(o) - set(plain) == {'next_token_logprob', 'next_token_logprob_mask'}
    _check_scene(o, cfg, f'c1_a8_m128 {mode}')
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    assert o['next_token_logprob_mask'][:, hc:hc + steps].all(), 'every decoded row of this fixture is a valid one'
    # against the reference's own logits on the steps the fixture keeps
    kept = z['logits'].shape[0]
    tok = o['next_token_idx'][:, hc:hc + kept]
    assert np.array_equal(tok, z['next_token_idx'][:, hc:hc + kept])
    err = float(np.abs(o['next_token_logprob'][:, hc:hc + kept] - _ref(z['logits'].transpose(1, 0, 2), tok)).max())
    print(f'c1_a8_m128 {mode}: against the reference logits {err:.3e}')
    assert err <= 2e-3
    if mode == 'graph':
        eager = _engine(c, token_logprob=True, store_logits=True).outputs()[0]
        for k in ('next_token_idx', 'logits', 'next_token_logprob', 'next_token_logprob_mask'):
            assert np.array_equal(o[k], eager[k]), k
    if mode == 'by-size':
        # no stored logits: the engine brings its own scratch on this path and the values do not change
        lean = _engine(c, token_logprob=True)
        assert lean.logits is None and lean.logits_scratch is not None
        assert np.array_equal(lean.outputs()[0]['next_token_logprob'], o['next_token_logprob'])
    if mode == 'fused':
        lean = _engine(c, token_logprob=True, options={'attn_mode': 1})
        assert lean.logits is None and lean.logits_scratch is None
        assert np.array_equal(lean.outputs()[0]['next_token_logprob'], o['next_token_logprob'])
        # the device epilogue carries the same arrays
        od = eng.outputs_device()[0]
        assert np.array_equal(od['next_token_logprob'].cpu().numpy(), o['next_token_logprob'])
        assert np.array_equal(od['next_token_logprob_mask'].cpu().numpy(), o['next_token_logprob_mask'])


def test_engine_sampled_tokens():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    A = c['z']['pos_a'].shape[0]
    u = np.random.default_rng(99).uniform(0, 1, size=(cfg.num_decode_steps, 1, A)).astype(np.float32)
    o = _engine(c, token_logprob=True, store_logits=True, sample_k=5, sample_uniforms=u).outputs()[0]
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    assert not np.array_equal(o['next_token_idx'], c['z']['next_token_idx']), 'it really samples'
    assert (o['next_token_idx'][:, hc:hc + steps] != o['logits'].argmax(-1).T).any(), 'some token is not the arg-max'
    _check_scene(o, cfg, 'sampled')
    valid = o['next_token_idx'][:, hc:hc + steps] >= 0
    assert np.array_equal(o['next_token_logprob_mask'][:, hc:hc + steps], valid) and valid.any()
    lean = _engine(c, token_logprob=True, sample_k=5, sample_uniforms=u).outputs()[0]       # logits through logits_scratch
    assert np.array_equal(lean['next_token_logprob'], o['next_token_logprob'])


def test_engine_with_insertion():
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    eng = _engine(c, token_logprob=True, store_logits=True, force_enter=True)
    o = eng.outputs()[0]
    assert np.array_equal(o['next_token_idx'], c['z']['next_token_idx'])
    A0, A = eng.hosts[0]['A'], o['next_token_idx'].shape[0]
    assert A > A0, 'the fixture inserts agents'
    _check_scene(o, cfg, 'insertion')
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    bos = eng.bos.cpu().numpy()[0]
    m, tok = o['next_token_logprob_mask'], o['next_token_idx']
    for a in range(A0, A):
        b = int(bos[a])
        assert hc <= b + 1 <= hc + steps
        assert not m[a, :b + 1].any(), (a, b)
        # from its first decoded column on: True wherever the row emitted a token (a step that predicts the row invalid emits -1)
        assert np.array_equal(m[a, b + 1:hc + steps], tok[a, b + 1:hc + steps] >= 0), (a, b)
        assert m[a, b + 1:hc + steps].any() or not (tok[a, b + 1:] >= 0).any(), (a, b)
    assert np.array_equal(m[:A0, hc:hc + steps], tok[:A0, hc:hc + steps] >= 0)
    assert m[A0:].any(), 'some inserted row carries log-probabilities'
    od = eng.outputs_device()[0]
    assert np.array_equal(od['next_token_logprob'].cpu().numpy(), o['next_token_logprob'])
    assert np.array_equal(od['next_token_logprob_mask'].cpu().numpy(), m)


def test_engine_with_a_replayed_ego():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    A, av = c['z']['pos_a'].shape[0], int(c['z']['ego_index'])
    flag = np.zeros(A, bool)
    flag[av] = True
    o = _engine(c, token_logprob=True, store_logits=True, replay=[flag]).outputs()[0]
    assert np.array_equal(o['replay_mask'], flag)
    assert not o['next_token_logprob_mask'][av].any() and (o['next_token_logprob'][av] == 0).all()
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    others = ~flag
    assert np.array_equal(o['next_token_logprob_mask'][others, hc:hc + steps], o['next_token_idx'][others, hc:hc + steps] >= 0)
    _check_scene(o, cfg, 'replayed ego')            # (the other rows react to the ego: only the bound against the stored logits)


# ------------------------------------------------------------------------------------------ module entries
_LP_KEYS = ('next_token_logprob', 'next_token_logprob_mask', 'pred_prob', 'rollout_logprob')


def _decoder_and_scenes():
    from infgen_amd import synth
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load
    c = load_case('c1_a8_m128')
    dec = _decoder(c['cfg'])
    _load(dec, c['sd'])
    dec = dec.to(torch.device('cuda:0')).eval()
    scenes = [synth.make_scene(9300 + i, 8, 128, c['cfg'], vocab=c['vocab'], grid=c['grid']) for i in range(3)]
    return c, dec, scenes


def test_module_batch_equals_single_calls_and_rollouts():
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_modules_gpu import _to_data
    c, dec, scenes = _decoder_and_scenes()
    cfg, dev = c['cfg'], torch.device('cuda:0')
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    base = dec.inference(_to_data(scenes[0], dev))
    assert not set(_LP_KEYS) & set(base.keys())
    dec.token_logprob = True
    out = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
    assert set(_LP_KEYS) <= set(out.keys())
    assert out['rollout_logprob'].shape == (3,) and out['rollout_logprob'].dtype == torch.float64
    ptr = out['agent_ptr'].tolist()
    for s, sc in enumerate(scenes):
        one = dec.inference(_to_data(sc, dev))
        assert set(one.keys()) == set(base.keys()) | set(_LP_KEYS)
        assert one['pred_prob'].shape == (ptr[s + 1] - ptr[s], steps) and one['rollout_logprob'].shape == ()
        assert torch.equal(out['next_token_idx'][ptr[s]:ptr[s + 1]], one['next_token_idx'])
        for k in _LP_KEYS[:3]:
            assert torch.equal(out[k][ptr[s]:ptr[s + 1]], one[k]), (s, k)
        assert torch.equal(out['rollout_logprob'][s], one['rollout_logprob']), s
        m, lp = one['next_token_logprob_mask'], one['next_token_logprob']
        assert torch.equal(one['pred_prob'], torch.where(m[:, hc:hc + steps], torch.exp(lp[:, hc:hc + steps]), torch.zeros((), device=dev)))
        assert m[:, hc:hc + steps].any() and float(one['pred_prob'].max()) <= 1.0
    rolls = dec.inference_rollouts(_to_data(scenes[1], dev), 3)
    assert len(rolls) == 3
    for r in rolls:
        vals = r['next_token_logprob'][r['next_token_logprob_mask']].double().cpu()
        exact = math.fsum(vals.tolist())
        # pairwise float64 tree over < 2^10 entries: at most 10 roundings of partial sums no larger than sum |x|
        assert abs(float(r['rollout_logprob']) - exact) <= 10 * 2.0 ** -53 * float(vals.abs().sum())
        assert r['rollout_logprob'].dtype == torch.float64 and r['rollout_logprob'].device.type == 'cuda'
    dec.token_logprob = False
    again = dec.inference(_to_data(scenes[0], dev))
    assert set(again.keys()) == set(base.keys())


def test_validation_step_pickles_the_four_keys(tmp_path):
    import pickle
    from infgen_amd import synth
    from infgen_amd.model import InfGen
    from test_model_gpu import _model_config, _raw_scene
    dev = torch.device('cuda:0')
    cfg = synth.standard_config()
    model = InfGen(_model_config(cfg), save_path=str(tmp_path), map_token_traj=synth.make_map_vocab(),
                   agent_tokens=synth.make_agent_vocab(cfg.token_size))
    sd = make_weights(seed=1, head_gain=64.0)
    model.load_state_dict({k: torch.from_numpy(sd[k[len('encoder.'):]]) if k.startswith('encoder.') and k[len('encoder.'):] in sd else v
                           for k, v in model.state_dict().items()}, strict=True)
    model = model.to(dev).eval()
    model.set('validation')
    model.noise = False
    model.encoder.token_logprob = True
    model.on_validation_start()
    out = model.validation_step(_raw_scene(4242, 12, 160, dev), 0)
    with open(tmp_path / 'idx_0_0_rollouts.pkl', 'rb') as f:
        roll = pickle.load(f)
    assert set(_LP_KEYS) <= set(roll)
    for k in _LP_KEYS:
        assert not roll[k].is_cuda and torch.equal(roll[k], out[k].cpu()), k
    assert roll['next_token_logprob'].shape == out['next_token_idx'].shape and roll['next_token_logprob_mask'].any()
    assert roll['pred_prob'].shape == (out['next_token_idx'].shape[0], cfg.num_decode_steps)
