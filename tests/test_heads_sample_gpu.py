"""GPU: top-k sampling inside the split heads kernel (k_heads_h<TERMS, LP, KS>, infgen_heads_sample, torch.ops.infgen_hip.heads_sample)
and the sampler's own log-probability (InfgenRollout.sample_logprob, RolloutEngine(sample_logprob=True), InfGenDecoder.sample_logprob).

Tokens are compared exactly: the kernel computes the logits infgen_heads stores and runs k_sample_topk's arithmetic on them.
Error bounds of the two log-probabilities against float64 references from the SAME fp32 logits - derived, not measured:
``token_logprob``: ``(n + 8) 2^-24 + 4 2^-24 max|logit|`` (worst-case fp32 summation of n terms, a couple of ulp in exp, the
rounding of maximum and result); ``sample_logprob``: the same with k in place of n - the sum of k terms lies in [1, k], one rounding
each for the difference and the result."""
import math

import numpy as np
import pytest
import torch

from conftest import load_case, make_weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
KS = 16                     # the kernel's sampling width (INFGEN_Q_HEADS_SAMPLE_K; checked below)
U_LAST = float(np.nextafter(np.float32(1), np.float32(0)))


def _bound(logits, n=None):
    lg = np.asarray(logits)
    return ((lg.shape[-1] if n is None else n) + 8) * EPS + 4 * EPS * float(np.abs(lg).max())


def _ref(logits, token):
    """float64 log_softmax of fp32 logits [..., n] gathered at token [...] (0 where token < 0)"""
    lg = torch.as_tensor(np.asarray(logits)).double()
    tok = torch.as_tensor(np.asarray(token)).long()
    ls = torch.log_softmax(lg, dim=-1).gather(-1, tok.clamp(min=0)[..., None])[..., 0]
    return torch.where(tok >= 0, ls, torch.zeros((), dtype=torch.float64)).numpy()


def _ref_sample(logits, token, k):
    """float64: top-k of the fp32 logits [..., n], log_softmax re-normalised over the k values, gathered at token [...] (0 where
    token < 0; NaN where the token is not among the k best)"""
    lg = torch.as_tensor(np.asarray(logits)).double()
    tok = torch.as_tensor(np.asarray(token)).long()
    tv, ti = torch.sort(lg, dim=-1, descending=True, stable=True)        # (equal values: the lower column first)
    ls = torch.log_softmax(tv[..., :k], dim=-1)
    hit = ti[..., :k] == tok[..., None]
    val = torch.where(hit, ls, torch.zeros((), dtype=torch.float64)).sum(-1)
    val = torch.where(hit.any(-1), val, torch.full((), float('nan'), dtype=torch.float64))
    return torch.where(tok >= 0, val, torch.zeros((), dtype=torch.float64)).numpy()


def _kth(logits, j):
    """column of the j-th entry (0-based) of every row under (value descending, column ascending)"""
    return torch.sort(torch.as_tensor(np.asarray(logits)), dim=-1, descending=True, stable=True)[1][..., j]


# ------------------------------------------------------------------------------------------ operator level
@pytest.fixture(scope='module')
def head_sd():
    sd = dict(make_weights(seed=3))
    tp = 'agent_encoder.token_predict_head'
    for k in ('mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias'):
        sd[f'tok128.{k}'] = sd[f'{tp}.{k}']
        sd[f'tie.{k}'] = sd[f'{tp}.{k}']
    sd['tok128.mlp.3.weight'], sd['tok128.mlp.3.bias'] = sd[f'{tp}.mlp.3.weight'][:128].copy(), sd[f'{tp}.mlp.3.bias'][:128].copy()
    # output rows 6, 9, 21 and 133 are copies of row 5 (the same float4, another rg lane, another t, another chunk), bias raised
    w3, b3 = sd[f'{tp}.mlp.3.weight'].copy(), sd[f'{tp}.mlp.3.bias'].copy()
    b3[5] = float(np.abs(b3).max()) + 64.0
    for c in (6, 9, 21, 133):
        w3[c], b3[c] = w3[5], b3[5]
    sd['tie.mlp.3.weight'], sd['tie.mlp.3.bias'] = w3, b3
    return sd


@pytest.fixture(scope='module')
def head_packs(head_sd):
    """token / state head packs per (token_size or 'tie', operand bits): the 128-token head is the first 128 outputs of the 2048 one"""
    from infgen_amd import packing
    dev = torch.device('cuda:0')
    packs = {}
    for bits in (11, 8):
        with packing.operand_bits(bits):
            st = torch.from_numpy(packing.pack_mlp_layer(head_sd, 'agent_encoder.state_predict_head', row_major_out=True)).to(dev)
            for n, prefix in ((2048, 'agent_encoder.token_predict_head'), (128, 'tok128'), ('tie', 'tie')):
                packs[n, bits] = (torch.from_numpy(packing.pack_mlp_layer(head_sd, prefix)).to(dev), st)
    return packs


class _Heads:
    def __init__(self, tokp, stp, x, token_size):
        from infgen_amd import _lib
        self.lib, self.P, self._lib = _lib.load(), _lib.ptr, _lib
        self.tokp, self.stp, self.x, self.n, self.rows, self.dev = tokp, stp, x, token_size, x.shape[0], x.device
        self.st = torch.cuda.current_stream().cuda_stream

    def _out(self):
        return (torch.empty(self.rows, self.n, device=self.dev), torch.zeros(self.rows, dtype=torch.int32, device=self.dev),
                torch.zeros(self.rows, dtype=torch.int32, device=self.dev))

    def plain_then_sample(self, k, u):
        """infgen_heads with the logits kept, then infgen_sample_topk on them"""
        P, lib = self.P, self.lib
        lg, nt, ns = self._out()
        self._lib.check(lib.infgen_heads(P(self.x), self.rows, P(self.tokp), P(self.stp), self.n, P(lg), P(nt), P(ns), self.st), 'infgen_heads')
        self._lib.check(lib.infgen_sample_topk(P(lg), self.rows, self.n, k, P(u), P(nt), self.st), 'infgen_sample_topk')
        return lg, nt, ns

    def sample(self, k, u, keep_logits=True, lp=True, slp=True, rc=False):
        """infgen_heads_sample; the outputs over-allocated with NaN / -1 (the tail must stay untouched)"""
        P, lib = self.P, self.lib
        lg, _, _ = self._out()
        nt = torch.full((self.rows + 7,), -1, dtype=torch.int32, device=self.dev)
        ns = torch.full((self.rows + 7,), -1, dtype=torch.int32, device=self.dev)
        a = torch.full((self.rows + 7,), float('nan'), device=self.dev)
        b = torch.full((self.rows + 7,), float('nan'), device=self.dev)
        r = lib.infgen_heads_sample(P(self.x), self.rows, P(self.tokp), P(self.stp), self.n, k, None if u is None else P(u),
                                    P(lg) if keep_logits else None, P(nt), P(ns), P(a) if lp else None, P(b) if slp else None, self.st)
        if rc:
            return r
        self._lib.check(r, 'infgen_heads_sample')
        for t in (a, b):
            assert torch.isnan(t[self.rows:]).all(), 'entries beyond rows were written'
        assert (nt[self.rows:] == -1).all() and (ns[self.rows:] == -1).all(), 'entries beyond rows were written'
        return lg, nt[:self.rows], ns[:self.rows], a[:self.rows], b[:self.rows]


def _uniforms(rows, seed, dev):
    u = np.random.default_rng(seed).uniform(0, 1, size=rows).astype(np.float32)
    u[0] = 0.0                      # the arg-max
    if rows > 1:
        u[1] = U_LAST               # the k-th entry
    return torch.from_numpy(u).to(dev)


def _check_lps(lp, slp, lg, nt, k, what):
    lg, nt = lg.cpu().numpy(), nt.cpu().numpy()
    lp, slp = lp.cpu().numpy().astype(np.float64), slp.cpu().numpy().astype(np.float64)
    e1, b1 = float(np.abs(lp - _ref(lg, nt)).max()), _bound(lg)
    ref_s = _ref_sample(lg, nt, k)
    assert np.isfinite(ref_s).all(), (what, 'a sampled token is not among the k best logits')
    e2, b2 = float(np.abs(slp - ref_s).max()), _bound(lg, k)
    print(f'{what}: token_logprob error {e1:.3e} (bound {b1:.3e}), sample_logprob error {e2:.3e} (bound {b2:.3e})')
    assert np.isfinite(lp).all() and np.isfinite(slp).all() and (lp <= 0).all() and (slp <= 0).all(), what
    assert e1 <= b1 and e2 <= b2, (what, e1, b1, e2, b2)
    assert (slp >= lp - (b1 + b2)).all(), (what, 're-normalising over fewer tokens cannot lower the probability')


@pytest.mark.parametrize('terms', [3, 1, 2], ids=['three-term', 'fp16', 'bf16'])
@pytest.mark.parametrize('token_size', [2048, 128])
@pytest.mark.parametrize('rows', [70, 16])
def test_fused_sampling_equals_heads_then_sample_topk(head_packs, rows, token_size, terms):
    from infgen_amd import _lib
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_HEADS_SAMPLE_K) == KS
    dev = torch.device('cuda:0')
    tokp, stp = head_packs[token_size, 8 if terms == 2 else 11]
    x = torch.from_numpy(np.random.default_rng(rows + token_size).standard_normal((rows, 128)).astype(np.float32)).to(dev)
    h = _Heads(tokp, stp, x, token_size)
    try:
        _lib.check(lib.infgen_set_gemm_terms(terms))
        for k in (2, 5, KS):
            what = f'rows={rows} n={token_size} terms={terms} k={k}'
            u = _uniforms(rows, 1000 * k + rows, dev)
            _lib.check(lib.infgen_set_attn_mode(1))                              # the split path whatever the row count: fused
            assert lib.infgen_heads_sample_fused(1, rows, k) == 1
            lg0, nt0, ns0 = h.plain_then_sample(k, u)
            lg, nt, ns, lp, slp = h.sample(k, u)
            assert torch.equal(lg, lg0), (what, 'the sampling instantiation stores other logits')
            assert torch.equal(nt, nt0), (what, 'tokens differ from infgen_heads + infgen_sample_topk')
            assert torch.equal(ns, ns0), what
            assert int(nt[0]) == int(lg[0].argmax()) and int(nt[0]) == int(_kth(lg[0].cpu(), 0)), (what, 'u = 0 is the arg-max')
            assert int(nt[1]) == int(_kth(lg[1].cpu(), k - 1)), (what, 'the largest u below 1 is the k-th entry')
            _check_lps(lp, slp, lg, nt, k, 'fused ' + what)
            _, nt_n, ns_n, lp_n, slp_n = h.sample(k, u, keep_logits=False)       # no logits are needed on this route
            assert torch.equal(nt_n, nt) and torch.equal(ns_n, ns) and torch.equal(lp_n, lp) and torch.equal(slp_n, slp), what
            _, nt_b, _, lp_b, slp_b = h.sample(k, u)
            assert torch.equal(nt_b, nt) and torch.equal(lp_b, lp) and torch.equal(slp_b, slp), 'a second launch must be bitwise equal'
            # each optional output alone changes nothing
            _, nt_o, _, _, slp_o = h.sample(k, u, keep_logits=False, lp=False)
            assert torch.equal(nt_o, nt) and torch.equal(slp_o, slp), what
            _, nt_o, _, lp_o, _ = h.sample(k, u, keep_logits=False, slp=False)
            assert torch.equal(nt_o, nt) and torch.equal(lp_o, lp), what
            # the stand-alone sampler's optional output: the same value from the same logits, bit for bit (one shared inline)
            nt_s = torch.zeros(rows, dtype=torch.int32, device=dev)
            slp_s = torch.full((rows + 7,), float('nan'), device=dev)
            _lib.check(lib.infgen_sample_topk_logprob(_lib.ptr(lg), rows, token_size, k, _lib.ptr(u), _lib.ptr(nt_s), _lib.ptr(slp_s),
                                                      h.st), 'infgen_sample_topk_logprob')
            assert torch.equal(nt_s, nt) and torch.equal(slp_s[:rows], slp) and torch.isnan(slp_s[rows:]).all(), what
            # by-size rule: these row counts take k_heads under attn_mode 2, then k_sample_topk / k_token_logprob over its logits
            _lib.check(lib.infgen_set_attn_mode(2))
            assert lib.infgen_heads_sample_fused(2, rows, k) == 0
            lg0, nt0, ns0 = h.plain_then_sample(k, u)
            lg2, nt2, ns2, lp2, slp2 = h.sample(k, u)
            assert torch.equal(lg2, lg0) and torch.equal(nt2, nt0) and torch.equal(ns2, ns0), what
            _check_lps(lp2, slp2, lg2, nt2, k, 'chain ' + what)
            # (each route equals infgen_heads + infgen_sample_topk on ITS logits, which is the check; k_heads and the split kernel are
            # different GEMMs whose logits differ in the last bits, so the two routes' tokens are not compared with each other)
            assert h.sample(k, u, keep_logits=False, rc=True) != 0
            assert b'needs a logits buffer' in lib.infgen_last_error()
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
        _lib.check(lib.infgen_set_gemm_terms(3))


@pytest.mark.parametrize('terms', [3, 1, 2], ids=['three-term', 'fp16', 'bf16'])
def test_equal_logits_take_the_lower_column_first(head_packs, terms):
    from infgen_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs['tie', 8 if terms == 2 else 11]
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((5, 128)).astype(np.float32)).to(dev)
    u = torch.tensor([0.0, 0.3, 0.5, 0.7, 0.95], device=dev)
    h = _Heads(tokp, stp, x, 2048)
    try:
        _lib.check(lib.infgen_set_gemm_terms(terms))
        _lib.check(lib.infgen_set_attn_mode(1))
        lg, nt, ns, lp, slp = h.sample(5, u)
        cols = [5, 6, 9, 21, 133]
        assert (lg[:, cols] == lg[:, 5:6]).all(), 'the five columns carry equal logits'
        assert (lg[:, cols].min(-1)[0] > torch.cat([lg[:, :5], lg[:, 134:]], -1).max(-1)[0]).all(), 'and they lead'
        assert nt.tolist() == cols, nt.tolist()
        assert float((slp.double() + math.log(5)).abs().max()) <= _bound(lg.cpu().numpy(), 5)
        _check_lps(lp, slp, lg, nt, 5, f'ties terms={terms}')
        lg0, nt0, _ = h.plain_then_sample(5, u)
        assert torch.equal(nt0, nt) and torch.equal(lg0, lg)
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
        _lib.check(lib.infgen_set_gemm_terms(3))


def test_error_paths_and_the_torch_op(head_packs):
    from infgen_amd import _lib, torch_ops  # noqa: F401
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs[128, 11]
    rows = 16
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((rows, 128)).astype(np.float32)).to(dev)
    u = _uniforms(rows, 7, dev)
    h = _Heads(tokp, stp, x, 128)
    try:
        for mode in (1, 2):
            _lib.check(lib.infgen_set_attn_mode(mode))
            for k, msg in ((0, b'k must be in 1..16'), (17, b'k must be in 1..16')):
                assert h.sample(k, u, rc=True) != 0 and msg in lib.infgen_last_error(), (mode, k)
            assert h.sample(5, None, rc=True) != 0 and b'uniform' in lib.infgen_last_error()
        # k > token_size: reachable only with a head narrower than 17 tokens, which the kernels do not take (token_size is a multiple
        # of 128), so the message is checked on the stand-alone entry with n = 8, and 129 on the 128-token head fails as k > 16 does
        assert h.sample(129, u, rc=True) != 0 and lib.infgen_last_error()
        lg8, t8 = torch.zeros(rows, 8, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        assert lib.infgen_sample_topk_logprob(_lib.ptr(lg8), rows, 8, 9, _lib.ptr(u), _lib.ptr(t8), None, h.st) != 0
        assert b'k must not exceed n' in lib.infgen_last_error()
        # k = 1 is the arg-max, a point mass
        _lib.check(lib.infgen_set_attn_mode(1))
        lg, nt, ns, lp, slp = h.sample(1, u)
        assert torch.equal(nt.long(), lg.argmax(-1)) and (slp == 0).all()
        assert float(np.abs(lp.cpu().numpy() - _ref(lg.cpu(), nt.cpu())).max()) <= _bound(lg.cpu())
        # the torch op on both routes
        lg5, nt5, ns5, lp5, slp5 = h.sample(5, u)
        for mode in (1, 2):
            _lib.check(lib.infgen_set_attn_mode(mode))
            t, s, l, a, b = torch.ops.infgen_hip.heads_sample(x, tokp, stp, 128, 5, u, True, True, True)
            assert t.dtype == torch.int32 and l.shape == (rows, 128) and a.shape == b.shape == (rows,)
            if mode == 1:
                assert torch.equal(t, nt5) and torch.equal(s, ns5) and torch.equal(l, lg5) and torch.equal(a, lp5) and torch.equal(b, slp5)
            _check_lps(a, b, l, t, 5, f'torch op mode {mode}')
            t2, s2, l2, a2, b2 = torch.ops.infgen_hip.heads_sample(x, tokp, stp, 128, 5, u, False, False, True)
            assert torch.equal(t2, t) and torch.equal(b2, b) and l2.shape == (0, 128) and a2.shape == (0,)
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))


# ------------------------------------------------------------------------------------------ engine
def _engine(c, scenes=None, **kw):
    from infgen_amd import engine
    w = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    eng = engine.RolloutEngine(w, scenes or [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw)
    eng.rollout()
    return eng


_STATE_KEYS = ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state')


def _check_scene(o, cfg, k, what):
    """both log-probabilities against the scene's own stored logits wherever the mask holds; zeros elsewhere"""
    hc, steps = cfg.hist_columns, o['logits'].shape[0]
    m, tok = o['next_token_logprob_mask'], o['next_token_idx']
    sl = slice(hc, hc + steps)
    lgs = o['logits'].transpose(1, 0, 2)
    t = np.where(m[:, sl], tok[:, sl], -1)
    slp = o['next_token_sample_logprob']
    assert slp.dtype == np.float32 and slp.shape == m.shape == tok.shape and (slp[~m] == 0).all() and m.any()
    e2, b2 = float(np.abs(slp[:, sl] - _ref_sample(lgs, t, k)).max()), _bound(o['logits'], k)
    print(f'{what}: sample_logprob error {e2:.3e} (bound {b2:.3e}), {int(m.sum())} entries')
    assert e2 <= b2 and (slp <= 0).all(), (what, e2, b2)
    if 'next_token_logprob' in o:
        lp = o['next_token_logprob']
        e1, b1 = float(np.abs(lp[:, sl] - _ref(lgs, t)).max()), _bound(o['logits'])
        assert e1 <= b1, (what, e1, b1)
        # exp(sample_logprob) >= exp(logprob) where masked, up to the two bounds
        assert (slp[m].astype(np.float64) >= lp[m].astype(np.float64) - (b1 + b2)).all(), what


def test_engine_fused_route_equals_the_chain():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    A = c['z']['pos_a'].shape[0]
    u = np.random.default_rng(99).uniform(0, 1, size=(cfg.num_decode_steps, 1, A)).astype(np.float32)
    kw = dict(sample_k=5, sample_uniforms=u)
    plain = _engine(c, options={'attn_mode': 1}, **kw)
    assert plain.logits is None and plain.logits_scratch is None, 'the fused route keeps no logits in memory'
    p = plain.outputs()[0]
    chain = _engine(c, options={'attn_mode': 2}, **kw)
    assert chain.logits_scratch is not None
    q = chain.outputs()[0]
    assert not np.array_equal(p['next_token_idx'], c['z']['next_token_idx']), 'it really samples'
    for key in _STATE_KEYS:
        assert np.array_equal(p[key], q[key]), key
    # the keys: exactly two more, the mask by token_logprob's rule
    both = _engine(c, options={'attn_mode': 1}, token_logprob=True, sample_logprob=True, store_logits=True, **kw)
    o = both.outputs()[0]
    only = _engine(c, options={'attn_mode': 1}, sample_logprob=True, **kw)
    assert only.logits_scratch is None
    s = only.outputs()[0]
    lp_only = _engine(c, options={'attn_mode': 1}, token_logprob=True, **kw).outputs()[0]
    assert set(s) - set(p) == {'next_token_sample_logprob', 'next_token_logprob_mask'}
    assert set(o) - set(lp_only) == {'next_token_sample_logprob', 'logits'}
    for key in _STATE_KEYS:
        assert np.array_equal(o[key], p[key]) and np.array_equal(s[key], p[key]), key
    assert np.array_equal(s['next_token_logprob_mask'], lp_only['next_token_logprob_mask'])
    assert np.array_equal(o['next_token_logprob_mask'], lp_only['next_token_logprob_mask'])
    assert np.array_equal(s['next_token_sample_logprob'], o['next_token_sample_logprob'])
    assert np.array_equal(o['next_token_logprob'], lp_only['next_token_logprob'])
    _check_scene(o, cfg, 5, 'fused engine')
    assert (o['next_token_sample_logprob'] < 0).any()
    # the chain computes the same quantity from its own logits
    qc = _engine(c, options={'attn_mode': 2}, token_logprob=True, sample_logprob=True, store_logits=True, **kw).outputs()[0]
    _check_scene(qc, cfg, 5, 'chain engine')
    # the device epilogue and the float64 sum
    od = both.outputs_device()[0]
    assert np.array_equal(od['next_token_sample_logprob'].cpu().numpy(), o['next_token_sample_logprob'])
    assert np.array_equal(od['next_token_logprob_mask'].cpu().numpy(), o['next_token_logprob_mask'])
    tot = both.rollout_sample_logprob()
    assert tot.dtype == torch.float64 and tot.shape == (1,) and tot.device.type == 'cuda'
    vals = o['next_token_sample_logprob'][o['next_token_logprob_mask']].astype(np.float64)
    # pairwise float64 tree over < 2^10 entries: at most 10 roundings of partial sums no larger than sum |x|
    assert abs(float(tot[0]) - math.fsum(vals.tolist())) <= 10 * 2.0 ** -53 * float(np.abs(vals).sum())


def test_engine_sampled_batch_equals_the_single_rollouts():
    """three scenes x two copies in one engine against six one-scene engines on the same uniforms, all sampling inside the heads
    kernel: the tokens and both log-probabilities are per-row quantities, so they are equal bit for bit, and so are the sums"""
    from infgen_amd import synth
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    scenes = [synth.make_scene(9300 + i, 8, 128, cfg, vocab=c['vocab'], grid=c['grid']) for i in range(3)]
    n = 2
    u = np.random.default_rng(41).uniform(0, 1, size=(cfg.num_decode_steps, len(scenes) * n, 8)).astype(np.float32)
    kw = dict(sample_k=5, token_logprob=True, sample_logprob=True, options={'attn_mode': 1})
    eng = _engine(c, scenes=scenes, copies=n, sample_uniforms=u, **kw)
    assert eng.logits_scratch is None
    outs = eng.outputs()
    eng.outputs_device()
    tot, tot_lp = eng.rollout_sample_logprob().cpu(), eng.rollout_logprob().cpu()
    assert len(outs) == len(scenes) * n and tot.shape == (len(scenes) * n,)
    keys = _STATE_KEYS + ('next_token_sample_logprob', 'next_token_logprob', 'next_token_logprob_mask')
    for s, o in enumerate(outs):
        one = _engine(c, scenes=[scenes[s // n]], sample_uniforms=u[:, s:s + 1], **kw)
        q = one.outputs()[0]
        for key in keys:
            assert np.array_equal(o[key], q[key]), (s, key)
        one.outputs_device()
        assert float(one.rollout_sample_logprob()[0]) == float(tot[s]) and float(one.rollout_logprob()[0]) == float(tot_lp[s]), s
        m = o['next_token_logprob_mask']
        assert (o['next_token_sample_logprob'][m] < 0).any() and float(tot[s]) < 0.0, (s, 'sampled: no point mass')
    # copies of one scene differ only by their uniforms
    assert not np.array_equal(outs[0]['next_token_idx'], outs[1]['next_token_idx'])


def test_engine_greedy_is_a_point_mass():
    c = load_case('c1_a8_m128')
    base = _engine(c, options={'attn_mode': 1}).outputs()[0]
    eng = _engine(c, options={'attn_mode': 1}, sample_logprob=True, token_logprob=True)
    o = eng.outputs()[0]
    assert set(o) - set(base) == {'next_token_sample_logprob', 'next_token_logprob', 'next_token_logprob_mask'}
    for key in _STATE_KEYS:
        assert np.array_equal(o[key], base[key]), key
    assert o['next_token_logprob_mask'].any() and (o['next_token_sample_logprob'] == 0).all()
    eng.outputs_device()
    assert float(eng.rollout_sample_logprob()[0]) == 0.0 and float(eng.rollout_logprob()[0]) < 0.0


def test_engine_with_insertion():
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    u = np.random.default_rng(5).uniform(0, 1, size=(cfg.num_decode_steps, 1, 1024)).astype(np.float32)
    kw = dict(store_logits=True, force_enter=True, sample_k=5, sample_uniforms=u, options={'attn_mode': 1})
    eng = _engine(c, token_logprob=True, sample_logprob=True, **kw)
    o = eng.outputs()[0]
    ref = _engine(c, token_logprob=True, **kw).outputs()[0]
    A0, A = eng.hosts[0]['A'], o['next_token_idx'].shape[0]
    assert A > A0, 'the fixture inserts agents'
    assert np.array_equal(o['next_token_idx'], ref['next_token_idx'])
    m = o['next_token_logprob_mask']
    assert np.array_equal(m, ref['next_token_logprob_mask']), 'inserted rows are masked as next_token_logprob_mask masks them'
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    bos = eng.bos.cpu().numpy()[0]
    for a in range(A0, A):
        assert not m[a, :int(bos[a]) + 1].any(), a
    assert m[A0:].any(), 'some inserted row carries log-probabilities'
    _check_scene(o, cfg, 5, 'insertion')
    od = eng.outputs_device()[0]
    assert np.array_equal(od['next_token_sample_logprob'].cpu().numpy(), o['next_token_sample_logprob'])


# ------------------------------------------------------------------------------------------ module entries
_S_KEYS = ('next_token_sample_logprob', 'next_token_logprob_mask', 'rollout_sample_logprob')


def test_module_batch_equals_single_calls_and_rollouts():
    from infgen_amd import synth
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    dec = _decoder(c['cfg'])
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    scenes = [synth.make_scene(9300 + i, 8, 128, c['cfg'], vocab=c['vocab'], grid=c['grid']) for i in range(3)]
    base = dec.inference(_to_data(scenes[0], dev))
    assert not set(_S_KEYS) & set(base.keys())
    dec.sample_logprob = True
    out = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
    assert set(_S_KEYS) <= set(out.keys()) and 'next_token_logprob' not in out.keys()
    assert out['rollout_sample_logprob'].shape == (3,) and out['rollout_sample_logprob'].dtype == torch.float64
    ptr = out['agent_ptr'].tolist()
    for s, sc in enumerate(scenes):
        one = dec.inference(_to_data(sc, dev))
        assert set(one.keys()) == set(base.keys()) | set(_S_KEYS)
        for k in _S_KEYS[:2]:
            assert torch.equal(out[k][ptr[s]:ptr[s + 1]], one[k]), (s, k)
        assert torch.equal(out['rollout_sample_logprob'][s], one['rollout_sample_logprob']), s
        # the module decodes greedily unless motion_beam_size says otherwise: a point mass
        assert one['next_token_logprob_mask'].any() and (one['next_token_sample_logprob'] == 0).all()
    # sampled, every rollout with its own uniforms from torch's RNG
    dec.agent_encoder.motion_beam_size = 5
    try:
        rolls = dec.inference_rollouts(_to_data(scenes[1], dev), 3)
        assert len(rolls) == 3
        for r in rolls:
            m, v = r['next_token_logprob_mask'], r['next_token_sample_logprob']
            assert (v[~m] == 0).all() and (v <= 0).all() and (v[m] < 0).any() and (v[m] >= -math.log(5) - 40.0).all()
            vals = v[m].double().cpu()
            assert abs(float(r['rollout_sample_logprob']) - math.fsum(vals.tolist())) <= 10 * 2.0 ** -53 * float(vals.abs().sum())
            assert r['rollout_sample_logprob'].dtype == torch.float64 and r['rollout_sample_logprob'].device.type == 'cuda'
        got = dec.inference_batch([_to_data(sc, dev) for sc in scenes[:2]])
        assert all(set(_S_KEYS) <= set(g.keys()) for g in got)
    finally:
        dec.agent_encoder.motion_beam_size = 1
    dec.sample_logprob = False
    again = dec.inference(_to_data(scenes[0], dev))
    assert set(again.keys()) == set(base.keys())


def test_validation_step_pickles_the_keys(tmp_path):
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
    model.encoder.sample_logprob = True
    model.on_validation_start()
    out = model.validation_step(_raw_scene(4242, 12, 160, dev), 0)
    with open(tmp_path / 'idx_0_0_rollouts.pkl', 'rb') as f:
        roll = pickle.load(f)
    for k in ('next_token_sample_logprob', 'rollout_sample_logprob'):
        assert k in roll and not roll[k].is_cuda and torch.equal(roll[k], out[k].cpu()), k
    assert roll['next_token_sample_logprob'].shape == out['next_token_idx'].shape
