"""GPU: temperature and nucleus (top-p) truncation of the top-k samplers: infgen_sample_topk_ex, infgen_heads_sample_ex,
infgen_insert_decide_topk_ex, InfgenRollout.sample_temperature / sample_top_p / sample_temp_row, RolloutEngine(sample_temperature=...),
InfGenDecoder.sample_temperature.

The float64 restatement of the arithmetic (``ref_draw``) works on the SAME fp32 logits.  Decisions that hang on the last bits are left
out by a margin rule: a row is skipped if ``|u sum - cdf[j]| <= 1e-5 sum`` for some j < m or, with top_p < 1, if
``|cdf[j] - top_p S_k| <= 1e-5 S_k`` for some j.  1e-5 sits above the fp32 error of a cdf entry relative to the sum, (k + 8) 2^-24 +
4 2^-24 max|logit| / T, at its worst case here (k = 16, max|logit| 13, T = 0.5: 7e-6).  ``sample_logprob`` is held to that bound (the
bound of 5.9 with the exponent scaled by 1 / T)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_case, make_weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
MARGIN = 1e-5


def ref_draw(lg, u, k, T, top_p):
    """float64: the six steps of DESIGN 5.10 on fp32 logits [rows][n] with uniforms [rows]; T a scalar or [rows] (0: greedy).
    -> dict(order [rows][k] columns, v [rows][k], pick, m, token, slp [rows][k] (the value for every possible pick), skip [rows])"""
    lg = np.asarray(lg, np.float32)
    rows = lg.shape[0]
    order = np.argsort(-lg.astype(np.float64), axis=-1, kind='stable')[:, :k]         # value descending, column ascending
    v = np.take_along_axis(lg, order, -1).astype(np.float64)
    T = np.broadcast_to(np.asarray(T, np.float32), (rows,))
    greedy = T == 0
    it = np.where(greedy, 1.0, (np.float32(1) / np.where(greedy, np.float32(1), T)).astype(np.float64))
    tp = np.where(greedy, 0.0, float(np.float32(top_p)))
    p = np.exp((v - v[:, :1]) * it[:, None])
    cdf = np.cumsum(p, -1)
    S = cdf[:, -1]
    mass = tp * S
    m = np.where(tp >= 1, k, 1 + np.argmax(cdf >= mass[:, None], -1))
    s = cdf[np.arange(rows), m - 1]
    x = np.asarray(u, np.float32).astype(np.float64) * s
    inside = np.arange(k)[None, :] < m[:, None]
    hit = (x[:, None] < cdf) & inside
    pick = np.where(hit.any(-1), np.argmax(hit, -1), m - 1)
    skip = ((np.abs(x[:, None] - cdf) <= MARGIN * s[:, None]) & inside).any(-1)
    cut = (tp < 1) & ~greedy
    skip |= cut & (np.abs(cdf - mass[:, None]) <= MARGIN * S[:, None]).any(-1)
    slp = (v - v[:, :1]) * it[:, None] - np.log(s)[:, None]
    return dict(order=order, v=v, pick=pick, m=m, token=order[np.arange(rows), pick], slp=slp, skip=skip, greedy=greedy)


def slp_bound(lg, k, T):
    return (k + 8) * EPS + 4 * EPS * float(np.abs(np.asarray(lg)).max()) / T


def _sampling(T=0.0, top_p=0.0, row=None):
    from infgen_amd import _lib
    return _lib.Sampling(float(T), float(top_p), None if row is None else row.data_ptr())


def _sample_ex(lg, k, u, sp, nucleus=True):
    """infgen_sample_topk_ex on device logits; outputs over-allocated (the tail must stay untouched)"""
    from infgen_amd import _lib
    lib = _lib.load()
    rows, n = lg.shape
    dev = lg.device
    tok = torch.full((rows + 7,), -1, dtype=torch.int32, device=dev)
    slp = torch.full((rows + 7,), float('nan'), device=dev)
    nuc = torch.full((rows + 7,), -1, dtype=torch.int32, device=dev)
    _lib.check(lib.infgen_sample_topk_ex(lg.data_ptr(), rows, n, k, u.data_ptr(), None if sp is None else C.byref(sp), tok.data_ptr(),
                                         slp.data_ptr(), nuc.data_ptr() if nucleus else None,
                                         torch.cuda.current_stream().cuda_stream), 'infgen_sample_topk_ex')
    assert (tok[rows:] == -1).all() and torch.isnan(slp[rows:]).all() and (nuc[rows:] == -1).all(), 'entries beyond rows were written'
    return tok[:rows], slp[:rows], nuc[:rows]


# ------------------------------------------------------------------------------------------ 1. the stand-alone sampler against float64
def test_sample_topk_ex_against_float64():
    dev = torch.device('cuda:0')
    skipped_total, sizes, cases = 0, set(), 0
    for rows in (70, 16, 257):
        for n in (2048, 128):
            rng = np.random.default_rng(1000 * rows + n)
            lg = (3 * rng.standard_normal((rows, n))).astype(np.float32)
            u = rng.random(rows).astype(np.float32)
            lg_d, u_d = torch.from_numpy(lg).to(dev), torch.from_numpy(u).to(dev)
            for k in (2, 5, 16):
                for T in (0.5, 1.0, 2.0):
                    for top_p in (0.3, 0.9, 1.0):
                        what = f'rows={rows} n={n} k={k} T={T} top_p={top_p}'
                        cases += 1
                        r = ref_draw(lg, u, k, T, top_p)
                        tok, slp, nuc = (t.cpu().numpy() for t in _sample_ex(lg_d, k, u_d, _sampling(T, top_p)))
                        keep = ~r['skip']
                        n_skip = int(r['skip'].sum())
                        skipped_total += n_skip
                        assert n_skip <= 1, (what, n_skip, 'rows left out by the margin rule')
                        assert np.array_equal(nuc[keep], r['m'][keep]), (what, 'nucleus sizes')
                        assert np.array_equal(tok[keep], r['token'][keep]), (what, 'tokens')
                        assert (nuc >= 1).all() and (nuc <= k).all()
                        want = r['slp'][np.arange(rows), r['pick']]
                        err, bound = float(np.abs(slp.astype(np.float64) - want)[keep].max()), slp_bound(lg, k, T)
                        if cases % 27 == 0:
                            print(f'{what}: sample_logprob error {err:.3e} (bound {bound:.3e}), {n_skip} rows left out')
                        assert err <= bound, (what, err, bound)
                        assert (slp <= 0).all() and np.isfinite(slp).all(), what
                        if top_p < 1:
                            sizes.update(int(x) for x in nuc)
    assert cases == 162 and skipped_total <= 10, (cases, skipped_total)
    assert min(sizes) == 1 and max(sizes) >= 10, ('the cut is exercised', sorted(sizes))


# ------------------------------------------------------------------------------------------ heads fixtures (as tests/test_heads_sample_gpu.py)
@pytest.fixture(scope='module')
def head_packs():
    """token / state head packs per (token_size or 'tie', operand bits); the construction of tests/test_heads_sample_gpu.py: the
    128-token head is the first 128 outputs of the 2048 one; 'tie': output rows 6, 9, 21 and 133 are copies of row 5, bias raised"""
    from infgen_amd import packing
    sd = dict(make_weights(seed=3))
    tp = 'agent_encoder.token_predict_head'
    for k in ('mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias'):
        sd[f'tok128.{k}'] = sd[f'{tp}.{k}']
        sd[f'tie.{k}'] = sd[f'{tp}.{k}']
    sd['tok128.mlp.3.weight'], sd['tok128.mlp.3.bias'] = sd[f'{tp}.mlp.3.weight'][:128].copy(), sd[f'{tp}.mlp.3.bias'][:128].copy()
    w3, b3 = sd[f'{tp}.mlp.3.weight'].copy(), sd[f'{tp}.mlp.3.bias'].copy()
    b3[5] = float(np.abs(b3).max()) + 64.0
    for c in (6, 9, 21, 133):
        w3[c], b3[c] = w3[5], b3[5]
    sd['tie.mlp.3.weight'], sd['tie.mlp.3.bias'] = w3, b3
    dev = torch.device('cuda:0')
    packs = {}
    for bits in (11, 8):
        with packing.operand_bits(bits):
            st = torch.from_numpy(packing.pack_mlp_layer(sd, 'agent_encoder.state_predict_head', row_major_out=True)).to(dev)
            for n, prefix in ((2048, tp), (128, 'tok128'), ('tie', 'tie')):
                packs[n, bits] = (torch.from_numpy(packing.pack_mlp_layer(sd, prefix)).to(dev), st)
    return packs


class _Heads:
    def __init__(self, tokp, stp, x, token_size):
        from infgen_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        self.tokp, self.stp, self.x, self.n, self.rows, self.dev = tokp, stp, x, token_size, x.shape[0], x.device
        self.st = torch.cuda.current_stream().cuda_stream

    def heads(self):
        lg = torch.empty(self.rows, self.n, device=self.dev)
        nt, ns = (torch.zeros(self.rows, dtype=torch.int32, device=self.dev) for _ in range(2))
        self._lib.check(self.lib.infgen_heads(self.x.data_ptr(), self.rows, self.tokp.data_ptr(), self.stp.data_ptr(), self.n,
                                              lg.data_ptr(), nt.data_ptr(), ns.data_ptr(), self.st), 'infgen_heads')
        return lg, nt, ns

    def sample(self, k, u, sp='old', logits=True):
        """infgen_heads_sample (sp == 'old') or infgen_heads_sample_ex -> logits, token, state, token_logprob, sample_logprob"""
        lg = torch.empty(self.rows, self.n, device=self.dev)
        nt, ns = (torch.full((self.rows + 7,), -1, dtype=torch.int32, device=self.dev) for _ in range(2))
        a, b = (torch.full((self.rows + 7,), float('nan'), device=self.dev) for _ in range(2))
        head = (self.x.data_ptr(), self.rows, self.tokp.data_ptr(), self.stp.data_ptr(), self.n, k, u.data_ptr())
        tail = (lg.data_ptr() if logits else None, nt.data_ptr(), ns.data_ptr(), a.data_ptr(), b.data_ptr(), self.st)
        if isinstance(sp, str):
            self._lib.check(self.lib.infgen_heads_sample(*head, *tail), 'infgen_heads_sample')
        else:
            self._lib.check(self.lib.infgen_heads_sample_ex(*head, None if sp is None else C.byref(sp), *tail), 'infgen_heads_sample_ex')
        assert torch.isnan(a[self.rows:]).all() and torch.isnan(b[self.rows:]).all() and (nt[self.rows:] == -1).all()
        return lg, nt[:self.rows], ns[:self.rows], a[:self.rows], b[:self.rows]


def _x(rows, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, 128)).astype(np.float32)).to(dev)


def _u(rows, seed, dev):
    return torch.from_numpy(np.random.default_rng(seed).random(rows).astype(np.float32)).to(dev)


# ------------------------------------------------------------------------------------------ 2. the defaults are the old result
def test_defaults_are_the_old_entries_bit_for_bit(head_packs):
    from infgen_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    rows, n = 70, 2048
    tokp, stp = head_packs[n, 11]
    h = _Heads(tokp, stp, _x(rows, 11, dev), n)
    try:
        _lib.check(lib.infgen_set_attn_mode(1))
        lg, _, _ = h.heads()
        for k in (5, 16):
            u = _u(rows, 100 + k, dev)
            tok0 = torch.zeros(rows, dtype=torch.int32, device=dev)
            slp0 = torch.zeros(rows, device=dev)
            _lib.check(lib.infgen_sample_topk_logprob(lg.data_ptr(), rows, n, k, u.data_ptr(), tok0.data_ptr(), slp0.data_ptr(), h.st))
            _, nt0, ns0, lp0, s0 = h.sample(k, u)
            assert (slp0 < 0).any() and not torch.equal(tok0.long(), lg.argmax(-1)), 'it really samples'
            for sp in (None, _sampling(1, 1), _sampling(0, 0)):                    # NULL, (1, 1), and the zero-filled struct
                tok, slp, nuc = _sample_ex(lg, k, u, sp)
                assert torch.equal(tok, tok0) and torch.equal(slp, slp0) and (nuc == k).all(), k
                _, nt, ns, lp, s = h.sample(k, u, sp=sp)
                assert torch.equal(nt, nt0) and torch.equal(ns, ns0) and torch.equal(lp, lp0) and torch.equal(s, s0), k
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))


# ------------------------------------------------------------------------------------------ 3. fused equals chain, bit for bit
_PAIRS = ((0.5, 0.9), (2.0, 0.3), (1.0, 0.9))


@pytest.mark.parametrize('terms', [3, 1, 2], ids=['three-term', 'fp16', 'bf16'])
@pytest.mark.parametrize('token_size', [2048, 128])
@pytest.mark.parametrize('rows', [70, 16])
def test_fused_equals_heads_then_sample_topk_ex(head_packs, rows, token_size, terms):
    from infgen_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs[token_size, 8 if terms == 2 else 11]
    h = _Heads(tokp, stp, _x(rows, rows + token_size, dev), token_size)
    t_row = torch.from_numpy(np.random.default_rng(rows).choice(np.float32([0, 0, 0.5, 1, 2]), rows)).to(dev)
    t_row[0], t_row[1] = 0.0, 0.7
    try:
        _lib.check(lib.infgen_set_gemm_terms(terms))
        _lib.check(lib.infgen_set_attn_mode(1))
        lg0, nt_greedy, ns0 = h.heads()
        for k in (5, 16):
            assert lib.infgen_heads_sample_fused(1, rows, k) == 1
            u = _u(rows, 1000 * k + rows, dev)
            _, nt_plain, _, lp_plain, _ = h.sample(k, u)
            for sp in [_sampling(T, p) for T, p in _PAIRS] + [_sampling(1.0, 0.9, t_row)]:
                what = f'rows={rows} n={token_size} terms={terms} k={k} T={sp.temperature} top_p={sp.top_p} per-row={bool(sp.temperature_row)}'
                tok, slp, nuc = _sample_ex(lg0, k, u, sp)
                lg, nt, ns, lp, s = h.sample(k, u, sp=sp)
                assert torch.equal(lg, lg0) and torch.equal(ns, ns0), what
                assert torch.equal(nt, tok), (what, 'tokens differ from infgen_heads + infgen_sample_topk_ex')
                assert torch.equal(s, slp), (what, 'sample_logprob differs')
                _, nt_n, _, lp_n, s_n = h.sample(k, u, sp=sp, logits=False)           # no logits are needed on this route
                assert torch.equal(nt_n, nt) and torch.equal(s_n, s) and torch.equal(lp_n, lp), what
                # token_logprob stays the model's own full softmax at temperature 1, of the token that was drawn
                want = torch.log_softmax(lg0.double(), -1).gather(-1, nt.long()[:, None])[:, 0]
                assert float((lp.double() - want).abs().max()) <= (token_size + 8) * EPS + 4 * EPS * float(lg0.abs().max()), what
                same = nt == nt_plain
                assert torch.equal(lp[same], lp_plain[same]), (what, 'the same token has the same full-softmax log-probability')
                if sp.temperature_row:
                    z = t_row == 0
                    assert z.any() and torch.equal(nt[z], nt_greedy[z]) and (s[z] == 0).all() and (nuc[z] == 1).all(), what
                    assert not torch.equal(nt[~z], nt_greedy[~z]), what
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
        _lib.check(lib.infgen_set_gemm_terms(3))


@pytest.mark.parametrize('terms', [3, 1, 2], ids=['three-term', 'fp16', 'bf16'])
def test_a_tie_straddles_the_nucleus_cut(head_packs, terms):
    """five equal leading logits (columns 5, 6, 9, 21, 133), k = 5: p = 1 each, cdf = 1..5 exactly.  top_p = 0.5 asks for mass 2.5, so
    the nucleus holds the three lowest columns - a tie is cut by column order, in both samplers alike"""
    from infgen_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs['tie', 8 if terms == 2 else 11]
    h = _Heads(tokp, stp, _x(5, 5, dev), 2048)
    u = torch.tensor([0.0, 0.3, 0.5, 0.7, 0.95], device=dev)
    try:
        _lib.check(lib.infgen_set_gemm_terms(terms))
        _lib.check(lib.infgen_set_attn_mode(1))
        lg0, _, _ = h.heads()
        cols = [5, 6, 9, 21, 133]
        assert (lg0[:, cols] == lg0[:, 5:6]).all(), 'the five columns carry equal logits'
        for T in (1.0, 0.5):
            sp = _sampling(T, 0.5)
            tok, slp, nuc = _sample_ex(lg0, 5, u, sp)
            _, nt, _, _, s = h.sample(5, u, sp=sp)
            assert torch.equal(nt, tok) and torch.equal(s, slp)
            assert nuc.tolist() == [3] * 5 and nt.tolist() == [5, 5, 6, 9, 9], (nuc.tolist(), nt.tolist())
            assert float((s.double() + math.log(3)).abs().max()) <= (5 + 8) * EPS
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
        _lib.check(lib.infgen_set_gemm_terms(3))


# ------------------------------------------------------------------------------------------ 4. limits
def test_limits(head_packs):
    from infgen_amd import _lib, torch_ops  # noqa: F401
    lib = _lib.load()
    dev = torch.device('cuda:0')
    rows, n, k = 70, 2048, 16
    tokp, stp = head_packs[n, 11]
    x, u = _x(rows, 21, dev), _u(rows, 22, dev)
    h = _Heads(tokp, stp, x, n)
    try:
        _lib.check(lib.infgen_set_attn_mode(1))
        lg0, nt_greedy, _ = h.heads()
        assert torch.equal(nt_greedy.long(), lg0.argmax(-1))
        # a nucleus of mass 1e-6 is the arg-max, a point mass
        for T in (1.0, 2.0):
            _, nt, _, _, s = h.sample(k, u, sp=_sampling(T, 1e-6))
            assert torch.equal(nt, nt_greedy) and (s == 0).all()
            tok, slp, nuc = _sample_ex(lg0, k, u, _sampling(T, 1e-6))
            assert torch.equal(tok, nt_greedy) and (slp == 0).all() and (nuc == 1).all()
        # per-row T = 0: infgen_heads' token
        zeros = torch.zeros(rows, device=dev)
        _, nt, _, _, s = h.sample(k, u, sp=_sampling(1, 1, zeros))
        assert torch.equal(nt, nt_greedy) and (s == 0).all()
        # T = 0.05: the arg-max wherever the two best logits are more than 1 apart (the rest then holds less than 15 e^-20 of the mass,
        # below the spacing of fp32 uniforms at 1).  This head's logits are closer than that, so the limit is taken on logits of
        # test 1's kind, through the stand-alone sampler (the same inline)
        wide = torch.from_numpy((3 * np.random.default_rng(23).standard_normal((rows, n))).astype(np.float32)).to(dev)
        top2 = torch.sort(wide, -1, descending=True)[0][:, :2]
        clear = (top2[:, 0] - top2[:, 1]) > 1.0
        assert clear.any() and not clear.all()
        tok, _, _ = _sample_ex(wide, k, u, _sampling(0.05, 1))
        assert torch.equal(tok[clear].long(), wide.argmax(-1)[clear])
        # the torch ops: trailing arguments, defaults as before
        t0, s0, _, _, b0 = torch.ops.infgen_hip.heads_sample(x, tokp, stp, n, k, u, False, False, True)
        _, nt_old, ns_old, _, slp_old = h.sample(k, u)
        assert torch.equal(t0, nt_old) and torch.equal(s0, ns_old) and torch.equal(b0, slp_old)
        sp = _sampling(0.5, 0.9)
        _, nt_ex, _, _, slp_ex = h.sample(k, u, sp=sp)
        t1, _, _, _, b1 = torch.ops.infgen_hip.heads_sample(x, tokp, stp, n, k, u, False, False, True, 0.5, 0.9)
        assert torch.equal(t1, nt_ex) and torch.equal(b1, slp_ex) and not torch.equal(t1, t0)
        t2, b2 = torch.ops.infgen_hip.sample_topk(lg0, k, u, True, temperature=0.5, top_p=0.9)
        assert torch.equal(t2, nt_ex) and torch.equal(b2, slp_ex)
        t3, b3 = torch.ops.infgen_hip.sample_topk(lg0, k, u, True, temperature_row=zeros)
        assert torch.equal(t3, nt_greedy) and (b3 == 0).all()
        # refusals reach the caller
        for T, p, msg in ((-1.0, 1.0, b'temperature'), (float('nan'), 1.0, b'temperature'), (float('inf'), 1.0, b'temperature'),
                          (1.0, 1.5, b'top_p'), (1.0, -0.1, b'top_p'), (1.0, float('nan'), b'top_p')):
            sp = _sampling(T, p)
            tok = torch.zeros(rows, dtype=torch.int32, device=dev)
            assert lib.infgen_sample_topk_ex(lg0.data_ptr(), rows, n, k, u.data_ptr(), C.byref(sp), tok.data_ptr(), None, None, h.st) != 0
            assert msg in lib.infgen_last_error(), (T, p, lib.infgen_last_error())
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))


# ------------------------------------------------------------------------------------------ 5. engine
_STATE_KEYS = ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state')


def _engine(c, scenes, **kw):
    from infgen_amd import engine
    w = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    eng = engine.RolloutEngine(w, scenes, c['vocab'], c['map_vocab'], c['grid'], **kw)
    eng.rollout()
    return eng


def test_engine_temperature_sweep_over_copies():
    from infgen_amd import synth
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    steps, hc, k = cfg.num_decode_steps, cfg.hist_columns, 5
    scenes = [synth.make_scene(9300 + i, 8, 128, cfg, vocab=c['vocab'], grid=c['grid']) for i in range(2)]
    temps = np.float32([0, 0.5, 1, 2])
    n, S = len(temps), 2 * len(temps)
    u = np.random.default_rng(77).random((steps, S, 8)).astype(np.float32)
    kw = dict(sample_k=k, sample_logprob=True, options={'attn_mode': 1})
    sweep = _engine(c, scenes, copies=n, sample_uniforms=u, sample_temperature=np.tile(temps, 2), store_logits=True, **kw)
    assert sweep.logits_scratch is None, 'a tempered rollout inside the rule keeps no logits scratch'
    outs = sweep.outputs()
    plain = _engine(c, scenes, copies=n, sample_uniforms=u, **kw).outputs()
    greedy = _engine(c, scenes, options={'attn_mode': 1}).outputs()
    keys = _STATE_KEYS + ('next_token_sample_logprob', 'next_token_logprob_mask')
    for s, o in enumerate(outs):
        T = float(temps[s % n])
        one = _engine(c, [scenes[s // n]], sample_uniforms=u[:, s:s + 1], sample_temperature=T, **kw).outputs()[0]
        for key in keys:
            assert np.array_equal(o[key], one[key]), (s, T, key, 'a copy equals its single-scene run')
        m = o['next_token_logprob_mask']
        if T == 0:
            for key in _STATE_KEYS:
                assert np.array_equal(o[key], greedy[s // n][key]), (s, key, 'T = 0 is the greedy rollout')
            assert (o['next_token_sample_logprob'] == 0).all()
        if T == 1:
            for key in keys:
                assert np.array_equal(o[key], plain[s][key]), (s, key, 'T = 1 is the engine without the arguments')
        # sample_logprob against the copy's own stored logits
        sl = slice(hc, hc + steps)
        lgs = o['logits'].transpose(1, 0, 2).reshape(-1, cfg.token_size)                   # [A * steps][n]
        tok, mask = o['next_token_idx'][:, sl].reshape(-1), m[:, sl].reshape(-1)
        r = ref_draw(lgs, np.zeros(len(lgs), np.float32), k, T, 1.0)
        pos = (r['order'] == tok[:, None])
        assert pos[mask].any(-1).all(), (s, 'a sampled token is not among the k best logits')
        want = np.where(pos, r['slp'], 0).sum(-1)
        got = o['next_token_sample_logprob'][:, sl].reshape(-1).astype(np.float64)
        if T > 0:
            err, bound = float(np.abs(got - want)[mask].max()), slp_bound(lgs, k, T)
            print(f'copy {s} T={T}: sample_logprob error {err:.3e} (bound {bound:.3e}), {int(mask.sum())} entries')
            assert err <= bound, (s, T, err, bound)
    assert not np.array_equal(outs[1]['next_token_idx'], outs[3]['next_token_idx']), 'the temperatures change the tokens'
    # reload rewrites the static buffer: the sweep reversed
    sweep.reload(scenes, sample_uniforms=u, sample_temperature=np.tile(temps[::-1], 2))
    sweep.rollout()
    back = sweep.outputs()
    for key in _STATE_KEYS:
        assert np.array_equal(back[3][key], greedy[0][key]), key


def test_engine_in_kernel_route_equals_the_chain():
    """attn_mode 1 samples inside k_heads_h and keeps no logits; attn_mode 2 at this size runs k_heads, then k_sample_topk over
    logits_scratch.  The rollouts - tokens, states, poses - are equal bit for bit under (0.5, 0.9).  The two routes' heads are different
    GEMMs (fp16 split against fp32 MFMA) whose logits differ in the last bits (tests/test_heads_sample_gpu.py compares the rollouts
    only, for the same reason), so ``sample_logprob`` agrees bitwise at operator level, where both routes read the same logits
    (test_fused_equals_heads_then_sample_topk_ex); here each route's value is held to the float64 restatement on ITS OWN stored
    logits, with the bound and the margin rule of test 1 (measured between the routes: 8.5e-7 at most, e.g. -0.10880053 against
    -0.10880138)."""
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    A = c['z']['pos_a'].shape[0]
    steps, hc, k, T, top_p = cfg.num_decode_steps, cfg.hist_columns, 5, 0.5, 0.9
    u = np.random.default_rng(99).random((steps, 1, A)).astype(np.float32)
    kw = dict(sample_k=k, sample_uniforms=u, sample_logprob=True, sample_temperature=T, sample_top_p=top_p)
    fused = _engine(c, [c['scene']], options={'attn_mode': 1}, **kw)
    assert fused.logits is None and fused.logits_scratch is None
    chain = _engine(c, [c['scene']], options={'attn_mode': 2}, **kw)
    assert chain.logits_scratch is not None
    p, q = fused.outputs()[0], chain.outputs()[0]
    for key in _STATE_KEYS:
        assert np.array_equal(p[key], q[key]), key
    assert np.array_equal(p['next_token_logprob_mask'], q['next_token_logprob_mask'])
    for mode, o in ((1, p), (2, q)):
        kept = _engine(c, [c['scene']], options={'attn_mode': mode}, store_logits=True, **kw)
        assert kept.logits_scratch is None              # (the chain reads store_logits' slice of the step)
        w = kept.outputs()[0]
        for key in _STATE_KEYS + ('next_token_sample_logprob',):
            assert np.array_equal(w[key], o[key]), (mode, key, 'storing the logits changes nothing')
        sl = slice(hc, hc + steps)
        lgs = w['logits'].transpose(1, 0, 2).reshape(-1, cfg.token_size)                   # [A * steps][n], row a * steps + t
        tok, mask = w['next_token_idx'][:, sl].reshape(-1), w['next_token_logprob_mask'][:, sl].reshape(-1)
        r = ref_draw(lgs, u[:, 0, :w['next_token_idx'].shape[0]].T.reshape(-1), k, T, top_p)
        keep = mask & ~r['skip']
        assert (mask & r['skip']).sum() <= 2 and keep.sum() >= 20, (mode, int(keep.sum()))
        assert np.array_equal(tok[keep], r['token'][keep]), (mode, 'tokens against float64')
        got = w['next_token_sample_logprob'][:, sl].reshape(-1).astype(np.float64)
        err, bound = float(np.abs(got - r['slp'][np.arange(len(tok)), r['pick']])[keep].max()), slp_bound(lgs, k, T)
        print(f'attn_mode {mode}: sample_logprob error {err:.3e} (bound {bound:.3e}), {int(keep.sum())} entries, nucleus sizes '
              f'{sorted(set(r["m"][keep].tolist()))}')
        assert err <= bound, (mode, err, bound)
    base = _engine(c, [c['scene']], options={'attn_mode': 1}, sample_k=5, sample_uniforms=u).outputs()[0]
    assert not np.array_equal(p['next_token_idx'], base['next_token_idx'])
    from infgen_amd import engine
    for bad in (dict(sample_temperature=-1.0), dict(sample_top_p=1.5), dict(insert_top_p=-0.5), dict(sample_temperature=[1.0, -2.0])):
        with pytest.raises((ValueError, AssertionError)):
            engine.RolloutEngine(fused.w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], sample_k=5, sample_uniforms=u, **bad)


# ------------------------------------------------------------------------------------------ 6. the insertion cell draw
def _decide(st, dec, k, sp):
    import graph_ref as gr  # noqa: F401
    from gpu_blocks import dev, device_block, lib_and_check
    lib, check = lib_and_check()
    b, ten = device_block(st)
    d = {key: torch.from_numpy(v.copy()).to(dev()) for key, v in dec.items()}
    P = lambda key: d[key].data_ptr()
    args = (C.byref(b), 0, 1, 10, P('lg_state'), P('lg_type'), P('shape'), P('lg_pos'), P('occ'), P('active'), P('n_new'),
            P('inserted'), P('new_row'), P('new_shape'), P('new_cell'), k, P('uniform'))
    if isinstance(sp, str):
        check(lib.infgen_insert_decide_topk(*args, None), 'infgen_insert_decide_topk')
    else:
        check(lib.infgen_insert_decide_topk_ex(*args, None if sp is None else C.byref(sp), None), 'infgen_insert_decide_topk_ex')
    torch.cuda.synchronize()
    return {key: v.cpu().numpy() for key, v in ten.items()}, {key: v.cpu().numpy() for key, v in d.items()}


def test_insert_decide_topk_ex():
    import graph_ref as gr
    from infgen_amd import synth
    gxy = synth.build_grid()
    G, S, k = gxy.shape[0], 9, 10
    assert G == 1961
    rng = np.random.default_rng(1961)
    st = gr.new_state(S, 32, 4, 32, G=G, R=15)
    st['grid_xy'] = np.asarray(gxy, np.float32).copy()
    st['n_agents'][:] = rng.integers(3, 20, S)
    st['pos'][:] = rng.uniform(-200, 200, st['pos'].shape).astype(np.float32)
    dec = gr.new_decisions(S, G)
    dec['lg_pos'][:] = (3 * rng.standard_normal((S, G))).astype(np.float32)
    dec['uniform'][:] = rng.random(S).astype(np.float32)
    dec['shape'][:] = rng.uniform(0.5, 5, (S, 3)).astype(np.float32)
    old_st, old = _decide(st, dec, k, 'old')
    assert (old['inserted'] == 1).all()
    for sp in (None, _sampling(1, 1), _sampling(0, 0)):
        new_st, new = _decide(st, dec, k, sp)
        for key in old:
            assert np.array_equal(old[key], new[key], equal_nan=True), key
        for key in old_st:
            assert np.array_equal(old_st[key], new_st[key]), key
    r = ref_draw(dec['lg_pos'], dec['uniform'], k, 0.5, 0.9)
    _, got = _decide(st, dec, k, _sampling(0.5, 0.9))
    keep = ~r['skip']
    assert r['skip'].sum() <= 1
    assert np.array_equal(got['new_cell'][keep], r['token'][keep]), (got['new_cell'], r['token'])
    assert (r['m'] < k).any(), 'the nucleus cuts the beam'
    plain = ref_draw(dec['lg_pos'], dec['uniform'], k, 1.0, 1.0)
    assert np.array_equal(old['new_cell'][~plain['skip']], plain['token'][~plain['skip']])
    assert (r['token'] != plain['token']).any(), 'the parameters change a cell'


def test_engine_insertion_cell_draw():
    """RolloutEngine(insert_temperature, insert_top_p) -> InfgenInsertion -> infgen_insert_seed -> k_insert_decide: the insertion
    fixture with sampled cells (insert_k = 10), eight copies with their own uniforms.  The defaults are the rollout of an engine built
    without the arguments, bit for bit; (0.5, 0.9) changes inserted cells; and the first iteration's draw - whose cell logits do not
    depend on the parameters - equals the float64 restatement on the engine's own lg_pos, under test 1's margin rule"""
    from infgen_amd import engine
    c = load_case('ins_sampled_a16_m256')
    cfg, m = c['cfg'], c['meta']
    cfg.disable_insertion = False
    k, n = int(m.get('insert_k', 10)), 8
    assert k == 10
    w = engine.PackedWeights(c['sd'], cfg, torch.device('cuda:0'))
    iu = np.random.default_rng(31).random((cfg.num_decode_steps, 10, n)).astype(np.float32)
    kw = dict(copies=n, force_enter=(m['insertion'] == 'forced'), insert_k=k, insert_uniforms=iu)

    def build(**extra):
        return engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw, **extra)

    def first_draw(eng, T, top_p):
        """the decisions of the first insertion iteration (decode step 1) against ref_draw on the cell logits they were drawn from"""
        gen = eng.run_gen(0, 2)                      # (the sub-loop runs from decode step 1 on; step 0 decodes greedily here)
        next(gen).synchronize()
        I = eng.ins
        lg_pos, cell = I['lg_pos'].cpu().numpy().reshape(n, -1), I['new_cell'].cpu().numpy()
        inserted = I['host_dec'].numpy()[0].copy() > 0
        for _ in gen:
            pass
        r = ref_draw(lg_pos, iu[1, 0], k, T, top_p)
        keep = inserted & ~r['skip']
        assert keep.sum() >= 1 and r['skip'].sum() <= 1, (inserted, r['skip'])
        assert np.array_equal(cell[keep], r['token'][keep]), (T, top_p, cell, r['token'])
        return r, inserted

    outs = {}
    for name, extra in (('old', {}), ('default', dict(insert_temperature=1.0, insert_top_p=1.0)),
                        ('hot', dict(insert_temperature=0.5, insert_top_p=0.9))):
        eng = build(**extra)
        eng.rollout()
        outs[name] = eng.outputs()
    keys = ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state', 'pred_type')
    for a, b in zip(outs['old'], outs['default']):
        for key in keys:
            assert np.array_equal(a[key], b[key]), key
    changed = [s for s, (a, b) in enumerate(zip(outs['old'], outs['hot']))
               if a['pos_a'].shape != b['pos_a'].shape or not np.array_equal(a['pos_a'], b['pos_a'])]
    assert changed, 'temperature 0.5 and nucleus 0.9 change no inserted cell in any of the eight copies'
    plain, ins_p = first_draw(build(), 1.0, 1.0)
    hot, ins_h = first_draw(build(insert_temperature=0.5, insert_top_p=0.9), 0.5, 0.9)
    assert np.array_equal(plain['order'], hot['order']), 'the first iteration ranks the same cell logits'
    print(f'first iteration: inserted {ins_p.tolist()} / {ins_h.tolist()}, nucleus sizes {hot["m"].tolist()}, '
          f'{int((plain["token"] != hot["token"]).sum())} of {n} cells differ; copies changed over the rollout: {changed}')
    with pytest.raises(ValueError):
        build(insert_temperature=0.0)


# ------------------------------------------------------------------------------------------ 7. module entries
def test_module_attributes():
    from infgen_amd import synth
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    dec = _decoder(cfg)
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    scene = synth.make_scene(9301, 8, 128, cfg, vocab=c['vocab'], grid=c['grid'])
    A = 8
    u = np.random.default_rng(5).random((cfg.num_decode_steps, 4, A)).astype(np.float32)
    dec.agent_encoder.motion_beam_size = 5
    dec.sample_logprob = True
    try:
        base = dec.inference(_to_data(scene, dev), sample_uniforms=u[:, :1])
        dec.sample_temperature, dec.sample_top_p = 0.5, 0.9
        out = dec.inference(_to_data(scene, dev), sample_uniforms=u[:, :1])
        assert not torch.equal(out['next_token_idx'], base['next_token_idx']), 'the attributes change the tokens'
        eng = _engine(c, [scene], sample_k=5, sample_uniforms=u[:, :1], sample_temperature=0.5, sample_top_p=0.9)
        assert np.array_equal(out['next_token_idx'].cpu().numpy(), eng.outputs()[0]['next_token_idx']), 'and reproduce the engine'
        got = dec.inference_batch([_to_data(scene, dev)], sample_uniforms=u[:, :1])[0]
        assert torch.equal(got['next_token_idx'], out['next_token_idx'])
        # top-p goes through reload like the temperature: the same engine serves a sweep; the cell draw's scalars reach its engine
        n_eng = len(dec._engines)
        dec.sample_top_p = 0.5
        other = dec.inference(_to_data(scene, dev), sample_uniforms=u[:, :1])
        assert len(dec._engines) == n_eng and not torch.equal(other['next_token_idx'], out['next_token_idx'])
        dec.sample_top_p = 0.9
        again = dec.inference(_to_data(scene, dev), sample_uniforms=u[:, :1])
        assert torch.equal(again['next_token_idx'], out['next_token_idx'])
        dec.insert_temperature, dec.insert_top_p = 0.5, 0.9
        dec.inference(_to_data(scene, dev), sample_uniforms=u[:, :1])
        assert any(e.insert_temperature == 0.5 and e.insert_top_p == 0.9 for e in dec._engines.values())
        dec.insert_temperature, dec.insert_top_p = 1.0, 1.0
        # one temperature per copy equals separate calls
        dec.sample_top_p = 1.0
        temps = [0.0, 0.5, 1.0, 2.0]
        rolls = dec.inference_rollouts(_to_data(scene, dev), 4, sample_temperature=temps, sample_uniforms=u)
        for i, T in enumerate(temps):
            dec.sample_temperature = T       # (0: greedy, for the module and the engine as for a per-row entry)
            one = dec.inference(_to_data(scene, dev), sample_uniforms=u[:, i:i + 1])
            for key in ('next_token_idx', 'next_token_sample_logprob'):
                assert torch.equal(rolls[i][key], one[key]), (i, T, key)
    finally:
        dec.agent_encoder.motion_beam_size = 1
        dec.sample_logprob = False
        dec.sample_temperature, dec.sample_top_p = 1.0, 1.0
        dec.insert_temperature, dec.insert_top_p = 1.0, 1.0


def test_validation_step_honours_the_attributes(tmp_path):
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
    enc = model.encoder
    enc.sample_logprob = True
    enc.agent_encoder.motion_beam_size = 5
    model.on_validation_start()
    torch.manual_seed(7)
    a = model.validation_step(_raw_scene(4242, 12, 160, dev), 0)['next_token_sample_logprob'].clone()
    enc.sample_top_p = 1e-6                                   # a point mass: every drawn token has sample_logprob 0
    torch.manual_seed(7)
    out = model.validation_step(_raw_scene(4242, 12, 160, dev), 1)           # (a batch whose pickle exists is skipped: another index)
    with open(tmp_path / 'idx_0_1_rollouts.pkl', 'rb') as f:
        roll = pickle.load(f)
    assert (a < 0).any() and (out['next_token_sample_logprob'] == 0).all()
    assert torch.equal(roll['next_token_sample_logprob'], out['next_token_sample_logprob'].cpu())
    assert float(roll['rollout_sample_logprob'].abs().max()) == 0.0
