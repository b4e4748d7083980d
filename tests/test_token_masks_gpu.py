"""GPU: constrained decoding - per-row allowed-token sets inside the heads kernels (k_heads_h<TERMS, LP, KS, true>, k_heads<true>,
k_sample_topk<true>; infgen_heads_sample_mask, infgen_sample_topk_mask, torch.ops.infgen_hip.heads_sample / sample_topk;
InfgenRollout.token_mask, RolloutEngine(token_masks=...), ClosedLoopSession.constrain, InfGenDecoder.token_constraints).

Oracle of the operator tests, per route: infgen_heads into stored logits, banned columns filled with -inf in torch, then the existing
infgen_sample_topk_ex with k_eff = min(k, allowed) - rows grouped by k_eff - or, for k = 1, the first maximum.  Tokens are compared
exactly.  The two log-probabilities are compared with float64 restatements from the SAME fp32 logits under the margin rule of
tests/test_heads_sample_gpu.py: ``(n + 8) 2^-24 + 4 2^-24 max|logit|`` for token_logprob (the full, unmasked softmax: n terms) and
the same with k_eff in place of n for sample_logprob (the sampler's own distribution holds k_eff terms)."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_case, make_weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
U_LAST = float(np.nextafter(np.float32(1), np.float32(0)))          # 1 - 2^-24
N_FIXED = 7


def _bound(logits, n=None):
    lg = np.asarray(logits)
    return ((lg.shape[-1] if n is None else n) + 8) * EPS + 4 * EPS * float(np.abs(lg).max())


def _first_max(lg):
    """first maximum per row (value descending, column ascending) on the host"""
    return torch.sort(lg.cpu(), dim=-1, descending=True, stable=True)[1][..., 0].to(torch.int32)


def _fixed_sets(n):
    """the fixed sets of the table, bool [N_FIXED][n]"""
    col = np.arange(n)
    s = np.zeros((N_FIXED, n), bool)
    s[0] = True                                       # all allowed
    s[1, 37] = True                                   # one token only
    s[2, [5, 65, n - 2]] = True                       # three tokens (k = 5 and k = 16 draw over three entries)
    s[3] = col >= n - 128                             # only the last 128-chunk
    s[4] = col % 16 < 4                               # one of the row's four lanes holds every survivor
    s[5] = (col >= 13) & (col < 77)                   # both boundaries inside a 32-bit word
    s[6] = ~np.isin(col, [5, 6])                      # (the 'tie' head: the two lowest of its equal maxima banned)
    return s


@pytest.fixture(scope='module')
def head_packs():
    from infgen_amd import packing
    sd = dict(make_weights(seed=3))
    tp = 'agent_encoder.token_predict_head'
    for k in ('mlp.0.weight', 'mlp.0.bias', 'mlp.1.weight', 'mlp.1.bias'):
        sd[f'tok128.{k}'] = sd[f'{tp}.{k}']
        sd[f'tie.{k}'] = sd[f'{tp}.{k}']
    sd['tok128.mlp.3.weight'], sd['tok128.mlp.3.bias'] = sd[f'{tp}.mlp.3.weight'][:128].copy(), sd[f'{tp}.mlp.3.bias'][:128].copy()
    # output rows 6, 9, 21 and 133 are copies of row 5 (the same float4, another lane, another t, another chunk), bias raised
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
    def __init__(self, tokp, stp, x, n):
        from infgen_amd import _lib
        self.L, self.lib, self.P = _lib, _lib.load(), _lib.ptr
        self.tokp, self.stp, self.x, self.n, self.rows, self.dev = tokp, stp, x, n, x.shape[0], x.device
        self.st = torch.cuda.current_stream().cuda_stream

    def plain(self):
        P = self.P
        lg = torch.empty(self.rows, self.n, device=self.dev)
        nt, ns = (torch.zeros(self.rows, dtype=torch.int32, device=self.dev) for _ in range(2))
        self.L.check(self.lib.infgen_heads(P(self.x), self.rows, P(self.tokp), P(self.stp), self.n, P(lg), P(nt), P(ns), self.st), 'infgen_heads')
        return lg, nt, ns

    def mask_struct(self, bits, mask_row, mask_type, types):
        """the five mask arguments of the C entries (the tensors stay the caller's to keep alive)"""
        P = self.P
        return [P(bits), int(bits.shape[0]), P(mask_row), (C.c_int * 3)(*mask_type), P(types)]

    def masked(self, k, u, tm, keep_logits=True, rc=False):
        """infgen_heads_sample_mask; the outputs over-allocated with NaN / -1 (the tail must stay untouched)"""
        P = self.P
        lg = torch.empty(self.rows, self.n, device=self.dev)
        nt, ns = (torch.full((self.rows + 7,), -1, dtype=torch.int32, device=self.dev) for _ in range(2))
        lp, slp = (torch.full((self.rows + 7,), float('nan'), device=self.dev) for _ in range(2))
        r = self.lib.infgen_heads_sample_mask(P(self.x), self.rows, P(self.tokp), P(self.stp), self.n, k, P(u), None,
                                              *(tm if tm is not None else (None, 0, None, None, None)),
                                              P(lg) if keep_logits else None, P(nt), P(ns),
                                              P(lp), P(slp), self.st)
        if rc:
            return r
        self.L.check(r, 'infgen_heads_sample_mask')
        assert torch.isnan(lp[self.rows:]).all() and torch.isnan(slp[self.rows:]).all(), 'entries beyond rows were written'
        assert (nt[self.rows:] == -1).all() and (ns[self.rows:] == -1).all(), 'entries beyond rows were written'
        return lg, nt[:self.rows], ns[:self.rows], lp[:self.rows], slp[:self.rows]

    def oracle(self, lg, allowed, k, u):
        """masked_fill(-inf) + the existing sampler with k_eff = min(k, allowed), rows grouped by k_eff -> token, sample_logprob, k_eff"""
        P = self.P
        ml = lg.masked_fill(~allowed, float('-inf'))
        keff = torch.clamp(allowed.sum(1), max=k).to(torch.int32)
        tok = torch.zeros(self.rows, dtype=torch.int32, device=self.dev)
        slp = torch.zeros(self.rows, device=self.dev)
        if k == 1:
            return _first_max(ml).to(self.dev), slp, keff
        for ke in sorted(set(keff.tolist())):
            idx = torch.nonzero(keff == ke)[:, 0]
            sub, su = ml[idx].contiguous(), u[idx].contiguous()
            t, s = torch.zeros(len(idx), dtype=torch.int32, device=self.dev), torch.zeros(len(idx), device=self.dev)
            self.L.check(self.lib.infgen_sample_topk_ex(P(sub), len(idx), self.n, ke, P(su), None, P(t), P(s), None, self.st),
                         'infgen_sample_topk_ex')
            tok[idx], slp[idx] = t, s
        return tok, slp, keff


def _selectors(rows, n_sets, dev):
    """per-row selectors, row types and per-type sets; rows with mask_row = -1 sit beside masked rows inside every 16-row group, and
    one selector names a set beyond the table (unconstrained)"""
    r = np.arange(rows)
    mask_row = np.where(r % 3 == 0, -1, r % N_FIXED).astype(np.int32)
    mask_row[r % 5 == 4] = (N_FIXED + r)[r % 5 == 4]          # the row's own set: its unconstrained arg-max banned
    mask_row[7] = n_sets + 3                                    # beyond the table
    types = (r % 4).astype(np.int32)                            # (3: no such type - unconstrained)
    mask_type = [5, -1, 2]
    return torch.from_numpy(mask_row).to(dev), torch.from_numpy(types).to(dev), mask_type


def _allowed_rows(sets, mask_row, types, mask_type):
    """the selection rule of a token mask (include/infgen_hip.h) restated on the host -> bool [rows][n]"""
    sets, mask_row, types = np.asarray(sets), mask_row.cpu().numpy(), types.cpu().numpy()
    out = np.ones((len(mask_row), sets.shape[1]), bool)
    for r, s in enumerate(mask_row):
        if s < 0:
            s = mask_type[types[r]] if 0 <= types[r] < 3 else -1
        if 0 <= s < len(sets):
            out[r] = sets[s]
    return out


def _lp_refs(lg, allowed, nt, keff, k):
    """float64: the full unmasked log-softmax at the token, and the sampler's own (masked, top-k_eff re-normalised) one"""
    lg64 = lg.cpu().double()
    tok = nt.cpu().long()
    full = torch.log_softmax(lg64, -1).gather(-1, tok[:, None])[:, 0].numpy()
    ml = lg64.masked_fill(~allowed.cpu(), float('-inf'))
    tv, ti = torch.sort(ml, dim=-1, descending=True, stable=True)
    own = np.zeros(len(tok))
    for r in range(len(tok)):
        ke = int(keff[r])
        ls = torch.log_softmax(tv[r, :ke], -1)
        hit = (ti[r, :ke] == tok[r]).nonzero()
        assert len(hit) == 1, (r, 'the emitted token is not among the k_eff best allowed logits')
        own[r] = float(ls[hit[0, 0]]) if k > 1 else 0.0
    return full, own


@pytest.mark.parametrize('terms', [3, 1, 2], ids=['three-term', 'fp16', 'bf16'])
@pytest.mark.parametrize('token_size', [2048, 128])
@pytest.mark.parametrize('rows', [70, 16])
def test_masked_heads_equal_masked_fill_then_sample(head_packs, rows, token_size, terms):
    from infgen_amd import _lib, constraints
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs[token_size, 8 if terms == 2 else 11]
    x = torch.from_numpy(np.random.default_rng(rows + token_size).standard_normal((rows, 128)).astype(np.float32)).to(dev)
    h = _Heads(tokp, stp, x, token_size)
    rnd = torch.from_numpy(np.random.default_rng(rows * 7 + terms).random(rows).astype(np.float32)).to(dev)
    uniforms = (('u=0', torch.zeros(rows, device=dev)), ('u=1-2^-24', torch.full((rows,), U_LAST, device=dev)), ('random', rnd))
    try:
        _lib.check(lib.infgen_set_gemm_terms(terms))
        for mode in (1, 2):                     # 1: the fused split kernel; 2: these row counts take k_heads + k_sample_topk
            _lib.check(lib.infgen_set_attn_mode(mode))
            lg0, nt0, ns0 = h.plain()
            # the table: the fixed sets, then one set per row that bans the row's unconstrained arg-max on this route
            own = np.ones((rows, token_size), bool)
            own[np.arange(rows), nt0.cpu().numpy()] = False
            sets = np.concatenate([_fixed_sets(token_size), own])
            bits = constraints.TokenMasks(sets).bits.to(dev)
            mask_row, types, mask_type = _selectors(rows, len(sets), dev)
            tm = h.mask_struct(bits, mask_row, mask_type, types)
            allowed_np = _allowed_rows(sets, mask_row, types, mask_type)
            allowed = torch.from_numpy(allowed_np).to(dev)
            assert allowed_np.all(1).sum() >= 2 and (~allowed_np.all(1)).sum() >= rows // 2
            for k in (1, 2, 5, 16):
                assert lib.infgen_heads_sample_fused(mode, rows, k) == (1 if mode == 1 and k > 1 else 0)
                for uname, u in uniforms:
                    what = f'rows={rows} n={token_size} terms={terms} mode={mode} k={k} {uname}'
                    lg, nt, ns, lp, slp = h.masked(k, u, tm)
                    tok_o, slp_o, keff = h.oracle(lg0, allowed, k, u)
                    assert torch.equal(lg, lg0), (what, 'stored logits stay the raw logits of the unmasked call')
                    assert torch.equal(ns, ns0), (what, 'the state head is left alone')
                    assert allowed[torch.arange(rows, device=dev), nt.long()].all(), (what, 'a banned token was emitted')
                    assert torch.equal(nt, tok_o), (what, 'tokens differ from masked_fill + infgen_sample_topk_ex(k_eff)')
                    assert torch.equal(slp, slp_o), (what, 'sample_logprob differs from the sampler over k_eff entries')
                    full, ownlp = _lp_refs(lg, allowed, nt, keff, k)
                    e1, b1 = float(np.abs(lp.cpu().numpy().astype(np.float64) - full).max()), _bound(lg.cpu().numpy())
                    e2 = float(np.abs(slp.cpu().numpy().astype(np.float64) - ownlp).max())
                    b2 = _bound(lg.cpu().numpy(), int(keff.max()))
                    print(f'{what}: token_logprob error {e1:.3e} (bound {b1:.3e}), sample_logprob error {e2:.3e} (bound {b2:.3e})')
                    assert e1 <= b1 and e2 <= b2, (what, e1, b1, e2, b2)
                    if k == 1:
                        assert (slp == 0).all(), what
                    if uname == 'u=0':            # the best allowed token, whatever k
                        assert torch.equal(nt, _first_max(lg0.masked_fill(~allowed, float('-inf'))).to(dev)), what
                        banned_best = ~allowed[torch.arange(rows, device=dev), nt0.long()]
                        assert banned_best.any() and (nt[banned_best] != nt0[banned_best]).all(), what
                if mode == 1:                     # no logits are needed on the fused route
                    _, nt_n, ns_n, lp_n, slp_n = h.masked(k, rnd, tm, keep_logits=False)
                    assert torch.equal(nt_n, nt) and torch.equal(ns_n, ns) and torch.equal(lp_n, lp) and torch.equal(slp_n, slp), what
                _, nt_b, _, lp_b, slp_b = h.masked(k, rnd, tm)
                assert torch.equal(nt_b, nt) and torch.equal(lp_b, lp) and torch.equal(slp_b, slp), 'a second launch must be bitwise equal'
                # the all-allowed table (through the masked kernels) and the all -1 selectors (the unmasked ones) reproduce the
                # unmasked call bitwise in every output
                base = h.masked(k, rnd, None)
                sel0 = torch.zeros(rows, dtype=torch.int32, device=dev)             # (referenced until the launches are done)
                sel_none = torch.full((rows,), -1, dtype=torch.int32, device=dev)
                every = h.mask_struct(bits, sel0, [-1, -1, -1], None)
                nobody = h.mask_struct(bits, sel_none, [-1, -1, -1], types)
                for name, t in (('all allowed', every), ('all -1', nobody)):
                    got = h.masked(k, rnd, t)
                    for a, b, key in zip(got, base, ('logits', 'token', 'state', 'token_logprob', 'sample_logprob')):
                        assert torch.equal(a, b), (what, name, key)
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))
        _lib.check(lib.infgen_set_gemm_terms(3))


@pytest.mark.parametrize('mode', [1, 2], ids=['fused', 'chain'])
def test_equal_logits_take_the_lowest_allowed_column(head_packs, mode):
    from infgen_amd import _lib, constraints
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs['tie', 11]
    rows = 20
    x = torch.from_numpy(np.random.default_rng(4).standard_normal((rows, 128)).astype(np.float32)).to(dev)
    h = _Heads(tokp, stp, x, 2048)
    bits = constraints.TokenMasks(_fixed_sets(2048)).bits.to(dev)
    sel = torch.full((rows,), 6, dtype=torch.int32, device=dev)
    tm = h.mask_struct(bits, sel, [-1, -1, -1], None)                  # 5 and 6 banned
    try:
        _lib.check(lib.infgen_set_attn_mode(mode))
        lg0, nt0, _ = h.plain()
        assert (nt0 == 5).all() and torch.equal(lg0[:, 5], lg0[:, 133])
        for k, u, want in ((1, 0.0, 9), (3, 0.0, 9), (3, U_LAST, 133), (2, U_LAST, 21)):
            _, nt, _, _, _ = h.masked(k, torch.full((rows,), u, device=dev), tm)
            assert (nt == want).all(), (k, u, nt.tolist())
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))


def test_ops_and_refusals(head_packs):
    """torch.ops.infgen_hip.heads_sample / sample_topk with the trailing mask arguments equal the C entries; what validate refuses"""
    from infgen_amd import _lib, constraints, torch_ops  # noqa: F401
    lib = _lib.load()
    dev = torch.device('cuda:0')
    tokp, stp = head_packs[2048, 11]
    rows = 16
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((rows, 128)).astype(np.float32)).to(dev)
    h = _Heads(tokp, stp, x, 2048)
    sets = _fixed_sets(2048)
    bits = constraints.TokenMasks(sets).bits.to(dev)
    mask_row, types, mask_type = _selectors(rows, len(sets), dev)
    mask_row = mask_row.clamp(max=N_FIXED - 1)
    tm = h.mask_struct(bits, mask_row, mask_type, types)
    u = torch.from_numpy(np.random.default_rng(2).random(rows).astype(np.float32)).to(dev)
    try:
        for mode in (1, 2):
            _lib.check(lib.infgen_set_attn_mode(mode))
            lg, nt, ns, lp, slp = h.masked(5, u, tm)
            o = torch.ops.infgen_hip.heads_sample(x, tokp, stp, 2048, 5, u, True, True, True, 1.0, 1.0, None, bits, mask_row, mask_type, types)
            for a, b in zip(o, (nt, ns, lg, lp, slp)):
                assert torch.equal(a, b), mode
            t2, s2 = torch.ops.infgen_hip.sample_topk(lg, 5, u, True, 1.0, 1.0, None, bits, mask_row, mask_type, types)
            if mode == 2:
                assert torch.equal(t2, nt) and torch.equal(s2, slp)
            allowed = torch.from_numpy(_allowed_rows(sets, mask_row, types, mask_type)).to(dev)
            assert allowed[torch.arange(rows, device=dev), t2.long()].all()
        bad = h.mask_struct(bits, mask_row, mask_type, types)
        bad[1] = -1
        assert h.masked(5, u, bad, rc=True) != 0 and b'n_sets' in lib.infgen_last_error()
        bad = h.mask_struct(bits, mask_row, mask_type, None)
        assert h.masked(5, u, bad, rc=True) != 0 and b'types' in lib.infgen_last_error()
        tok = torch.zeros(rows, dtype=torch.int32, device=dev)
        lg48 = torch.zeros(rows, 48, device=dev)
        r = lib.infgen_sample_topk_mask(_lib.ptr(lg48), rows, 48, 2, _lib.ptr(u), None, *tm, _lib.ptr(tok), None, None, h.st)
        assert r != 0 and b'multiple of 32' in lib.infgen_last_error()
    finally:
        _lib.check(lib.infgen_set_attn_mode(2))


# ------------------------------------------------------------------------------------------ engine level
_KEYS = ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state', 'pred_type')


def _engine(c, scenes, cfg=None, **kw):
    from infgen_amd import engine
    w = engine.PackedWeights(c['sd'], cfg or c['cfg'], torch.device('cuda:0'))
    eng = engine.RolloutEngine(w, scenes, c['vocab'], c['map_vocab'], c['grid'], **kw)
    eng.rollout()
    return eng


def _all_allowed(n):
    from infgen_amd import constraints
    return constraints.TokenMasks(np.ones((1, n), bool), type_sets=[0, 0, 0])


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'k5'])
@pytest.mark.parametrize('mode', [1, 2], ids=['split', 'by-size'])
def test_engine_all_allowed_masks_change_nothing(mode, sampled):
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    kw = dict(options={'attn_mode': mode}, token_logprob=True, store_logits=True)
    if sampled:
        kw.update(sample_k=5, sample_logprob=True,
                  sample_uniforms=np.random.default_rng(3).random((cfg.num_decode_steps, 1, 8)).astype(np.float32))
    base = _engine(c, [c['scene']], **kw).outputs()[0]
    eng = _engine(c, [c['scene']], token_masks=_all_allowed(cfg.token_size), **kw)
    assert eng._ctx.token_mask >= 1, 'the context names the registered mask'
    got = eng.outputs()[0]
    for key in base:
        assert np.array_equal(np.asarray(base[key]), np.asarray(got[key]), equal_nan=np.asarray(base[key]).dtype.kind == 'f'), key


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'k5'])
def test_engine_all_allowed_masks_change_nothing_with_insertion(sampled):
    """insertion on (forced seeds: rows really are appended): every output of outputs() is bitwise what it is without masks"""
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    kw = dict(force_enter=True, token_logprob=True, store_logits=True)
    if sampled:
        kw.update(sample_k=5, sample_logprob=True,
                  sample_uniforms=np.random.default_rng(6).random((cfg.num_decode_steps, 1, 1024)).astype(np.float32))
    base = _engine(c, [c['scene']], cfg=cfg, **kw).outputs()[0]
    eng = _engine(c, [c['scene']], cfg=cfg, token_masks=_all_allowed(cfg.token_size), **kw)
    assert eng._ctx.token_mask >= 1
    got = eng.outputs()[0]
    assert base['num_inserted'] > 0 and got['num_inserted'] == base['num_inserted'], 'rows were inserted'
    assert set(base) == set(got)
    for key in base:
        a, b = np.asarray(base[key]), np.asarray(got[key])
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'), key


def _check_tokens_in_sets(out, cfg, allowed_of_row, skip_rows=()):
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    tok = out['next_token_idx'][:, hc:hc + steps]
    live = out['next_token_logprob_mask'][:, hc:hc + steps]
    checked = 0
    for r in range(tok.shape[0]):
        if r in skip_rows:
            continue
        for t in np.flatnonzero(live[r]):
            assert allowed_of_row(r)[tok[r, t]], (r, t, int(tok[r, t]), 'a generated row emitted a token outside its set')
            checked += 1
    return checked


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'k5'])
def test_engine_per_type_sets_with_a_row_override(sampled):
    from infgen_amd import constraints
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    masks = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0})
    one = np.zeros((1, cfg.token_size), bool)
    one[0, 100:164] = True
    table = constraints.TokenMasks(np.concatenate([masks.allowed, one]), type_sets=masks.type_sets)
    override = np.full((1, 8), -1, np.int32)
    override[0, 2] = 3
    kw = dict(options={'attn_mode': 1}, token_logprob=True)
    if sampled:
        kw.update(sample_k=5, sample_uniforms=np.random.default_rng(8).random((cfg.num_decode_steps, 1, 8)).astype(np.float32))
    free = _engine(c, [c['scene']], **kw)
    eng = _engine(c, [c['scene']], token_masks=table, token_mask_row=override, **kw)
    types = eng.atype.cpu().numpy()[0]
    allowed = table.allowed

    def allowed_of_row(r):
        return allowed[3] if r == 2 else allowed[table.type_sets[types[r]]]
    out = eng.outputs()[0]
    assert _check_tokens_in_sets(out, cfg, allowed_of_row) > 20
    f = free.outputs()[0]
    hc = cfg.hist_columns
    m = f['next_token_logprob_mask'][:, hc:]
    ft = f['next_token_idx'][:, hc:hc + m.shape[1]]
    outside = sum(int(not allowed_of_row(r)[ft[r, t]]) for r in range(ft.shape[0]) for t in np.flatnonzero(m[r]))
    assert outside > 0, 'the unconstrained rollout leaves the sets: the test constrains something'
    # host-side selectors are range-checked before any launch
    with pytest.raises(ValueError, match='outside'):
        eng.reload([c['scene']], token_mask_row=np.full((1, 8), 4, np.int32), **({'sample_uniforms': kw['sample_uniforms']} if sampled else {}))
    with pytest.raises(ValueError, match='outside the table'):
        eng.reload([c['scene']], token_mask_type=[0, 1, 9], **({'sample_uniforms': kw['sample_uniforms']} if sampled else {}))


def test_engine_graph_follows_reloaded_selectors():
    """a captured-graph engine equals the eager one, and after reload(token_mask_row=...) the replayed graph follows the new
    selectors (the table and the selectors live in static buffers)"""
    from infgen_amd import constraints
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    masks = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0, 'no_reverse': True})
    one = np.zeros((1, cfg.token_size), bool)
    one[0, 300:333] = True
    table = constraints.TokenMasks(np.concatenate([masks.allowed, one]), type_sets=masks.type_sets)
    rows_a = np.full((1, 8), -1, np.int32)
    rows_b = rows_a.copy()
    rows_b[0, 1] = 3
    kw = dict(options={'attn_mode': 1}, token_masks=table)
    eager_a = _engine(c, [c['scene']], token_mask_row=rows_a, **kw).outputs()[0]
    eager_b = _engine(c, [c['scene']], token_mask_row=rows_b, **kw).outputs()[0]
    g = _engine(c, [c['scene']], token_mask_row=rows_a, use_graph=True, **kw)
    g.rollout()                                   # (the first rollout runs eagerly, the second captures and replays)
    for key in _KEYS:
        assert np.array_equal(g.outputs()[0][key], eager_a[key]), key
    graph = g._graph
    assert graph is not None
    g.reload([c['scene']], token_mask_row=rows_b)
    assert g._graph is graph, 'new selectors keep the captured graph'
    g.rollout()
    for key in _KEYS:
        assert np.array_equal(g.outputs()[0][key], eager_b[key]), key
    assert not np.array_equal(eager_a['next_token_idx'], eager_b['next_token_idx'])


def test_session_constrain_equals_stepwise_engine():
    """session.constrain() at step t equals an engine whose selector buffer is rewritten between infgen_decode_step calls"""
    from infgen_amd import _lib, constraints
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    one = np.zeros((2, cfg.token_size), bool)
    one[0] = True
    one[1, 500:540] = True
    table = constraints.TokenMasks(one)
    t_change = 3
    mask = np.zeros(8, bool)
    mask[0] = True
    kw = dict(options={'attn_mode': 1}, token_masks=table, replay=[mask])
    from infgen_amd import engine
    w = engine.PackedWeights(c['sd'], cfg, torch.device('cuda:0'))
    sel = torch.full((1, 32), -1, dtype=torch.int32, device='cuda:0')
    sel[0, 3] = 1
    # the session
    eng = engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw)
    ses = eng.session()
    hc = cfg.hist_columns
    ref_plan = engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw).teacher_token.clone()
    for t in range(cfg.num_decode_steps):
        if t == t_change:
            ses.constrain(sel[:, :eng.A_cap])
        ses.command(tokens=ref_plan[:, hc + t].clamp(min=0))
        ses.advance()
    tok_s = eng.token.clone()
    # the same through infgen_decode_step with the buffer rewritten in between
    e2 = engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], **kw)
    s2 = e2.session()
    for t in range(cfg.num_decode_steps):
        if t == t_change:
            e2.mask_row.copy_(sel[:, :e2.A_cap].reshape(-1))
        s2.command(tokens=ref_plan[:, hc + t].clamp(min=0))
        _lib.check(e2.lib.infgen_command_rows(C.byref(e2._ctx), t, 0, _lib.ptr(s2._tok), _lib.ptr(s2._pose), _lib.ptr(s2._mask),
                                              _lib.ptr(e2._shape10), _lib.ptr(s2.cost), e2.ops.stream), 'infgen_command_rows')
        _lib.check(e2.lib.infgen_decode_step(C.byref(e2._ctx), t, e2.ops.stream), 'infgen_decode_step')
    assert torch.equal(tok_s, e2.token)
    row3 = tok_s[0, hc + t_change + 1:, 3].cpu().numpy()
    assert ((row3 >= 500) & (row3 < 540) | (row3 < 0)).all() and (row3 >= 0).any(), row3
    before = tok_s[0, hc:hc + t_change + 1, 3].cpu().numpy()
    assert not ((before >= 500) & (before < 540)).all(), 'the row was free before constrain()'


def test_decoder_token_constraints():
    """InfGenDecoder.token_constraints applies through inference, inference_batch and inference_rollouts, reproduces the engine, and
    engines are not shared between different constraints"""
    from infgen_amd import constraints, synth
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    dec = _decoder(cfg)
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    scene = synth.make_scene(9301, 8, 128, cfg, vocab=c['vocab'], grid=c['grid'])
    slow = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0})
    slower = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 2.0})
    try:
        free = dec.inference(_to_data(scene, dev))
        n0 = len(dec._engines)
        dec.token_constraints = slow
        out = dec.inference(_to_data(scene, dev))
        assert len(dec._engines) == n0 + 1, 'a constrained call does not reuse the unconstrained engine'
        assert not torch.equal(out['next_token_idx'], free['next_token_idx']), 'the constraint changes the tokens'
        eng = _engine(c, [scene], token_masks=slow)
        assert np.array_equal(out['next_token_idx'].cpu().numpy(), eng.outputs()[0]['next_token_idx']), 'and reproduces the engine'
        got = dec.inference_batch([_to_data(scene, dev)])[0]
        assert torch.equal(got['next_token_idx'], out['next_token_idx'])
        for roll in dec.inference_rollouts(_to_data(scene, dev), 2):
            assert torch.equal(roll['next_token_idx'], out['next_token_idx']), 'greedy copies equal the single rollout'
        eng_slow = next(e for e in dec._engines.values() if e.token_masks is slow)
        dec.token_constraints = (slower, slower.type_sets)
        other = dec.inference(_to_data(scene, dev))
        # (the module holds two engines; the oldest goes) - the new constraint got an engine of its own, the held one was not reloaded
        assert any(e.token_masks is slower for e in dec._engines.values()) and eng_slow.token_masks is slow
        assert not torch.equal(other['next_token_idx'], out['next_token_idx'])
        dec.token_constraints = None
        again = dec.inference(_to_data(scene, dev))
        assert torch.equal(again['next_token_idx'], free['next_token_idx'])
    finally:
        dec.token_constraints = None



def test_engine_inserted_rows_follow_their_types_set():
    """scenario insertion on: the rows the rollout appends have mask_row = -1 and take their type's set, with no extra launch"""
    from infgen_amd import constraints
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    table = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0})
    A0 = np.asarray(c['scene']['agent']['state_idx']).shape[0]
    kw = dict(force_enter=True, token_logprob=True)
    eng = _engine(c, [c['scene']], cfg=cfg, token_masks=table, **kw)
    out = eng.outputs()[0]
    A = out['pos_a'].shape[0]
    assert out['num_inserted'] > 0 and A == A0 + out['num_inserted']
    types = eng.atype.cpu().numpy()[0]
    allowed = table.allowed
    assert _check_tokens_in_sets(out, cfg, lambda r: allowed[table.type_sets[types[r]]]) > 20
    assert _check_tokens_in_sets(out, cfg, lambda r: allowed[table.type_sets[types[r]]], skip_rows=range(A0)) > 0, \
        'inserted rows decoded tokens, all inside their type\'s set'
    free = _engine(c, [c['scene']], cfg=cfg, **kw).outputs()[0]
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    ft, fm = free['next_token_idx'][:, hc:hc + steps], free['next_token_logprob_mask'][:, hc:hc + steps]
    assert any(not allowed[table.type_sets[types[r]]][ft[r, t]] for r in range(min(A0, ft.shape[0])) for t in np.flatnonzero(fm[r])), \
        'the unconstrained rollout leaves the sets'


def test_engine_replayed_rows_keep_plan_tokens_outside_their_set():
    from infgen_amd import constraints
    c = load_case('c1_a8_m128')
    cfg, hc = c['cfg'], c['cfg'].hist_columns
    table = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0})
    allowed = table.allowed
    probe = _engine(c, [c['scene']], options={'attn_mode': 1})
    types = probe.atype.cpu().numpy()[0][:8]
    A = probe.outputs()[0]['next_token_idx'].shape[0]
    flag = np.zeros(A, bool)
    flag[[1, 4]] = True
    ptok = np.array(probe.outputs()[0]['next_token_idx'])
    for r in (1, 4):                                   # the plan: a token the row's set bans, at every future column
        ptok[r, hc:] = int(np.flatnonzero(~allowed[table.type_sets[types[r]]])[-1])
    pst = np.ones_like(ptok)
    eng = _engine(c, [c['scene']], options={'attn_mode': 1}, token_masks=table, token_logprob=True, replay=[(flag, ptok, pst)])
    out = eng.outputs()[0]
    assert np.array_equal(out['next_token_idx'][flag][:, hc:], ptok[flag][:, hc:]), 'replayed rows keep their plan'
    assert not any(allowed[table.type_sets[types[r]]][ptok[r, hc]] for r in (1, 4))
    assert _check_tokens_in_sets(out, cfg, lambda r: allowed[table.type_sets[types[r]]], skip_rows=(1, 4)) > 10
    assert not out['next_token_logprob_mask'][flag].any()


@pytest.mark.parametrize('sampled', [False, True], ids=['greedy', 'k5'])
@pytest.mark.parametrize('mode', [1, 2], ids=['fused', 'chain'])
def test_engine_routes_equal_their_stepwise_restatement(mode, sampled):
    """each route against a restatement from ITS stored logits and the mask: masked_fill(-inf), then the existing unmasked sampler
    (k_eff = k: every set here allows more than k tokens) or the first maximum.  The fused route keeps no logits in memory; the
    same engine with store_logits emits the same tokens and lends its logits to the restatement"""
    from infgen_amd import constraints, torch_ops  # noqa: F401  (registers torch.ops.infgen_hip)
    c = load_case('c1_a8_m128')
    cfg, hc, steps, k = c['cfg'], c['cfg'].hist_columns, c['cfg'].num_decode_steps, 5
    table = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0, 'no_reverse': True})
    assert (table.allowed.sum(1) > k).all()
    override = np.full((1, 8), -1, np.int32)
    override[0, 5] = 1
    kw = dict(options={'attn_mode': mode}, token_masks=table, token_mask_row=override, token_logprob=True)
    u = np.random.default_rng(12).random((steps, 1, 8)).astype(np.float32)
    if sampled:
        kw.update(sample_k=k, sample_uniforms=u, sample_logprob=True)
    kept = _engine(c, [c['scene']], store_logits=True, **kw)
    o = kept.outputs()[0]
    if mode == 1:
        bare = _engine(c, [c['scene']], **kw)
        assert bare.logits is None and bare.logits_scratch is None, 'the fused route keeps no logits in memory'
        for key in ('next_token_idx', 'next_state_idx', 'next_token_logprob') + (('next_token_sample_logprob',) if sampled else ()):
            assert np.array_equal(bare.outputs()[0][key], o[key]), key
    types = kept.atype.cpu().numpy()[0]
    A = o['next_token_idx'].shape[0]
    sets = [1 if r == 5 else table.type_sets[types[r]] for r in range(A)]
    allowed = torch.from_numpy(np.stack([table.allowed[s_] for s_ in sets]))              # [A][n]
    lg = torch.from_numpy(np.asarray(o['logits']))                                        # [steps][A][n]
    ml = lg.masked_fill(~allowed[None], float('-inf')).reshape(steps * A, -1).contiguous()
    if sampled:
        uu = torch.from_numpy(np.ascontiguousarray(u[:, 0, :A].reshape(-1)))
        want, wslp = torch.ops.infgen_hip.sample_topk(ml.cuda(), k, uu.cuda(), True)
        want, wslp = want.cpu().numpy().reshape(steps, A).T, wslp.cpu().numpy().reshape(steps, A).T
    else:
        want = _first_max(ml).numpy().reshape(steps, A).T
    live = o['next_token_logprob_mask'][:, hc:hc + steps]
    got = o['next_token_idx'][:, hc:hc + steps]
    assert live.sum() > 20 and np.array_equal(got[live], want[live]), 'tokens differ from the step-wise restatement'
    if sampled:
        assert np.array_equal(o['next_token_sample_logprob'][:, hc:hc + steps][live], wslp[live])
    # token_logprob stays the model's full, unmasked softmax
    full = torch.log_softmax(lg.double(), -1).gather(-1, torch.from_numpy(got.T.astype(np.int64)).clamp(min=0)[..., None])[..., 0].numpy().T
    err, bound = float(np.abs(o['next_token_logprob'][:, hc:hc + steps].astype(np.float64) - full)[live].max()), _bound(lg.numpy())
    print(f'mode={mode} sampled={sampled}: token_logprob error {err:.3e} (bound {bound:.3e})')
    assert err <= bound


def test_decoder_token_constraints_on_a_two_graph_batch():
    """inference(Batch) under token_constraints: each graph's rows equal the single-scene call (tokens and states exactly, poses to
    round-off: the bar of the batch-versus-single tests), and every emitted token lies in its type's set"""
    from infgen_amd import constraints, synth
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    cfg, hc = c['cfg'], c['cfg'].hist_columns
    dec = _decoder(cfg)
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    scenes = [synth.make_scene(9400 + i, a, m, cfg, vocab=c['vocab'], grid=c['grid']) for i, (a, m) in enumerate(((8, 128), (6, 100)))]
    table = constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0})
    try:
        free = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
        dec.token_constraints = table
        out = dec.inference(batch_datas([_to_data(sc, dev) for sc in scenes]))
        assert not torch.equal(out['next_token_idx'], free['next_token_idx']), 'the constraint changes the tokens'
        ptr = out['agent_ptr'].tolist()
        assert len(ptr) == 3
        for s, sc in enumerate(scenes):
            one = dec.inference(_to_data(sc, dev))
            rows = slice(ptr[s], ptr[s + 1])
            assert torch.equal(out['next_token_idx'][rows], one['next_token_idx']), s
            assert torch.equal(out['next_state_idx'][rows], one['next_state_idx']), s
            assert float((out['pos_a'][rows] - one['pos_a']).abs().max()) <= 1e-5
            types = np.asarray(sc['agent']['type']).reshape(-1)
            tok = one['next_token_idx'].cpu().numpy()[:, hc:]
            st = one['next_state_idx'].cpu().numpy()[:, hc:]
            for r in range(tok.shape[0]):
                t_ok = tok[r][(tok[r] >= 0) & (st[r] > 0)]
                assert table.allowed[table.type_sets[int(types[r])]][t_ok].all(), (s, r)
    finally:
        dec.token_constraints = None
