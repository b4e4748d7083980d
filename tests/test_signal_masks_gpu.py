"""Signal-aware decoding on the GPU: k_signal_mask and k_signal_records against the two restatements of
tests/signal_ref.py, and the engine plumbing on the fixtures c1_a8_m128 and ins_forced_a16_m256."""
import ctypes as C

import numpy as np
import pytest
import torch

import collision_ref as cr
import signal_ref as sr
from conftest import load_case
from rider_helpers import _emitted_in_sets, _make, _t, _weights

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4, 0x5A5A5A5A          # words in front of and behind every output (16 bytes: the outputs stay aligned)


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda:0')
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _call(case, t, first_new=None, **over):
    """infgen_signal_records + infgen_signal_mask through ctypes on a case of signal_ref.make_case, every output between guard words
    -> (rc, message, dict of outputs)"""
    from infgen_amd import _lib, constraints, torch_ops
    lib, P = _lib.load(), _lib.ptr
    S, A, T, K = case['S'], case['A'], case['T'], case['token_size']
    end = torch_ops.collision_end_poses(_t(case['vocab']))
    ins = dict(pos=_t(case['pos']), head=_t(case['head']), state=_t(case['state']), n_agents=_t(case['n_agents']), atype=_t(case['atype']),
               shape=_t(case['shape']), lines=_t(case['lines']), n_lines=_t(case['n_lines']), phase=_t(case['phase']), end=end)
    rec = torch_ops.signal_records(ins['lines'], ins['n_lines'])
    ins.update(rec=rec)
    if case['base_rows'] is not None:
        ins.update(mask_bits=_t(constraints.pack_bits(case['sets']).view(np.int32)), mask_row=_t(case['mask_row']))
    before = {k: v.clone() for k, v in ins.items()}
    words = K // 32
    gb, bits = _guarded(S * A * words, torch.int32)
    gc, count = _guarded(S * A, torch.int32)
    gi, info = _guarded(S * A * 4, torch.float32)
    a = dict(pos=P(ins['pos']), head=P(ins['head']), state=P(ins['state']), n_agents=P(ins['n_agents']),
             first_new=None if first_new is None else P(first_new), type=P(ins['atype']), shape=P(ins['shape']), S=S, A_cap=A, T=T, c=case['c'],
             end_pose=P(end), token_size=K, records=P(rec), phase=P(ins['phase']), n_phase=int(case['phase'].shape[1]), K=case['K'], t=t,
             copies=case['copies'], setback=sr.SETBACK, align=sr.ALIGN, types=(C.c_int * 3)(*sr.TYPES), mask_bits=P(ins.get('mask_bits')),
             mask_n_sets=4 if 'mask_bits' in ins else 0, mask_row=P(ins.get('mask_row')),
             mask_type=(C.c_int * 3)(0, 1, 2) if 'mask_bits' in ins else None, out_bits=P(bits), out_count=P(count), out_info=P(info),
             stream=None)
    a.update(over)
    rc = lib.infgen_signal_mask(*a.values())
    torch.cuda.synchronize()
    msg = lib.infgen_last_error().decode() if rc else ''
    assert _intact(gb, S * A * words) and _intact(gc, S * A) and _intact(gi, S * A * 4), 'guard words'
    assert all(torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)) for k, v in ins.items()), 'inputs unchanged'
    return rc, msg, dict(bits=bits.clone(), count=count.cpu().numpy(), info=info.view(S * A, 4).cpu().numpy(), rec=rec,
                         untouched=bool((bits == SENTINEL).all()) and bool((count == SENTINEL).all()))


def _judge(case, out, r32, r64, label):
    """the operator's output against the two restatements: bit for bit outside NEAR, counts, info"""
    K = case['token_size']
    got = cr.unpack(out['bits'].cpu().numpy(), K)
    near, ruled, base = r64['near'], r64['ruled'], r64['base']
    assert not r64['row_open'].any() and not r64['info_open'].any()
    sure = ruled & (out['count'] > 0)                                     # (a row that took the fallback holds base(i): judged below)
    differ = (got != r32['pre']) & ~near & sure[:, None]
    print(f'{label}: {int(ruled.sum())} ruled rows, {int(r64["governed"].sum())} governed, {int(near.sum())} near tokens, '
          f'{int((got != r32["allowed"]).sum())} bits differ from float32, {int((out["count"] == 0).sum())} fallbacks')
    assert not differ.any(), np.argwhere(differ)[:10]
    for r in range(case['S'] * case['A']):
        if not ruled[r]:
            assert np.array_equal(got[r], base[r]) and out['count'][r] == base[r].sum(), r
        elif out['count'][r] > 0:
            assert out['count'][r] == got[r].sum() and abs(int(out['count'][r]) - int(r32['count'][r])) <= int(near[r].sum()), r
        else:
            assert np.array_equal(got[r], base[r]) and not (r32['pre'][r] & ~near[r]).any(), r
    # info: line and flag exact, gap within 8 ulp of the magnitudes that enter
    info, want = out['info'], r64['info']
    assert np.array_equal(info[:, 1:], want[:, 1:]) and np.array_equal(info[:, 1:], r32['info'][:, 1:])
    tol = 8 * 2.0 ** -23 * r64['scale']
    err = np.abs(info[:, 0].astype(np.float64) - want[:, 0])
    if (want[:, 1] >= 0).any():
        print('  gap: largest error / tolerance', float((err / np.maximum(tol, 1e-30))[want[:, 1] >= 0].max()))
    assert (err <= tol).all(), (err.max(), np.argmax(err - tol))


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize('with_base', [False, True], ids=['all', 'base'])
@pytest.mark.parametrize('name', list(sr.CASES))
def test_operator_equals_the_float32_restatement_outside_near_tokens(name, with_base):
    case = sr.make_case(name, with_base)
    outs = {}
    for t in sr.STEPS:
        rc, msg, out = _call(case, t)
        assert rc == 0, msg
        _judge(case, out, sr.case_reference(name, with_base, t, False), sr.case_reference(name, with_base, t, True), f'{name} t {t}')
        outs[t] = out
    rc, msg, again = _call(case, 0)
    assert rc == 0 and torch.equal(outs[0]['bits'], again['bits']) and np.array_equal(outs[0]['count'], again['count'])
    assert np.array_equal(outs[0]['info'], again['info'])
    assert torch.equal(outs[4]['bits'], outs[1]['bits']) and np.array_equal(outs[4]['info'], outs[1]['info']), 'the phase table is cyclic'
    assert not torch.equal(outs[0]['bits'], outs[2]['bits'])
    flags = outs[0]['info'][:, 2]
    assert (flags == 2).any() and (flags == 1).any() and (flags == 0).any()
    if with_base:
        assert outs[0]['count'][sr.FALLBACK_ROW] == 0, 'the fallback row takes the fallback'


def test_first_new_keeps_appended_rows_out():
    name = 'k64'
    case = sr.make_case(name, False)
    rc, msg, out = _call(case, 0, first_new=_t(case['first_new']))
    assert rc == 0, msg
    r32, r64 = sr.case_reference(name, False, 0, False, True), sr.case_reference(name, False, 0, True, True)
    _judge(case, out, r32, r64, 'first_new')
    got = cr.unpack(out['bits'].cpu().numpy(), 64)
    beyond = np.zeros((sr.S_CASE, sr.A_CASE), bool)
    beyond[3, 3:] = beyond[5, 4:] = True
    assert got[beyond.reshape(-1)].all() and (out['info'][beyond.reshape(-1), 2] == 0).all()
    assert sr.case_reference(name, False, 0, True)['governed'].reshape(sr.S_CASE, sr.A_CASE)[3, 3:].any(), 'they would have been governed'


def test_records_equal_the_restatement():
    from infgen_amd import torch_ops
    case = sr.make_case('k64', False)
    want = sr.records(case['lines'], case['n_lines'], np.float32)
    rec = torch_ops.signal_records(_t(case['lines']), _t(case['n_lines'])).cpu().numpy()
    assert np.array_equal(rec[..., 4:].view(np.int32), want[..., 4:].view(np.int32)), 'half and the zeros, bit for bit'
    assert np.array_equal(rec[..., :2].view(np.int32), want[..., :2].view(np.int32)), 'the midpoint, bit for bit'
    assert np.allclose(rec[..., 2:4], want[..., 2:4], rtol=0, atol=2.0 ** -23)
    dead = want[..., 4] < 0
    assert dead.sum() == 64 + 63 + 3 and np.array_equal(rec[dead], np.tile(sr.DEAD.astype(np.float32), (int(dead.sum()), 1)))


def test_every_refusal_returns_an_error_and_launches_nothing():
    case = sr.make_case('k64', False)
    nan, inf = float('nan'), float('inf')
    odd = torch.zeros(64, device='cuda:0')
    bad = [dict(setback=-1.0), dict(setback=nan), dict(setback=inf), dict(align=-1.5), dict(align=1.5), dict(align=nan), dict(K=0), dict(K=65),
           dict(n_phase=0), dict(t=-1), dict(copies=0), dict(copies=4), dict(token_size=48), dict(token_size=4128), dict(A_cap=1025),
           dict(records=None), dict(phase=None), dict(end_pose=None), dict(shape=None), dict(types=None), dict(out_bits=None),
           dict(records=odd.data_ptr() + 4), dict(out_info=odd.data_ptr() + 8), dict(c=6), dict(c=-1)]
    for over in bad:
        over = dict(over)
        rc, msg, out = _call(case, over.pop('t', 0), **over)
        assert rc != 0 and msg.startswith('infgen_signal_mask: signal mask:'), (over, rc, msg)
        assert out['untouched'] or 'out_bits' in over, over
    from infgen_amd import _lib
    lib = _lib.load()
    assert lib.infgen_signal_records(None, None, 1, 1, None, None) != 0
    ln, n, o = (torch.zeros(64, device='cuda:0') for _ in range(3))
    for K in (0, 65):
        assert lib.infgen_signal_records(ln.data_ptr(), n.data_ptr(), 1, K, o.data_ptr(), None) != 0
    assert lib.infgen_token_mask_signal(0, None, None, None, None, None, None, 1, 1, 1, 0.0, 0.0, None, None, None) != 0


# ------------------------------------------------------------------------------------------ engine level
ALL_TYPES = ('veh', 'ped', 'cyc')


def _lines_ahead(c, w, gap=0.3, half=3.0, copies=1):
    """one stop line per initial row of the fixture, `gap` metres (behind the setback) in front of its bumper at the last history
    column and across its heading; -> lines [1][K][4], and the engine without signals they were read from (after its prologue)"""
    free = _make(c, w, options={'attn_mode': 1})
    free.prologue()
    hc = c['cfg'].hist_columns
    n = int(free.n_agents[0])
    p, h = free.pos[0, hc - 1, :n].cpu().numpy().astype(np.float64), free.head[0, hc - 1, :n].cpu().numpy().astype(np.float64)
    hl = 0.5 * free._shape10[0, :n, 0].cpu().numpy().astype(np.float64)
    lines = np.zeros((1, n, 4), np.float32)
    for i in range(n):
        mid = p[i] + (hl[i] + gap + 0.5) * np.array([np.cos(h[i]), np.sin(h[i])])
        lines[0, i] = sr._line(mid, h[i], half)
    return lines, free


def _signal_op(eng, col, t, base=None, signalled=None, **kw):
    """the operator applied to column col of the engine's state at step t, with the tables of `signalled` (default: the engine's own)"""
    from infgen_amd import torch_ops  # noqa: F401
    signalled = signalled or eng
    conf, k = signalled.obey_signals, signalled._signal
    extra = {} if base is None else dict(mask_bits=base[0], mask_row=base[1])
    return torch.ops.infgen_hip.signal_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, k['shape'].view(eng.S, eng.A_cap, 3), col,
                                            signalled._coll_end, k['records'], k['phase'], t, eng.copies, conf['setback'], conf['align'],
                                            list(conf['types']), **extra, **kw)


def _stepwise(eng, steps, each=None):
    eng.prologue()
    eng._refresh_opts(groups=True)
    for t in range(steps):
        eng.step(t)
        if each is not None:
            each(t)


def _same_outputs(x, y):
    assert set(x) == set(y)
    for key in x:
        p, q = np.asarray(x[key]), np.asarray(y[key])
        assert p.shape == q.shape and np.array_equal(p, q, equal_nan=p.dtype.kind == 'f'), key


def _crossings(eng, col, rec, closed, setback=0.5, align=0.5, rows=None):
    """rows (s, i) whose front point went across a closed line that governed them, between the stored columns col and col + 1: float64
    on the stored poses, with a millimetre of slack on every comparison"""
    pos, head, st = (getattr(eng, k)[:, col:col + 2].cpu().numpy().astype(np.float64) for k in ('pos', 'head', 'state'))
    shp = eng._shape10.cpu().numpy().astype(np.float64)
    out = []
    for s in range(eng.S):
        for i in range(int(eng.n_agents[s])):
            if st[s, 0, i] == 0 or st[s, 1, i] == 0 or (rows is not None and not rows[s, i]):
                continue
            hla, hwa = 0.5 * shp[s, i, 0], 0.5 * shp[s, i, 1]
            f = [pos[s, k, i] + hla * np.array([np.cos(head[s, k, i]), np.sin(head[s, k, i])]) for k in (0, 1)]
            fwd = np.array([np.cos(head[s, 0, i]), np.sin(head[s, 0, i])])
            for j in np.flatnonzero(closed & (rec[:, 4] >= 0)):
                m, nrm = rec[j, :2], rec[j, 2:4]
                tau = np.array([nrm[1], -nrm[0]])
                g = [(fk - m) @ nrm + setback for fk in f]
                lat = [(fk - m) @ tau for fk in f]
                if fwd @ nrm >= align + 1e-3 and g[0] <= -1e-3 and g[1] > 1e-3:
                    x = (lat[0] * g[1] - lat[1] * g[0]) / (g[1] - g[0])
                    if abs(x) <= rec[j, 4] + hwa - 1e-3:
                        out.append((s, i, int(j)))
    return out


def test_tokens_stay_in_their_sets_and_no_front_point_crosses_a_closed_line():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps, K = cfg.hist_columns, cfg.num_decode_steps, cfg.token_size
    lines, free = _lines_ahead(c, w)
    phase = np.ones((1, 1, lines.shape[1]), np.uint8)
    eng = _make(c, w, obey_signals=dict(lines=lines, phase=phase, types=ALL_TYPES), options={'attn_mode': 1})
    rec = sr.records(lines, [lines.shape[1]], np.float32)[0].astype(np.float64)
    closed = np.ones(lines.shape[1], bool)
    tally = dict(checked=0, bitten=0, crossed=0, governed=0)

    def each(t):
        col = hc - 1 + t
        bits, count, info = _signal_op(eng, col, t)
        assert torch.equal(eng.signal_bits, bits) and torch.equal(eng.signal_allowed, count) and torch.equal(eng.signal_info, info), t
        tally['checked'] += _emitted_in_sets(eng, col, bits)
        cnt = count.view(eng.S, eng.A_cap).cpu().numpy()
        tally['bitten'] += int(((cnt > 0) & (cnt < K)).sum())
        tally['governed'] += int((info[:, 1] >= 0).sum())
        ruled = (info.view(eng.S, eng.A_cap, 4)[..., 2] > 0).cpu().numpy() & (cnt > 0)
        tally['crossed'] += len(_crossings(eng, col, rec, closed, rows=ruled))
    _stepwise(eng, steps, each)
    fcross = [0]
    _stepwise(free, steps, lambda t: fcross.__setitem__(0, fcross[0] + len(_crossings(free, hc - 1 + t, rec, closed))))
    print(tally, 'the rollout without signals crosses', fcross[0])
    assert tally['checked'] > 20 and tally['bitten'] > 0 and tally['governed'] > 0
    assert fcross[0] > 0, 'the rollout without signals crosses some line: the check below shows something'
    assert tally['crossed'] == 0


def test_an_all_open_phase_table_is_the_engine_without_signals():
    c = load_case('c1_a8_m128')
    w = _weights(c)
    kw = dict(token_logprob=True, store_logits=True)
    a = _make(c, w, **kw)
    a.rollout()
    assert a._signal is None and a.signal_bits is None and a._ctx.token_mask == 0, 'no buffers, no handle'
    lines, _ = _lines_ahead(c, w)
    b = _make(c, w, obey_signals=dict(lines=lines, phase=np.zeros((1, 3, lines.shape[1]), np.uint8), types=ALL_TYPES), **kw)
    b.rollout()
    assert b._ctx.token_mask >= 1 and int((b.signal_info[:, 2] == 1).sum()) > 0 and int((b.signal_info[:, 1] >= 0).sum()) == 0
    _same_outputs(a.outputs()[0], b.outputs()[0])
    b.reload([c['scene']], obey_signals=False)
    b.rollout()
    assert b.signal_bits is None
    _same_outputs(a.outputs()[0], b.outputs()[0])


def test_collision_road_signal_and_route_masks_compose_in_that_order_and_detach():
    from infgen_amd import constraints
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, K = cfg.hist_columns, cfg.token_size
    routes, n = constraints.routes_from_logged(c['scene'], start=hc - 1)
    lines, _ = _lines_ahead(c, w, gap=1.0)
    sig = dict(lines=lines, phase=np.ones((1, 1, lines.shape[1]), np.uint8), types=ALL_TYPES)
    rt = dict(routes=routes, n_points=n, corridor=1.5, pace=0.5)
    eng = _make(c, w, avoid_collisions=True, stay_on_road=dict(margin=0.5, detail=5), obey_signals=sig, follow_routes=rt,
                options={'attn_mode': 1})
    bitten = [0, 0]

    def each(t):
        col = hc - 1 + t
        bits, count, info = _signal_op(eng, col, t, base=(eng.road_bits, eng._road['ident']))
        assert torch.equal(eng.signal_bits, bits) and torch.equal(eng.signal_allowed, count) and torch.equal(eng.signal_info, info), t
        road, sg = cr.unpack(eng.road_bits.cpu().numpy(), K), cr.unpack(bits.cpu().numpy(), K)
        cnt = count.cpu().numpy()
        assert not (sg & ~road)[cnt > 0].any(), 'a subset of the road stage wherever the count is > 0'
        assert np.array_equal(sg[cnt == 0], road[cnt == 0]), 'the fallback returns the road stage\'s set'
        bitten[0] += int(((cnt > 0) & (cnt < road.sum(axis=1))).sum())
        # the route stage refines the signal stage's bits
        k, conf = eng._route, eng.follow_routes
        rbits, rcount, _ = torch.ops.infgen_hip.route_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, k['shape'].view(eng.S, eng.A_cap, 3),
                                                           col, eng._coll_end, k['records'], k['total'], eng.copies, conf['corridor'],
                                                           conf['back'], conf['pace'], conf['finish'], list(conf['types']),
                                                           mask_bits=eng.signal_bits, mask_row=eng._signal['ident'])
        assert torch.equal(eng.route_bits, rbits) and torch.equal(eng.route_allowed, rcount), t
        rtc = rcount.cpu().numpy()
        rset = cr.unpack(rbits.cpu().numpy(), K)
        assert not (rset & ~sg)[rtc > 0].any() and np.array_equal(rset[rtc == 0], sg[rtc == 0]), 'route falls back on the signal set'
        bitten[1] += int(((rtc > 0) & (rtc < sg.sum(axis=1))).sum())
        _emitted_in_sets(eng, col, rbits)
    _stepwise(eng, 4, each)
    assert bitten[0] > 0 and bitten[1] > 0
    # detached: the route stage reads the road rider's bits again
    eng.reload([c['scene']], obey_signals=False)
    three = _make(c, w, avoid_collisions=True, stay_on_road=dict(margin=0.5, detail=5), follow_routes=rt, options={'attn_mode': 1})
    eng.rollout()
    three.rollout()
    _same_outputs(eng.outputs()[0], three.outputs()[0])
    assert torch.equal(eng.route_bits, three.route_bits)


def test_set_signals_between_steps_and_graph_replay():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    lines, _ = _lines_ahead(c, w)
    Kl = lines.shape[1]
    red, green = np.ones((1, 2, Kl), np.uint8), np.zeros((1, 2, Kl), np.uint8)
    green[0, 1, ::2] = 1
    kw = dict(options={'attn_mode': 1}, obey_signals=dict(lines=lines, phase=red, types=ALL_TYPES), token_logprob=True)
    g = _make(c, w, use_graph=True, **kw)
    g.rollout()
    g.rollout()                       # (the first rollout runs eagerly, the second captures and replays)
    assert g._graph is not None
    e = _make(c, w, **kw)
    _stepwise(e, steps)
    _same_outputs(g.outputs()[0], e.outputs()[0])
    assert torch.equal(g.signal_bits, e.signal_bits) and torch.equal(g.signal_info, e.signal_info)
    # a new phase table drops the captured graph, as set_routes does; the next rollout captures again and the new table rules it
    g.set_signals(phase=green)
    assert g._graph is None and torch.equal(g._signal['phase'].cpu(), torch.from_numpy(green))
    g.rollout()
    assert g._graph is not None, 'captured again'
    e_green = _make(c, w, **dict(kw, obey_signals=dict(lines=lines, phase=green, types=ALL_TYPES)))
    _stepwise(e_green, steps)
    _same_outputs(g.outputs()[0], e_green.outputs()[0])
    assert torch.equal(g.signal_bits, e_green.signal_bits) and torch.equal(g.signal_info, e_green.signal_info)
    assert not torch.equal(e_green.token, e.token), 'the new table changes the rollout'
    # a reload that brings tables of the same extents drops the graph too: no graph is replayed over rewritten tables
    g.reload([c['scene']], obey_signals=dict(lines=lines, phase=red, types=ALL_TYPES))
    assert g._graph is None
    # a switch after step 2 of a stepwise rollout: from step 3 on the sets are those of the new table
    e2 = _make(c, w, **kw)

    def each(t):
        if t == 2:
            e2.set_signals(phase=green)
        if t >= 3:
            bits, count, info = _signal_op(e2, hc - 1 + t, t)
            assert torch.equal(e2.signal_bits, bits) and torch.equal(e2.signal_info, info)
    _stepwise(e2, steps, each)
    assert torch.equal(e2._signal['phase'].cpu(), torch.from_numpy(green))
    assert torch.equal(e2.token[:, :hc + 3], e.token[:, :hc + 3]) and not torch.equal(e2.token, e.token)
    # new lines rebuild the records in place; other extents take new buffers
    moved = lines + np.float32(0.25)
    g.set_signals(lines=moved)
    assert np.array_equal(g._signal['records'].cpu().numpy()[0], sr.records(moved, [Kl], np.float32)[0])
    g.set_signals(phase=np.ones((1, 3, Kl), np.uint8))
    assert g._graph is None and g._signal['n_phase'] == 3
    with pytest.raises(ValueError):
        _make(c, w).set_signals(phase=red)


def test_insertion_engine_appended_rows_keep_their_base_in_their_first_step():
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    w = _weights(c, cfg)
    probe = _make(c, w, force_enter=True)
    probe.prologue()
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    n = int(probe.n_agents[0])
    p, h = probe.pos[0, hc - 1, :n].cpu().numpy().astype(np.float64), probe.head[0, hc - 1, :n].cpu().numpy().astype(np.float64)
    lines = np.stack([sr._line(p[i] + 4.0 * np.array([np.cos(h[i]), np.sin(h[i])]), h[i], 30.0) for i in range(n)])[None].astype(np.float32)
    eng = _make(c, w, force_enter=True, obey_signals=dict(lines=lines, phase=np.ones((1, 1, n), np.uint8), types=ALL_TYPES))
    eng.rollout()
    assert eng.outputs()[0]['num_inserted'] > 0
    first = eng.ins['first_new']
    bits, count, info = _signal_op(eng, hc - 1 + steps - 1, steps - 1, first_new=first)
    assert torch.equal(eng.signal_bits, bits) and torch.equal(eng.signal_allowed, count) and torch.equal(eng.signal_info, info)
    cols = torch.arange(eng.A_cap, device='cuda:0')[None]
    new = (cols >= first[:, None]).reshape(-1)
    assert (info[new, 2] == 0).all() and (count[new] == cfg.token_size).all(), 'rows from first_new on keep their base'
    appended = (cols >= n) & (cols < first[:, None])
    assert bool(appended.any()) and bool((info.view(eng.S, eng.A_cap, 4)[..., 2][appended & (eng.state[:, hc - 1 + steps - 1] != 0)] > 0).all()), \
        'rows appended in earlier steps are ruled'


# ------------------------------------------------------------------------------------------ branching, snapshots, sessions, the module
def test_branching_and_snapshots_need_no_signal_state():
    """the scheme of tests/test_branching_gpu.py with signals on: a branched slot equals the rollout that had that history all
    along; a restore followed by set_signals continues under the new table, as an engine that was given it at that step"""
    from test_branching_gpu import _branched_against_control, _full, _sampled, _uniforms
    from test_replay_gpu import _case, _same
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    tb = steps // 2
    lines, _ = _lines_ahead(c, _weights(c))
    Kl = lines.shape[1]
    cyc = np.ones((1, 4, Kl), np.uint8)
    cyc[0, 2:] = 0
    other = 1 - cyc
    conf = dict(lines=lines, phase=cyc, types=ALL_TYPES)
    E = _branched_against_control(c, tb, obey_signals=conf)
    assert int((E.signal_info[:, 2] >= 1).sum()) > 0
    u = _uniforms(c)
    S_ = _sampled(c, u, obey_signals=conf)
    S_.run(0, tb)
    snap = S_.snapshot(tb)
    S_.run(tb, steps)
    first = _full(S_)
    S_.restore(snap)
    S_.set_signals(phase=other)
    S_.run(tb, steps)
    again = _full(S_)
    ctl = _sampled(c, u, obey_signals=conf)
    ctl.run(0, tb)
    ctl.set_signals(phase=other)
    ctl.run(tb, steps)
    want = _full(ctl)
    _same(again, want, 'restored, then under the new phase table')
    assert torch.equal(S_.signal_bits, ctl.signal_bits) and torch.equal(S_.signal_info, ctl.signal_info)
    assert not torch.equal(again['token'], first['token']), 'the new table changes the rollout'


def test_session_signal_is_the_operators_and_set_signals_takes_hold():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    w = _weights(c)
    lines, _ = _lines_ahead(c, w)
    Kl = lines.shape[1]
    mask = np.zeros(8, bool)
    mask[0] = True
    eng = _make(c, w, options={'attn_mode': 1}, replay=[mask],
                obey_signals=dict(lines=lines, phase=np.ones((1, 1, Kl), np.uint8), types=ALL_TYPES))
    plan = eng.teacher_token.clone()
    ses = eng.session()
    governed = [0, 0]
    for t in range(steps):
        if t == 4:
            ses.set_signals(phase=np.zeros((1, 1, Kl), np.uint8))
        ses.command(tokens=plan[:, hc + t].clamp(min=0))
        ses.advance()
        bits, count, info = _signal_op(eng, hc - 1 + t, t)
        obs = ses.observe()
        assert torch.equal(obs['signal'].reshape(-1, 4), info) and torch.equal(obs['allowed_tokens'].reshape(-1), count), t
        assert torch.equal(eng.signal_bits, bits)
        _emitted_in_sets(eng, hc - 1 + t, bits, skip=eng.replay_row.bool().cpu().numpy())
        governed[t >= 4] += int((info[:, 1] >= 0).sum())
    assert governed[0] > 0 and governed[1] == 0, 'closed until the planner opens every line'


def test_decoder_passes_the_signals_to_every_entry():
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    dec = _decoder(cfg)
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    scene = c['scene']
    lines, _ = _lines_ahead(c, _weights(c))
    Kl = lines.shape[1]
    free = dec.inference(_to_data(scene, dev))
    n0 = len(dec._engines)
    conf = dict(lines=lines, phase=np.ones((1, 1, Kl), np.uint8), types=ALL_TYPES)
    dec.obey_signals = conf
    one = dec.inference(_to_data(scene, dev))
    assert len(dec._engines) == n0 + 1, 'a call with signals does not reuse the engine without them'
    eng = _make(c, _weights(c), obey_signals=conf)
    eng.rollout()
    want = torch.from_numpy(np.asarray(eng.outputs()[0]['next_token_idx'])).to(dev)
    assert torch.equal(one['next_token_idx'], want) and not torch.equal(one['next_token_idx'], free['next_token_idx'])
    # copies: a scene's lines apply to each of its copies; a batch: one table per scene
    rolls = dec.inference_rollouts(_to_data(scene, dev), 2)
    assert all(torch.equal(r['next_token_idx'], want) for r in rolls)
    dec.obey_signals = dict(conf, lines=np.concatenate([lines, lines]), phase=np.ones((2, 1, Kl), np.uint8))
    both = dec.inference_batch([_to_data(scene, dev), _to_data(scene, dev)])
    assert all(torch.equal(r['next_token_idx'], want) for r in both)
    dec.obey_signals = conf
    ses = dec.closed_loop(_to_data(scene, dev), controlled='ego')
    assert ses.eng.obey_signals is not None and ses.observe()['signal'].shape == (1, ses.eng.A_cap, 4)
    ses.set_signals(phase=np.zeros((1, 1, Kl), np.uint8))
    dec.obey_signals = dict(conf, lines=np.concatenate([lines, lines]), phase=np.ones((2, 1, Kl), np.uint8))
    with pytest.raises(ValueError, match='scenes'):
        dec.inference(_to_data(scene, dev))
