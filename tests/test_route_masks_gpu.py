"""Route-following decoding on the GPU: k_route_mask and k_route_records against the two restatements of
tests/route_ref.py, and the engine plumbing on the fixtures c1_a8_m128 and ins_forced_a16_m256."""
import ctypes as C

import numpy as np
import pytest
import torch

import collision_ref as cr
import route_ref as rr
from conftest import load_case
from rider_helpers import _emitted_in_sets, _make, _t, _weights

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4, 0x5A5A5A5A          # words in front of and behind every output (16 bytes: the outputs stay aligned)


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda:0')
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _call(case, pace, first_new=None, **over):
    """infgen_route_records + infgen_route_mask through ctypes on a case of route_ref.make_case, every output between guard words
    -> (rc, message, dict of outputs)"""
    from infgen_amd import _lib, constraints, torch_ops
    lib, P = _lib.load(), _lib.ptr
    S, A, T, K, Pn = case['S'], case['A'], case['T'], case['token_size'], case['P']
    end = torch_ops.collision_end_poses(_t(case['vocab']))
    ins = dict(pos=_t(case['pos']), head=_t(case['head']), state=_t(case['state']), n_agents=_t(case['n_agents']), atype=_t(case['atype']),
               shape=_t(case['shape']), routes=_t(case['routes']), n_points=_t(case['n_points']), end=end)
    rec, total = torch_ops.route_records(ins['routes'], ins['n_points'])
    ins.update(rec=rec, total=total)
    if case['base_rows'] is not None:
        ins.update(mask_bits=_t(constraints.pack_bits(case['sets']).view(np.int32)), mask_row=_t(case['mask_row']))
    before = {k: v.clone() for k, v in ins.items()}
    words = K // 32
    gb, bits = _guarded(S * A * words, torch.int32)
    gc, count = _guarded(S * A, torch.int32)
    gp, prog = _guarded(S * A * 4, torch.float32)
    a = dict(pos=P(ins['pos']), head=P(ins['head']), state=P(ins['state']), n_agents=P(ins['n_agents']),
             first_new=None if first_new is None else P(first_new), type=P(ins['atype']), shape=P(ins['shape']), S=S, A_cap=A, T=T, c=case['c'],
             end_pose=P(end), token_size=K, records=P(rec), total=P(total), P=Pn, copies=case['copies'], corridor=rr.CORRIDOR, back=rr.BACK,
             pace=pace, finish=rr.FINISH, types=(C.c_int * 3)(*rr.TYPES), mask_bits=P(ins.get('mask_bits')),
             mask_n_sets=4 if 'mask_bits' in ins else 0, mask_row=P(ins.get('mask_row')),
             mask_type=(C.c_int * 3)(0, 1, 2) if 'mask_bits' in ins else None, out_bits=P(bits), out_count=P(count), out_progress=P(prog),
             stream=None)
    a.update(over)
    rc = lib.infgen_route_mask(*a.values())
    torch.cuda.synchronize()
    msg = lib.infgen_last_error().decode() if rc else ''
    assert _intact(gb, S * A * words) and _intact(gc, S * A) and _intact(gp, S * A * 4), 'guard words'
    assert all(torch.equal(v.view(torch.int32), before[k].view(torch.int32)) for k, v in ins.items()), 'inputs unchanged'
    return rc, msg, dict(bits=bits.clone(), count=count.cpu().numpy(), progress=prog.view(S * A, 4).cpu().numpy(), rec=rec, total=total,
                         untouched=bool((bits == SENTINEL).all()) and bool((count == SENTINEL).all()))


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize('with_base', [False, True], ids=['all', 'base'])
@pytest.mark.parametrize('name', list(rr.CASES))
def test_operator_equals_the_float32_restatement_outside_near_tokens(name, with_base):
    case = rr.make_case(name, with_base)
    K = case['token_size']
    for pace in rr.PACES:
        r32, r64 = rr.case_reference(name, with_base, pace, False), rr.case_reference(name, with_base, pace, True)
        rc, msg, out = _call(case, pace)
        assert rc == 0, msg
        got = cr.unpack(out['bits'].cpu().numpy(), K)
        near, ruled, base = r64['near'], r64['ruled'], r64['base']
        assert not r64['row_open'].any()
        pre = np.where((out['count'] > 0)[:, None], got, False)      # (a row that took the fallback holds base(i): judged below)
        sure = ruled & (out['count'] > 0)
        differ = (got != r32['pre']) & ~near & sure[:, None]
        print(f'{name} pace {pace}: {int(ruled.sum())} ruled rows, {int(near.sum())} near tokens, {int((got != r32["allowed"]).sum())} bits '
              f'differ from float32, {int((out["count"] == 0).sum())} fallbacks')
        assert not differ.any(), np.argwhere(differ)[:10]
        for r in range(case['S'] * case['A']):
            if not ruled[r]:
                assert np.array_equal(got[r], base[r]) and out['count'][r] == base[r].sum(), r
            elif out['count'][r] > 0:
                assert out['count'][r] == got[r].sum() and abs(int(out['count'][r]) - int(r32['count'][r])) <= int(near[r].sum()), r
            else:
                assert np.array_equal(got[r], base[r]) and not (r32['pre'][r] & ~near[r]).any(), r
        # progress: flags exact, s0 and d0 within 8 ulp of the magnitudes that enter
        pr, want = out['progress'], r64['progress']
        assert np.array_equal(pr[:, 3], want[:, 3]) and np.array_equal(pr[:, 3], r32['progress'][:, 3])
        tol = 8 * 2.0 ** -23 * (r64['scale'] + want[:, 2])
        err = np.abs(pr[:, :3].astype(np.float64) - want[:, :3]).max(axis=1)
        print('  progress: largest error / tolerance', float((err / np.maximum(tol, 1e-30))[want[:, 3] > 0].max()))
        assert (err <= tol).all(), (err.max(), np.argmax(err - tol))
        rc, msg, again = _call(case, pace)
        assert rc == 0 and torch.equal(out['bits'], again['bits']) and np.array_equal(out['count'], again['count'])
        assert np.array_equal(out['progress'], again['progress'])
    flags = rr.case_reference(name, with_base, 0.0, True)['progress'][:, 3]
    assert (flags == 2).any() and (flags == 1).any() and (flags == 0).any()
    if with_base and name != 'k96_a5_p3':
        assert (out['count'] == 0).any(), 'some row takes the fallback'


def test_first_new_keeps_appended_rows_out():
    name = 'k64_a32_p32'
    case = rr.make_case(name, False)
    rc, msg, out = _call(case, 0.5, first_new=_t(case['first_new']))
    assert rc == 0, msg
    r32, r64 = rr.case_reference(name, False, 0.5, False, True), rr.case_reference(name, False, 0.5, True, True)
    got = cr.unpack(out['bits'].cpu().numpy(), 64)
    assert not ((got != r32['allowed']) & ~r64['near']).any()
    beyond = np.zeros((4, 32), bool)
    beyond[2:, 4:] = True
    assert got[beyond.reshape(-1)].all() and (out['progress'][beyond.reshape(-1), 3] == 0).all()
    assert r64['ruled'].reshape(4, 32)[:2, 4:].any()


def test_records_equal_the_in_order_float32_sum():
    from infgen_amd import torch_ops
    for name in ('k64_a5_p2', 'k96_a5_p3', 'k2048_a32_p32'):
        case = rr.make_case(name, False)
        want, total = rr.records(case['routes'], case['n_points'], np.float32)
        rec, tot = torch_ops.route_records(_t(case['routes']), _t(case['n_points']))
        rec, tot = rec.cpu().numpy(), tot.cpu().numpy()
        assert np.array_equal(tot.view(np.int32), total.view(np.int32)), 'total, bit for bit'
        assert np.array_equal(rec[..., 4:].view(np.int32), want[..., 4:].view(np.int32)), 'L and cum, bit for bit'
        assert np.array_equal(rec[..., :2], want[..., :2]), 'p0: exact copies'
        assert np.allclose(rec[..., 2:4], want[..., 2:4], rtol=0, atol=2.0 ** -23)
        dead = want[..., 4] < 0
        assert np.array_equal(rec[dead], np.tile(rr.DEAD.astype(np.float32), (int(dead.sum()), 1)))
    assert dead.any() and (total == 0).any()


def test_every_refusal_returns_an_error_and_launches_nothing():
    case = rr.make_case('k64_a5_p2', False)
    nan, inf = float('nan'), float('inf')
    odd = torch.zeros(64, device='cuda:0')
    bad = [dict(corridor=-1.0), dict(corridor=nan), dict(back=-0.5), dict(back=inf), dict(finish=-1.0), dict(finish=nan), dict(pace=-0.1),
           dict(pace=1.5), dict(pace=nan), dict(P=1), dict(P=33), dict(copies=0), dict(copies=3), dict(token_size=48), dict(token_size=4128),
           dict(A_cap=1025), dict(records=None), dict(total=None), dict(end_pose=None), dict(shape=None), dict(types=None), dict(out_bits=None),
           dict(records=odd.data_ptr() + 4), dict(out_progress=odd.data_ptr() + 8), dict(c=6), dict(c=-1)]
    for over in bad:
        over = dict(over)
        rc, msg, out = _call(case, over.pop('pace', 0.0), **over)
        assert rc != 0 and msg.startswith('infgen_route_mask: route mask:'), (over, rc, msg)
        assert out['untouched'] or 'out_bits' in over, over
    from infgen_amd import _lib
    lib = _lib.load()
    assert lib.infgen_route_records(None, None, 1, 1, 2, None, None, None) != 0
    r, n, o, t = (torch.zeros(64, device='cuda:0') for _ in range(4))
    for P in (1, 33):
        assert lib.infgen_route_records(r.data_ptr(), n.data_ptr(), 1, 1, P, o.data_ptr(), t.data_ptr(), None) != 0
    assert lib.infgen_token_mask_route(0, None, None, None, None, None, None, 2, 1, 0.0, 0.0, 0.0, 0.0, None, None, None) != 0


# ------------------------------------------------------------------------------------------ engine level
def _routes(c, shift=0.0, start=None):
    """the fixture's logged positions as routes, optionally moved `shift` metres to the left of each agent's first segment"""
    from infgen_amd import constraints
    routes, n = constraints.routes_from_logged(c['scene'], start=c['cfg'].hist_columns - 1 if start is None else start)
    if shift:
        d = routes[:, :, 1] - routes[:, :, 0]
        L = np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9)
        routes = routes + (shift * np.stack([-d[..., 1], d[..., 0]], -1) / L)[:, :, None].astype(np.float32)
    return routes.astype(np.float32), n


def _route_op(eng, col, base=None, routed=None, **kw):
    """the operator applied to column col of the engine's state, with the tables of `routed` (default: the engine's own)"""
    from infgen_amd import torch_ops  # noqa: F401
    routed = routed or eng
    conf, k = routed.follow_routes, routed._route
    extra = {} if base is None else dict(mask_bits=base[0], mask_row=base[1])
    return torch.ops.infgen_hip.route_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, k['shape'].view(eng.S, eng.A_cap, 3), col,
                                           routed._coll_end, k['records'], k['total'], eng.copies, conf['corridor'], conf['back'], conf['pace'],
                                           conf['finish'], list(conf['types']), **extra, **kw)


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


def test_rows_stay_in_the_corridor_and_tokens_in_their_sets():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps, corridor = cfg.hist_columns, cfg.num_decode_steps, 1.5
    routes, n = _routes(c)
    eng = _make(c, w, follow_routes=dict(routes=routes, n_points=n, corridor=corridor), options={'attn_mode': 1})
    log, checked = [], [0]

    def each(t):
        bits, count, prog = _route_op(eng, hc - 1 + t)
        assert torch.equal(eng.route_bits, bits) and torch.equal(eng.route_allowed, count) and torch.equal(eng.route_progress, prog), t
        checked[0] += _emitted_in_sets(eng, hc - 1 + t, bits)
        log.append(prog.cpu().numpy())
    _stepwise(eng, steps, each)
    log = np.stack(log)                                    # [steps][rows][4]
    assert checked[0] > 20 and (log[..., 3] == 1).any()

    def worst(lg):
        """per row the largest d0 over the steps at which it is ruled, less max(corridor, its first d0)"""
        out = np.full(lg.shape[1], -np.inf)
        for r in range(lg.shape[1]):
            on = lg[:, r, 3] == 1
            if on.any():
                out[r] = lg[on, r, 1].max() - max(corridor, lg[on, r, 1][0])
        return out
    # the same rollout without routes leaves some corridor (else the assertion below would show nothing): measured with the operator
    free = _make(c, w, options={'attn_mode': 1})
    flog = []
    _stepwise(free, steps, lambda t: flog.append(_route_op(free, hc - 1 + t, routed=eng)[2].cpu().numpy()))
    print('free: worst excess', np.round(worst(np.stack(flog)), 3), 'routed:', np.round(worst(log), 3))
    assert (worst(np.stack(flog)) > 1e-3).any(), 'the free rollout leaves the corridor of its own log'
    assert (worst(log) <= 1e-3).all(), worst(log)


def test_a_wide_corridor_is_the_engine_without_routes():
    c = load_case('c1_a8_m128')
    w = _weights(c)
    kw = dict(token_logprob=True, store_logits=True)
    a = _make(c, w, **kw)
    a.rollout()
    assert a._route is None and a.route_bits is None and a._ctx.token_mask == 0, 'no buffers, no handle'
    routes, n = _routes(c)
    b = _make(c, w, follow_routes=dict(routes=routes, n_points=n, corridor=1e6, back=1e6, pace=0.0), **kw)
    b.rollout()
    assert b._ctx.token_mask >= 1 and int((b.route_progress[:, 3] == 1).sum()) > 0
    _same_outputs(a.outputs()[0], b.outputs()[0])
    b.reload([c['scene']], follow_routes=False)
    b.rollout()
    _same_outputs(a.outputs()[0], b.outputs()[0])


def test_collision_road_and_route_masks_compose_and_detach():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, K = cfg.hist_columns, cfg.token_size
    routes, n = _routes(c, shift=1.0)
    eng = _make(c, w, avoid_collisions=True, stay_on_road=dict(margin=0.5, detail=5),
                follow_routes=dict(routes=routes, n_points=n, corridor=1.5, pace=0.5), options={'attn_mode': 1})
    bitten = [0]

    def each(t):
        col = hc - 1 + t
        bits, count, prog = _route_op(eng, col, base=(eng.road_bits, eng._road['ident']))
        assert torch.equal(eng.route_bits, bits) and torch.equal(eng.route_allowed, count), t
        road, route = cr.unpack(eng.road_bits.cpu().numpy(), K), cr.unpack(bits.cpu().numpy(), K)
        cnt = count.cpu().numpy()
        assert not (route & ~road)[cnt > 0].any(), 'a subset of the road stage wherever the count is > 0'
        assert np.array_equal(route[cnt == 0], road[cnt == 0]), 'the fallback returns the road stage\'s set'
        bitten[0] += int(((cnt > 0) & (cnt < road.sum(axis=1))).sum())
        _emitted_in_sets(eng, col, bits)
    _stepwise(eng, 4, each)
    assert bitten[0] > 0
    # detached: the heads read the road rider's bits again
    eng.reload([c['scene']], follow_routes=False)
    both = _make(c, w, avoid_collisions=True, stay_on_road=dict(margin=0.5, detail=5), options={'attn_mode': 1})
    eng.rollout()
    both.rollout()
    _same_outputs(eng.outputs()[0], both.outputs()[0])
    assert torch.equal(eng.road_bits, both.road_bits)


def test_set_routes_between_steps_and_graph_replay():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    w = _weights(c)
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    routes, n = _routes(c)
    moved, _ = _routes(c, shift=2.0)
    kw = dict(options={'attn_mode': 1}, follow_routes=dict(routes=routes, n_points=n, corridor=1.5, pace=0.3), token_logprob=True)
    g = _make(c, w, use_graph=True, **kw)
    g.rollout()
    g.rollout()                       # (the first rollout runs eagerly, the second captures and replays)
    assert g._graph is not None
    e = _make(c, w, **kw)
    _stepwise(e, steps)
    _same_outputs(g.outputs()[0], e.outputs()[0])
    assert torch.equal(g.route_bits, e.route_bits) and torch.equal(g.route_progress, e.route_progress)
    # new routes after step 2: from there on the sets are those of the new records
    e2 = _make(c, w, **kw)

    def each(t):
        if t == 2:
            e2.set_routes(moved, n)
        if t >= 3:
            bits, count, prog = _route_op(e2, hc - 1 + t)
            assert torch.equal(e2.route_bits, bits) and torch.equal(e2.route_progress, prog)
    _stepwise(e2, steps, each)
    want, _ = rr.records(moved, n, np.float32)
    assert np.array_equal(e2._route['records'].cpu().numpy()[:, :routes.shape[1], :, 4:], want[..., 4:])
    assert not torch.equal(e2.route_progress, e.route_progress)
    g.set_routes(moved, n)
    assert g._graph is None


def test_insertion_engine_appended_rows_keep_their_base():
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    w = _weights(c, cfg)
    routes, n = _routes(c)
    eng = _make(c, w, force_enter=True, follow_routes=dict(routes=routes, n_points=n, corridor=1.5))
    eng.rollout()
    out = eng.outputs()[0]
    assert out['num_inserted'] > 0
    first = routes.shape[1]
    prog = eng.route_progress.view(eng.S, eng.A_cap, 4).cpu().numpy()
    assert (prog[:, first:, 2] == 0).all() and (prog[:, first:, 3] == 0).all(), 'appended rows have no route'
    assert (eng.route_allowed.view(eng.S, eng.A_cap)[:, first:] == cfg.token_size).all()


# ------------------------------------------------------------------------------------------ branching, snapshots, sessions, the module
def test_branching_and_snapshots_keep_the_routes():
    """the scheme of tests/test_branching_gpu.py with routes on: a branched slot equals the rollout that had that history all
    along; a restore followed by set_routes continues under the new routes, as an engine that was given them at that step"""
    from test_branching_gpu import _branched_against_control, _control_uniforms, _full, _sampled, _uniforms
    from test_replay_gpu import _case, _same
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    tb = steps // 2
    routes, n = _routes(c)
    moved, _ = _routes(c, shift=2.0)
    conf = dict(routes=routes, n_points=n, corridor=1.5, pace=0.3)
    E = _branched_against_control(c, tb, follow_routes=conf)
    assert int((E.route_progress[:, 3] == 1).sum()) > 0 and int((E.route_allowed < c['cfg'].token_size).sum()) > 0
    # snapshot at tb, run on, come back, new routes, run on again
    u = _uniforms(c)
    S_ = _sampled(c, u, follow_routes=conf)
    S_.run(0, tb)
    snap = S_.snapshot(tb)
    S_.run(tb, steps)
    first = _full(S_)
    S_.restore(snap)
    S_.set_routes(moved, n)
    S_.run(tb, steps)
    again = _full(S_)
    ctl = _sampled(c, u, follow_routes=conf)
    ctl.run(0, tb)
    ctl.set_routes(moved, n)
    ctl.run(tb, steps)
    want = _full(ctl)
    _same(again, want, 'restored, then under the new routes')
    assert torch.equal(S_.route_bits, ctl.route_bits) and torch.equal(S_.route_progress, ctl.route_progress)
    assert not torch.equal(again['token'], first['token']), 'the new routes change the rollout'


def test_session_route_progress_is_the_operators_and_set_routes_takes_hold():
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    routes, n = _routes(c)
    moved, _ = _routes(c, shift=2.0)
    mask = np.zeros(8, bool)
    mask[0] = True
    eng = _make(c, _weights(c), options={'attn_mode': 1}, replay=[mask], follow_routes=dict(routes=routes, n_points=n, corridor=1.5))
    plan = eng.teacher_token.clone()
    ses = eng.session()
    ruled = 0
    for t in range(steps):
        if t == 4:
            ses.set_routes(moved, n)
        ses.command(tokens=plan[:, hc + t].clamp(min=0))
        ses.advance()
        bits, count, prog = _route_op(eng, hc - 1 + t)
        obs = ses.observe()
        assert torch.equal(obs['route_progress'].reshape(-1, 4), prog) and torch.equal(obs['allowed_tokens'].reshape(-1), count), t
        assert torch.equal(eng.route_bits, bits)
        _emitted_in_sets(eng, hc - 1 + t, bits, skip=eng.replay_row.bool().cpu().numpy())
        ruled += int((prog[:, 3] == 1).sum())
    assert ruled > 0
    want, _ = rr.records(moved, n, np.float32)
    assert np.array_equal(eng._route['records'].cpu().numpy()[:, :8, :, 4:], want[..., 4:])


def test_decoder_passes_the_routes_to_every_entry():
    from infgen_amd import constraints
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    cfg = c['cfg']
    dec = _decoder(cfg)
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    scene = c['scene']
    routes, n = constraints.routes_from_logged(scene, start=cfg.hist_columns - 1)
    moved = routes + np.float32(1.5)
    free = dec.inference(_to_data(scene, dev))
    n0 = len(dec._engines)
    conf = dict(routes=moved, n_points=n, corridor=1.0, pace=0.5)
    dec.follow_routes = conf
    one = dec.inference(_to_data(scene, dev))
    assert len(dec._engines) == n0 + 1, 'a routed call does not reuse the engine without routes'
    eng = _make(c, _weights(c), follow_routes=conf)
    eng.rollout()
    want = torch.from_numpy(np.asarray(eng.outputs()[0]['next_token_idx'])).to(dev)
    assert torch.equal(one['next_token_idx'], want) and not torch.equal(one['next_token_idx'], free['next_token_idx'])
    # copies: a scene's routes apply to each of its copies; a batch: one set of routes per scene
    rolls = dec.inference_rollouts(_to_data(scene, dev), 2)
    assert all(torch.equal(r['next_token_idx'], want) for r in rolls)
    dec.follow_routes = dict(conf, routes=np.concatenate([moved, moved]), n_points=np.concatenate([n, n]))
    both = dec.inference_batch([_to_data(scene, dev), _to_data(scene, dev)])
    assert all(torch.equal(r['next_token_idx'], want) for r in both)
    dec.follow_routes = conf
    ses = dec.closed_loop(_to_data(scene, dev), controlled='ego')
    assert ses.eng.follow_routes is not None and ses.observe()['route_progress'].shape == (1, ses.eng.A_cap, 4)
    ses.set_routes(routes, n)
    dec.follow_routes = dict(conf, routes=np.concatenate([moved, moved]), n_points=np.concatenate([n, n]))
    with pytest.raises(ValueError, match='scenes'):
        dec.inference(_to_data(scene, dev))
