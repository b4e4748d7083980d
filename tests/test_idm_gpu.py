"""IDM commands on the GPU: k_idm_command against the two restatements of tests/idm_ref.py, the platoon scenario
stepped on the device, and the engine / session plumbing on the fixtures c1_a8_m128 and ins_forced_a16_m256."""
import ctypes as C

import numpy as np
import pytest
import torch

import idm_ref as ir
import route_ref as rr
from conftest import load_case
from rider_helpers import _make, _t, _weights
from test_idm_cpu import check_platoon

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 4, 0x5A5A5A5A          # words in front of and behind every output (16 bytes: the outputs stay aligned)


def _guarded(n, dtype):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda:0')
    return buf, buf[GUARD:GUARD + n].view(dtype)


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def _call(case, par, **over):
    """infgen_route_records + infgen_idm_command through ctypes, every output between guard words and pre-filled with the sentinel
    -> (rc, message, dict of outputs)"""
    from infgen_amd import _lib, torch_ops
    lib, P = _lib.load(), _lib.ptr
    S, A, T = case['S'], case['A'], case['T']
    ins = dict(pos=_t(case['pos']), head=_t(case['head']), state=_t(case['state']), n_agents=_t(case['n_agents']), atype=_t(case['atype']),
               shape=_t(case['shape']), ctl=_t(case['ctl']), routes=_t(case['routes']), n_points=_t(case['n_points']))
    if par.get('v_des') is not None:
        ins['v_des'] = _t(par['v_des'])
    rec, total = torch_ops.route_records(ins['routes'], ins['n_points'])
    ins.update(rec=rec, total=total)
    before = {k: v.clone() for k, v in ins.items()}
    gp, pose = _guarded(S * A * 3, torch.float32)
    gs, state = _guarded(S * A * 8, torch.float32)
    gl, lead = _guarded(S * A, torch.int32)
    a = dict(pos=P(ins['pos']), head=P(ins['head']), state=P(ins['state']), n_agents=P(ins['n_agents']), type=P(ins['atype']),
             shape=P(ins['shape']), ctl_row=P(ins['ctl']), S=S, A_cap=A, T=T, c=case['c'], records=P(rec), total=P(total), P=case['P'],
             copies=case['copies'], v_des=P(ins.get('v_des')), dt=par['dt'], v0_type=(C.c_float * 3)(*par['v0']), headway=par['headway'],
             s_min=par['s_min'], a_max=par['a_max'], b_comf=par['b_comf'], b_max=par['b_max'], lateral=par['lateral'], keep=par['keep'],
             types=(C.c_int * 3)(*par['types']), stop_at_end=par['stop_at_end'], cmd_pose=P(pose), out_state=P(state), out_lead=P(lead),
             stream=None)
    for k, v in over.items():
        a[k] = (C.c_float * 3)(*v) if k == 'v0_type' and v is not None else v
    rc = lib.infgen_idm_command(*a.values())
    torch.cuda.synchronize()
    msg = lib.infgen_last_error().decode() if rc else ''
    assert _intact(gp, S * A * 3) and _intact(gs, S * A * 8) and _intact(gl, S * A), 'guard words'
    assert all(torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)) for k, v in ins.items()), 'inputs unchanged'
    untouched = all(bool((x.view(torch.int32) == SENTINEL).all()) for x in (pose, state, lead))
    return rc, msg, dict(pose_bits=pose.view(torch.int32).view(S * A, 3).cpu().numpy(), pose=pose.view(S * A, 3).cpu().numpy(),
                         state=state.view(S * A, 8).cpu().numpy(), lead=lead.cpu().numpy().astype(np.int64), untouched=untouched)


def _against(out, r32, r64, par, label, quiet=False):
    """the operator bar: lead and flag exact outside near rows.  Every float output on the rows whose lead agrees in all three
    evaluations - less the rows whose own, lead's or target's segment is open inside the band (another segment: another normal, another
    heading) and the ill-conditioned ones, both counted by the CPU test under its cap - row by row within max(4 x the float32
    restatement's own largest error against float64 on those rows, 8 * 2^-23 x that row's magnitude that enters).  -> rows compared"""
    ruled, near = r64['ruled'], r64['near']
    sure = ~near
    assert np.array_equal(out['lead'][sure], r32['lead'][sure]) and np.array_equal(out['lead'][sure], r64['lead'][sure]), label
    assert np.array_equal(out['state'][:, 7], ruled.astype(np.float32)), label
    assert (out['pose_bits'][~ruled] == SENTINEL).all(), 'cmd_pose of unruled rows keeps its sentinel'
    assert not out['state'][~ruled].any() and (out['lead'][~ruled] == -1).all(), label
    rows = ruled & ~r64['ambiguous'] & ~r64['ill'] & (out['lead'] == r64['lead']) & (r32['lead'] == r64['lead'])
    assert rows.sum() >= 0.9 * ruled.sum() - 1, (label, int(rows.sum()), int(ruled.sum()))
    got, w32, w64, floor = ir.outputs(out), ir.outputs(r32), ir.outputs(r64), ir.floors(r64, par)
    worst = {}
    for k in got:
        fin = rows & np.isfinite(w64[k])
        assert np.array_equal(got[k][rows & ~fin], w32[k][rows & ~fin]), (label, k)          # (gap = +inf without a lead)
        err = np.abs(got[k][fin].astype(np.float64) - w64[k][fin])
        own = np.abs(w32[k][fin].astype(np.float64) - w64[k][fin]).max()
        bar = np.maximum(4.0 * own, 8.0 * ir.EPS32 * floor[k][fin])
        worst[k] = float((err / bar).max())
    if not quiet:
        print(f'{label}: {int(ruled.sum())} ruled, {int(near.sum())} near, {int(r64["ambiguous"].sum())} with an open segment, '
              f'{int(r64["ill"].sum())} ill, {int(rows.sum())} compared; largest error / bar ' + ' '.join(f'{k} {v:.2f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (label, worst)
    return int(rows.sum())


# ------------------------------------------------------------------------------------------ operator level
@pytest.mark.parametrize('name', list(ir.CASES))
def test_operator_against_the_restatements(name):
    case = ir.make_case(name)
    for variant in ir.VARIANTS:
        par = ir.variant_params(case, variant)
        rc, msg, out = _call(case, par)
        assert rc == 0, msg
        _against(out, ir.case_reference(name, variant, False), ir.case_reference(name, variant, True), par, f'{name} {variant}')
        rc, msg, again = _call(case, par)
        assert rc == 0 and all(np.array_equal(out[k].view(np.int32) if out[k].dtype == np.float32 else out[k],
                                              again[k].view(np.int32) if again[k].dtype == np.float32 else again[k])
                               for k in ('pose_bits', 'state', 'lead')), 'a second call gives identical bits'


def test_first_column_with_nothing_live_before_it():
    case = dict(ir.make_case('a32_p3_c2'))
    case['state'] = case['state'].copy()
    case.update(c=1)
    case['state'][:, 0] = 0
    par = ir.params()
    rc, msg, out = _call(case, par)
    assert rc == 0, msg
    r64 = ir.reference(case, par, np.float64)
    assert r64['ruled'].any() and (out['state'][:, 2] == 0).all() and (r64['state'][:, 2] == 0).all()
    assert (r64['near'] | r64['ill']).sum() <= 0.1 * r64['ruled'].sum()                       # (this variant of the case is not the CPU test's)
    _against(out, ir.reference(case, par, np.float32), r64, par, 'c = 1')


def test_every_refusal_returns_an_error_and_launches_nothing():
    case, par = ir.make_case('a5_p2'), ir.params()
    nan, inf = float('nan'), float('inf')
    odd = torch.zeros(64, device='cuda:0')
    bad = [dict(dt=0.0), dict(dt=-0.5), dict(dt=nan), dict(dt=inf), dict(a_max=0.0), dict(a_max=nan), dict(b_comf=0.0), dict(b_comf=inf),
           dict(b_max=-1.0), dict(b_max=nan), dict(v0_type=(15.0, 0.0, 6.0)), dict(v0_type=(nan, 1.5, 6.0)), dict(v0_type=(15.0, 1.5, inf)),
           dict(v0_type=None), dict(headway=-0.1), dict(headway=nan), dict(s_min=-1.0), dict(s_min=inf), dict(lateral=-0.5), dict(lateral=nan),
           dict(keep=-0.1), dict(keep=1.5), dict(keep=nan), dict(P=1), dict(P=33), dict(copies=0), dict(copies=3), dict(c=0), dict(c=-1),
           dict(c=case['T']), dict(A_cap=1025), dict(pos=None), dict(head=None), dict(state=None), dict(n_agents=None), dict(type=None),
           dict(shape=None), dict(ctl_row=None), dict(records=None), dict(total=None), dict(types=None), dict(cmd_pose=None),
           dict(records=odd.data_ptr() + 4), dict(out_state=odd.data_ptr() + 8)]
    for over in bad:
        rc, msg, out = _call(case, par, **over)
        assert rc != 0 and msg.startswith('infgen_idm_command: idm:'), (over, rc, msg)
        assert out['untouched'], over
    for over in (dict(out_state=None), dict(out_lead=None), dict(v_des=None)):                # optional
        rc, msg, out = _call(case, par, **over)
        assert rc == 0, (over, msg)


# ------------------------------------------------------------------------------------------ the platoon on the device
def test_platoon_on_the_device():
    from infgen_amd import torch_ops  # noqa: F401
    case, par = ir.platoon_case(), ir.params()
    S, A, c = case['S'], case['A'], case['c']
    pos, head = _t(case['pos']), _t(case['head'])
    rec, total = torch_ops.route_records(_t(case['routes']), _t(case['n_points']))
    fixed = [_t(case[k]) for k in ('state', 'n_agents', 'atype', 'shape', 'ctl')]
    log, snaps, compared = [], [], 0
    for _ in range(ir.PLATOON['steps']):
        cmd = torch.cat([pos[:, c], head[:, c, :, None]], -1).contiguous()                    # the fill: stand still
        state, lead = torch.ops.infgen_hip.idm_command(pos, head, *fixed, c, rec, total, cmd)
        snaps.append((pos.clone(), head.clone(), cmd.clone(), state, lead))
        pos[:, c - 1], head[:, c - 1] = pos[:, c].clone(), head[:, c].clone()                 # the device's own targets, fed back
        pos[:, c], head[:, c] = cmd[..., :2], cmd[..., 2]
    for t, (p, h, cmd, state, lead) in enumerate(snaps):      # against the restatements ON THE DEVICE'S INPUTS of that step: no drift
        now = dict(case, pos=p.cpu().numpy(), head=h.cpu().numpy())
        out = dict(pose=cmd.view(S * A, 3).cpu().numpy(), state=state.cpu().numpy(), lead=lead.cpu().numpy().astype(np.int64))
        r32, r64 = ir.reference(now, par, np.float32), ir.reference(now, par, np.float64)
        out['pose_bits'] = np.where(r64['ruled'][:, None], 0, SENTINEL)                       # (the fill stands in for the sentinel:)
        assert np.array_equal(out['pose'][0], np.append(now['pos'][0, c, 0], now['head'][0, c, 0]))      # the uncontrolled row stands still
        compared += _against(out, r32, r64, par, f'platoon step {t}', quiet=t % 8 != 0)
        log.append(out['state'][1:, :4].astype(np.float64))
    assert compared == 3 * ir.PLATOON['steps'], 'every controlled row at every step'
    check_platoon(np.array(log))


# ------------------------------------------------------------------------------------------ engine level
def _routes(c):
    from infgen_amd import constraints
    return constraints.routes_from_logged(c['scene'], start=c['cfg'].hist_columns - 1)


def _controlled(A, rows):
    m = np.zeros(A, bool)
    m[list(rows)] = True
    return m


def _op_on_observation(eng, obs, tab, **params):
    """torch.ops.infgen_hip.idm_command on what observe() shows (and the stored columns behind it) -> pose [S, A_cap, 3], state, lead"""
    from infgen_amd import torch_ops  # noqa: F401  (registers the ops)
    cmd = torch.cat([obs['pos'], obs['head'][..., None]], -1).contiguous()
    state, lead = torch.ops.infgen_hip.idm_command(eng.pos, eng.head, eng.state, obs['n_agents'], obs['type'], obs['shape'], obs['controlled'],
                                                   obs['column'], tab['records'], tab['total'], cmd, eng.copies, **params)
    return cmd, state, lead


def test_session_driven_by_the_controller():
    from test_closed_loop_gpu import _plan
    from test_replay_gpu import _same, _snap
    c = load_case('c1_a8_m128')
    cfg, w = c['cfg'], _weights(c)
    hc, A = cfg.hist_columns, 8
    routes, n = _routes(c)
    n = n.copy()
    rows = [r for r in range(A) if n[0, r] >= 2][:3]
    rows, still = rows[:2], rows[2]
    n[0, still] = 0                                                                           # a controlled row without a route
    mask = _controlled(A, rows + [still])
    eng = _make(c, w, replay=[mask], store_logits=True)
    ses = eng.session(pose='exact')
    stood = moved = 0
    while not ses.done:
        col = hc - 1 + ses.t
        before = (eng.pos[0, col, still].clone(), eng.head[0, col, still].clone())
        ses.command_idm(routes=routes, n_points=n)
        obs = ses.observe()
        cmd, state, lead = _op_on_observation(eng, obs, eng._idm_route)
        assert torch.equal(ses._pose, cmd), 'the poses handed to k_command_rows are the operator\'s on the observation'
        assert torch.equal(obs['idm_state'].reshape(-1, 8), state) and torch.equal(obs['idm_lead'].reshape(-1), lead)
        handed = ses._pose.clone()
        ses.advance()
        live = eng.state[0, col + 1] != 0
        for r in rows + [still]:
            if bool(live[r]):                   # pose='exact': the commanded pose itself is stored
                assert torch.equal(eng.pos[0, col + 1, r], handed[0, r, :2]) and torch.equal(eng.head[0, col + 1, r], handed[0, r, 2])
        if bool(live[still]):
            assert torch.equal(eng.pos[0, col + 1, still], before[0]) and torch.equal(eng.head[0, col + 1, still], before[1])
            stood += 1
        moved += int((state.view(eng.S, eng.A_cap, 8)[0, rows, 7] == 1).sum())
    assert stood > 0 and moved > 0
    up = _make(c, w, replay=[(mask,) + _plan(eng, 0, A, True)], store_logits=True)
    up.rollout()
    _same(_snap(up), _snap(eng), 'the recorded plan with poses, up front')


def test_engine_tables_and_follow_routes_tables_agree():
    c = load_case('c1_a8_m128')
    w = _weights(c)
    routes, n = _routes(c)
    mask = _controlled(8, [0, 1, 2])
    own = _make(c, w, replay=[mask], options={'attn_mode': 1})
    fr = _make(c, w, replay=[mask], follow_routes=dict(routes=routes, n_points=n, corridor=1e6, back=1e6), options={'attn_mode': 1})
    with pytest.raises(ValueError, match='routes=.*follow_routes='):
        own.prologue()
        own.idm_command(own.hc - 1)
    a, b = own.session(), fr.session()
    for t in range(3):
        a.command_idm(routes=routes, n_points=n, keep=1.0)
        b.command_idm(keep=1.0)
        assert torch.equal(a._pose, b._pose) and torch.equal(a.observe()['idm_state'], b.observe()['idm_state'])
        assert torch.equal(a.observe()['idm_lead'], b.observe()['idm_lead'])
        tab = own._idm_route
        a.advance(); b.advance()
    a.command_idm(routes=routes, n_points=n)
    assert own._idm_route is tab, 'the tables are rebuilt only when the routes change'
    a.command_idm(routes=routes + np.float32(1.0), n_points=n)
    assert not np.array_equal(own._idm_route['host'][0], routes)
    assert (a.observe()['idm_state'][..., 7] == 1).any()


def test_run_idm_with_insertion_on():
    from infgen_amd import closed_loop
    c = load_case('ins_forced_a16_m256')
    cfg = c['cfg']
    cfg.disable_insertion = False
    w = _weights(c, cfg)
    routes, n = _routes(c)
    A0 = routes.shape[1]
    rows = [r for r in range(A0) if n[0, r] >= 2]
    eng = _make(c, w, replay=[_controlled(A0, rows)], force_enter=True)
    ses = eng.session()
    leads = []
    while not ses.done:
        ses.command_idm(routes=routes, n_points=n, lateral=200.0)          # (a bound so wide that whatever is ahead along the route leads)
        leads.append(ses.observe()['idm_lead'].clone())
        ses.advance()
    out = ses.outputs()[0]
    assert out['num_inserted'] > 0 and int(eng.replay_row[:, A0:].sum()) == 0
    leads = torch.stack(leads).cpu().numpy()
    assert (leads[:, 0, A0:] == -1).all(), 'appended rows are never ruled'
    print('leads named:', sorted(set(leads[:, 0, rows].reshape(-1).tolist())))
    # an inserted row is an obstacle like any other once live: at the last column, the original row nearest to an inserted one, on a
    # straight route through it (of all such pairs the nearest, so no third agent's centre lies between the two)
    col = eng.T - 1
    live = ((eng.state[0, col] != 0) & (torch.arange(eng.A_cap, device=eng.device) < eng.n_agents[0])).cpu().numpy()
    p = eng.pos[0, col].cpu().numpy().astype(np.float64)
    first, later = [r for r in range(A0) if live[r]], [j for j in range(A0, eng.A_cap) if live[j]]
    assert first and later
    r, j = min(((r, j) for r in first for j in later), key=lambda q: np.linalg.norm(p[q[0]] - p[q[1]]))
    line, cnt = np.zeros((1, eng.A_cap, 2, 2), np.float32), np.zeros((1, eng.A_cap), np.int32)
    line[0, r], cnt[0, r] = [p[r], p[r] + 2.0 * (p[j] - p[r])], 2
    one = torch.zeros(eng.S, eng.A_cap, dtype=torch.uint8, device=eng.device)
    one[0, r] = 1
    res = eng.idm_command(col, ctl_row=one, routes=line, n_points=cnt, lateral=0.0, types=(1, 1, 1))
    assert int(res['lead'][r]) == j >= A0 and float(res['state'][r, 7]) == 1.0, 'an inserted row is named as a lead'
    again = _make(c, w, replay=[_controlled(A0, rows)], force_enter=True)
    closed_loop.run_idm(again.session(), routes=routes, n_points=n, lateral=200.0)
    assert torch.equal(again.token, eng.token) and torch.equal(again.pos, eng.pos)


def test_an_engine_that_never_calls_the_controller_is_unchanged():
    c = load_case('c1_a8_m128')
    w = _weights(c)
    a, b = _make(c, w), _make(c, w)
    routes, n = _routes(c)
    b.prologue()
    b.idm_command(b.hc - 1, ctl_row=torch.ones(b.S, b.A_cap, dtype=torch.uint8, device=b.device), routes=routes, n_points=n)
    a.rollout()
    b.rollout()
    assert torch.equal(a.token, b.token) and torch.equal(a.pos, b.pos)
    d = _make(c, w)
    d.rollout()
    assert torch.equal(a.token, d.token)


def test_decoder_passes_idm_through():
    from infgen_amd import closed_loop
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    c = load_case('c1_a8_m128')
    dec = _decoder(c['cfg'])
    _load(dec, c['sd'])
    dev = torch.device('cuda:0')
    dec = dec.to(dev).eval()
    routes, n = _routes(c)
    out = dec.closed_loop(_to_data(c['scene'], dev), controlled='ego', idm=dict(routes=routes, n_points=n, keep=0.0))
    ses = dec.closed_loop(_to_data(c['scene'], dev), controlled='ego')
    assert 'idm_state' not in ses.observe()
    want = closed_loop.run_idm(ses, routes=routes, n_points=n, keep=0.0).outputs()
    assert (ses.observe()['idm_state'][..., 7] == 1).any()
    assert set(out) == set(want) and torch.equal(out['next_token_idx'], want['next_token_idx']) and bool(out['replay_mask'].any())
