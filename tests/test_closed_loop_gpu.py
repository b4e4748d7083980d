"""GPU: closed-loop stepping sessions (infgen_amd/closed_loop.py): k_command_rows against its float64 restatement,
and sessions against the free rollout and against log replay given the same plan up front (bit for bit)."""
import ctypes as C

import numpy as np
import pytest
import torch

import closed_loop_ref as ref
from test_replay_gpu import STATE, _case, _eng, _mask, _same, _snap

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- 1: the kernel
def _launch(vocab, k, kind, with_pose):
    """one infgen_command_rows launch through torch.ops.infgen_hip.command_rows over a hand-built state block"""
    from infgen_amd import _lib, torch_ops  # noqa: F401  (registers the ops)
    dev = torch.device('cuda:0')
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(1)
    S, T, A = ref.S, ref.T, ref.A_CAP
    t = dict(n_agents=d(k['n_agents']), atype=d(k['atype']), shape=d(k['shape']), pos=d(k['pos']), head=d(k['head']),
             state=d(k['state']), flag=d(k['flag']), vocab=d(vocab),
             tt=d(rng.integers(-5, 3000, (S, T, A)).astype(np.int32)), ts=d(rng.integers(0, 4, (S, T, A)).astype(np.int32)),
             tp=d(rng.standard_normal((S, T, A, 2)).astype(np.float32)), th=d(rng.standard_normal((S, T, A)).astype(np.float32)))
    before = {x: t[x].clone() for x in ('tt', 'ts', 'tp', 'th')}
    c, P = _lib.Rollout(), _lib.ptr
    c.S, c.A_cap, c.T, c.token_size = S, A, T, int(vocab.shape[1])
    c.n_agents, c.type, c.pos, c.head, c.state, c.vocab = P(t['n_agents']), P(t['atype']), P(t['pos']), P(t['head']), P(t['state']), P(t['vocab'])
    c.teacher_token, c.teacher_state, c.replay_row = P(t['tt']), P(t['ts']), P(t['flag'])
    if with_pose:
        c.teacher_pos, c.teacher_head = P(t['tp']), P(t['th'])
    ctx = torch.frombuffer(bytearray(bytes(c)), dtype=torch.uint8)
    kw = dict(cmd_token=d(k['cmd_tok'])) if kind == 0 else dict(cmd_pose=d(k['cmd_pose']), shape=t['shape'])
    cost = torch.ops.infgen_hip.command_rows(ctx, k['t'], t['tt'], t['ts'], cmd_mask=d(k['mask']), **kw)
    torch.cuda.synchronize()
    # every entry of the plan outside (written rows, column n) is bit-identical
    keep = torch.ones(S, T, A, dtype=torch.bool, device=dev)
    keep[:, k['n']] = ~d(k['written'])
    for x in ('tt', 'ts', 'tp', 'th'):
        if with_pose or x in ('tt', 'ts'):
            assert torch.equal(t[x][keep], before[x][keep]), x
        else:
            assert torch.equal(t[x], before[x]), x
    n = k['n']
    return (t['tt'][:, n].cpu().numpy(), t['ts'][:, n].cpu().numpy(), t['tp'][:, n].cpu().numpy(), t['th'][:, n].cpu().numpy(),
            cost.cpu().numpy())


def test_command_kernel_against_the_float64_restatement():
    cases = ref.kernel_cases()
    share, _ = ref.decided_share(cases)
    assert share >= 0.98
    n_rows = n_out = 0
    for i, (vocab, k) in enumerate(cases):
        for with_pose in (False, True):
            tok, st, tp, th, cost = _launch(vocab, k, 1, with_pose)
            w, m = k['written'], k['matched']
            assert np.array_equal(st[w], k['exp_state'][w]), i
            assert (tok[w & ~m] == -1).all() and (cost[~m] == 0).all()
            decided = m & (k['gap'] > k['margin'])
            err = np.abs(cost[m] - k['cost'][m]).max()
            print(f'case {i} pose arrays {with_pose}: {int(m.sum())} matched rows, {int((m & ~decided).sum())} inside the margin '
                  f'{k["margin"]:.2e}, max cost error {err:.2e}, wrong ids {int((tok[decided] != k["exp_tok"][decided]).sum())}')
            assert np.array_equal(tok[decided], k['exp_tok'][decided]), i
            assert err <= k['margin'], i
            if with_pose:            # the commanded pose is stored as it is; rows that left hold zeros
                assert np.array_equal(tp[m], k['cmd_pose'][m][:, :2]) and np.array_equal(th[m], k['cmd_pose'][m][:, 2])
                assert (tp[w & ~m] == 0).all() and (th[w & ~m] == 0).all()
            else:
                n_rows += int(m.sum()); n_out += int((m & ~decided).sum())
    assert n_out <= 0.02 * n_rows, (n_out, n_rows)
    # token commands: the ids as given, state valid; with pose arrays the token's integration is the stored pose
    vocab, k = cases[5]
    tok, st, tp, th, cost = _launch(vocab, k, 0, True)
    m = k['matched']
    assert np.array_equal(tok[m], k['cmd_tok'][m]) and (st[m] == ref.VALID).all() and (tok[k['written'] & ~m] == -1).all()
    assert (cost == 0).all()
    for s, r in zip(*np.nonzero(m)):
        x, y, h = ref.integrate(vocab[k['atype'][s, r], k['cmd_tok'][s, r], 5], k['pos'][s, k['c'], r], k['head'][s, k['c'], r])
        assert abs(tp[s, r, 0] - x) <= 1e-4 and abs(tp[s, r, 1] - y) <= 1e-4 and abs(np.angle(np.exp(1j * (th[s, r] - h)))) <= 1e-4


# ---------------------------------------------------------------------------------------------- sessions
def _plan(eng, s, A, pose):
    """the stored columns of scene s's first A rows as a host plan (tokens, states[, pos, head]) of (A, T) arrays"""
    torch.cuda.synchronize()
    g = lambda x: x[s, :, :A].cpu().numpy()
    p = (g(eng.token).T.copy(), g(eng.state).T.copy())
    return p + (g(eng.pos).transpose(1, 0, 2).copy(), g(eng.head).T.copy()) if pose else p


def _drive(ses, fn):
    costs = []
    while not ses.done:
        fn(ses)
        ses.advance()
        costs.append(ses.cost.clone())
    return torch.stack(costs)


def test_token_commands_step_by_step_equal_the_free_rollout():
    c = _case('c1_a8_m128')
    hc, av, A = c['cfg'].hist_columns, c['av'], 8
    free = _eng(c)
    fs = _snap(free)
    ego_tok = free.token[0, :, av].clone()                         # [T] on the device
    eng = _eng(c, run=False, replay=[_mask(A, [av])])
    ses = eng.session()
    assert ses.t == 0 and not ses.done and (eng.teacher_token[:, hc:] == -1).all()
    _drive(ses, lambda z: z.command(tokens=ego_tok[hc + z.t].reshape(1)))
    assert ses.done and ses.t == c['cfg'].num_decode_steps
    _same(_snap(eng), fs, 'session against the free rollout')
    o = free.outputs()[0]
    up = _eng(c, replay=[(_mask(A, [av]), o['next_token_idx'], np.ones_like(o['next_state_idx']))])
    _same(_snap(up), _snap(eng), 'session against the plan given up front')
    assert np.array_equal(ses.outputs()[0]['next_token_idx'], o['next_token_idx'])


def _pose_commands(c, free):
    """the free rollout's ego poses moved by a fixed offset -> [T, 3] on the device"""
    av = c['av']
    off = torch.tensor([4.0, -3.0, 0.2], device=free.pos.device)
    return torch.cat([free.pos[0, :, av], free.head[0, :, av, None]], -1) + off


def test_pose_commands_exact():
    c = _case('c1_a8_m128')
    hc, av, A = c['cfg'].hist_columns, c['av'], 8
    free = _eng(c)
    cmd = _pose_commands(c, free)
    eng = _eng(c, run=False, replay=[_mask(A, [av])])
    ses = eng.session(pose='exact')
    cost = _drive(ses, lambda z: z.command(poses=cmd[hc + z.t].reshape(1, 3)))
    torch.cuda.synchronize()
    assert torch.equal(eng.pos[0, hc:, av], cmd[hc:, :2]) and torch.equal(eng.head[0, hc:, av], cmd[hc:, 2])
    assert (eng.state[0, hc:, av] == 1).all() and (eng.token[0, hc:, av] >= 0).all()
    assert (cost[:, 0, av] > 0).all() and (cost[:, 0, :av] == 0).all()
    others = [r for r in range(A) if r != av]
    assert not torch.equal(eng.token[0, hc:, others], free.token[0, hc:, others]), 'the other agents react to the commanded ego'
    up = _eng(c, replay=[(_mask(A, [av]),) + _plan(eng, 0, A, True)])
    _same(_snap(up), _snap(eng), 'the recorded plan with poses, up front')


def test_pose_commands_token():
    c = _case('c1_a8_m128')
    cfg, hc, av, A = c['cfg'], c['cfg'].hist_columns, c['av'], 8
    free = _eng(c)
    cmd = _pose_commands(c, free)
    eng = _eng(c, run=False, replay=[_mask(A, [av])])
    ses = eng.session(pose='token')
    assert eng.teacher_pos is None
    _drive(ses, lambda z: z.command(poses=cmd[hc + z.t].reshape(1, 3)))
    tok, _, pos, head = _plan(eng, 0, A, True)
    vocab = np.stack([c['vocab'][k] for k in ('veh', 'ped', 'cyc')])
    ty = int(eng.atype[0, av])
    for col in range(hc, cfg.num_columns):       # the stored pose is the matched token's integration from the previous stored pose
        x, y, h = ref.integrate(vocab[ty, tok[av, col], 5], pos[av, col - 1], head[av, col - 1])
        assert abs(pos[av, col, 0] - x) <= 1e-4 and abs(pos[av, col, 1] - y) <= 1e-4, col
        # and that token is the restatement's choice for the command (or inside the fp32 margin of it)
        shp = eng._shape10[0, av].cpu().numpy()
        costs = ref.costs(vocab[ty, :, 5], pos[av, col - 1], head[av, col - 1], cmd[col].cpu().numpy(), shp[1], shp[0])
        margin = ref.MARGIN_EPS * float(np.spacing(np.float32(np.abs(pos[av]).max() + 10)))
        assert costs[tok[av, col]] - costs.min() <= margin, col
    assert not np.array_equal(pos[av, hc:], cmd[hc:, :2].cpu().numpy())
    up = _eng(c, replay=[(_mask(A, [av]), tok, _plan(eng, 0, A, False)[1])])
    _same(_snap(up), _snap(eng), 'the recorded tokens without poses, up front')


def _sync_debug_honoured():
    """does this torch build raise on a device -> host copy under set_sync_debug_mode('error')?"""
    x = torch.zeros(1, device='cuda:0')
    torch.cuda.set_sync_debug_mode('error')
    try:
        x.item()
        return False
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode('default')


def test_reactive_controller_without_host_sync():
    c = _case('c1_a8_m128')
    hc, av, A = c['cfg'].hist_columns, c['av'], 8
    eng = _eng(c, run=False, replay=[_mask(A, [av])])
    ses = eng.session(pose='token')
    rows = torch.arange(eng.A_cap, device=eng.device)
    scene = torch.arange(eng.S, device=eng.device)
    inf = torch.full((), float('inf'), device=eng.device)

    def controller(z):
        """keep the heading; advance 3 m, less the closer the nearest valid agent ahead is"""
        o = z.observe()
        ego = o['ego_index'].long()
        p, h = o['pos'][scene, ego], o['head'][scene, ego]
        d = o['pos'] - p[:, None]
        ahead = d[..., 0] * torch.cos(h)[:, None] + d[..., 1] * torch.sin(h)[:, None]
        seen = (o['state'] != 0) & (rows[None] < o['n_agents'][:, None]) & (ahead > 0.5)
        near = torch.where(seen, d.norm(dim=-1), inf).amin(1)
        step = 3.0 * torch.clamp(near / 20.0, 0.2, 1.0)
        z.command(poses=torch.stack([p[:, 0] + step * torch.cos(h), p[:, 1] + step * torch.sin(h), h], -1))
    controller(ses); ses.advance()                  # (the first step loads kernels and looks at the packs once)
    honoured = _sync_debug_honoured()
    print('set_sync_debug_mode is honoured:', honoured)
    assert honoured, 'this torch build does not report device -> host copies: the no-sync clause cannot be checked'
    torch.cuda.set_sync_debug_mode('error')
    try:
        _drive(ses, controller)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    tok, st = _plan(eng, 0, A, False)
    assert len(set(tok[av, hc:].tolist())) > 1, 'the controller reacted: not one token throughout'
    up = _eng(c, replay=[(_mask(A, [av]), tok, st)])
    _same(_snap(up), _snap(eng), 'the recorded plan, up front')


def test_batch_and_copies():
    from infgen_amd import synth
    c = _case('c1_a8_m128')
    cfg, hc = c['cfg'], c['cfg'].hist_columns
    scenes = [c['scene'], synth.make_scene(synth.scene_seed(1, 1), 8, 128, cfg, vocab=c['vocab'], grid=c['grid'])]
    avs = [int(np.asarray(sc['agent']['av_index']).reshape(-1)[0]) for sc in scenes]
    masks = [_mask(8, [a]) for a in avs]
    steps = cfg.num_decode_steps
    dev = torch.device('cuda:0')
    cmds = (torch.arange(steps, device=dev)[:, None] * 131 + torch.arange(4, device=dev)[None, :] * 517 + 11) % cfg.token_size   # [steps, 4]
    assert len({tuple(cmds[:, s].tolist()) for s in range(4)}) == 4
    eng = _eng(c, scenes, run=False, replay=masks, copies=2)
    assert eng.S == 4
    _drive(eng.session(), lambda z: z.command(tokens=cmds[z.t].int()))
    for s in range(4):
        one = _eng(c, [scenes[s // 2]], run=False, replay=[masks[s // 2]])
        _drive(one.session(), lambda z: z.command(tokens=cmds[z.t, s].reshape(1)))
        a, b = _snap(eng, s), _snap(one, 0)
        assert torch.equal(a['token'][hc:, avs[s // 2]], cmds[:, s].int()), s
        for k in ('token', 'state', 'gridtok'):
            assert torch.equal(a[k], b[k]), (s, k)
        # (the bars of tests/test_batch_inference_gpu.py for batch == single)
        assert float((a['pos'] - b['pos']).abs().max()) <= 1e-5 and float((a['head'] - b['head']).abs().max()) <= 1e-5, s
        assert float((a['logits'] - b['logits']).abs().max()) <= 1e-4, s


def test_insertion_on():
    c = _case('ins_forced_a16_m256', insertion=True)
    hc, av = c['cfg'].hist_columns, c['av']
    A0 = np.asarray(c['scene']['agent']['state_idx']).shape[0]
    free = _eng(c, force_enter=True)
    o = free.outputs()[0]
    assert o['num_inserted'] > 0
    ego_tok = free.token[0, :, av].clone()
    eng = _eng(c, run=False, replay=[_mask(A0, [av])], force_enter=True)
    ses = eng.session()
    n_steps = []

    def feed(z):
        n_steps.append(eng.n_agents.clone())
        z.command(tokens=ego_tok[hc + z.t].reshape(1))
    _drive(ses, feed)
    s = ses.outputs()[0]
    A = o['pos_a'].shape[0]
    assert s['num_inserted'] == o['num_inserted'] and s['pos_a'].shape[0] == A
    for k in ('next_token_idx', 'next_state_idx'):
        assert np.array_equal(s[k], o[k]), k
    assert torch.equal(eng.bos[0, :A], free.bos[0, :A]) and torch.equal(eng.n_agents, free.n_agents)
    assert eng.ins['inserted_rows'][0] == free.ins['inserted_rows'][0]
    bos = free.bos[0, A0:A].cpu().numpy()
    for t, n in enumerate(n_steps):                 # rows in the scene when step t begins: inserted up to the previous step
        assert int(n[0]) == A0 + int((bos <= t).sum()), t
    assert np.array_equal(s['replay_mask'][:A0], _mask(A0, [av])) and not s['replay_mask'][A0:].any()
    assert int(eng.replay_row.sum()) == 1


def test_errors_and_lifecycle():
    c = _case('c1_a8_m128')
    hc, av, A = c['cfg'].hist_columns, c['av'], 8
    z = c['z']
    with pytest.raises(ValueError):
        _eng(c, run=False, teacher=[(z['next_token_idx'], z['next_state_idx'])]).session()
    with pytest.raises(ValueError):
        _eng(c, run=False).session()                                 # nothing to control
    eng = _eng(c, run=False, replay=[_mask(A, [av])])
    with pytest.raises(ValueError):
        eng.session(pose='nearest')
    free = _eng(c)
    cmd = _pose_commands(c, free)
    ses = eng.session(pose='exact')
    with pytest.raises(RuntimeError):
        ses.advance()                                                # no command yet
    with pytest.raises(ValueError):
        ses.command(tokens=cmd[hc, :1].int(), poses=cmd[hc].reshape(1, 3))
    with pytest.raises(ValueError):
        ses.command(poses=cmd[hc].reshape(3))
    with pytest.raises(RuntimeError):
        ses.outputs()                                                # not done
    _drive(ses, lambda x: x.command(poses=cmd[hc + x.t].reshape(1, 3)))
    first = _snap(eng)
    with pytest.raises(RuntimeError):
        ses.advance()                                                # past the last step
    with pytest.raises(RuntimeError):
        ses.command(poses=cmd[hc].reshape(1, 3))
    eng.reset()
    with pytest.raises(RuntimeError):
        ses.observe()                                                # reset() ended it
    ses2 = eng.session(pose='exact')
    assert ses2.t == 0 and (eng.teacher_token[:, hc:] == -1).all()
    _drive(ses2, lambda x: x.command(poses=cmd[hc + x.t].reshape(1, 3)))
    _same(_snap(eng), first, 'a new session after reset()')
    # a pose command needs the rows' shapes
    eng3 = _eng(c, run=False, replay=[_mask(A, [av])])
    ses3 = eng3.session()
    eng3._shape10 = None
    with pytest.raises(ValueError):
        ses3.command(poses=cmd[hc].reshape(1, 3))
    from infgen_amd import _lib
    r = eng3.lib.infgen_command_rows(C.byref(eng3._ctx), 0, 1, None, _lib.ptr(ses3._pose), None, None, None, None)
    assert r != 0 and b'shape' in eng3.lib.infgen_last_error()
    # 'ego' by name on an engine without replay=, and leaving the scene: the row stays out
    eng4 = _eng(c, run=False)
    ses4 = eng4.session(controlled='ego')
    assert int(eng4.replay_row.sum()) == 1 and bool(eng4.replay_row[0, av])
    ego_tok = free.token[0, :, av].clone()
    _drive(ses4, lambda x: x.command(tokens=ego_tok[hc + x.t].reshape(1), mask=torch.tensor([x.t != 3], device=eng4.device)))
    torch.cuda.synchronize()
    assert (eng4.state[0, hc:hc + 3, av] == 1).all() and (eng4.state[0, hc + 3:, av] == 0).all()
    assert (eng4.token[0, hc + 3:, av] == -1).all()
    eng4.rollout()                                                   # the engine generates every row again
    _same(_snap(eng4), _snap(free), 'rollout() after a session')


def test_module_entry():
    from test_batch_inference_gpu import _dec
    from test_modules_gpu import _to_data
    dev = torch.device('cuda:0')
    c = _case('a24_m256_edge')
    hc = c['cfg'].hist_columns
    dec = _dec(c)
    free = dec.inference(_to_data(c['scene'], dev))
    ego = int(free['ego_index'])
    tok = free['next_token_idx'][ego].clone()
    ses = dec.closed_loop(_to_data(c['scene'], dev), controlled='ego')
    _drive(ses, lambda z: z.command(tokens=tok[hc + z.t].reshape(1)))
    out = ses.outputs()
    d = _to_data(c['scene'], dev)
    ag = d['agent']
    av = int(ag['av_index'].reshape(-1)[0])
    plan_tok, plan_st = ag['token_idx'].clone(), torch.ones_like(ag['state_idx'])
    plan_tok[av] = tok.to(plan_tok.dtype)
    want = dec.inference(d, replay='ego', replay_plan=dict(token_idx=plan_tok, state_idx=plan_st))
    assert set(out.keys()) == set(want.keys()) and 'replay_mask' in out
    for k in want.keys():
        a, b = out[k], want[k]
        if isinstance(b, torch.Tensor):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
    assert torch.equal(out['next_token_idx'], free['next_token_idx'])
