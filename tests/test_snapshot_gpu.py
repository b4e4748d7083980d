"""GPU: snapshots ("snapshots" of include/infgen_hip.h) - infgen_snapshot_scenes / infgen_restore_scenes against the
restatement of tests/snapshot_ref.py over the hand-built context of the branching operator test, a rewound rollout against the one
that was never interrupted, fan-out against branch, sessions with look-ahead, errors and lifecycle.  Everything is compared bit
for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import snapshot_ref as ref
from test_branching_gpu import SCRATCH, STEP_MAJOR, _Buf, _context, _full, _sampled, _uniforms
from test_replay_gpu import _case, _eng, _same, _snap

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GROUP = [0, 0, 0, 1, 1, 1]


def _bytes(lib, ctx, t):
    from infgen_amd import _lib
    n = C.c_longlong(-1)
    _lib.check(lib.infgen_snapshot_bytes(C.byref(ctx), t, C.byref(n)), 'infgen_snapshot_bytes')
    return n.value


# ---------------------------------------------------------------------------------------------- 1. the operator
def _np(bufs):
    """the context's payloads as flat uint8 numpy arrays, under the names of snapshot_ref.segments"""
    torch.cuda.synchronize()
    return {k: v.data().cpu().numpy().copy() for k, v in bufs.items()}


@pytest.mark.parametrize('A_cap', (32, 96))
def test_snapshot_and_restore_against_the_restatement(A_cap):
    from infgen_amd import _lib
    c = _case('c1_a8_m128')
    lib = _lib.load()
    # A_cap 96: two byte arrays off 16-byte alignment (byte by byte on the context side), blocks of several chunks, a partial last one
    shifts = dict(imask=1, catflag=4) if A_cap == 96 else {}
    b, bufs, lay = _context(A_cap, c['cfg'], shifts)
    S, steps, ring, L = lay['S'], lay['steps'], lay['ring'], lay['L']
    T, R, ts = c['cfg'].num_columns, c['cfg'].num_recurrent_steps_val, 96
    stream = torch.cuda.current_stream(DEV).cuda_stream
    n_bad = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    stride = _bytes(lib, b, steps) + 32          # room for any step, and a gap the calls must not touch
    assert stride - 32 == ref.entry_bytes(A_cap, T, ring, L, R, ts, steps)
    N = 3                                                                # entries 0, 1: the save under test; entry 2: another step's

    def save(t, slots, first=0, map_scene=True):
        sl = torch.tensor(slots, dtype=torch.int32, device=DEV)
        b.map_scene = lay['keep'].data_ptr() if map_scene else None
        _lib.check(lib.infgen_snapshot_scenes(C.byref(b), t, sl.data_ptr(), len(slots), snap.ptr + first * stride, stride,
                                              head.ptr + first * 16, n_bad.data_ptr(), stream), 'infgen_snapshot_scenes')
        torch.cuda.synchronize()
        return int(n_bad[0])

    def restore(t, index, map_scene=True):
        ix = torch.tensor(index, dtype=torch.int32, device=DEV)
        b.map_scene = lay['keep'].data_ptr() if map_scene else None
        _lib.check(lib.infgen_restore_scenes(C.byref(b), t, ix.data_ptr(), snap.ptr, stride, head.ptr, N, n_bad.data_ptr(), stream),
                   'infgen_restore_scenes')
        torch.cuda.synchronize()
        return int(n_bad[0])

    def heads():
        return head.data().cpu().numpy().view(np.int32).reshape(N, 4).astype(np.int64)

    def intact():
        return all(v.guards_intact() for v in bufs.values()) and snap.guards_intact() and head.guards_intact()

    for t in (0, 3, steps):
        segs = ref.segments(A_cap, T, ring, L, R, ts, t)
        need = ref.entry_bytes(A_cap, T, ring, L, R, ts, t)
        assert _bytes(lib, b, t) == need
        snap, head = _Buf(N * stride, 90), _Buf(N * 16, 91)
        snap0 = snap.data().cpu().numpy().copy()
        # ---- save slots [4, 1]: the context is unchanged, the entries equal the restatement, nothing else of the buffer is written
        ctx0 = _np(bufs)
        assert save(t, [4, 1]) == 0
        ctx1 = _np(bufs)
        assert all(np.array_equal(ctx0[k], ctx1[k]) for k in ctx0), 'a save writes the context'
        got = snap.data().cpu().numpy().reshape(N, stride)
        for e, slot in enumerate((4, 1)):
            exp = ref.entry(ctx0, segs, S, slot)
            assert exp.size == need and np.array_equal(got[e, :need], exp), (t, e)
            assert np.array_equal(got[e, need:], snap0.reshape(N, stride)[e, need:]), 'bytes past the entry are written'
        assert np.array_equal(got[2], snap0.reshape(N, stride)[2])
        assert heads()[:2].tolist() == ref.head_rows([4, 1], S, GROUP, t)[0].tolist()
        assert intact()
        # ---- entry 2: slot 3 at another step
        other = 3 if t != 3 else 2
        assert save(other, [3], first=2) == 0
        hd = heads()
        assert hd[2].tolist() == [3, 1, other, 1]
        entries = snap.data().cpu().numpy().reshape(N, stride).copy()
        # ---- every context buffer takes a second pattern (x -> 7 x + 13 mod 256 moves every byte)
        for v in bufs.values():
            v.data().copy_(v.data() * 7 + 13)
        ctx2 = _np(bufs)
        assert all((ctx2[k] != ctx0[k]).all() for k in ctx0)
        # ---- restore: fan-out of entry 1 (slot 1's) to slots 0 and 1, an entry of the other group, one of another step, keep, out of range
        index = [1, 1, 0, 2, -1, 9]
        eff, bad = ref.effective_index(index, hd, S, GROUP, t)
        assert (eff, bad) == ([1, 1, -1, -1, -1, -1], 3)
        assert restore(t, index) == bad
        exp = {k: v.copy() for k, v in ctx2.items()}
        for s, e in enumerate(eff):
            if e >= 0:
                assert ref.apply_entry(exp, segs, S, s, entries[e]) == need
        now = _np(bufs)
        for k in now:
            assert np.array_equal(now[k], exp[k]), (k, t)
        for name in SCRATCH:
            assert np.array_equal(now[name], ctx2[name]), name
        for name in STEP_MAJOR:                           # the slices of the steps that have not run are nobody's to move
            assert np.array_equal(now[name].reshape(steps, -1)[t:], ctx2[name].reshape(steps, -1)[t:]), name
        for name in ('pos', 'imask', 'X', ('ringK', 0), ('ringV', L - 1)):
            blocks = (ring if isinstance(name, tuple) else 1, S, -1)
            assert np.array_equal(now[name].reshape(blocks)[:, 0], ctx0[name].reshape(blocks)[:, 1]), 'slot 0 holds what slot 1 held'
            assert np.array_equal(now[name].reshape(blocks)[:, 1], ctx0[name].reshape(blocks)[:, 1])
            assert np.array_equal(now[name].reshape(blocks)[:, 2:], ctx2[name].reshape(blocks)[:, 2:])
        assert np.array_equal(snap.data().cpu().numpy().reshape(N, stride), entries), 'a restore writes the snapshot'
        assert intact()
        # ---- entry 0 into both free slots of its group; a negative entry that is not -1 counts
        index = [-2, -1, -1, -1, 0, 0]
        assert restore(t, index) == 1
        now2 = _np(bufs)
        for s in (4, 5):
            ref.apply_entry(exp, segs, S, s, entries[0])
        for k in now2:
            assert np.array_equal(now2[k], exp[k]), (k, t)
        assert intact()

    # a slot out of range: its entry is not written, its head says so, it is counted, and no restore applies it
    snap, head = _Buf(N * stride, 92), _Buf(N * 16, 93)
    snap0 = snap.data().cpu().numpy().copy().reshape(N, stride)
    ctx0 = _np(bufs)
    assert save(3, [6, 2, -1]) == 2
    got = snap.data().cpu().numpy().reshape(N, stride)
    assert np.array_equal(got[0], snap0[0]) and np.array_equal(got[2], snap0[2]) and not np.array_equal(got[1], snap0[1])
    assert heads().tolist() == ref.head_rows([6, 2, -1], S, GROUP, 3)[0].tolist() == [[6, -1, 3, 0], [2, 0, 3, 1], [-1, -1, 3, 0]]
    assert restore(3, [0, 1, 2, 0, -1, -1]) == 3
    now = _np(bufs)
    exp = {k: v.copy() for k, v in ctx0.items()}
    ref.apply_entry(exp, ref.segments(A_cap, T, ring, L, R, ts, 3), S, 1, got[1])
    assert all(np.array_equal(now[k], exp[k]) for k in now) and intact()
    # no map_scene: every slot is its own group
    assert save(3, [4, 1, 0], map_scene=False) == 0
    assert heads()[:, 1].tolist() == [4, 1, 0]
    assert restore(3, [1, 1, -1, -1, 0, 2], map_scene=False) == 2          # 0 <- slot 1's and 5 <- slot 0's are refused
    assert intact()
    # refused: t out of range, NULL arrays, a short or odd stride, a buffer off alignment, an insertion context
    sl = torch.tensor([4, 1], dtype=torch.int32, device=DEV)
    ix = torch.full((S,), -1, dtype=torch.int32, device=DEV)
    P = lambda x: x.data_ptr()
    need = _bytes(lib, b, 3)

    def both(t=3, sel=True, sp=snap.ptr, st=stride, hd=head.ptr):
        return (lib.infgen_snapshot_scenes(C.byref(b), t, P(sl) if sel else None, 2, sp, st, hd, None, stream),
                lib.infgen_restore_scenes(C.byref(b), t, P(ix) if sel else None, sp, st, hd, 2, None, stream))

    for kw, msg in ((dict(t=-1), b't must be'), (dict(t=steps + 1), b't must be'), (dict(sel=False), b'null'), (dict(sp=None), b'null'),
                    (dict(hd=None), b'null'), (dict(st=need - 16), b'infgen_snapshot_bytes'), (dict(st=need + 8), b'multiple of 16'),
                    (dict(sp=snap.ptr + 8), b'16-byte aligned')):
        for rc in both(**kw):
            assert rc < 0 and msg in lib.infgen_last_error(), kw
    b.first_new = P(ix)
    for rc in both():
        assert rc < 0 and b'insertion' in lib.infgen_last_error()
    torch.cuda.synchronize()
    assert intact()


# ---------------------------------------------------------------------------------------------- 2. rewinding a rollout
def _tempered(c, u, **kw):
    """the sampled engine of the branching tests with a per-scene temperature buffer (all 1): the test changes it on the device"""
    return _sampled(c, u, sample_temperature=np.ones(4, np.float32), **kw)


@pytest.fixture(scope='module')
def control():
    """the uninterrupted sampled rollout every rewound one has to equal: computed once, read only"""
    c = _case('c1_a8_m128')
    eng = _tempered(c, _uniforms(c))
    eng.run(0, c['cfg'].num_decode_steps)
    return _full(eng)


@pytest.mark.parametrize('where', ('first', 'middle', 'last'))
def test_a_rewound_rollout_equals_the_uninterrupted_one(where, control):
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    t = dict(first=0, middle=steps // 2, last=steps - 1)[where]
    E = _tempered(c, _uniforms(c))
    if t:
        E.run(0, t)
    snap = E.snapshot(t)
    assert snap.n == 4 and snap.t == t and snap.stride == _bytes(E.lib, E._ctx, t)
    E.run(t, steps)
    first = _full(E)
    _same(first, control, 'the first pass')
    # the state is overwritten: the same steps again from where the rollout ended, under another temperature
    E.sample_temp_row.fill_(3.0)
    E.run(t, steps)
    torch.cuda.synchronize()
    n_diff = int((E.token != control['token']).sum())
    print(f't = {t}: the overwriting pass differs from the control in {n_diff} stored tokens')
    assert n_diff > 0, 'the overwriting pass leaves the control\'s tokens: it shows nothing'
    E.sample_temp_row.fill_(1.0)
    E.restore(snap)
    assert E._rollout_lp is None and E._rollout_slp is None
    E.run(t, steps)
    again = _full(E)
    torch.cuda.synchronize()
    assert int(E.snapshot_bad[0]) == 0 and int(E.restore_bad[0]) == 0
    _same(again, first, f'rewound to {t} against the first pass')
    _same(again, control, f'rewound to {t} against the uninterrupted rollout')


# ---------------------------------------------------------------------------------------------- 3. fan-out equals branch
def test_fan_out_of_one_entry_equals_a_branch():
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    t = steps // 2
    u = _uniforms(c)
    A, B = _sampled(c, u), _sampled(c, u)
    for eng in (A, B):
        eng.run(0, t)
    A.branch([0, 0, 0, 0], t)
    snap = B.snapshot(t, slots=[0])
    B.restore(snap, torch.tensor([-1, 0, 0, 0], device=DEV))
    B.restore(snap, [-1, 0, 0, -1])                               # a host index, applied again: nothing changes
    torch.cuda.synchronize()
    assert int(A.branch_bad[0]) == 0 and int(B.restore_bad[0]) == 0
    state = lambda e: {**_snap(e), **{k: getattr(e, k).clone() for k in ('X', 'pred_traj', 'pred_head', 'pred_state', 'token_logprob',
                                                                           'sample_logprob', 'tmask', 'imask', 'catflag', 'bos')},
                       **{f'{k}{l}': x.clone() for k in ('ringK', 'ringV') for l, x in enumerate(getattr(e, k))}}
    _same(state(B), state(A), 'fan-out against branch, the state')
    assert torch.equal(B.token[1], B.token[0]) and torch.equal(B.X.view(4, -1)[3], B.X.view(4, -1)[0])
    for eng in (A, B):
        eng.run(t, steps)
    _same(_full(B), _full(A), 'fan-out against branch, the rollouts')


# ---------------------------------------------------------------------------------------------- 4. sessions
WEIGHTS = dict(w_accel=1.0, w_yaw=1.0, accel_limit=0.0, yaw_limit=0.0, w_gap=1.0, gap_limit=50.0)


@pytest.mark.parametrize('pose', ('token', 'exact'))
def test_session_with_lookahead_equals_the_session_without(pose):
    from infgen_amd import branching
    c = _case('c1_a8_m128')
    cfg, hc, av = c['cfg'], c['cfg'].hist_columns, c['av']
    steps, H = cfg.num_decode_steps, 3
    look_at = (0, steps // 2, steps - 2)                   # at the last of them the horizon is cut to the two steps that are left
    step = torch.arange(steps, device=DEV)[:, None]
    cmds = ((step * 131 + torch.arange(4, device=DEV)[None, :] * 517 + 11) % cfg.token_size).int()
    tries = ((cmds.long() * 3 + 37) % cfg.token_size).int()
    free = _eng(c)
    base = torch.cat([free.pos[0, :, av], free.head[0, :, av, None]], -1)        # [T, 3]: the free rollout's ego poses
    off = torch.tensor([[1.0, 0.5, 0.05], [-2.0, 1.0, -0.1], [3.0, -1.5, 0.15], [0.5, 2.5, -0.2]], device=DEV)

    def poses(table, t):                                   # the slot's pose command of step t: the free pose moved by an offset
        return base[hc + t][None] + off[(table[t] % 4).long()]

    def give(ses, table):
        if pose == 'token':
            ses.command(tokens=table[ses.t])
        else:
            ses.command(poses=poses(table, ses.t))

    def drive(ses, until, look=False):
        got = {}
        while ses.t < until:
            if look and ses.t in look_at:
                t0 = ses.t
                h = min(H, steps - t0)
                if pose == 'token':
                    got[t0] = ses.lookahead(H, tokens=tries[t0:t0 + h], weights=WEIGHTS)
                else:
                    got[t0] = ses.lookahead(H, poses=torch.stack([poses(tries, t0 + i) for i in range(h)]), weights=WEIGHTS)
                assert ses.t == t0 and ses._kind is None
            give(ses, cmds)
            ses.advance()
        return got

    kw = dict(run=False, copies=4, step_scores=True)
    plain = _eng(c, **kw)
    sp = plain.session(pose=pose, controlled='ego')
    drive(sp, steps)
    looked = _eng(c, **kw)
    sl = looked.session(pose=pose, controlled='ego')
    lw = drive(sl, steps, look=True)
    torch.cuda.synchronize()
    assert sorted(lw) == list(look_at) and int(looked.restore_bad[0]) == 0 and int(looked.snapshot_bad[0]) == 0
    _same(_snap(looked), _snap(plain), 'session with look-ahead against the session without')
    assert torch.equal(looked.step_score.view(torch.int32), plain.step_score.view(torch.int32))
    assert torch.equal(sl.cost, sp.cost)
    op, ol = sp.outputs(), sl.outputs()
    for s in range(4):
        for key in ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state', 'logits'):
            assert np.array_equal(ol[s][key], op[s][key]), (s, key)
    # the returned weights: a separate engine that really runs the tried commands from that history
    real = _eng(c, **kw)
    for t0 in look_at:
        sr = real.session(pose=pose, controlled='ego')
        drive(sr, t0)
        h = min(H, steps - t0)
        for i in range(h):
            give(sr, tries)
            sr.advance()
        exp = branching.score_log_weight(real.step_score, t0, t0 + h, WEIGHTS, copies=4)
        assert lw[t0].shape == (1, 4) and torch.equal(lw[t0], exp), (t0, lw[t0], exp)
        assert float(lw[t0].abs().sum()) > 0, 'the weights are all zero: they show nothing'
        # and the tries are not the commands: the look-ahead did move the state
        assert not torch.equal(real.pos[:, hc + t0], plain.pos[:, hc + t0])


def test_session_snapshot_and_restore_rewind_the_session():
    c = _case('c1_a8_m128')
    cfg = c['cfg']
    steps, tb = cfg.num_decode_steps, cfg.num_decode_steps // 2
    cmds = ((torch.arange(steps, device=DEV)[:, None] * 131 + torch.arange(4, device=DEV)[None, :] * 517 + 11) % cfg.token_size).int()
    a, b = _eng(c, run=False, copies=4), _eng(c, run=False, copies=4)
    sa, sb = a.session(controlled='ego'), b.session(controlled='ego')
    while not sa.done:
        sa.command(tokens=cmds[sa.t])
        sa.advance()
    snap = None
    while not sb.done:
        if sb.t == tb and snap is None:
            snap = sb.snapshot()
            for _ in range(2):                               # two steps under other commands, then back
                sb.command(tokens=(cmds[sb.t] + 5) % cfg.token_size)
                sb.advance()
            sb.command(tokens=cmds[sb.t])                    # a pending command is dropped by the restore
            sb.restore(snap)
            assert sb.t == tb and sb._kind is None
            assert int((b.teacher_token[:, b.hc + tb:] != -1).sum()) == 0
            with pytest.raises(RuntimeError, match='no command'):
                sb.advance()
        sb.command(tokens=cmds[sb.t])
        sb.advance()
    _same(_snap(b), _snap(a), 'a rewound session against the straight one')


# ---------------------------------------------------------------------------------------------- 5. with the other features on
def test_rewind_under_collision_masks_token_masks_and_step_scores():
    from infgen_amd import constraints
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    t, u = steps // 2, _uniforms(c)
    kw = dict(avoid_collisions=True, step_scores=True, sample_temperature=np.ones(4, np.float32),
              token_masks=constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0}))
    ctl = _sampled(c, u, **kw)
    ctl.run(0, steps)
    want, want_score = _full(ctl), ctl.step_score.clone()
    E = _sampled(c, u, **kw)
    E.run(0, t)
    snap = E.snapshot(t)
    E.sample_temp_row.fill_(3.0)
    E.run(t, steps)
    torch.cuda.synchronize()
    assert not torch.equal(E.step_score.view(torch.int32), want_score.view(torch.int32)) or not torch.equal(E.token, want['token'])
    E.step_score.fill_(-1.0)                                 # the whole block comes back, the steps before t from the entry
    E.sample_temp_row.fill_(1.0)
    E.restore(snap)
    torch.cuda.synchronize()
    assert torch.equal(E.step_score[:, :t].view(torch.int32), want_score[:, :t].view(torch.int32)), 'the step-score log comes back'
    E.run(t, steps)
    _same(_full(E), want, 'rewound under collision masks, token masks and step scores')
    assert torch.equal(E.step_score.view(torch.int32), want_score.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 6. errors and lifecycle
def test_errors_and_lifecycle():
    from infgen_amd import snapshots, torch_ops  # noqa: F401  (registers torch.ops.infgen_hip)
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    u = _uniforms(c)
    ins = _eng(_case('c1_a8_m128', insertion=True), run=False, copies=2)
    with pytest.raises(ValueError, match='insertion'):
        ins.snapshot(0)
    eng = _sampled(c, u)
    cold = _eng(c, run=False, copies=4)
    with pytest.raises(RuntimeError, match='prologue'):
        cold.snapshot(0)
    for t in (-1, steps + 1):
        with pytest.raises(ValueError, match='outside'):
            eng.snapshot(t)
    eng.run(0, 3)
    snap = eng.snapshot(3)
    with pytest.raises(RuntimeError, match='prologue'):
        cold.restore(snap)
    cold.prologue()
    with pytest.raises(ValueError, match='another engine layout'):
        cold.restore(snap)
    other = _eng(c, run=False, copies=2)
    other.prologue()
    with pytest.raises(ValueError, match='another engine layout'):
        other.restore(snap)
    with pytest.raises(ValueError, match=r'slots\[1\] = 4'):
        eng.snapshot(3, slots=[0, 4])
    with pytest.raises(ValueError, match=r'index\[1\] = 4 is neither'):
        eng.restore(snap, [0, 4, -1, -1])
    with pytest.raises(ValueError, match='shape'):
        eng.restore(snap, [0, 1])
    with pytest.raises(ValueError, match='integer'):
        eng.restore(snap, torch.zeros(4))
    # out=: a buffer of too few entries, or taken for an earlier step, is refused; one of enough capacity is reused
    small = eng.snapshot(3, slots=[0, 1])
    with pytest.raises(ValueError, match='out= holds 2 entries'):
        eng.snapshot(3, out=small)
    with pytest.raises(ValueError, match='out= holds'):
        eng.snapshot(steps, slots=[0, 1], out=small)
    with pytest.raises(ValueError, match='layout'):
        other.snapshot(0, out=small)
    room = eng.snapshot_buffer()
    assert room.capacity == 4 and room.stride == snapshots.entry_bytes(eng, steps) and room.n == 0
    with pytest.raises(ValueError, match='no entry'):
        eng.restore(room)
    again = eng.snapshot(3, out=room)
    assert again is room and room.n == 4 and room.t == 3
    need = snap.stride
    torch.cuda.synchronize()
    assert torch.equal(room.buf[:, :need], snap.buf) and torch.equal(room.head, snap.head)
    # a device slot vector is not read: the slot out of range is counted, its entry goes nowhere
    dev_snap = eng.snapshot(3, slots=torch.tensor([2, 7], device=DEV))
    before = {**_snap(eng), 'X': eng.X.clone(), 'ringK0': eng.ringK[0].clone()}
    # an identity restore changes nothing
    eng.restore(snap)
    eng.restore(dev_snap)
    eng.restore(snap, torch.tensor([[0, 1, 2, 9]], device=DEV))
    torch.cuda.synchronize()
    assert int(eng.snapshot_bad[0]) == 1 and int(eng.restore_bad[0]) == 1
    assert dev_snap.head.tolist() == [[2, 0, 3, 1], [7, -1, 3, 0]]
    _same({**_snap(eng), 'X': eng.X.clone(), 'ringK0': eng.ringK[0].clone()}, before, 'identity restores')
    # the torch ops: the same bytes as the methods
    buf, head = torch.zeros_like(snap.buf), torch.zeros_like(snap.head)
    bad = torch.ops.infgen_hip.snapshot_scenes(eng.ctx_tensor(), 3, torch.arange(4, device=DEV), buf, head)
    eng.run(3, steps)
    plain = _full(eng)
    bad2 = torch.ops.infgen_hip.restore_scenes(eng.ctx_tensor(), 3, torch.arange(4, device=DEV), buf, head)
    eng.run(3, steps)
    torch.cuda.synchronize()
    assert int(bad[0]) == 0 and int(bad2[0]) == 0 and torch.equal(buf, snap.buf) and torch.equal(head, snap.head)
    eng._rollout_lp = eng._rollout_slp = None
    _same(_full(eng), plain, 'torch.ops.infgen_hip.restore_scenes')
    with pytest.raises(RuntimeError, match='t must be'):
        torch.ops.infgen_hip.snapshot_scenes(eng.ctx_tensor(), steps + 1, torch.arange(4, device=DEV), buf, head)
    # a snapshot does not outlive its batch
    eng.reload([c['scene']], sample_uniforms=u)
    eng.prologue()
    with pytest.raises(ValueError, match='before a reload'):
        eng.restore(snap)
    eng.restore(eng.snapshot(0))
