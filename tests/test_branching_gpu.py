"""GPU: branching rollouts ("branching" of include/infgen_hip.h) - infgen_branch_scenes against a torch restatement
over a hand-built context, a branched rollout against the rollout that had that history all along, closed-loop sessions,
infgen_resample_parents and the resamplers against tests/branch_ref.py, errors and lifecycle."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import branch_ref as ref
from test_replay_gpu import _case, _eng, _same, _snap

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device('cuda:0')

# ---------------------------------------------------------------------------------------------- 1. the operator
# every non-const pointer member of InfgenRollout, classified by THIS test (not by the implementation's table): what a branch has to
# move, and the scratch a decode step rewrites before it reads it, which a branch must leave alone.  A member the header gains and
# this list does not know fails the test.
SCENE_MAJOR = ('pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag', 'bos', 'X', 'pred_traj', 'pred_head', 'pred_state')
RINGS = ('ringK', 'ringV')
STEP_MAJOR = ('logits', 'token_logprob', 'sample_logprob')
SCRATCH = ('Q', 'U', 'Ka', 'Va', 'AGG', 'Z', 'SIG', 'raw2', 'cat', 'fus_in', 'tmp1', 'tmp2', 'next_token', 'next_state',
           'logits_scratch', 'tap_x')
LEAD, TAIL, SENT = 256, 256, 0xA5


def _writable_pointers():
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    body = re.search(r'typedef struct InfgenRollout \{(.*?)\} InfgenRollout;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for stmt in body.split(';'):
        stmt = stmt.strip()
        if '*' in stmt and not stmt.startswith('const'):
            names.append(re.match(r'[\w\s]+\*\s*(\w+)', stmt).group(1))
    return names


class _Buf:
    """a device allocation with a sentinel lead and tail around `n` payload bytes that start `shift` bytes off 16-byte alignment"""

    def __init__(self, n, buf_id, shift=0):
        self.n, self.lo = n, LEAD + shift
        self.raw = torch.full((self.lo + n + TAIL,), SENT, dtype=torch.uint8, device=DEV)
        assert self.raw.data_ptr() % 16 == 0
        idx = torch.arange(n, device=DEV, dtype=torch.int64)
        self.raw[self.lo:self.lo + n] = ((idx * 131 + (idx >> 8) * 7 + (idx >> 16) * 3 + buf_id * 53) & 0xff).to(torch.uint8)
        self.ptr = self.raw.data_ptr() + self.lo

    def data(self):
        return self.raw[self.lo:self.lo + self.n]

    def guards_intact(self):
        return bool((self.raw[:self.lo] == SENT).all()) and bool((self.raw[self.lo + self.n:] == SENT).all())


def _context(A_cap, cfg, shifts):
    from infgen_amd import _lib
    S, T, W, L = 6, cfg.num_columns, cfg.window, cfg.num_agent_layers
    ring, R, steps, ts = W + 1, cfg.num_recurrent_steps_val, cfg.num_columns - 2, 96
    b = _lib.Rollout()
    b.S, b.A_cap, b.T, b.M_cap, b.W, b.ring, b.R = S, A_cap, T, 32, W, ring, R
    b.token_size, b.grid_size, b.num_layers, b.store_logits = ts, 64, L, 1
    per_scene = dict(pos=T * A_cap * 8, head=T * A_cap * 4, state=T * A_cap * 4, token=T * A_cap * 4, grid=T * A_cap * 4,
                     tmask=T * A_cap, imask=T * A_cap, catflag=T * A_cap, bos=A_cap * 4, X=A_cap * 512,
                     pred_traj=A_cap * R * 8, pred_head=A_cap * R * 4, pred_state=A_cap * R * 4,
                     logits=A_cap * ts * 4, token_logprob=A_cap * 4, sample_logprob=A_cap * 4)
    bufs, k = {}, 0
    for name in SCENE_MAJOR:
        bufs[name] = _Buf(S * per_scene[name], k, shifts.get(name, 0)); k += 1
        setattr(b, name, bufs[name].ptr)
    for name in RINGS:
        for l in range(L):
            bufs[name, l] = _Buf(ring * S * A_cap * 512, k); k += 1
            getattr(b, name)[l] = bufs[name, l].ptr
    for name in STEP_MAJOR:
        bufs[name] = _Buf(steps * S * per_scene[name], k); k += 1
        setattr(b, name, bufs[name].ptr)
    for name in SCRATCH:
        bufs[name] = _Buf(S * A_cap * 512, k); k += 1
        setattr(b, name, bufs[name].ptr)
    ms = torch.tensor([0, 0, 0, 1, 1, 1], dtype=torch.int32, device=DEV)
    b.map_scene = ms.data_ptr()
    lay = dict(S=S, steps=steps, ring=ring, L=L, per_scene=per_scene, keep=ms)
    return b, bufs, lay


def _expected(before, lay, parent, t):
    """the restatement: buf[s] = buf[parent[s]] per scene block; the [0, t) prefix only for the step-major buffers"""
    S, steps, ring = lay['S'], lay['steps'], lay['ring']
    p = torch.as_tensor(parent, device=DEV, dtype=torch.long)
    exp = {}
    for key, old in before.items():
        name = key[0] if isinstance(key, tuple) else key
        if name in SCENE_MAJOR:
            exp[key] = old.view(S, -1)[p].reshape(-1)
        elif name in RINGS:
            exp[key] = old.view(ring, S, -1)[:, p].reshape(-1)
        elif name in STEP_MAJOR:
            v = old.view(steps, S, -1).clone()
            v[:t] = v[:t, p]
            exp[key] = v.reshape(-1)
        else:
            exp[key] = old
    return exp


@pytest.mark.parametrize('A_cap', (32, 96))
def test_branch_scenes_against_the_torch_restatement(A_cap):
    from infgen_amd import _lib
    c = _case('c1_a8_m128')
    lib = _lib.load()
    names = _writable_pointers()
    assert set(names) == set(SCENE_MAJOR + RINGS + STEP_MAJOR + SCRATCH), 'a writable member of InfgenRollout this test does not classify'
    # A_cap 96: two byte arrays off 16-byte alignment (the byte-by-byte path), blocks of several chunks and a partial last chunk
    shifts = dict(imask=1, catflag=4) if A_cap == 96 else {}
    b, bufs, lay = _context(A_cap, c['cfg'], shifts)
    steps = lay['steps']
    n_bad = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream

    def call(parent, t, expect_bad, map_scene=True):
        before = {k: v.data().clone() for k, v in bufs.items()}
        par = torch.tensor(parent, dtype=torch.int32, device=DEV)
        b.map_scene = lay['keep'].data_ptr() if map_scene else None
        _lib.check(lib.infgen_branch_scenes(C.byref(b), t, par.data_ptr(), n_bad.data_ptr(), stream), 'infgen_branch_scenes')
        torch.cuda.synchronize()
        assert int(n_bad[0]) == expect_bad, (parent, t, int(n_bad[0]))
        eff = ref.effective(parent, 3 if map_scene else 1)
        exp = _expected(before, lay, eff, t)
        for k, v in bufs.items():
            assert torch.equal(v.data(), exp[k]), (k, parent, t)
            assert v.guards_intact(), (k, parent, t)
        moved = [s for s in range(lay['S']) if eff[s] != s]
        return before, moved

    for t in (0, 3, steps):
        before, moved = call([0, 0, 2, 3, 3, 3], t, 0)
        assert moved == [1, 4, 5]
        # (the restatement above already pins these; spelled out) fixed-point slots and the steps >= t of the logs are unchanged
        for key in ('pos', 'logits', ('ringK', 0)):
            now, old = bufs[key].data(), before[key]
            blocks = (lay['ring'] if key == ('ringK', 0) else steps if key == 'logits' else 1, lay['S'], -1)
            assert torch.equal(now.view(blocks)[:, [0, 2, 3]], old.view(blocks)[:, [0, 2, 3]])
        assert torch.equal(bufs['logits'].data().view(steps, -1)[t:], before['logits'].view(steps, -1)[t:])
        if t > 0:
            assert not torch.equal(bufs['logits'].data().view(steps, -1)[:t], before['logits'].view(steps, -1)[:t])
    # entries that break the contract: -1, S, the other group, chains - counted, read as the identity; the good ones are applied
    _, moved = call([0, 0, 1, -1, 6, 3], 3, 4)            # 1 <- 0 is good; 2 <- 1 (1 is moved), -1, S, and 5 <- 3 (3's entry is no fixed point)
    assert moved == [1]
    _, moved = call([0, 4, 2, 3, 3, 0], 3, 2)             # 1 <- 4 and 5 <- 0 cross the groups; 4 <- 3 is good
    assert moved == [4]
    _, moved = call([2 ** 31 - 1, -2 ** 31, 2, 3, 3, 3], steps, 2)
    assert moved == [4, 5]
    _, moved = call([0, 0, 2, 3, 3, 3], 3, 3, map_scene=False)      # no map_scene: every scene is its own group
    assert moved == []
    # refused: t out of range, a null parent, an insertion context
    par = torch.arange(6, dtype=torch.int32, device=DEV)
    for t in (-1, steps + 1):
        assert lib.infgen_branch_scenes(C.byref(b), t, par.data_ptr(), None, stream) != 0 and b't must be' in lib.infgen_last_error()
    assert lib.infgen_branch_scenes(C.byref(b), 0, None, None, stream) != 0
    b.first_new = par.data_ptr()
    assert lib.infgen_branch_scenes(C.byref(b), 0, par.data_ptr(), None, stream) != 0 and b'insertion' in lib.infgen_last_error()


# ---------------------------------------------------------------------------------------------- 2. branched rollouts
# the uniforms of the sampled engines: seed 11, one independent stream per (step, slot, row).  Under it the unbranched control
# alone shows slots 1 and 0 (and 3 and 2) apart in stored tokens after every branch point used here (asserted below).
SEED = 11
EXTRA = ('token_logprob', 'sample_logprob', 'pred_traj', 'pred_head', 'pred_state')


def _uniforms(c):
    steps = c['cfg'].num_decode_steps
    return np.random.default_rng(SEED).random((steps, 4, 8), dtype=np.float32)


def _sampled(c, u, **kw):
    eng = _eng(c, run=False, copies=4, sample_k=5, sample_uniforms=u, token_logprob=True, sample_logprob=True, **kw)
    eng.prologue()
    return eng


def _full(eng):
    """everything a rollout leaves: stored columns, logits of all steps, both logs, pred_*, the rollout log-likelihoods"""
    out = _snap(eng)
    out.update({k: getattr(eng, k).clone() for k in EXTRA})
    eng.outputs_device()
    out['rollout_logprob'] = eng.rollout_logprob().clone()
    out['rollout_sample_logprob'] = eng.rollout_sample_logprob().clone()
    torch.cuda.synchronize()
    return out


def _control_uniforms(u, tb):
    uc = u.copy()
    uc[:tb, 1] = u[:tb, 0]
    uc[:tb, 3] = u[:tb, 2]
    return uc


def _branched_against_control(c, tb, **kw):
    steps, hc = c['cfg'].num_decode_steps, c['cfg'].hist_columns
    u = _uniforms(c)
    E = _sampled(c, u, **kw)
    E.run(0, tb)
    E.branch([0, 0, 2, 2], tb)
    E.run(tb, steps)
    C_ = _sampled(c, _control_uniforms(u, tb), **kw)
    C_.run(0, steps)
    torch.cuda.synchronize()
    assert int(E.branch_bad[0]) == 0
    e, ctl = _full(E), _full(C_)
    _same(e, ctl, f'branched at {tb} against the control')
    tok = ctl['token']
    assert torch.equal(tok[1, :hc + tb], tok[0, :hc + tb]) and torch.equal(tok[3, :hc + tb], tok[2, :hc + tb])
    n01 = int((tok[1, hc + tb:] != tok[0, hc + tb:]).sum())
    print(f'tb = {tb}: slots 1 / 0 differ in {n01} stored tokens after the branch point')
    assert n01 > 0, 'the branch does not diverge: choose other uniforms'
    return E


@pytest.mark.parametrize('where', ('first', 'middle', 'last'))
def test_a_branched_rollout_equals_the_rollout_with_that_history(where):
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    _branched_against_control(c, dict(first=1, middle=steps // 2, last=steps - 1)[where])


def test_branched_rollout_under_collision_and_token_masks():
    from infgen_amd import constraints
    c = _case('c1_a8_m128')
    tb = c['cfg'].num_decode_steps // 2
    _branched_against_control(c, tb, avoid_collisions=True)
    _branched_against_control(c, tb, token_masks=constraints.TokenMasks.from_vocab(c['vocab'], {'max_speed': 4.0}))


def test_identity_branch_changes_nothing():
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    u = _uniforms(c)
    A, B = _sampled(c, u), _sampled(c, u)
    A.run(0, steps)
    B.run(0, 4)
    B.branch(torch.arange(4, device=DEV), 4)
    B.branch(np.arange(4).reshape(1, 4), 4)
    B.run(4, steps)
    _same(_full(B), _full(A), 'identity branch')
    for k in ('X', 'ringK', 'ringV'):
        a, b = getattr(A, k), getattr(B, k)
        assert all(torch.equal(x, y) for x, y in (zip(a, b) if isinstance(a, list) else [(a, b)])), k


# ---------------------------------------------------------------------------------------------- 3. sessions
@pytest.mark.parametrize('pose', ('token', 'exact'))
def test_session_branch(pose):
    c = _case('c1_a8_m128')
    cfg, hc, av = c['cfg'], c['cfg'].hist_columns, c['av']
    steps, tb = cfg.num_decode_steps, cfg.num_decode_steps // 2
    cmds = ((torch.arange(steps, device=DEV)[:, None] * 131 + torch.arange(4, device=DEV)[None, :] * 517 + 11) % cfg.token_size).int()
    ctl_cmds = cmds.clone()
    ctl_cmds[:tb, 1], ctl_cmds[:tb, 3] = cmds[:tb, 0], cmds[:tb, 2]
    free = _eng(c)                                           # pose commands: the free rollout's ego poses, moved per slot
    base = torch.cat([free.pos[0, :, av], free.head[0, :, av, None]], -1)        # [T, 3]
    off = torch.tensor([[1.0, 0.5, 0.05], [-2.0, 1.0, -0.1], [3.0, -1.5, 0.15], [0.5, 2.5, -0.2]], device=DEV)

    def drive(ses, table, branch_at=None):
        while not ses.done:
            if ses.t == branch_at:
                ses.branch([0, 0, 2, 2])
                o = ses.observe()
                torch.cuda.synchronize()
                for k in ('pos', 'head', 'state', 'token'):
                    assert torch.equal(o[k][1], o[k][0]) and torch.equal(o[k][3], o[k][2]), k
            if pose == 'token':
                ses.command(tokens=table[ses.t])
            else:
                slot = table[ses.t] % 4                      # which offset the slot's command of this step takes
                ses.command(poses=base[hc + ses.t][None] + off[slot.long()])
            ses.advance()
        return ses

    slots = torch.arange(4, device=DEV).repeat(steps, 1).int()
    ctl_slots = slots.clone()
    ctl_slots[:tb, 1], ctl_slots[:tb, 3] = 0, 2
    e = _eng(c, run=False, copies=4)
    se = drive(e.session(pose=pose, controlled='ego'), cmds if pose == 'token' else slots, branch_at=tb)
    k = _eng(c, run=False, copies=4)
    sk = drive(k.session(pose=pose, controlled='ego'), ctl_cmds if pose == 'token' else ctl_slots)
    _same(_snap(e), _snap(k), 'session branched against the control session')
    oe, ok = se.outputs(), sk.outputs()
    for s in range(4):
        for key in ('next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'pred_state', 'logits'):
            assert np.array_equal(oe[s][key], ok[s][key]), (s, key)
    tok = _snap(e)['token']
    assert not torch.equal(tok[1, hc + tb:], tok[0, hc + tb:]), 'the clone follows its own commands after the branch'


# ---------------------------------------------------------------------------------------------- 4. parent vectors
@pytest.mark.parametrize('S0,copies', ((1, 1), (3, 2), (2, 33), (1, 1024)))
def test_resample_parents_against_the_restatement(S0, copies):
    from infgen_amd import branching
    from test_branching_cpu import _ancestors
    rng = np.random.default_rng(S0 * 131 + copies)
    for kind in ('random', 'same', 'identity', 'outside'):
        anc = _ancestors(rng, S0, copies, kind).astype(np.int32)
        got = branching.resample_parents(torch.from_numpy(anc).to(DEV), copies).cpu().numpy().astype(np.int64)
        exp = ref.resample_parents(anc, copies)
        assert np.array_equal(got, exp), kind
        clean = ref.sanitise(anc, copies)
        assert (got[got] == got).all() and ref.bad_entries(got, copies) == []
        for g0 in range(0, S0 * copies, copies):
            assert sorted(got[g0:g0 + copies]) == sorted(clean[g0:g0 + copies])
        named = np.unique(clean)
        assert (got[named] == named).all()
        shaped = branching.resample_parents(torch.from_numpy(anc.reshape(S0, copies)).to(DEV), copies)
        assert tuple(shaped.shape) == (S0, copies) and np.array_equal(shaped.cpu().numpy().reshape(-1), exp)
    with pytest.raises(ValueError):
        branching.resample_parents(torch.zeros(4, dtype=torch.int32, device=DEV), 1025)


def test_resamplers_against_numpy_and_into_branch():
    from infgen_amd import branching
    rng = np.random.default_rng(5)
    # integer weights and u away from the bin edges k / n of the cumulative sums: float order cannot matter
    w = rng.integers(1, 9, (3, 4)).astype(np.float64)
    u = np.asarray([0.3137, 0.7713, 0.0519])
    cdf = np.cumsum(w / w.sum(1, keepdims=True), 1)
    at = (u[:, None] + np.arange(4)) / 4
    assert np.abs(cdf[:, None, :] - at[:, :, None]).min() > 1e-6
    sa = branching.systematic_ancestors(torch.from_numpy(np.log(w)).to(DEV), torch.from_numpy(u).to(DEV))
    assert sa.dtype == torch.int32 and np.array_equal(sa.cpu().numpy(), ref.systematic_ancestors(np.log(w), u))
    score = rng.integers(0, 3, (3, 4)).astype(np.float32)
    for keep in (1, 2, 4):
        kb = branching.keep_best(torch.from_numpy(score).to(DEV), keep)
        assert np.array_equal(kb.cpu().numpy(), ref.keep_best(score, keep)), keep
    # into branch: three scenes x four copies
    from infgen_amd import synth
    c = _case('c1_a8_m128')
    scenes = [c['scene']] + [synth.make_scene(synth.scene_seed(1, k), 8, 128, c['cfg'], vocab=c['vocab'], grid=c['grid']) for k in (1, 2)]
    eng = _eng(c, scenes, run=False, copies=4)
    eng.prologue()
    eng.run(0, 3)
    parent = branching.resample_parents(sa, 4)
    eng.branch(parent, 3)
    eng.branch(branching.keep_best(torch.from_numpy(score).to(DEV), 2), 3)
    torch.cuda.synchronize()
    assert int(eng.branch_bad[0]) == 0
    p = parent.cpu().numpy().reshape(-1)
    assert ref.bad_entries(p, 4) == [] and (p != np.arange(12)).any()


# ---------------------------------------------------------------------------------------------- 5. errors and lifecycle
def test_errors_and_lifecycle():
    from infgen_amd import torch_ops  # noqa: F401  (registers torch.ops.infgen_hip)
    c = _case('c1_a8_m128')
    steps = c['cfg'].num_decode_steps
    u = _uniforms(c)
    ins = _eng(_case('c1_a8_m128', insertion=True), run=False, copies=2)
    with pytest.raises(ValueError, match='insertion'):
        ins.branch([0, 0], 0)
    eng = _eng(c, run=False, copies=4, sample_k=5, sample_uniforms=u, token_logprob=True, sample_logprob=True)
    with pytest.raises(RuntimeError, match='prologue'):
        eng.branch([0, 0, 2, 2], 0)
    eng.rollout()
    plain = _full(eng)
    assert eng._rollout_lp is not None
    for t in (-1, steps + 1):
        with pytest.raises(ValueError, match='outside'):
            eng.branch([0, 0, 2, 2], t)
    with pytest.raises(ValueError, match=r'parent\[2\] = 1 .*fixed point'):
        eng.branch([0, 0, 1, 3], 2)
    with pytest.raises(ValueError, match=r'parent\[3\] = 4'):
        eng.branch(np.asarray([0, 1, 2, 4]), 2)
    with pytest.raises(ValueError, match='shape'):
        eng.branch([0, 0], 2)
    with pytest.raises(ValueError, match='integer'):
        eng.branch(torch.zeros(4), 2)
    two = _eng(c, [c['scene'], c['scene']], run=False, copies=2)
    two.prologue()
    with pytest.raises(ValueError, match=r'parent\[2\] = 1 .*another copy group'):
        two.branch([0, 0, 1, 3], 0)
    one = _eng(c, run=False)
    one.prologue()
    one.branch([0], 0)
    flat = _eng(c, [c['scene'], c['scene']])
    assert int(flat.branch_bad[0]) == 0                   # (the counter exists before the first branch)
    with pytest.raises(ValueError, match='copies == 1'):
        flat.branch([0, 0], 0)
    kept = _snap(flat)
    flat.branch(torch.tensor([1, 0], device=DEV), 0)      # a device vector is not read: both entries count, nothing moves
    torch.cuda.synchronize()
    assert int(flat.branch_bad[0]) == 2
    _same(_snap(flat), kept, 'copies == 1: a device parent moves nothing')
    # a branched run, then reset() + rollout(): the unbranched rollout again, bit for bit
    eng.prologue()
    eng.run(0, 3)
    eng.branch(torch.tensor([[0, 0, 2, 2]], device=DEV), 3)
    assert eng._rollout_lp is None and eng._rollout_slp is None
    eng.run(3, steps)
    branched = _full(eng)
    assert not torch.equal(branched['token'], plain['token'])
    eng.reset()
    eng.rollout()
    _same(_full(eng), plain, 'rollout() after a branched run')
    # the torch op: the same bytes as the method
    eng.prologue()
    eng.run(0, 3)
    bad = torch.ops.infgen_hip.branch_scenes(eng.ctx_tensor(), 3, torch.tensor([0, 0, 2, 2], device=DEV))
    eng.run(3, steps)
    assert int(bad[0]) == 0
    _same(_full(eng), branched, 'torch.ops.infgen_hip.branch_scenes')
    with pytest.raises(RuntimeError, match='t must be'):
        torch.ops.infgen_hip.branch_scenes(eng.ctx_tensor(), steps + 1, torch.arange(4, device=DEV))
