"""Timing of branching rollouts (``RolloutEngine.branch``, k_branch_scenes); bench.py is untouched.

    python tools/bench_branching.py [--parent DIR] [--rounds 3] [--log profiles/branching.log]

Set-up: 32 C3 scenes x 32 copies (1024 slots, 64 agents, 1024 map tokens, 16 decode steps), ``sample_k = 5``, ``token_logprob``,
``avoid_collisions`` off.  Every sample is a fresh process; the variants of a figure alternate A B A B ... so that drift of the
machine lands on all of them alike, and medians are reported.  Figures:

    (a) branch      one ``branch`` at the middle step that moves half of the slots (copies 16..31 of every scene become clones of
                    copies 0..15), between device events: the bytes moved (read + written) and GB/s - against the same move
                    restated as per-buffer torch ``index_select`` + ``index_copy_`` calls.  Both are idempotent, so the samples of
                    one process alternate too.
    (b) pruning     every 4 steps ``keep_best(score, copies / 2)`` with score = "no box of the slot has overlapped another so far"
                    (separating-axis test on the stored poses, torch) and the sum of ``token_logprob`` so far as tie-break; the
                    box-overlap rate of the final rollouts and the rollout time, with and without pruning (the unpruned variant
                    computes the same scores and drops them, so the difference is the resampling and the branch).  The tie-break
                    is the running sum over every row of the layout, not ``rollout_logprob()`` (which exists only after the
                    epilogue); with 64 agents in 64 rows, no padding and no forced rows, both sum the same entries.
    (c) unbranched  the sampled rollout without any branch in this tree and in ``--parent`` (a built checkout of the parent
                    commit): the same launches, so no change is expected.  Skipped without ``--parent``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import json, sys
root, mode, warmup, reps, shapes_json = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(shapes_json) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
S0, N = 32, 32
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(S0)]
steps, hc = cfg.num_decode_steps, cfg.hist_columns
u = np.random.default_rng(7).random((steps, S0 * N, 64), dtype=np.float32)
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, copies=N, sample_k=5, sample_uniforms=u, token_logprob=True)
S, A = eng.S, eng.A_cap

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)

def overlapping(c):
    """[S, A] bool: the row's box overlaps another row's of its slot at column c (separating-axis test, fp32)"""
    half = 0.5 * eng._shape10[:, :, :2]
    p, h, ok = eng.pos[:, c], eng.head[:, c], eng.state[:, c] != 0
    ux = torch.stack([torch.cos(h), torch.sin(h)], -1); vx = torch.stack([-torch.sin(h), torch.cos(h)], -1)
    d = p[:, None] - p[:, :, None]
    sep = torch.full((S, A, A), -1e30, device=dev)
    for ax in (ux[:, :, None], vx[:, :, None], ux[:, None], vx[:, None]):
        ri = half[:, :, None, 0] * (ux[:, :, None] * ax).sum(-1).abs() + half[:, :, None, 1] * (vx[:, :, None] * ax).sum(-1).abs()
        rj = half[:, None, :, 0] * (ux[:, None] * ax).sum(-1).abs() + half[:, None, :, 1] * (vx[:, None] * ax).sum(-1).abs()
        sep = torch.maximum(sep, (d * ax).sum(-1).abs() - (ri + rj))
    pair = ok[:, :, None] & ok[:, None] & ~torch.eye(A, dtype=torch.bool, device=dev)[None]
    return ((sep < 0) & pair).any(-1), ok

def overlap_rate():
    hit = tot = 0
    for c in range(hc, hc + steps):
        o, ok = overlapping(c)
        hit += int(o.sum()); tot += int(ok.sum())
    return hit / max(tot, 1)

out = dict(rows=int(eng.rows), slots=S, steps=steps)
if mode == 'branch':
    from infgen_amd import branching
    tb = steps // 2
    eng.prologue(); eng.run(0, tb)
    slot = torch.arange(S, device=dev).view(S0, N)
    parent = torch.where(slot % N >= N // 2, slot - N // 2, slot).int().contiguous()
    dst = torch.nonzero(parent.view(-1) != slot.view(-1)).view(-1); src = parent.view(-1)[dst].long()
    scene_major = [eng.pos, eng.head, eng.state, eng.token, eng.gridtok, eng.tmask, eng.imask, eng.catflag, eng.bos,
                   eng.X.view(S, -1), eng.pred_traj, eng.pred_head, eng.pred_state]
    rings = [r.view(eng.ring, S, -1) for r in eng.ringK + eng.ringV]
    logs = [eng.token_logprob.view(steps, S, -1)[:tb]]
    def restated():
        for b in scene_major:
            b.index_copy_(0, dst, b.index_select(0, src))
        for b in rings + logs:
            b.index_copy_(1, dst, b.index_select(1, src))
    per_slot = sum(b[0].numel() * b.element_size() for b in scene_major) + sum(b[:, 0].numel() * b.element_size() for b in rings + logs)
    out.update(moved_slots=int(dst.numel()), bytes_per_slot=int(per_slot), torch_calls=2 * (len(scene_major) + len(rings) + len(logs)))
    before = {k: getattr(eng, k).clone() for k in ('pos', 'token', 'X', 'token_logprob')}
    eng.branch(parent, tb); k1 = {k: getattr(eng, k).clone() for k in before}
    for k, v in before.items():
        getattr(eng, k).copy_(v)
    restated(); torch.cuda.synchronize()
    out['same_bytes'] = all(torch.equal(getattr(eng, k), k1[k]) for k in before) and int(eng.branch_bad[0]) == 0
    eng.branch(parent, tb); torch.cuda.synchronize()
    ka, ta = [], []
    for _ in range(reps):
        ka.append(timed(lambda: eng.branch(parent, tb)))
        ta.append(timed(restated))
    moved = 2.0 * per_slot * int(dst.numel())
    out.update(ms=float(np.median(ka)), kernel_ms=ka, torch_ms=float(np.median(ta)), torch_all_ms=ta, bytes_moved=moved,
               kernel_gbs=moved / (1e6 * float(np.median(ka))), torch_gbs=moved / (1e6 * float(np.median(ta))))
elif mode in ('prune', 'noprune'):
    from infgen_amd import branching
    def rollout():
        eng.prologue()
        clean = torch.ones(S, dtype=torch.bool, device=dev)
        for t0 in range(0, steps, 4):
            t1 = min(t0 + 4, steps)
            eng.run(t0, t1)
            if t1 == steps:
                break
            for c in range(hc + t0, hc + t1):
                clean &= ~overlapping(c)[0].any(-1)
            lp = eng.token_logprob[:t1].view(t1, S, A).sum((0, 2))
            score = (clean.double() * 1e9 + lp.double()).view(S0, N)
            par = branching.keep_best(score, N // 2)
            if mode == 'prune':
                eng.branch(par, t1)
                clean = clean[par.view(-1).long()]
    for _ in range(warmup):
        rollout()
    torch.cuda.synchronize()
    ms = [timed(rollout) for _ in range(reps)]
    out.update(ms=float(np.median(ms)), all_ms=ms, overlap_rate=overlap_rate())
else:                                  # 'plain': the unbranched sampled rollout (runs in the parent's tree too)
    for _ in range(warmup):
        eng.rollout()
    torch.cuda.synchronize()
    ms = [timed(eng.rollout) for _ in range(reps)]
    out.update(ms=float(np.median(ms)), all_ms=ms)
print(json.dumps(out))
'''


def run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'worker {cmd[4]} failed ({out.returncode}): {out.stderr[-1500:]}')
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (figure c)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--branch-reps', type=int, default=15)
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'branching.log'))
    a = ap.parse_args()
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    worker = lambda root, mode, reps=a.reps: run([sys.executable, '-c', WORKER, root, mode, str(a.warmup), str(reps), shapes])
    figures = [('(a) one branch moving half of 1024 slots at the middle step', [('branch', lambda: worker(REPO, 'branch', a.branch_reps))]),
               ('(b) keep_best every 4 steps', [('without pruning', lambda: worker(REPO, 'noprune')), ('with pruning', lambda: worker(REPO, 'prune'))])]
    if a.parent:
        parent = os.path.abspath(a.parent)
        figures.append(('(c) unbranched sampled rollout', [('parent', lambda: worker(parent, 'plain')), ('this', lambda: worker(REPO, 'plain'))]))
    results = []

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, 'w') as f:
            f.write('\n'.join(json.dumps(r) for r in results) + '\n')

    for figure, variants in figures:
        entry = dict(figure=figure, rounds=0)
        results.append(entry)
        got = {name: [] for name, _ in variants}
        for r in range(a.rounds):
            for name, fn in variants:          # alternating: one sample of every variant per round
                s = fn()
                got[name].append(s)
                ms = [x['ms'] for x in got[name]]
                entry[name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), samples=ms)
                for k in ('overlap_rate', 'moved_slots', 'bytes_per_slot', 'bytes_moved', 'torch_calls', 'same_bytes', 'rows', 'slots', 'steps'):
                    if k in s:
                        entry[name][k] = s[k]
                if name == 'branch':
                    tm = statistics.median(x['torch_ms'] for x in got[name])
                    entry[name].update(torch_median_ms=tm, torch_samples=[x['torch_ms'] for x in got[name]],
                                       kernel_gbs=s['bytes_moved'] / (1e6 * entry[name]['median_ms']), torch_gbs=s['bytes_moved'] / (1e6 * tm),
                                       not_slower_than_torch=entry[name]['median_ms'] <= tm)
                print(f'{figure}: round {r} {name}: {s["ms"]:.3f} ms', flush=True)
                write()
            entry['rounds'] = r + 1
        if 'parent' in entry:
            entry['gate'] = 'pass' if entry['this']['median_ms'] <= entry['parent']['max_ms'] else 'FAIL'
        write()
        print(json.dumps(entry), flush=True)


if __name__ == '__main__':
    main()
