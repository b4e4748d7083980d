"""Timing of snapshots (``RolloutEngine.snapshot`` / ``restore``, k_snapshot_scenes); bench.py is untouched.

    python tools/bench_snapshot.py [--parent DIR] [--rounds 3] [--log profiles/snapshot.log]

Set-up of (a) and (b): that of tools/bench_branching.py - 32 C3 scenes x 32 copies (1024 slots, 64 agents, 1024 map tokens, 16
decode steps), ``sample_k = 5``, ``token_logprob``.  Every sample is a fresh process; the variants of a figure alternate so that
drift of the machine lands on all of them alike; medians with their spread are reported.  Figures:

    (a) copy speed  at the middle step, between device events and alternating inside one process: ``snapshot`` of 512 of the 1024
                    slots (copies 0..15 of every scene), ``restore`` of those entries, one ``branch`` that moves the same 512
                    slots' worth of bytes (tools/bench_branching.py's figure a), and the save restated as per-buffer torch
                    ``index_select`` + ``copy_`` calls.  Bytes moved count read + written.
    (b) unchanged   the unbranched sampled rollout (bench_branching's 'plain' worker) and the greedy ``bench.py`` line in this tree
                    and in ``--parent`` (a built checkout of the parent commit): the same launches, so no change is expected.
                    Skipped without ``--parent``.
    (c) MPC cost    a closed-loop session over 4 C3 scenes x 8 copies with ``step_scores``, the ego commanded by tokens: every
                    session step preceded by ``lookahead(4, ...)`` against the plain session.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_branching import WORKER as PLAIN_WORKER, run  # noqa: E402

WORKER = r'''
import json, sys
root, mode, warmup, reps, shapes_json = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(shapes_json) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
S0, N = (32, 32) if mode == 'copy' else (4, 8)
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(S0)]
steps = cfg.num_decode_steps
w = engine.PackedWeights(sd, cfg, dev)

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)

med = lambda x: float(np.median(x))
out = dict(steps=steps)
if mode == 'copy':
    u = np.random.default_rng(7).random((steps, S0 * N, 64), dtype=np.float32)
    eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, copies=N, sample_k=5, sample_uniforms=u, token_logprob=True)
    S, tb = eng.S, steps // 2
    eng.prologue(); eng.run(0, tb)
    slot = torch.arange(S, device=dev).view(S0, N)
    saved = slot[:, :N // 2].reshape(-1).int().contiguous()                   # copies 0..15 of every scene
    parent = torch.where(slot % N >= N // 2, slot - N // 2, slot).int().contiguous()
    snap = eng.snapshot(tb, slots=saved)
    index = torch.full((S,), -1, dtype=torch.int32, device=dev); index[saved.long()] = torch.arange(saved.numel(), dtype=torch.int32, device=dev)
    scene_major = [eng.pos, eng.head, eng.state, eng.token, eng.gridtok, eng.tmask, eng.imask, eng.catflag, eng.bos,
                   eng.X.view(S, -1), eng.pred_traj, eng.pred_head, eng.pred_state]
    rings = [r.view(eng.ring, S, -1) for r in eng.ringK + eng.ringV]
    logs = [eng.token_logprob.view(steps, S, -1)[:tb]]
    src = saved.long()
    stage = [torch.empty_like(b.index_select(0, src)) for b in scene_major] + [torch.empty_like(b.index_select(1, src)) for b in rings + logs]
    def restated():
        k = 0
        for b in scene_major:
            stage[k].copy_(b.index_select(0, src)); k += 1
        for b in rings + logs:
            stage[k].copy_(b.index_select(1, src)); k += 1
    before = {k: getattr(eng, k).clone() for k in ('pos', 'token', 'X', 'token_logprob')}
    eng.restore(snap, index); eng.branch(parent, tb); eng.restore(snap, index); restated(); torch.cuda.synchronize()
    per_slot = snap.stride
    out.update(slots=S, saved_slots=int(saved.numel()), bytes_per_slot=int(per_slot), snapshot_bytes=int(snap.nbytes),
               bad=int(eng.snapshot_bad[0]) + int(eng.restore_bad[0]), torch_calls=2 * len(stage))
    t = dict(save=[], restore=[], branch=[], torch=[])
    for _ in range(reps):
        t['save'].append(timed(lambda: eng.snapshot(tb, slots=saved, out=snap)))
        t['restore'].append(timed(lambda: eng.restore(snap, index)))
        t['branch'].append(timed(lambda: eng.branch(parent, tb)))
        t['torch'].append(timed(restated))
    moved = 2.0 * per_slot * int(saved.numel())
    out['bytes_moved'] = moved
    for k, v in t.items():
        out[k + '_ms'] = med(v); out[k + '_all_ms'] = v; out[k + '_gbs'] = moved / (1e6 * med(v))
    out['ms'] = out['save_ms']
else:                                   # 'mpc' / 'session': a token-commanded ego, with and without a look-ahead per step
    eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, copies=N, step_scores=True)
    S = eng.S
    cmds = ((torch.arange(steps, device=dev)[:, None] * 131 + torch.arange(S, device=dev)[None, :] * 517 + 11) % cfg.token_size).int()
    tries = torch.stack([(cmds + 7 * h + 3) % cfg.token_size for h in range(4)], 1)          # [steps, 4, S]
    def session():
        ses = eng.session(controlled='ego')
        while not ses.done:
            if mode == 'mpc':
                lw = ses.lookahead(4, tokens=tries[ses.t])
                best = lw.argmax(1)                                     # the choice is made on the device and not used further
            ses.command(tokens=cmds[ses.t])
            ses.advance()
    for _ in range(warmup):
        session()
    torch.cuda.synchronize()
    ms = [timed(session) for _ in range(reps)]
    out.update(ms=med(ms), all_ms=ms, slots=S, per_step_ms=med(ms) / steps)
print(json.dumps(out))
'''


def bench_line(root, steps, warmup):
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                          '--no-cpu-baseline', '--no-parity', '--no-literal', '--no-strict', '--no-balance'],
                         capture_output=True, text=True, timeout=1500, cwd=root)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'bench.py in {root} failed ({out.returncode}): {out.stderr[-1500:]}')
    line = json.loads(lines[-1])
    return dict(ms=line['value'], unit=line.get('unit'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (figure b)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--copy-reps', type=int, default=15)
    ap.add_argument('--bench-steps', type=int, default=3)
    ap.add_argument('--figures', default='abc')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'snapshot.log'))
    a = ap.parse_args()
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    worker = lambda src, root, mode, reps=a.reps: run([sys.executable, '-c', src, root, mode, str(a.warmup), str(reps), shapes])
    figures = []
    if 'a' in a.figures:
        figures.append(('(a) save / restore of 512 of 1024 slots at the middle step', [('copy', lambda: worker(WORKER, REPO, 'copy', a.copy_reps))]))
    if 'c' in a.figures:
        figures.append(('(c) session of 32 slots, one lookahead(4) per step against none, ms per session',
                        [('plain session', lambda: worker(WORKER, REPO, 'session')), ('mpc session', lambda: worker(WORKER, REPO, 'mpc'))]))
    if 'b' in a.figures and a.parent:
        parent = os.path.abspath(a.parent)
        figures.append(('(b1) unbranched sampled rollout, ms', [('parent', lambda: worker(PLAIN_WORKER, parent, 'plain')),
                                                                 ('this', lambda: worker(PLAIN_WORKER, REPO, 'plain'))]))
        figures.append(('(b2) greedy bench.py line, agent-steps/s (higher is better)',
                        [('parent', lambda: bench_line(parent, a.bench_steps, a.warmup)), ('this', lambda: bench_line(REPO, a.bench_steps, a.warmup))]))
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
                entry[name] = dict(median=statistics.median(ms), min=min(ms), max=max(ms), samples=ms)
                for k in ('slots', 'saved_slots', 'bytes_per_slot', 'snapshot_bytes', 'bytes_moved', 'torch_calls', 'bad', 'steps', 'per_step_ms'):
                    if k in s:
                        entry[name][k] = s[k]
                if name == 'copy':
                    del entry[name]['median'], entry[name]['min'], entry[name]['max'], entry[name]['samples']
                    for k in ('save', 'restore', 'branch', 'torch'):
                        v = [x[k + '_ms'] for x in got[name]]
                        m = statistics.median(v)
                        entry[name][k] = dict(median_ms=m, min_ms=min(v), max_ms=max(v), samples=v, gbs=s['bytes_moved'] / (1e6 * m))
                print(f'{figure}: round {r} {name}: {s["ms"]:.3f}', flush=True)
                write()
            entry['rounds'] = r + 1
        write()
        print(json.dumps(entry), flush=True)


if __name__ == '__main__':
    main()
