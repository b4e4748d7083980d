"""Timing of collision-aware decoding (per-step token masks from the agents' boxes, k_collision_mask); bench.py is
untouched.

    python tools/bench_collision_masks.py --parent DIR [--rounds 3] [--log profiles/collision_masks.log] [--skip-bench | --skip-rollouts]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process, and the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Figures:

    bench       the default line, ``bench.py --gpus 1 --steps S --warmup W`` in the parent's tree and in this one (feature off)
    greedy      1024 C3 scenes, greedy: parent / this with the feature off / this with ``avoid_collisions=True``

A sample is one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events (their median).  Every sample also
reports the rollout's box-overlap rate - the share of (agent, step) pairs whose box, at the end of a decode step, overlaps another
agent's of the same scene (separating-axis test on the stored poses, fp32, torch) - and the feature-on samples the time of one
k_collision_mask launch on the rollout's last column by device events (the median of 20 launches behind a warm-up one).
Gate: with the feature off, the median of this tree is not above the parent's own maximum.  The feature-on variant is recorded, not
gated.  A failed gate exits non-zero after the log is written; the log is rewritten after every sample.
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
root, scenes_n, mode, warmup, reps = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(sys.argv[6]) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
kw = dict(avoid_collisions=True) if mode == 'avoid' else {}
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, **kw)
for _ in range(warmup):
    eng.rollout()
torch.cuda.synchronize()
ms = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); eng.rollout(); e1.record(); e1.synchronize()
    ms.append(e0.elapsed_time(e1))

def overlap_rate():
    hc, steps, S, A = cfg.hist_columns, cfg.num_decode_steps, eng.S, eng.A_cap
    half = 0.5 * eng._shape10[:, :, :2]
    hit = tot = 0
    for c in range(hc, hc + steps):
        p, h, ok = eng.pos[:, c], eng.head[:, c], eng.state[:, c] != 0
        u = torch.stack([torch.cos(h), torch.sin(h)], -1); v = torch.stack([-torch.sin(h), torch.cos(h)], -1)
        d = p[:, None] - p[:, :, None]                                   # [S][i][j]
        sep = torch.full((S, A, A), -1e30, device=dev)
        for ax in (u[:, :, None], v[:, :, None], u[:, None], v[:, None]):   # axes of i, then of j
            ri = half[:, :, None, 0] * (u[:, :, None] * ax).sum(-1).abs() + half[:, :, None, 1] * (v[:, :, None] * ax).sum(-1).abs()
            rj = half[:, None, :, 0] * (u[:, None] * ax).sum(-1).abs() + half[:, None, :, 1] * (v[:, None] * ax).sum(-1).abs()
            sep = torch.maximum(sep, (d * ax).sum(-1).abs() - (ri + rj))
        pair = ok[:, :, None] & ok[:, None] & ~torch.eye(A, dtype=torch.bool, device=dev)[None]
        hit += int(((sep < 0) & pair).any(-1).sum()); tot += int(ok.sum())
    return hit / max(tot, 1)

out = dict(ms=float(np.median(ms)), all_ms=ms, rows=int(eng.rows), overlap_rate=overlap_rate())
if mode == 'avoid':
    from infgen_amd import torch_ops
    c = cfg.hist_columns - 1 + cfg.num_decode_steps - 1
    call = lambda: torch.ops.infgen_hip.collision_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, eng._shape10, c, eng._coll_end, 1, 0.0)
    call(); torch.cuda.synchronize()
    us = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    out['kernel_us'] = float(np.median(us))      # (the op's output allocation rides along: an upper bound of the launch)
    out['fallback_rows_last_step'] = int((eng.collision_allowed == 0).sum())
print(json.dumps(out))
'''


def run(cmd, cwd=None):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=cwd)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'{" ".join(cmd[:3])} ... failed ({out.returncode}): {out.stderr[-800:]}')
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--scenes', type=int, default=1024)
    ap.add_argument('--bench-steps', type=int, default=5)
    ap.add_argument('--bench-warmup', type=int, default=2)
    ap.add_argument('--skip-bench', action='store_true')
    ap.add_argument('--skip-rollouts', action='store_true')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'collision_masks.log'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')

    def rollout(root, mode):
        return run([sys.executable, '-c', WORKER, root, str(a.scenes), mode, str(a.warmup), str(a.reps), shapes])

    def bench(root):
        r = run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', str(a.bench_warmup)], cwd=root)
        return dict(ms=r['ms_per_step'])

    figures = [(f'greedy {a.scenes} scenes', [('parent', lambda: rollout(parent, 'plain')), ('this', lambda: rollout(REPO, 'plain')),
                                              ('this + avoid_collisions', lambda: rollout(REPO, 'avoid'))])]
    if a.skip_rollouts:
        figures = []
    if not a.skip_bench:
        figures.append((f'bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup} (ms per step)',
                        [('parent', lambda: bench(parent)), ('this', lambda: bench(REPO))]))
    results, ok = [], True

    def write():
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, 'w') as f:
            f.write('\n'.join(json.dumps(r) for r in results) + '\n')

    for figure, variants in figures:
        got = {name: [] for name, _ in variants}
        entry = dict(figure=figure, rounds=0)
        results.append(entry)
        for r in range(a.rounds):
            for name, fn in variants:          # alternating: one sample of every variant per round
                s = fn()
                got[name].append(s['ms'])
                print(f'{figure}: round {r} {name}: {s["ms"]:.3f} ms', flush=True)
                ms = got[name]
                entry[name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), samples=ms)
                for k in ('overlap_rate', 'kernel_us', 'fallback_rows_last_step'):
                    if k in s:
                        entry[name][k] = s[k]
                write()
            entry['rounds'] = r + 1
        par, new = entry['parent'], entry['this']
        entry['gate'] = 'pass' if new['median_ms'] <= par['max_ms'] else 'FAIL'
        if 'this + avoid_collisions' in entry:
            entry['feature_cost_ms'] = entry['this + avoid_collisions']['median_ms'] - new['median_ms']
        ok = ok and entry['gate'] == 'pass'
        write()
        print(json.dumps(entry), flush=True)
    if not ok:
        raise SystemExit("gate failed: with the feature off this tree's median is above the parent's own maximum")


if __name__ == '__main__':
    main()
