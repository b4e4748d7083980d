"""Timing of constrained decoding (per-row allowed-token masks inside the heads kernels); bench.py is untouched.

    python tools/bench_token_masks.py --parent DIR [--rounds 3] [--log profiles/token_masks_timing.log] [--skip-bench]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process, and the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Three figures:

    bench       the default line, ``bench.py --gpus 1 --steps S --warmup W`` in the parent's tree and in this one (masks off)
    greedy      1024 C3 scenes, greedy: parent / this without masks / this with a per-type mask from
                ``TokenMasks.from_vocab(vocab, {'max_speed': 8.0, 'no_reverse': True})`` / this with a table that allows every
                token (the masked kernels on the very same rollout: a from_vocab mask changes the trajectories, and with them
                the edge counts of every later step, so only this variant isolates what the kernels cost)
    sampled     32 C3 scenes x 32 copies, sample_k = 5: the same three variants

For greedy and sampled a sample is one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events (their
median).  Reported per variant: the median over the samples and their spread (min .. max).  Gate: with masks off, the median of this
tree is not above the parent's own maximum.  The masked variants are recorded, not gated.  A failed gate exits non-zero after the
log is written; the log is rewritten after every sample, so a run that is cut short leaves what it measured.
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
root, scenes_n, copies, k, mode, warmup, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], int(sys.argv[6]), int(sys.argv[7])
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(sys.argv[8]) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
kw = {}
if k > 1:
    kw = dict(sample_k=k, sample_uniforms=np.random.default_rng(7).uniform(0, 1, size=(cfg.num_decode_steps, scenes_n * copies, 64)).astype(np.float32))
allowed = None
if mode in ('masked', 'all'):
    from infgen_amd import constraints
    masks = constraints.TokenMasks.from_vocab(vocab, {'max_speed': 8.0, 'no_reverse': True})
    if mode == 'all':      # the masked kernels on the unmasked rollout: every token allowed
        masks = constraints.TokenMasks(np.ones((1, cfg.token_size), bool), type_sets=[0, 0, 0])
    kw['token_masks'] = masks
    allowed = [int(n) for n in masks.allowed.sum(1)]
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, copies=copies, **kw)
for _ in range(warmup):
    eng.rollout()
torch.cuda.synchronize()
ms = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); eng.rollout(); e1.record(); e1.synchronize()
    ms.append(e0.elapsed_time(e1))
print(json.dumps(dict(ms=float(np.median(ms)), all_ms=ms, rows=int(eng.rows), allowed_per_set=allowed)))
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
    ap.add_argument('--bench-steps', type=int, default=5)
    ap.add_argument('--bench-warmup', type=int, default=2)
    ap.add_argument('--skip-bench', action='store_true')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'token_masks_timing.log'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')

    def rollout(root, scenes, copies, k, mode):
        return run([sys.executable, '-c', WORKER, root, str(scenes), str(copies), str(k), mode, str(a.warmup), str(a.reps), shapes])

    def bench(root):
        r = run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', str(a.bench_warmup)], cwd=root)
        return dict(ms=r['ms_per_step'])

    figures = [('greedy 1024 scenes', [('parent', lambda: rollout(parent, 1024, 1, 1, 'plain')),
                                       ('this', lambda: rollout(REPO, 1024, 1, 1, 'plain')),
                                       ('this + all-allowed mask', lambda: rollout(REPO, 1024, 1, 1, 'all')),
                                       ('this + mask', lambda: rollout(REPO, 1024, 1, 1, 'masked'))]),
               ('sampled 32 scenes x 32 copies, sample_k 5', [('parent', lambda: rollout(parent, 32, 32, 5, 'plain')),
                                                              ('this', lambda: rollout(REPO, 32, 32, 5, 'plain')),
                                                              ('this + all-allowed mask', lambda: rollout(REPO, 32, 32, 5, 'all')),
                                                              ('this + mask', lambda: rollout(REPO, 32, 32, 5, 'masked'))])]
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
                if s.get('allowed_per_set'):
                    entry['allowed_tokens_per_type'] = s['allowed_per_set']
                write()
            entry['rounds'] = r + 1
        par, new = entry['parent'], entry['this']
        entry['gate'] = 'pass' if new['median_ms'] <= par['max_ms'] else 'FAIL'
        if 'this + mask' in entry:
            entry['mask_cost_ms'] = entry['this + mask']['median_ms'] - new['median_ms']
            entry['mask_cost_percent'] = 100.0 * entry['mask_cost_ms'] / new['median_ms']
            entry['masked_kernels_cost_ms'] = entry['this + all-allowed mask']['median_ms'] - new['median_ms']
        ok = ok and entry['gate'] == 'pass'
        write()
        print(json.dumps(entry), flush=True)
    if not ok:
        raise SystemExit("gate failed: with masks off this tree's median is above the parent's own maximum")


if __name__ == '__main__':
    main()
