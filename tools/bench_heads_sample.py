"""Timing of top-k sampling inside the split heads kernel ("Sampling inside the heads kernel"); bench.py is untouched.

    python tools/bench_heads_sample.py --parent DIR [--scenes 32] [--copies 32] [--rounds 3] [--log profiles/heads_sample.log]

The reference's validation workload (``config.multi_rollout``): ``--scenes`` C3 scenes x ``--copies`` rollouts each, ``sample_k=5``,
insertion off.  ``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every
sample is a fresh process (one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events; the sample is
their median), and the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Reported per
variant: the median over the samples, their spread (min .. max), the engine's device bytes and the peak during the timed rollouts.

    parent      the parent commit: k_heads_h stores the logits, k_sample_topk reads them back
    this        this tree: the sampling instantiation, no logits in memory
    this + lp   this tree with token_logprob and sample_logprob both on

Gate: the median of ``this`` is not above the parent's own maximum (not slower beyond the parent's run-to-run spread).  A failed
gate exits non-zero.
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
root, scenes_n, copies, mode, warmup, reps = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]), int(sys.argv[6])
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(sys.argv[7]) as f:
    shapes = {k: tuple(v) for k, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
u = np.random.default_rng(7).uniform(0, 1, size=(cfg.num_decode_steps, scenes_n * copies, 64)).astype(np.float32)
w = engine.PackedWeights(sd, cfg, dev)
torch.cuda.synchronize()
base = torch.cuda.memory_allocated(dev)
kw = dict(token_logprob=True, sample_logprob=True) if mode == 'lp' else {}
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, copies=copies, sample_k=5, sample_uniforms=u, **kw)
for _ in range(warmup):
    eng.rollout()
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats(dev)
ms = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); eng.rollout(); e1.record(); e1.synchronize()
    ms.append(e0.elapsed_time(e1))
print(json.dumps(dict(ms=float(np.median(ms)), all_ms=ms, rows=int(eng.rows), scratch=eng.logits_scratch is not None,
                      engine_bytes=int(torch.cuda.memory_allocated(dev) - base),
                      peak_bytes=int(torch.cuda.max_memory_allocated(dev) - base))))
'''


def sample(root, scenes, copies, mode, warmup, reps):
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    out = subprocess.run([sys.executable, '-c', WORKER, root, str(scenes), str(copies), mode, str(warmup), str(reps), shapes],
                         capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'sample {root} {mode} failed ({out.returncode}): {out.stderr[-800:]}')
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--scenes', type=int, default=32)
    ap.add_argument('--copies', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'heads_sample.log'))
    a = ap.parse_args()
    variants = [('parent', os.path.abspath(a.parent), 'plain'), ('this', REPO, 'plain'), ('this + lp', REPO, 'lp')]
    got = {name: [] for name, _, _ in variants}
    for r in range(a.rounds):
        for name, root, mode in variants:          # alternating: one sample of every variant per round
            got[name].append(sample(root, a.scenes, a.copies, mode, a.warmup, a.reps))
            print(f'round {r} {name}: {got[name][-1]["ms"]:.3f} ms', flush=True)
    lines, stats = [], {}
    for name, _, _ in variants:
        ms = [s['ms'] for s in got[name]]
        last = got[name][-1]
        stats[name] = dict(variant=name, scenes=a.scenes, copies=a.copies, rows=last['rows'], sample_k=5, median_ms=statistics.median(ms),
                           min_ms=min(ms), max_ms=max(ms), samples=ms, logits_scratch=last['scratch'],
                           engine_bytes=last['engine_bytes'], peak_bytes=last['peak_bytes'])
        lines.append(json.dumps(stats[name]))
    par, new, lp = stats['parent'], stats['this'], stats['this + lp']
    ok = new['median_ms'] <= par['max_ms']
    lines.append(json.dumps(dict(figure='sampled rollout', parent_ms=par['median_ms'], this_ms=new['median_ms'],
                                 gain_ms=par['median_ms'] - new['median_ms'], parent_min_ms=par['min_ms'], parent_max_ms=par['max_ms'],
                                 this_lp_ms=lp['median_ms'], peak_bytes_with_scratch=par['peak_bytes'],
                                 peak_bytes_without=new['peak_bytes'], gate='pass' if ok else 'FAIL')))
    for l in lines:
        print(l, flush=True)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if not ok:
        raise SystemExit('gate failed: the sampled rollout is slower than the parent beyond its spread')


if __name__ == '__main__':
    main()
