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

With ``--temperature T --top-p P`` the variants are instead

    parent      the parent commit
    this        this tree with the default sampler (T = 1, top_p = 1: the same arithmetic)
    this T/P    this tree with sample_temperature = T, sample_top_p = P
    this sweep  this tree with one temperature per copy (0, then 0.5 .. 2 in equal steps) and top_p = P

and the gate is that the median of ``this`` lies inside the parent's own min .. max; the other two are recorded, not gated.  Use
``--rounds 5``; the log then defaults to ``profiles/sampling_controls.log``.
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
if mode.startswith('tp:') or mode.startswith('sweep:'):
    kind, T, P = mode.split(':')
    per_copy = np.concatenate([[0.0], np.linspace(0.5, 2.0, copies - 1)]).astype(np.float32) if copies > 1 else np.float32([1.0])
    kw = dict(sample_temperature=float(T) if kind == 'tp' else np.tile(per_copy, scenes_n), sample_top_p=float(P))
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
    ap.add_argument('--log', default=None, help='default: profiles/heads_sample.log, or profiles/sampling_controls.log with '
                                                 '--temperature / --top-p')
    ap.add_argument('--temperature', type=float, default=None, help='with --top-p: time the tempered / nucleus variants instead')
    ap.add_argument('--top-p', type=float, default=None)
    a = ap.parse_args()
    controls = a.temperature is not None or a.top_p is not None
    if a.log is None:
        a.log = os.path.join(REPO, 'profiles', 'sampling_controls.log' if controls else 'heads_sample.log')
    variants = [('parent', os.path.abspath(a.parent), 'plain'), ('this', REPO, 'plain'), ('this + lp', REPO, 'lp')]
    if controls:
        T, P = (1.0 if a.temperature is None else a.temperature), (1.0 if a.top_p is None else a.top_p)
        variants = variants[:2] + [(f'this T={T:g} top_p={P:g}', REPO, f'tp:{T}:{P}'), ('this sweep', REPO, f'sweep:{T}:{P}')]
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
    if controls:
        par, new = stats['parent'], stats['this']
        ok = par['min_ms'] <= new['median_ms'] <= par['max_ms']
        lines.append(json.dumps(dict(figure='sampling controls', parent_ms=par['median_ms'], parent_min_ms=par['min_ms'],
                                     parent_max_ms=par['max_ms'], this_default_ms=new['median_ms'],
                                     **{name: stats[name]['median_ms'] for name, _, _ in variants[2:]}, gate='pass' if ok else 'FAIL')))
        for l in lines:
            print(l, flush=True)
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        if not ok:
            raise SystemExit("gate failed: the default sampler's median lies outside the parent's own min .. max")
        return
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
