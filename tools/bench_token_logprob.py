"""Timing of the per-token log-probability output ("Token log-probabilities"); bench.py is untouched.

    python tools/bench_token_logprob.py --parent DIR [--scenes 1024] [--scenes-small 256] [--rounds 3] [--log profiles/token_logprob.log]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process (one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events; the sample is their median), and
the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Reported per variant: the median
over the samples and their spread (min .. max).

    1  N scenes of the C3 shape, greedy, flag off: this tree against the parent (the difference must lie inside the parent's own spread)
    2  the same with token_logprob=True (fused path), as a percentage over 1
    3  n scenes: token_logprob=True against the parent's only way - store_logits=True, then log_softmax + gather in torch over the steps
       (both times, and the bytes each allocates beyond the flag-off engine's buffers)

The log ends with one line per figure.  Gate 1: the flag-off median lies inside the parent's own min .. max.  Gate 3: the parent's
way minus the new path exceeds the sum of the two spreads.  Figure 2 is recorded as a percentage.  A failed gate exits non-zero.
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
    shapes = {k: tuple(v) for k, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
w = engine.PackedWeights(sd, cfg, dev)
torch.cuda.synchronize()
base = torch.cuda.memory_allocated(dev)
kw = {'on': dict(token_logprob=True), 'off': {}, 'store': dict(store_logits=True)}[mode]
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, **kw)
hc, steps = cfg.hist_columns, cfg.num_decode_steps

def once():
    eng.rollout()
    if mode == 'store':        # the parent's only way to the chosen token's log-probability
        tok = eng.token[:, hc:hc + steps].permute(1, 0, 2).reshape(steps, -1).long().clamp(min=0)
        return torch.stack([torch.log_softmax(eng.logits[t], dim=-1).gather(-1, tok[t][:, None])[:, 0] for t in range(steps)])
    return eng.token_logprob if mode == 'on' else None
for _ in range(warmup):
    once()
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats(dev)
ms = []
for _ in range(reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); once(); e1.record(); e1.synchronize()
    ms.append(e0.elapsed_time(e1))
print(json.dumps(dict(ms=float(np.median(ms)), all_ms=ms, engine_bytes=int(torch.cuda.memory_allocated(dev) - base),
                      peak_bytes=int(torch.cuda.max_memory_allocated(dev) - base))))
'''


def sample(root, scenes, mode, warmup, reps):
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    out = subprocess.run([sys.executable, '-c', WORKER, root, str(scenes), mode, str(warmup), str(reps), shapes],
                         capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'sample {root} {mode} failed ({out.returncode}): {out.stderr[-800:]}')
    return json.loads(lines[-1])


def summary(name, samples):
    ms = [s['ms'] for s in samples]
    return dict(variant=name, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), samples=ms,
                engine_bytes=samples[-1]['engine_bytes'], peak_bytes=samples[-1]['peak_bytes'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--scenes', type=int, default=1024)
    ap.add_argument('--scenes-small', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'token_logprob.log'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    legs = [('figures 1+2', a.scenes, [('parent off', parent, 'off'), ('this off', REPO, 'off'), ('this on', REPO, 'on')]),
            ('figure 3', a.scenes_small, [('parent store_logits + torch', parent, 'store'), ('this on', REPO, 'on'),
                                          ('this off', REPO, 'off')])]
    lines, stats, failed = [], {}, []
    for title, n, variants in legs:
        if n <= 0:
            continue
        got = {name: [] for name, _, _ in variants}
        for r in range(a.rounds):
            for name, root, mode in variants:          # alternating: one sample of every variant per round
                got[name].append(sample(root, n, mode, a.warmup, a.reps))
                print(f'{title} round {r} {name}: {got[name][-1]["ms"]:.3f} ms', flush=True)
        for name, _, _ in variants:
            stats[title, name] = summary(name, got[name])
            lines.append(json.dumps(dict(leg=title, scenes=n, **stats[title, name])))
            print(lines[-1], flush=True)
    spread = lambda s: s['max_ms'] - s['min_ms']
    if a.scenes > 0:
        par, off, on = (stats['figures 1+2', k] for k in ('parent off', 'this off', 'this on'))
        # gate 1: the flag-off median lies inside the run-to-run spread of the parent's own samples
        g1 = par['min_ms'] <= off['median_ms'] <= par['max_ms']
        lines.append(json.dumps(dict(figure=1, scenes=a.scenes, parent_off_ms=par['median_ms'], this_off_ms=off['median_ms'],
                                     diff_ms=off['median_ms'] - par['median_ms'], parent_min_ms=par['min_ms'],
                                     parent_max_ms=par['max_ms'], gate='pass' if g1 else 'FAIL')))
        lines.append(json.dumps(dict(figure=2, scenes=a.scenes, this_on_ms=on['median_ms'], spread_ms=spread(on),
                                     percent_over_flag_off=100.0 * (on['median_ms'] / off['median_ms'] - 1.0), gate='recorded, no gate')))
        failed += [] if g1 else ['figure 1']
    if a.scenes_small > 0:
        st, on, off = (stats['figure 3', k] for k in ('parent store_logits + torch', 'this on', 'this off'))
        # gate 3: faster than the parent's only way by more than the two spreads together
        g3 = st['median_ms'] - on['median_ms'] > spread(st) + spread(on)
        lines.append(json.dumps(dict(figure=3, scenes=a.scenes_small, parent_store_ms=st['median_ms'], this_on_ms=on['median_ms'],
                                     gain_ms=st['median_ms'] - on['median_ms'], combined_spread_ms=spread(st) + spread(on),
                                     parent_store_extra_bytes=st['engine_bytes'] - off['engine_bytes'],
                                     parent_store_extra_peak_bytes=st['peak_bytes'] - off['engine_bytes'],
                                     this_on_extra_bytes=on['engine_bytes'] - off['engine_bytes'], gate='pass' if g3 else 'FAIL')))
        failed += [] if g3 else ['figure 3']
    for l in lines:
        if l.startswith('{"figure"'):
            print(l, flush=True)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if failed:
        raise SystemExit('gate failed: ' + ', '.join(failed))


if __name__ == '__main__':
    main()
