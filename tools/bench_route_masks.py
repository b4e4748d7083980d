"""Timing of route-following decoding (per-step token masks from per-agent routes, k_route_mask); bench.py is
untouched.

    python tools/bench_route_masks.py --parent DIR [--rounds 3] [--log profiles/route_masks.log] [--skip-bench | --skip-rollouts]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process, and the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Figures:

    bench       the default line, ``bench.py --gpus 1 --steps S --warmup W`` in the parent's tree and in this one (feature off)
    greedy      1024 C3 scenes, greedy: parent / this with the feature off / this with ``follow_routes`` - every agent's own logged
                positions from the current column on, every second column, cut to 8 waypoints, corridor 2 m, pace 0; vehicles and
                cyclists are ruled

A sample is one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events (their median).  Every sample of this
tree also reports the lateral error of the rollout - d0 of ``torch.ops.infgen_hip.route_mask`` on the stored poses of every decode
column, over the (row, column) pairs of vehicles and cyclists that are in the scene and have a route: median, 90th and 99th
percentile, maximum and the share beyond the corridor.  The feature-on samples add the time of one k_route_mask launch on the
rollout's last column - the C entry on the engine's own buffers between device events, the median of 20 launches behind a warm-up
one - and the rows that took the fallback.
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
root_is_this = hasattr(engine.RolloutEngine, 'set_routes')      # (the parent's tree has no route operators)
dev = torch.device('cuda:0')
with open(sys.argv[6]) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
CORRIDOR = 2.0
kw = {}
if root_is_this:
    from infgen_amd import constraints
    r8, n8 = constraints.routes_from_logged(distinct, stride=2, start=cfg.hist_columns - 1, points=8)
    routes, n_points = r8[np.arange(scenes_n) % 8], n8[np.arange(scenes_n) % 8]
    if mode == 'routes':
        kw = dict(follow_routes=dict(routes=routes, n_points=n_points, corridor=CORRIDOR))
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
out = dict(ms=float(np.median(ms)), all_ms=ms, rows=int(eng.rows))
if root_is_this:
    from infgen_amd import torch_ops
    hc, steps = cfg.hist_columns, cfg.num_decode_steps
    full_r = torch.zeros(eng.S, eng.A_cap, 8, 2, device=dev); full_n = torch.zeros(eng.S, eng.A_cap, dtype=torch.int32, device=dev)
    full_r[:, :routes.shape[1]] = torch.from_numpy(routes).to(dev); full_n[:, :routes.shape[1]] = torch.from_numpy(n_points).to(dev)
    rec, total = torch_ops.route_records(full_r, full_n)
    eng._end_pose_table()
    end = eng._coll_end
    shape = torch.zeros(eng.S, eng.A_cap, 3, device=dev)
    d = []
    for t in range(steps + 1):              # every decode column and the last one produced
        c = hc - 1 + t
        prog = torch.ops.infgen_hip.route_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, shape, c, end, rec, total, 1,
                                               CORRIDOR, 0.5, 0.0, 0.0)[2]
        d.append(prog[prog[:, 3] > 0, 1])
    d = torch.cat(d).double()
    q = torch.quantile(d, torch.tensor([0.5, 0.9, 0.99], dtype=torch.float64, device=dev)).tolist()
    out['lateral_error_m'] = dict(pairs=int(d.numel()), median=q[0], p90=q[1], p99=q[2], max=float(d.max()),
                                  share_beyond_corridor=float((d > CORRIDOR).double().mean()))
if mode == 'routes':
    import ctypes as C
    from infgen_amd import _lib
    P, c, k, conf = _lib.ptr, cfg.hist_columns - 1 + cfg.num_decode_steps - 1, eng._route, eng.follow_routes
    sw = (C.c_int * 3)(*conf['types'])
    # the C entry on the engine's own buffers: the launch alone, no allocation
    call = lambda: _lib.check(eng.lib.infgen_route_mask(
        P(eng.pos), P(eng.head), P(eng.state), P(eng.n_agents), None, P(eng.atype), P(k['shape']), eng.S, eng.A_cap, eng.T, c,
        P(eng._coll_end), cfg.token_size, P(k['records']), P(k['total']), k['P'], eng.copies, conf['corridor'], conf['back'], conf['pace'],
        conf['finish'], sw, None, 0, None, None, P(k['bits']), P(k['allowed']), P(k['progress']), eng.ops.stream), 'infgen_route_mask')
    call(); torch.cuda.synchronize()
    us = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    out['kernel_us'] = float(np.median(us))
    out['ruled_rows_last_step'] = int((eng.route_progress[:, 3] == 1).sum())
    out['fallback_rows_last_step'] = int(((eng.route_allowed == 0) & (eng.route_progress[:, 3] == 1)).sum())
    out['decode_steps'] = int(cfg.num_decode_steps)
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
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'route_masks.log'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')

    def rollout(root, mode):
        return run([sys.executable, '-c', WORKER, root, str(a.scenes), mode, str(a.warmup), str(a.reps), shapes])

    def bench(root):
        r = run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', str(a.bench_warmup)], cwd=root)
        return dict(ms=r['ms_per_step'])

    figures = [(f'greedy {a.scenes} scenes', [('parent', lambda: rollout(parent, 'plain')), ('this', lambda: rollout(REPO, 'plain')),
                                              ('this + follow_routes', lambda: rollout(REPO, 'routes'))])]
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
                for k in ('lateral_error_m', 'kernel_us', 'ruled_rows_last_step', 'fallback_rows_last_step', 'decode_steps'):
                    if k in s:
                        entry[name][k] = s[k]
                write()
            entry['rounds'] = r + 1
        par, new = entry['parent'], entry['this']
        entry['gate'] = 'pass' if new['median_ms'] <= par['max_ms'] else 'FAIL'
        if 'this + follow_routes' in entry:
            on = entry['this + follow_routes']
            entry['feature_cost_ms'] = on['median_ms'] - new['median_ms']
            entry['feature_cost_us_per_step'] = 1e3 * entry['feature_cost_ms'] / on['decode_steps']
        ok = ok and entry['gate'] == 'pass'
        write()
        print(json.dumps(entry), flush=True)
    if not ok:
        raise SystemExit("gate failed: with the feature off this tree's median is above the parent's own maximum")


if __name__ == '__main__':
    main()
