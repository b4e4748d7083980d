"""Timing of road-aware decoding (per-step token masks from the map's road edges, k_road_mask); bench.py is
untouched.

    python tools/bench_road_masks.py --parent DIR [--rounds 3] [--log profiles/road_masks.log] [--skip-bench | --skip-rollouts]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process, and the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Figures:

    bench       the default line, ``bench.py --gpus 1 --steps S --warmup W`` in the parent's tree and in this one (feature off)
    greedy      1024 C3 scenes, greedy: parent / this with the feature off / this with ``stay_on_road=True``

A sample is one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events (their median).  Every sample of this
tree also reports the rollout's off-road rate - the share of (agent, step) pairs whose end box or path rectangle of the step overlaps
a road-edge record (two chords per EDGE map token of the synthetic maps) that the pose before the step did not straddle;
separating-axis test on the stored poses, fp32, torch - for the rows the rule governs (vehicles and cyclists), for all agents, for
pedestrians alone, and, as shares of all pairs, by cause: the row took the fallback at that step (``road_allowed == 0``, read step
by step in one more rollout), another governed row, a pedestrian, a replayed row (this workload replays none).  The feature-on
samples add the records per scene, the table's bytes and the time of one k_road_mask launch on the rollout's last column - the C
entry on the engine's own buffers between device events, the median of 20 launches behind a warm-up one.
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
root_is_this = hasattr(engine.RolloutEngine, '_load_road')      # (the parent's tree has no road operators)
dev = torch.device('cuda:0')
with open(sys.argv[6]) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
kw = dict(stay_on_road=True) if mode == 'road' else {}
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

def sat(d, ua, va, ea, ub, vb, eb):
    sep = None
    for ax in (ua, va, ub, vb):
        r = (ea[..., 0] * (ua * ax).sum(-1).abs() + ea[..., 1] * (va * ax).sum(-1).abs() +
             eb[..., 0] * (ub * ax).sum(-1).abs() + eb[..., 1] * (vb * ax).sum(-1).abs())
        g = (d * ax).sum(-1).abs() - r
        sep = g if sep is None else torch.maximum(sep, g)
    return sep

def offroad_hits(rec, nrec):
    """-> (off, ok) bool [steps][S][A]: the (agent, step) pairs whose end box or path rectangle of the step overlaps a record the
    pose before the step did not straddle, and the pairs that are in the scene before and after the step"""
    hc, steps, S, A = cfg.hist_columns, cfg.num_decode_steps, eng.S, eng.A_cap
    half = 0.5 * eng._shape10[:, :, :2]
    R = rec.shape[1]
    ms = torch.arange(S, device=dev) // eng.copies
    off_all = torch.zeros(steps, S, A, dtype=torch.bool, device=dev)
    ok_all = torch.zeros(steps, S, A, dtype=torch.bool, device=dev)
    for s0 in range(0, S, 64):                                            # (64 scenes at a time: [64][A][R] temporaries)
        sl = slice(s0, min(S, s0 + 64))
        rc = rec[ms[sl]]                                                  # [s][R][8]
        valid = (torch.arange(R, device=dev)[None] < nrec[ms[sl]][:, None]) & (rc[..., 7] >= 0)
        ub, vb = rc[:, None, :, 4:6], torch.stack([-rc[..., 5], rc[..., 4]], -1)[:, None]
        eb = torch.stack([rc[..., 6], torch.zeros_like(rc[..., 6])], -1)[:, None]
        unit = lambda h: (torch.stack([torch.cos(h), torch.sin(h)], -1)[:, :, None], torch.stack([-torch.sin(h), torch.cos(h)], -1)[:, :, None])
        hf = half[sl][:, :, None]
        for t in range(steps):
            c = hc - 1 + t
            p0, p1, h0, h1 = eng.pos[sl, c], eng.pos[sl, c + 1], eng.head[sl, c], eng.head[sl, c + 1]
            mid = lambda p: (rc[:, None, :, 0:2] - p[:, :, None]) + rc[:, None, :, 2:4]
            u0, v0 = unit(h0); u1, v1 = unit(h1)
            straddled = sat(mid(p0), u0, v0, hf, ub, vb, eb) < 0
            end = sat(mid(p1), u1, v1, hf, ub, vb, eb) < 0
            d = p1 - p0
            L = d.norm(dim=-1)
            up = torch.where((L > 0)[..., None], d / L.clamp(min=1e-30)[..., None], torch.tensor([1.0, 0.0], device=dev))
            vp = torch.stack([-up[..., 1], up[..., 0]], -1)
            ep = torch.stack([0.5 * L, half[sl][..., 1]], -1)
            path = (sat(mid(p0) - 0.5 * d[:, :, None], up[:, :, None], vp[:, :, None], ep[:, :, None], ub, vb, eb) < 0) & (L > 0)[..., None]
            off_all[t, sl] = ((end | path) & ~straddled & valid[:, None]).any(-1)
            ok_all[t, sl] = (eng.state[sl, c] != 0) & (eng.state[sl, c + 1] != 0)
    return off_all, ok_all

share = lambda hit, of: float(hit.sum()) / max(int(of.sum()), 1)
out = dict(ms=float(np.median(ms)), all_ms=ms, rows=int(eng.rows))
if root_is_this:
    from infgen_amd import torch_ops
    steps = cfg.num_decode_steps
    rec, nrec = torch_ops.road_records_from_map(eng.map_pos, eng.map_orient, eng._map_cat[1], eng._map_cat[0], eng.n_map,
                                                eng._map_vocab.view(-1, 11, 2), 2)
    fallback = torch.zeros(steps, eng.S, eng.A_cap, dtype=torch.bool, device=dev)
    if mode == 'road':          # one more rollout, step by step: which rows took the fallback at which step
        eng.prologue()
        eng._refresh_opts(groups=True)
        for t in range(steps):
            eng.step(t)
            fallback[t] = (eng.road_allowed == 0).view(eng.S, eng.A_cap)
    off, ok = offroad_hits(rec, nrec)
    ped = (eng.atype == 1)[None]
    replayed = (eng.replay_row.bool() if eng.replay_row is not None else torch.zeros_like(eng.atype, dtype=torch.bool))[None]
    ruled = ok & ~ped & ~replayed
    out['offroad_rate'] = share(off & ruled, ruled)                       # vehicles and cyclists the rule governs
    out['offroad_rate_all_agents'] = share(off & ok, ok)
    out['offroad_by_cause'] = dict(                                       # shares of ALL (agent, step) pairs in the scene
        fallback_taken=share(off & ruled & fallback, ok), ruled_other=share(off & ruled & ~fallback, ok),
        pedestrians=share(off & ok & ped & ~replayed, ok), replayed_rows=share(off & ok & replayed, ok))
    out['pedestrian_offroad_rate'] = share(off & ok & ped, ok & ped)
    out['fallback_rows'] = int(fallback.sum())
if mode == 'road':
    import ctypes as C
    from infgen_amd import _lib
    P, c = _lib.ptr, cfg.hist_columns - 1 + cfg.num_decode_steps - 1
    sw = (C.c_int * 3)(1, 0, 1)
    # the C entry on the engine's own buffers: the launch alone, no allocation
    call = lambda: _lib.check(eng.lib.infgen_road_mask(
        P(eng.pos), P(eng.head), P(eng.state), P(eng.n_agents), None, P(eng.atype), P(eng._road['shape']), eng.S, eng.A_cap, eng.T, c,
        P(eng._coll_end), P(eng._road_paths), cfg.token_size, P(eng.road_records), P(eng.road_n_records), eng._road_cap, eng.copies, 1, 0.0,
        sw, None, 0, None, None, P(eng.road_bits), P(eng.road_allowed), eng.ops.stream), 'infgen_road_mask')
    call(); torch.cuda.synchronize()
    us = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    out['kernel_us'] = float(np.median(us))
    out['records_per_scene'] = float(eng.road_n_records.float().mean())
    out['record_table_bytes'] = int(eng.road_records.numel() * 4)
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
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'road_masks.log'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')

    def rollout(root, mode):
        return run([sys.executable, '-c', WORKER, root, str(a.scenes), mode, str(a.warmup), str(a.reps), shapes])

    def bench(root):
        r = run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', str(a.bench_warmup)], cwd=root)
        return dict(ms=r['ms_per_step'])

    figures = [(f'greedy {a.scenes} scenes', [('parent', lambda: rollout(parent, 'plain')), ('this', lambda: rollout(REPO, 'plain')),
                                              ('this + stay_on_road', lambda: rollout(REPO, 'road'))])]
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
                for k in ('offroad_rate', 'offroad_rate_all_agents', 'offroad_by_cause', 'pedestrian_offroad_rate', 'fallback_rows', 'kernel_us',
                          'records_per_scene', 'record_table_bytes'):
                    if k in s:
                        entry[name][k] = s[k]
                write()
            entry['rounds'] = r + 1
        par, new = entry['parent'], entry['this']
        entry['gate'] = 'pass' if new['median_ms'] <= par['max_ms'] else 'FAIL'
        if 'this + stay_on_road' in entry:
            entry['feature_cost_ms'] = entry['this + stay_on_road']['median_ms'] - new['median_ms']
        ok = ok and entry['gate'] == 'pass'
        write()
        print(json.dumps(entry), flush=True)
    if not ok:
        raise SystemExit("gate failed: with the feature off this tree's median is above the parent's own maximum")


if __name__ == '__main__':
    main()
