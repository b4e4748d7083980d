"""Timing of the step scores (``RolloutEngine(step_scores=...)``, k_step_score); bench.py is untouched.

    python tools/bench_step_scores.py [--parent DIR] [--rounds 3] [--log profiles/step_scores.log]

Two set-ups, both C3 scenes (64 agents, 1024 map tokens, 16 decode steps): GREEDY, 1024 scenes decoded greedily, and COPIES,
32 scenes x 32 copies with ``sample_k = 5``.  Every sample is a fresh process; the variants of a figure alternate A B A B ... so that
drift of the machine lands on all of them alike, and medians are reported with their spreads.  Figures, per set-up:

    (a) off         ms per rollout with scoring off in this tree and in ``--parent`` (a built checkout of the parent commit): the off
                    path adds no launch.  Skipped without ``--parent``.
    (b) on          the same with ``step_scores=True`` (records from the map's EDGE tokens), against this tree's scoring-off
                    rollout: the added time per rollout and per step.
    (c) kernel      one ``infgen_step_score`` launch on the engine's final columns between device events, against the torch
                    restatement of the same terms: ``overlapping(c)`` of tools/bench_branching.py for the overlap term and the
                    smallest separation, the same axis test against the record rectangles for the off-road term (boxes only: the
                    restatement leaves the path rectangle out, so it does less), norms and wrapped differences for the comfort terms.
    (d) guided      COPIES only: ``rollout_guided(every=4, keep=copies // 2)`` against the unguided scoring rollout: ms per
                    rollout, and the overlap and off-road rates of the final copies - overlapping (off-road) live rows over live
                    rows, summed over all steps of the score log.
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
root, setup, mode, warmup, reps, shapes_json = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth
dev = torch.device('cuda:0')
with open(shapes_json) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
S0, N = (1024, 1) if setup == 'greedy' else (32, 32)
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(S0)]
steps, hc = cfg.num_decode_steps, cfg.hist_columns
kw = {}
if N > 1:
    kw.update(copies=N, sample_k=5, sample_uniforms=np.random.default_rng(7).random((steps, S0 * N, 64), dtype=np.float32))
if mode != 'off':
    kw.update(step_scores=True)
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, **kw)
S, A = eng.S, eng.A_cap

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)

def rates():
    x = eng.step_score.double()
    live = float(x[..., 0].sum())
    return float(x[..., 1].sum()) / max(live, 1.0), float(x[..., 3].sum()) / max(live, 1.0)

def axes_sep(d, ux, vx, half, oux, ovx, ohalf):
    """the four-axis separation of boxes (ux, vx, half) [.., 1 or n, ..] from boxes (oux, ovx, ohalf), centre differences d"""
    sep = None
    for ax in (ux, vx, oux, ovx):
        ri = half[..., 0] * (ux * ax).sum(-1).abs() + half[..., 1] * (vx * ax).sum(-1).abs()
        rj = ohalf[..., 0] * (oux * ax).sum(-1).abs() + ohalf[..., 1] * (ovx * ax).sum(-1).abs()
        g = (d * ax).sum(-1).abs() - (ri + rj)
        sep = g if sep is None else torch.maximum(sep, g)
    return sep

def restated(c):
    """the terms of one step score in torch, for column c -> [S, 6]"""
    half = 0.5 * eng._shape10[:, :, :2]
    p, h, ok = eng.pos[:, c], eng.head[:, c], eng.state[:, c] != 0
    ux = torch.stack([torch.cos(h), torch.sin(h)], -1); vx = torch.stack([-torch.sin(h), torch.cos(h)], -1)
    sep = axes_sep(p[:, None] - p[:, :, None], ux[:, :, None], vx[:, :, None], half[:, :, None], ux[:, None], vx[:, None], half[:, None])
    pair = ok[:, :, None] & ok[:, None] & ~torch.eye(A, dtype=torch.bool, device=dev)[None]
    sep = torch.where(pair, sep, torch.full_like(sep, float('inf')))
    over = (sep < 0).any(-1)
    rec = eng.road_records.repeat_interleave(N, 0)                                  # [S, R, 8]
    used = (torch.arange(rec.shape[1], device=dev)[None] < eng.road_n_records.repeat_interleave(N)[:, None]) & (rec[..., 7] >= 0)
    rel = (rec[:, None, :, 0:2] - p[:, :, None]) + rec[:, None, :, 2:4]
    oux = rec[:, None, :, 4:6]; ovx = torch.stack([-rec[..., 5], rec[..., 4]], -1)[:, None]
    ohalf = torch.stack([rec[..., 6], torch.zeros_like(rec[..., 6])], -1)[:, None]
    rsep = axes_sep(rel, ux[:, :, None], vx[:, :, None], half[:, :, None], oux, ovx, ohalf)
    ruled = (eng.atype != 1) & ok
    off = ((rsep < 0) & used[:, None]).any(-1) & ruled
    ok1 = ok & (eng.state[:, c - 1] != 0); ok2 = ok1 & (eng.state[:, c - 2] != 0)
    d1 = (p - eng.pos[:, c - 1]).norm(dim=-1); d0 = (eng.pos[:, c - 1] - eng.pos[:, c - 2]).norm(dim=-1)
    acc = torch.where(ok2, (d1 - d0).abs() / 0.25, torch.zeros_like(d1)).amax(-1)
    dh = torch.remainder(h - eng.head[:, c - 1] + np.pi, 2 * np.pi) - np.pi
    yaw = torch.where(ok1, dh.abs() / 0.5, torch.zeros_like(dh)).amax(-1)
    return torch.stack([ok.sum(-1).float(), over.sum(-1).float(), sep.amin((-1, -2)), off.sum(-1).float(), acc, yaw], -1)

out = dict(rows=int(eng.rows), slots=S, steps=steps)
if mode in ('off', 'on'):
    for _ in range(warmup):
        eng.rollout()
    torch.cuda.synchronize()
    ms = [timed(eng.rollout) for _ in range(reps)]
    out.update(ms=float(np.median(ms)), all_ms=ms)
    if mode == 'on':
        out.update(records_per_scene=int(eng.road_n_records.max()), overlap_rate=rates()[0], offroad_rate=rates()[1])
elif mode == 'kernel':
    eng.rollout()
    c = hc + steps - 1
    from infgen_amd import _lib
    import ctypes as C
    sc = eng.step_scores
    score, row = torch.zeros(S, 8, device=dev), torch.zeros(S, A, device=dev, dtype=torch.uint8)
    P = _lib.ptr
    def launch(sweep=sc['sweep']):
        _lib.check(eng.lib.infgen_step_score(P(eng.pos), P(eng.head), P(eng.state), P(eng.n_agents), P(eng.atype), P(eng._score_boxes()), S, A,
                                             eng.T, c, P(eng.road_records), P(eng.road_n_records), eng._road_cap, N, sweep, 0.0,
                                             (C.c_int * 3)(1, 0, 1), 0.5, P(score), 8, P(row), eng.ops.stream), 'infgen_step_score')
    launch(0); torch.cuda.synchronize()
    want = restated(c); torch.cuda.synchronize()
    counts_equal = bool((score[:, [0, 1, 3]] == want[:, [0, 1, 3]]).all())
    fin = torch.isfinite(want[:, 2])
    err = float((score[fin][:, [2, 4, 5]] - want[fin][:, [2, 4, 5]]).abs().max())
    ka, ta = [], []
    for _ in range(reps):
        ka.append(timed(launch))
        ta.append(timed(lambda: restated(c)))
    out.update(ms=float(np.median(ka)), all_ms=ka, torch_ms=float(np.median(ta)), torch_all_ms=ta, counts_equal_without_sweep=counts_equal,
               max_abs_diff_of_the_float_terms=err, records_per_scene=int(eng.road_n_records.max()))
else:                                  # 'guided' / 'unguided'
    fn = (lambda: eng.rollout_guided(every=4, keep=N // 2)) if mode == 'guided' else eng.rollout
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [timed(fn) for _ in range(reps)]
    out.update(ms=float(np.median(ms)), all_ms=ms, overlap_rate=rates()[0], offroad_rate=rates()[1])
print(json.dumps(out))
'''


def run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'worker {cmd[4:6]} failed ({out.returncode}): {out.stderr[-1500:]}')
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (figure a)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-reps', type=int, default=15)
    ap.add_argument('--setups', default='greedy,copies')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'step_scores.log'))
    a = ap.parse_args()
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    worker = lambda root, setup, mode, reps=a.reps: run([sys.executable, '-c', WORKER, root, setup, mode, str(a.warmup), str(reps), shapes])
    figures = []
    for setup in a.setups.split(','):
        what = '1024 greedy C3 scenes' if setup == 'greedy' else '32 C3 scenes x 32 copies, sample_k = 5'
        if a.parent:
            parent = os.path.abspath(a.parent)
            figures.append((f'(a) scoring off, {what}', [('parent', lambda s=setup: worker(parent, s, 'off')), ('this', lambda s=setup: worker(REPO, s, 'off'))]))
        figures.append((f'(b) scoring on, {what}', [('off', lambda s=setup: worker(REPO, s, 'off')), ('on', lambda s=setup: worker(REPO, s, 'on'))]))
        figures.append((f'(c) one k_step_score launch against the torch restatement, {what}',
                        [('kernel', lambda s=setup: worker(REPO, s, 'kernel', a.kernel_reps))]))
        if setup == 'copies':
            figures.append((f'(d) rollout_guided(every=4, keep=16), {what}',
                            [('unguided', lambda: worker(REPO, 'copies', 'unguided')), ('guided', lambda: worker(REPO, 'copies', 'guided'))]))
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
                for k in ('overlap_rate', 'offroad_rate', 'records_per_scene', 'counts_equal_without_sweep', 'max_abs_diff_of_the_float_terms',
                          'rows', 'slots', 'steps'):
                    if k in s:
                        entry[name][k] = s[k]
                if name == 'kernel':
                    tm = [x['torch_ms'] for x in got[name]]
                    entry[name].update(torch_median_ms=statistics.median(tm), torch_min_ms=min(tm), torch_max_ms=max(tm), torch_samples=tm)
                print(f'{figure}: round {r} {name}: {s["ms"]:.3f} ms', flush=True)
                write()
            entry['rounds'] = r + 1
        if 'parent' in entry:
            entry['this_median_inside_parents_spread'] = entry['parent']['min_ms'] <= entry['this']['median_ms'] <= entry['parent']['max_ms']
            entry['this_median_not_above_parents_max'] = entry['this']['median_ms'] <= entry['parent']['max_ms']
        if 'on' in entry:
            add = entry['on']['median_ms'] - entry['off']['median_ms']
            entry.update(added_ms_per_rollout=add, added_us_per_step=1e3 * add / entry['on']['steps'])
        write()
        print(json.dumps(entry), flush=True)


if __name__ == '__main__':
    main()
