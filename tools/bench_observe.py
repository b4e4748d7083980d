"""Timing of the agent-frame observation (``observe_rows``, k_observe_rows); bench.py is untouched.

    python tools/bench_observe.py [--parent DIR] [--rounds 3] [--log profiles/observe.log]

All on 1024 C3 scenes (64 agents, 1024 map tokens).  Every sample is a fresh process; the variants of a figure alternate
A B A B ... and medians are reported with their spreads.  Figures:

    (a) kernel      one ``infgen_observe_rows`` launch - all 65536 rows of the final column, K = 16, Km = 32, radius = map_radius = 60 -
                    between device events, against the same result from torch ops on the same device tensors: explicit
                    differences [S, A, A] and [S, A, M], ``topk`` of the masked squared distances, gathers and the rotations.
                    Inside one process the two alternate; peak device memory of each above what the engine holds; the share of
                    rows whose indices agree (torch's topk does not promise the tie rule).
    (b) session     an ego-controlled session over all decode steps with and without one
                    ``observe(frame='agent', rows='controlled', neighbors=16, map_tokens=32, radius=60, map_radius=60)`` per step.
    (c) unchanged   the greedy ``bench.py --gpus 1`` line in this tree against ``--parent`` (a built checkout of the parent commit):
                    a rollout that never observes launches what the parent launches.  Skipped without ``--parent``.
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
S0, K, KM, RAD = 1024, 16, 32, 60.0
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
scenes = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(S0)]
steps, hc = cfg.num_decode_steps, cfg.hist_columns
w = engine.PackedWeights(sd, cfg, dev)
eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid)
S, A, M = eng.S, eng.A_cap, eng.M_cap
med = lambda x: float(np.median(x))

def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)

def peak(fn):
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(); base = torch.cuda.memory_allocated()
    r = fn(); torch.cuda.synchronize()
    return r, (torch.cuda.max_memory_allocated() - base) / 2 ** 20

def restated(c):
    """the observation of column c from torch ops -> nbr_index, map_index, nbr_feat [.., :2], map_feat [.., :2]"""
    p, h = eng.pos[:, c], eng.head[:, c]
    live = (eng.state[:, c] != 0) & (torch.arange(A, device=dev)[None] < eng.n_agents[:, None])
    ci, si = torch.cos(h), torch.sin(h)
    inf = torch.tensor(float('inf'), device=dev)
    d = p[:, None] - p[:, :, None]                                              # [S, A(i), A(j), 2] = pos[j] - pos[i]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    ok = live[:, None] & live[:, :, None] & ~torch.eye(A, dtype=torch.bool, device=dev)[None] & (d2 <= RAD * RAD)
    val, idx = torch.topk(torch.where(ok, d2, inf), K, dim=-1, largest=False)
    nbr_index = torch.where(torch.isfinite(val), idx, torch.full_like(idx, -1))
    dj = torch.gather(d, 2, idx[..., None].expand(-1, -1, -1, 2))
    nx = dj[..., 0] * ci[..., None] + dj[..., 1] * si[..., None]; ny = dj[..., 1] * ci[..., None] - dj[..., 0] * si[..., None]
    hj = torch.gather(h[:, None].expand(-1, A, -1), 2, idx)
    cj, sj = torch.cos(hj), torch.sin(hj)
    vel = (p - eng.pos[:, c - 1]) / 0.5 * ((eng.state[:, c - 1] != 0) & live)[..., None]
    vj = torch.gather(vel[:, None].expand(-1, A, -1, -1), 2, idx[..., None].expand(-1, -1, -1, 2))
    shp = torch.gather(eng._shape10[:, None, :, :2].expand(-1, A, -1, -1), 2, idx[..., None].expand(-1, -1, -1, 2))
    ty = torch.gather(eng.atype[:, None].expand(-1, A, -1), 2, idx).float()
    nbr = torch.stack([nx, ny, cj * ci[..., None] + sj * si[..., None], sj * ci[..., None] - cj * si[..., None],
                       vj[..., 0] * ci[..., None] + vj[..., 1] * si[..., None], vj[..., 1] * ci[..., None] - vj[..., 0] * si[..., None],
                       shp[..., 0], shp[..., 1], ty, torch.ones_like(nx)], -1) * (nbr_index >= 0)[..., None]
    mp = eng.map_pos
    dm = mp[:, None] - p[:, :, None]                                            # [S, A, M, 2]
    m2 = dm[..., 0] * dm[..., 0] + dm[..., 1] * dm[..., 1]
    okm = live[:, :, None] & (torch.arange(M, device=dev)[None] < eng.n_map[:, None])[:, None] & (m2 <= RAD * RAD)
    mval, midx = torch.topk(torch.where(okm, m2, inf), KM, dim=-1, largest=False)
    map_index = torch.where(torch.isfinite(mval), midx, torch.full_like(midx, -1))
    dmj = torch.gather(dm, 2, midx[..., None].expand(-1, -1, -1, 2))
    mx = dmj[..., 0] * ci[..., None] + dmj[..., 1] * si[..., None]; my = dmj[..., 1] * ci[..., None] - dmj[..., 0] * si[..., None]
    ho = torch.gather(eng.map_orient[:, None].expand(-1, A, -1), 2, midx)
    cm, sm = torch.cos(ho), torch.sin(ho)
    mt = torch.gather(eng._map_cat[1][:, None].expand(-1, A, -1), 2, midx).float()
    mapf = torch.stack([mx, my, cm * ci[..., None] + sm * si[..., None], sm * ci[..., None] - cm * si[..., None], mt,
                        torch.ones_like(mx)], -1) * (map_index >= 0)[..., None]
    return nbr_index, map_index, nbr, mapf

out = dict(rows=int(eng.rows), slots=S, steps=steps, K=K, Km=KM, radius=RAD)
if mode == 'kernel':
    eng.rollout()
    c = hc + steps - 1
    res = eng.observe_rows(c, neighbors=K, radius=RAD, map_tokens=KM, map_radius=RAD)
    kernel = lambda: eng.observe_rows(c, neighbors=K, radius=RAD, map_tokens=KM, map_radius=RAD, out=res)
    _, kpeak = peak(lambda: eng.observe_rows(c, neighbors=K, radius=RAD, map_tokens=KM, map_radius=RAD))
    want, tpeak = peak(lambda: restated(c))
    ni, mi = res['nbr_index'].view(S, A, K), res['map_index'].view(S, A, KM)
    same_n = float((ni == want[0]).all(-1).float().mean()); same_m = float((mi == want[1]).all(-1).float().mean())
    both = (ni == want[0]) & (ni >= 0)
    err = float((res['nbr_feat'].view(S, A, K, 10) - want[2]).abs()[both].max())
    del want
    for _ in range(warmup):
        kernel(); restated(c)
    torch.cuda.synchronize()
    ka, ta = [], []
    for _ in range(reps):
        ka.append(timed(kernel)); ta.append(timed(lambda: restated(c)))
    out.update(ms=med(ka), all_ms=ka, torch_ms=med(ta), torch_all_ms=ta, kernel_peak_mib=kpeak, torch_peak_mib=tpeak,
               rows_with_equal_nbr_index=same_n, rows_with_equal_map_index=same_m, max_abs_diff_of_equal_nbr_entries=err,
               mean_nbr_count=float(res['nbr_count'].float().mean()), mean_map_count=float(res['map_count'].float().mean()))
else:                                  # 'session_plain' / 'session_observe'
    free = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid)
    free.rollout()
    plan = torch.stack([free.token[torch.arange(S, device=dev), t, free.av.long()] for t in range(free.T)])     # [T, S]
    del free
    def session():
        ses = eng.session(controlled='ego')
        while not ses.done:
            if mode == 'session_observe':
                ses.observe(frame='agent', rows='controlled', neighbors=K, radius=RAD, map_tokens=KM, map_radius=RAD)
            ses.command(tokens=plan[hc + ses.t])
            ses.advance()
    for _ in range(warmup):
        session()
    torch.cuda.synchronize()
    ms = [timed(session) for _ in range(reps)]
    out.update(ms=med(ms), all_ms=ms, per_step_ms=med(ms) / steps)
print(json.dumps(out))
'''


def run(cmd, **kw):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, **kw)
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'{cmd[1:4]} failed ({out.returncode}): {out.stderr[-1500:]}')
    return json.loads(lines[-1])


def bench_line(root, steps, warmup):
    line = run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                '--no-cpu-baseline', '--no-parity', '--no-literal', '--no-strict', '--no-balance'], cwd=root)
    return dict(ms=line['value'], unit=line.get('unit'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (figure c)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--kernel-reps', type=int, default=15)
    ap.add_argument('--bench-steps', type=int, default=3)
    ap.add_argument('--figures', default='abc')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'observe.log'))
    a = ap.parse_args()
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    worker = lambda mode, reps=a.reps: run([sys.executable, '-c', WORKER, REPO, mode, str(a.warmup), str(reps), shapes])
    figures = []
    if 'a' in a.figures:
        figures.append(('(a) one observe_rows launch against torch ops, 65536 rows, K 16, Km 32, radii 60 (ms)',
                        [('kernel', lambda: worker('kernel', a.kernel_reps))]))
    if 'b' in a.figures:
        figures.append(('(b) ego-controlled session of 1024 scenes, one agent-frame observation per step (ms per session)',
                        [('plain', lambda: worker('session_plain')), ('observe', lambda: worker('session_observe'))]))
    if 'c' in a.figures and a.parent:
        parent = os.path.abspath(a.parent)
        figures.append((f'(c) greedy bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.warmup} line (its own unit)',
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
                entry[name].update({k: v for k, v in s.items() if k not in ('ms', 'all_ms', 'torch_ms', 'torch_all_ms')})
                if name == 'kernel':
                    tm = [x['torch_ms'] for x in got[name]]
                    entry[name].update(torch_median=statistics.median(tm), torch_min=min(tm), torch_max=max(tm), torch_samples=tm,
                                       torch_over_kernel=statistics.median(tm) / statistics.median(ms))
                print(f'{figure}: round {r} {name}: {s["ms"]:.4f}', flush=True)
                write()
            entry['rounds'] = r + 1
        if 'parent' in entry:
            entry['this_median_inside_parents_spread'] = entry['parent']['min'] <= entry['this']['median'] <= entry['parent']['max']
        if 'observe' in entry:
            add = entry['observe']['median'] - entry['plain']['median']
            entry.update(added_ms_per_session=add, added_us_per_step=1e3 * add / entry['observe']['steps'])
        write()
        print(json.dumps(entry), flush=True)


if __name__ == '__main__':
    main()
