"""Timing and effect of signal-aware decoding (per-step token masks from stop lines and phases, k_signal_mask);
bench.py is untouched.

    python tools/measure_signal_masks.py --parent DIR [--rounds 3] [--log profiles/signal_masks.log] [--skip-bench | --skip-rollouts]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process, and the variants alternate A B C A B C ... so that drift of the machine lands on all of them alike.  Figures:

    bench       the default line, ``bench.py --gpus 1 --steps S --warmup W`` in the parent's tree and in this one (feature off)
    greedy      1024 C3 scenes, greedy: parent / this with the feature off / this with ``obey_signals`` - one stop line per map
                polygon whose light_type is STOP (``constraints.stop_lines_from_map``, at most 64 per scene), each on a 16-step cycle
                that is red for 8 steps, with a per-line offset (``constraints.signal_phase``); vehicles and cyclists are ruled

A sample is one engine, ``--warmup`` rollouts, then ``--reps`` timed ones between device events (their median).  Every sample of this
tree also reports the crossing share of the rollout: ``torch.ops.infgen_hip.signal_mask`` with an all-ones base over every stored
decode column, and the share of (ruled row, step) pairs whose emitted token the operator bans - the row's front point went across a
closed line that governed it; ``banned_row_steps`` counts the pairs in which the operator bans at least one token.  The feature-on
samples add the time of one k_signal_mask launch on the rollout's LAST column only - the C entry on the engine's own buffers between
device events, the median of 20 launches behind a warm-up one - and that step's rows with a banned token and fallback rows.
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
root_is_this = hasattr(engine.RolloutEngine, 'set_signals')      # (the parent's tree has no signal operators)
dev = torch.device('cuda:0')
with open(sys.argv[6]) as f:
    shapes = {k_: tuple(v) for k_, v in json.load(f).items()}
cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
sd = synth.fill_state_dict(shapes, seed=1, rich=True)
vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
distinct = [synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, half_extent=60.0, ego_last=True, vocab=vocab, grid=grid) for i in range(8)]
scenes = [distinct[i % 8] for i in range(scenes_n)]
PERIOD, RED = 16, 8
kw = {}
if root_is_this:
    from infgen_amd import constraints
    capped = []
    for d in distinct:                          # at most 64 STOP polygons per scene: the rest are read as GO
        light = np.asarray(d['map_polygon']['light_type']).copy()
        light[np.flatnonzero(light == 0)[64:]] = 1
        capped.append(dict(d, map_polygon=dict(d['map_polygon'], light_type=light)))
    l8, n8, _ = constraints.stop_lines_from_map(capped, states=(0,))
    K = l8.shape[1]
    rng = np.random.default_rng(7)
    p8 = np.stack([constraints.signal_phase(K, PERIOD, 0, RED, offset=rng.integers(0, PERIOD, K)) for _ in range(8)])
    pick = np.arange(scenes_n) % 8
    conf = dict(lines=l8[pick], n_lines=n8[pick], phase=p8[pick])
    if mode == 'signals':
        kw = dict(obey_signals=conf)
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
    rec = torch_ops.signal_records(torch.from_numpy(conf['lines']).to(dev), torch.from_numpy(conf['n_lines']).to(dev))
    phase = torch.from_numpy(np.ascontiguousarray(conf['phase'])).to(dev)
    eng._end_pose_table()
    end, shape = eng._coll_end, eng._shape10.reshape(eng.S, eng.A_cap, 3)
    ruled_n = crossed_n = banned_n = 0
    for t in range(steps):
        c = hc - 1 + t
        bits, count, info = torch.ops.infgen_hip.signal_mask(eng.pos, eng.head, eng.state, eng.n_agents, eng.atype, shape, c, end, rec,
                                                             phase, t, 1, 0.5, 0.5)
        tok = eng.token[:, c + 1].reshape(-1).long()
        ok = (info[:, 2] > 0) & (count > 0) & (tok >= 0) & (eng.state[:, c + 1].reshape(-1) != 0)
        word = bits.gather(1, (tok.clamp(min=0) // 32)[:, None])[:, 0]
        banned = ((word >> (tok.clamp(min=0) % 32).int()) & 1) == 0
        ruled_n += int(ok.sum()); crossed_n += int((ok & banned).sum()); banned_n += int((ok & (count < cfg.token_size)).sum())
    out['crossing'] = dict(ruled_row_steps=ruled_n, banned_row_steps=banned_n, crossed=crossed_n,
                           share_of_ruled=crossed_n / max(ruled_n, 1), share_of_banned=crossed_n / max(banned_n, 1),
                           lines_per_scene=float(conf['n_lines'].mean()))
if mode == 'signals':
    import ctypes as C
    from infgen_amd import _lib
    P, t, k, sg = _lib.ptr, cfg.num_decode_steps - 1, eng._signal, eng.obey_signals
    c = cfg.hist_columns - 1 + t
    sw = (C.c_int * 3)(*sg['types'])
    # the C entry on the engine's own buffers: the launch alone, no allocation
    call = lambda: _lib.check(eng.lib.infgen_signal_mask(
        P(eng.pos), P(eng.head), P(eng.state), P(eng.n_agents), None, P(eng.atype), P(k['shape']), eng.S, eng.A_cap, eng.T, c,
        P(eng._coll_end), cfg.token_size, P(k['records']), P(k['phase']), k['n_phase'], k['K'], t, eng.copies, sg['setback'], sg['align'],
        sw, None, 0, None, None, P(k['bits']), P(k['allowed']), P(k['info']), eng.ops.stream), 'infgen_signal_mask')
    call(); torch.cuda.synchronize()
    us = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); call(); e1.record(); e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    out['kernel_us'] = float(np.median(us))
    out['ruled_rows_last_step'] = int((eng.signal_info[:, 2] > 0).sum())
    out['banned_rows_last_step'] = int((eng.signal_allowed < cfg.token_size).sum())
    out['fallback_rows_last_step'] = int((eng.signal_allowed == 0).sum())
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
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'signal_masks.log'))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')

    def rollout(root, mode):
        return run([sys.executable, '-c', WORKER, root, str(a.scenes), mode, str(a.warmup), str(a.reps), shapes])

    def bench(root):
        r = run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', str(a.bench_warmup)], cwd=root)
        return dict(ms=r['ms_per_step'])

    figures = [(f'greedy {a.scenes} scenes', [('parent', lambda: rollout(parent, 'plain')), ('this', lambda: rollout(REPO, 'plain')),
                                              ('this + obey_signals', lambda: rollout(REPO, 'signals'))])]
    if a.skip_rollouts:
        figures = []
    if not a.skip_bench:
        figures.append((f'bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup} (ms per step)',
                        [('parent', lambda: bench(parent)), ('this', lambda: bench(REPO))]))
    results, ok = [], True

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
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
                for k in ('crossing', 'kernel_us', 'ruled_rows_last_step', 'banned_rows_last_step', 'fallback_rows_last_step',
                          'decode_steps'):
                    if k in s:
                        entry[name][k] = s[k]
                write()
            entry['rounds'] = r + 1
        par, new = entry['parent'], entry['this']
        entry['gate'] = 'pass' if new['median_ms'] <= par['max_ms'] else 'FAIL'
        if 'this + obey_signals' in entry:
            on = entry['this + obey_signals']
            entry['feature_cost_ms'] = on['median_ms'] - new['median_ms']
            entry['feature_cost_us_per_step'] = 1e3 * entry['feature_cost_ms'] / on['decode_steps']
        ok = ok and entry['gate'] == 'pass'
        write()
        print(json.dumps(entry), flush=True)
    if not ok:
        raise SystemExit("gate failed: with the feature off this tree's median is above the parent's own maximum")


if __name__ == '__main__':
    main()
