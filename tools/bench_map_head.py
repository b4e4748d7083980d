"""The cost of the map-token head, parent commit against this tree, alternating on one box:
  (a) InfGenDecoder.inference(Batch) on 512 ragged C3-like scenes (40-64 agents, 800-1024 map tokens) with pt_pred_mask /
      pt_target_mask from InfGen.sample_pt_pred (torch seed 0; 16 points per polyline);
  (b) the same call with all-False masks;
  (c) the plain `python bench.py` line.
Every figure: `--runs` fresh processes per tree (each reports the median of 5 timed calls after a warm-up), the two trees
alternating, medians reported.  Writes the log to profiles/r09_map_head.log (or --log).

python tools/bench_map_head.py --parent DIR [--runs 5] [--scenes 512] [--log FILE]
   DIR: a built checkout of the parent commit (libinfgen_hip.so in place)."""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(i):
    from infgen_amd import synth
    cfg = synth.standard_config()
    rng = np.random.default_rng([i, 71])
    A, M = int(rng.integers(40, 65)), 16 * int(rng.integers(50, 65))
    return synth.make_scene(i, A, M, cfg, ego_last=bool(rng.integers(0, 2)), edge_cases=False, slip=0.1)


def child(mode, scenes_file, reps=5):
    """runs in the measured tree (cwd): one process, one figure"""
    sys.path.insert(0, os.getcwd())
    sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
    import torch
    from infgen_amd import synth
    from infgen_amd.model.infgen import InfGen
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    from conftest import make_weights
    with open(scenes_file, 'rb') as f:
        scenes = pickle.load(f)
    dev = torch.device('cuda:0')
    dec = _decoder(synth.standard_config())
    _load(dec, make_weights(seed=1, head_gain=1.0))
    dec = dec.to(dev).eval()
    b = batch_datas([_to_data(sc, dev) for sc in scenes])
    M = np.diff(b['pt_token']['ptr'].cpu().numpy())
    tm = torch.zeros(int(M.sum()) // 16, 3, 16, dtype=torch.bool)
    tm[:, 0] = True
    d = {'pt_token': {'traj_mask': tm}}
    torch.manual_seed(0)
    InfGen.sample_pt_pred(None, d)
    for k in ('pt_pred_mask', 'pt_target_mask'):
        m = d['pt_token'][k] if mode == 'masks' else torch.zeros_like(d['pt_token'][k])
        b['pt_token'][k] = m.to(dev)
    fresh = lambda: dict(b, agent=dict(b['agent']), batch_size_a=b['batch_size_a'].clone())
    out = dec.inference(fresh())
    n_pred = int(out['map_next_token_prob'].shape[0])
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.inference(fresh())
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print(json.dumps(dict(ms=1e3 * float(np.median(ts)), n_pred=n_pred, tokens=int(M.sum()))), flush=True)


def _run(cmd, cwd, timeout):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if r.returncode:
        raise RuntimeError(f'{cmd} in {cwd} failed: {r.stderr[-3000:]}')
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', help='built checkout of the parent commit')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--scenes', type=int, default=512)
    ap.add_argument('--log', default=os.path.join(ROOT, 'profiles', 'r09_map_head.log'))
    ap.add_argument('--child', choices=['masks', 'empty'])
    ap.add_argument('--scenes-file')
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.scenes_file)
    sys.path.insert(0, ROOT)
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    with ProcessPoolExecutor(8, mp_context=mp.get_context('spawn')) as pool:
        scenes = list(pool.map(_scene, range(args.scenes), chunksize=8))
    fd, sf = tempfile.mkstemp(suffix='.pkl')
    with os.fdopen(fd, 'wb') as f:
        pickle.dump(scenes, f)
    trees = {'parent': os.path.abspath(args.parent), 'branch': ROOT}
    res = {(m, t): [] for m in ('masks', 'empty', 'bench') for t in trees}
    me = os.path.abspath(__file__)
    for i in range(args.runs):
        for t, d in trees.items():
            for m in ('masks', 'empty'):
                r = _run([sys.executable, me, '--child', m, '--scenes-file', sf], d, 600)
                res[(m, t)].append(r)
                print(f'run {i} {t:6s} {m:5s} {r}', flush=True)
            r = _run([sys.executable, 'bench.py'], d, 600)
            res[('bench', t)].append(dict(value=r['value'], ms=r['ms_per_step']))
            print(f'run {i} {t:6s} bench {r["value"] / 1e6:.2f} M', flush=True)
    os.unlink(sf)
    med = lambda xs: float(np.median(xs))
    lines = [f'# tools/bench_map_head.py: {args.scenes} ragged C3-like scenes, {args.runs} runs per tree, parent and branch alternating',
             f'# n_pred with masks: {res[("masks", "branch")][0]["n_pred"]} of {res[("masks", "branch")][0]["tokens"]} tokens '
             f'(the parent returns 0)']
    for m, what in (('masks', '(a) inference(Batch), sample_pt_pred masks'), ('empty', '(b) inference(Batch), empty masks')):
        p, b = [r['ms'] for r in res[(m, 'parent')]], [r['ms'] for r in res[(m, 'branch')]]
        lines.append(f'{what}: parent {" ".join(f"{x:.1f}" for x in p)} ms (median {med(p):.1f}, spread {min(p):.1f} - {max(p):.1f}); '
                     f'branch {" ".join(f"{x:.1f}" for x in b)} ms (median {med(b):.1f}); branch / parent {med(b) / med(p):.4f}')
    p, b = [r['value'] / 1e6 for r in res[('bench', 'parent')]], [r['value'] / 1e6 for r in res[('bench', 'branch')]]
    lines.append(f'(c) python bench.py: parent {" ".join(f"{x:.2f}" for x in p)} M (median {med(p):.2f}, spread {min(p):.2f} - '
                 f'{max(p):.2f}); branch {" ".join(f"{x:.2f}" for x in b)} M (median {med(b):.2f})')
    with open(args.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
