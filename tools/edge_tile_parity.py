"""Bits and time of the fused edge-attention kernels against the parent commit ("k_edge_fused": the shared blocks of
csrc/edge_tile.cuh); bench.py is untouched.

    python tools/edge_tile_parity.py --parent DIR [--rounds 3] [--log profiles/edge_tile_parity.log]

``DIR`` holds a built checkout of the parent commit (its ``infgen_amd`` package with libinfgen_hip.so).  Every sample is a fresh
process with its own time limit; the first one that does not exit 0 ends the run.

    bits   one process per tree writes, into a temporary directory, agg' of the operator calls of tests/test_ops_gpu.py::
           test_edge_fused_instantiations_give_the_same_bits (k_edge_fused under edge_loop 6 / 4 / 8 / 8, k_edge_fused3) and
           pos / head / state / token / X / logits of one 16-step rollout of a ragged 8-scene batch with layers_p 1 and 0 and
           edge_kernel 0 and 2.  Required: every file byte-equal between the trees.
    time   the rollout bench.py times (its default scene count, agents, map tokens and rollout steps, read from bench.py) and a
           256-scene rollout of 16-agent scenes (8192 padded rows: two k_layers_p launches of 256 workgroups per decode step).  Parent and
           this tree alternate over ``--rounds`` rounds; a sample is the median of ``--reps`` timed rollouts after ``--warmup``.
           Gate: this tree's median lies inside the parent's own min .. max, or is no further above the parent's median than the
           parent's own spread (max - min) - all that three samples resolve.

A failed gate (or a file that differs) exits non-zero.
"""
import argparse
import filecmp
import json
import os
import pickle
import re
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r'''
import ctypes as C, json, os, pickle, sys
root, job, arg, shapes_path = sys.argv[1:5]
sys.path.insert(0, root)
import numpy as np, torch
from infgen_amd import engine, synth, packing, _lib
assert os.path.dirname(os.path.abspath(engine.__file__)).startswith(os.path.abspath(root)), engine.__file__
dev = torch.device('cuda:0')
with open(shapes_path) as f:
    shapes = {k: tuple(v) for k, v in json.load(f).items()}
lib = _lib.load()

def graph(rng, n_dst, n_src, max_deg, empty_rows):
    off, cnt, src, e = [], [], [], 0
    for i in range(n_dst):
        d = 0 if i in empty_rows else int(rng.integers(1, max_deg + 1))
        s = rng.choice(n_src, size=min(d, n_src), replace=False)
        off.append(e); cnt.append(len(s)); src += list(s); e += len(s)
    return np.array(off, np.int32), np.array(cnt, np.int32), np.array(src, np.int32)

def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

def save(out, name, t):
    t.detach().cpu().contiguous().numpy().tofile(os.path.join(out, name + '.bin'))

if job == 'bits':
    out = arg
    sd = synth.fill_state_dict(shapes, seed=3, rich=True)
    ops = engine.Ops(dev)
    pack = to_dev(packing.pack_attention_layer(sd, 'agent_encoder.a2a_attn_layers.1'))
    o = _lib.Options()
    _lib.check(lib.infgen_get_options(C.byref(o)))
    for n_dst, n_src, max_deg in ((45, 150, 130), (16, 40, 9)):
        rng = np.random.default_rng(n_dst + max_deg)
        off, cnt, src = graph(rng, n_dst, n_src, max_deg, (0, 7, n_dst - 1))
        E = len(src)
        r = torch.nn.functional.layer_norm(torch.from_numpy(rng.standard_normal((E, 128)).astype(np.float32) *
                                                            rng.uniform(0.2, 5.0, (E, 1)).astype(np.float32)), (128,)).to(dev).contiguous()
        q, k, v = to_dev(rng.standard_normal((n_dst, 128))), to_dev(rng.standard_normal((n_src, 128))), to_dev(rng.standard_normal((n_src, 128)) * 3.0)
        offd, cntd, srcd = (torch.from_numpy(a).to(dev) for a in (off, cnt, src))
        for i, (kern, loop) in enumerate(((0, 6), (0, 4), (0, 8), (0, 8), (2, 6))):
            o.edge_kernel, o.edge_loop, o.use = kern, loop, 0
            agg = torch.full((n_dst, 128), float('nan'), device=dev)
            with _lib.thread_options(o):
                ops.edge_attn(n_dst, q, pack, k, v, offd, cntd, srcd, r, agg, None, None, wide='fused')
            torch.cuda.synchronize()
            save(out, f'op_{n_dst}_{i}_k{kern}_g{loop}', agg)
    cfg = synth.standard_config(num_recurrent_steps_val=80)          # 16 decode steps
    sd = synth.fill_state_dict(shapes, seed=1, rich=True, head_gain=64.0)
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scenes = [synth.make_scene(8599, 64, 1024, cfg, vocab=vocab, grid=grid)]
    scenes += [synth.make_scene(8600 + i, a, m, cfg, ego_last=(i % 2 == 0), vocab=vocab, grid=grid, slip=0.3)
               for i, (a, m) in enumerate([(64, 1024), (9, 100), (40, 300), (64, 700), (33, 512), (17, 64), (50, 900)])]
    w = engine.PackedWeights(sd, cfg, dev)
    for lp in (1, 0):
        for kern in (0, 2):
            e = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, store_logits=True, use_graph=False,
                                     options=dict(layers_p=lp, edge_kernel=kern))
            e.rollout()
            torch.cuda.synchronize()
            for key in ('pos', 'head', 'state', 'token', 'X', 'logits'):
                save(out, f'rollout_lp{lp}_k{kern}_{key}', getattr(e, key))
            del e
    print(json.dumps(dict(files=len(os.listdir(out)))))
else:
    warmup, reps = int(sys.argv[5]), int(sys.argv[6])
    with open(arg, 'rb') as f:
        cfg, scenes, vocab, map_vocab, grid = pickle.load(f)
    sd = synth.fill_state_dict(shapes, seed=1, rich=True)
    w = engine.PackedWeights(sd, cfg, dev)
    eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid, store_logits=False)
    for _ in range(warmup):
        eng.rollout()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); eng.rollout(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps(dict(ms=float(np.median(ms)), all_ms=ms, rows=int(eng.rows))))
'''


def child(root, job, arg, extra=(), limit=600):
    shapes = os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')
    try:
        out = subprocess.run([sys.executable, '-c', WORKER, root, job, arg, shapes, *map(str, extra)],
                             capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise SystemExit(f'{job} {root}: no result within {limit} s - stopping')
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    if out.returncode or not lines:
        raise SystemExit(f'{job} {root} failed ({out.returncode}) - stopping: {out.stderr[-1500:]}')
    return json.loads(lines[-1])


def bench_defaults():
    """bench.py as a module and the scene count, agents, map tokens and rollout steps of its headline (its argparse defaults)"""
    sys.path.insert(0, REPO)
    import bench
    src = open(os.path.join(REPO, 'bench.py')).read()
    get = lambda flag: int(re.search(r"add_argument\('--%s', type=int, default=(\d+)" % flag, src).group(1))
    return bench, dict(scenes=get('scenes'), agents=get('agents'), map_tokens=get('map-tokens'), rollout_steps=get('rollout-steps'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='a built checkout of the parent commit')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--procs', type=int, default=8, help='processes that build the scenes')
    ap.add_argument('--log', default=os.path.join(REPO, 'profiles', 'edge_tile_parity.log'))
    a = ap.parse_args()
    trees = [('parent', os.path.abspath(a.parent)), ('this', REPO)]
    lines, ok = [], True
    with tempfile.TemporaryDirectory() as tmp:
        # ---- bits
        for name, root in trees:
            os.makedirs(os.path.join(tmp, name))
            child(root, 'bits', os.path.join(tmp, name))
        files = sorted(os.listdir(os.path.join(tmp, 'parent')))
        diff = [f for f in files if not filecmp.cmp(os.path.join(tmp, 'parent', f), os.path.join(tmp, 'this', f), shallow=False)]
        if sorted(os.listdir(os.path.join(tmp, 'this'))) != files:
            diff.append('(the trees wrote different file lists)')
        lines.append(json.dumps(dict(figure='bits', files=len(files), bytes=sum(os.path.getsize(os.path.join(tmp, 'parent', f)) for f in files),
                                     differing=diff, gate='pass' if not diff else 'FAIL')))
        print(lines[-1], flush=True)
        ok = ok and not diff
        # ---- time: the scenes are built once, here (no GPU in this process), and read by every sample
        bench, hd = bench_defaults()
        from infgen_amd import synth
        cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=hd['rollout_steps'])
        workloads = [('headline', hd['scenes'], hd['agents'], hd['map_tokens']), ('256 scenes x 16 agents (k_layers_p)', 256, 16, 256)]
        for wname, n, agents, map_tokens in workloads:
            scenes, vocab, map_vocab, grid = bench.build_scenes(cfg, list(range(n)), agents, map_tokens, procs=a.procs)
            path = os.path.join(tmp, 'scenes.pkl')
            with open(path, 'wb') as f:
                pickle.dump((cfg, scenes, vocab, map_vocab, grid), f)
            del scenes
            got = {name: [] for name, _ in trees}
            for r in range(a.rounds):
                for name, root in trees:             # alternating: drift of the machine lands on both alike
                    got[name].append(child(root, 'time', path, (a.warmup, a.reps)))
                    print(f'{wname} round {r} {name}: {got[name][-1]["ms"]:.3f} ms', flush=True)
            st = {}
            for name, _ in trees:
                ms = [s['ms'] for s in got[name]]
                st[name] = dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), samples=ms)
            par, new = st['parent'], st['this']
            inside = par['min_ms'] <= new['median_ms'] <= par['max_ms'] or new['median_ms'] < par['min_ms']
            within = new['median_ms'] - par['median_ms'] <= par['max_ms'] - par['min_ms']
            lines.append(json.dumps(dict(figure=wname, scenes=n, agents=agents, map_tokens=map_tokens, rows=got['this'][-1]['rows'],
                                         parent=par, this=new, inside_parent_range=inside, within_parent_spread=within,
                                         gate='pass' if (inside or within) else 'FAIL')))
            print(lines[-1], flush=True)
            ok = ok and (inside or within)
    lines.append(json.dumps(dict(verdict='pass' if ok else 'FAIL')))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if not ok:
        raise SystemExit('gate failed: bits differ from the parent, or a rollout is slower than the parent beyond its spread')


if __name__ == '__main__':
    main()
