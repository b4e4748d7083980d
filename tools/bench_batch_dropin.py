"""multi-graph inference on one MI355X: a ragged PyG-style Batch of C3-like scenes (40-64 agents, 800-1024 map tokens, R = 80,
about 10 % of the scenes with a row filtered at hc - 1) through InfGenDecoder.inference, next to
  - the ingest kernel alone (infgen_ingest_batch, HIP events),
  - RolloutEngine.reload_batch (the offsets' host copy + checks + the ingest),
  - engine.rollout of the same batch (the rollout-only floor),
  - the per-scene list entry (inference_batch on the split scenes: the host setup path ragged scenes take).
python tools/bench_batch_dropin.py [scenes] [reps]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _scene(args):
    from infgen_amd import synth
    i, = args
    cfg = synth.standard_config()
    rng = np.random.default_rng([i, 71])
    A, M = int(rng.integers(40, 65)), int(rng.integers(800, 1025))
    filtered = i % 10 == 3                                   # edge_cases with the ego last: a row filtered before the ego
    return synth.make_scene(i, A, M, cfg, ego_last=filtered or bool(rng.integers(0, 2)), edge_cases=filtered, slip=0.1)


def main():
    import bench
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    from infgen_amd import synth
    from infgen_amd.engine import read_batch_layout
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_boundary_cpu import _decoder
    from test_modules_gpu import _load, _to_data
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device('cuda:0')
    cfg = synth.standard_config()
    t0 = time.perf_counter()
    with ProcessPoolExecutor(8, mp_context=mp.get_context('spawn')) as pool:
        scenes = list(pool.map(_scene, [(i,) for i in range(S)], chunksize=8))
    t_build = time.perf_counter() - t0
    sd = synth.fill_state_dict(bench.load_shapes(), seed=1, rich=True)
    dec = _decoder(cfg)
    _load(dec, sd)
    dec = dec.to(dev).eval()
    datas = [_to_data(sc, dev) for sc in scenes]
    b = batch_datas(datas)
    A = np.diff(b['agent']['ptr'].cpu().numpy())
    M = np.diff(b['pt_token']['ptr'].cpu().numpy())
    nfilt = sum(int((sc['agent']['state_idx'][:, cfg.hist_columns - 1] == 0).any()) for sc in scenes)

    def wall(fn, n):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t_ = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t_)
        return float(np.median(ts)), float(np.min(ts))

    fresh = lambda: dict(b, agent=dict(b['agent']), batch_size_a=b['batch_size_a'].clone())
    t_inf = wall(lambda: dec.inference(fresh()), reps)
    eng = next(e for k, e in dec._engines.items() if k[0] == 'graphs')
    lay = read_batch_layout(b, eng.T, eng.hc, 1024)
    # the ingest alone, HIP events on the launch stream
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ing = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        ev0.record()
        eng._ingest(b, lay)
        ev1.record()
        torch.cuda.synchronize()
        ing.append(ev0.elapsed_time(ev1))
    ing = ing[1:]
    t_reload = wall(lambda: eng.reload_batch(b), reps)
    t_roll = wall(eng.rollout, reps)
    t_epi = wall(lambda: (setattr(eng, '_bc_host', None), eng.outputs_batch()), reps)
    t_list = wall(lambda: dec.inference_batch([dict(d) for d in datas]), max(2, reps // 2))
    steps = int(A.sum()) * cfg.num_recurrent_steps_val
    lines = [
        f'workload: {S} ragged scenes, agents {A.min()}-{A.max()} (sum {A.sum()}), map tokens {M.min()}-{M.max()}, '
        f'R = {cfg.num_recurrent_steps_val}, {nfilt} scenes with a row filtered at hc - 1; engine S = {eng.S}, A_cap = {eng.A_cap}, '
        f'M_cap = {eng.M_cap}; scene build {t_build:.1f} s (host, not timed below)',
        f'ingest kernel (HIP events)        median {np.median(ing):8.3f} ms  min {np.min(ing):8.3f} ms',
        f'reload_batch (ptr copy + ingest)  median {1e3 * t_reload[0]:8.3f} ms  min {1e3 * t_reload[1]:8.3f} ms',
        f'engine.rollout                    median {1e3 * t_roll[0]:8.1f} ms  min {1e3 * t_roll[1]:8.1f} ms  '
        f'({steps / t_roll[0] / 1e6:.2f} M agent-steps/s)',
        f'batched epilogue (outputs_batch)  median {1e3 * t_epi[0]:8.1f} ms  min {1e3 * t_epi[1]:8.1f} ms',
        f'inference(Batch) end to end       median {1e3 * t_inf[0]:8.1f} ms  min {1e3 * t_inf[1]:8.1f} ms  '
        f'({steps / t_inf[0] / 1e6:.2f} M agent-steps/s, {t_roll[0] / t_inf[0]:.3f} of rollout-only throughput, '
        f'{t_inf[0] / t_roll[0]:.3f} x rollout)',
        f'inference_batch(list, host path)  median {1e3 * t_list[0]:8.1f} ms  min {1e3 * t_list[1]:8.1f} ms  '
        f'({steps / t_list[0] / 1e6:.2f} M agent-steps/s)',
    ]
    for ln in lines:
        print(ln, flush=True)


if __name__ == '__main__':
    main()
