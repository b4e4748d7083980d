"""the token-ablation models against the full-token model on one MI355X: one rollout of a batch of BASELINE C3-shaped scenes
(64 agents, 1024 map tokens, R = 80) per variant, with scenario insertion off and on (the natural seed head), timed with HIP
events around RolloutEngine.rollout.  Prints one JSON line per (variant, insertion).
python tools/bench_ablation.py [scenes] [reps]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = {'full': {}, 'grid': dict(use_grid_token=False), 'head': dict(use_head_token=False),
            'state': dict(use_state_token=False), 'grid_head': dict(use_grid_token=False, use_head_token=False)}


def _scene(i):
    from infgen_amd import synth
    cfg = synth.standard_config()
    return synth.make_scene(synth.scene_seed(3, i), 64, 1024, cfg, slip=0.3)


def _shapes(variant):
    from infgen_amd import synth
    golden = os.path.join(ROOT, 'tests', 'golden')
    with open(os.path.join(golden, 'state_dict_shapes.json')) as f, open(os.path.join(golden, 'state_dict_shapes_ablation.json')) as g:
        full, deltas = {k: tuple(v) for k, v in json.load(f).items()}, json.load(g)
    return full if variant == 'full' else synth.ablation_shapes(full, deltas[variant])


def main():
    from concurrent.futures import ProcessPoolExecutor
    from infgen_amd import engine, synth
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    dev = torch.device('cuda:0')
    t0 = time.time()
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        scenes = list(ex.map(_scene, range(S), chunksize=16))
    print(f'# {S} scenes made in {time.time() - t0:.1f} s', flush=True)
    base = synth.standard_config()
    vocab, map_vocab = synth.make_agent_vocab(base.token_size), synth.make_map_vocab()
    grid = synth.build_grid(base.grid_range, base.grid_interval, base.pl2seed_radius)
    for insertion in (False, True):
        for v, flags in VARIANTS.items():
            cfg = synth.standard_config()
            for k, x in flags.items():
                setattr(cfg, k, x)
            cfg.disable_insertion = not insertion
            sd = synth.fill_state_dict(_shapes(v), seed=1, rich=True, head_gain=64.0)
            w = engine.PackedWeights(sd, cfg, dev)
            eng = engine.RolloutEngine(w, scenes, vocab, map_vocab, grid)
            eng.rollout()                                   # warm-up (buffers, tables, edge capacities)
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.rollout()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            n = eng.n_agents.cpu().numpy()
            steps = eng.agent_steps()
            print(json.dumps(dict(variant=v, insertion=insertion, scenes=S, A_cap=eng.A_cap, ms=round(float(np.median(ms)), 2),
                                  ms_all=[round(x, 2) for x in ms], agents_final_mean=round(float(n.mean()), 1),
                                  agent_steps_per_s=round(steps / (np.median(ms) / 1e3)))), flush=True)
            del eng, w
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
