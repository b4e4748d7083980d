"""host time of the scene setup in front of the first launch: setup + padding (RolloutEngine._setup_scenes + _scene_arrays)
of 512 host scenes, no GPU - a ragged batch (20-39 agents, 150-199 map tokens) and a one-shape batch (40 agents, 200 map
tokens); median / min / max of the repeats after one warm-up (profiles/scene_setup_merge.txt).
python tools/bench_scene_setup.py [scenes] [reps]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def main():
    from infgen_amd import synth
    from make_golden_scene_setup import blank_engine, scene_arrays
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    cfg = synth.standard_config()
    vocab = synth.make_agent_vocab(cfg.token_size)
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    rng = np.random.default_rng(3)
    batches = {
        'ragged': [synth.make_scene(100 + i, int(rng.integers(20, 40)), int(rng.integers(150, 200)), cfg, ego_last=bool(i % 2),
                                    vocab=vocab, grid=grid) for i in range(S)],
        'one-shape': [synth.make_scene(5000 + i, 40, 200, cfg, ego_last=bool(i % 2), vocab=vocab, grid=grid) for i in range(S)]}
    for name, scenes in batches.items():
        e = blank_engine(cfg, S, m_cap=224)
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            scene_arrays(e, scenes)
            ts.append(1e3 * (time.perf_counter() - t0))
        ts = ts[1:]
        print(f'{name:10s} {S} scenes: median {np.median(ts):7.1f} ms  min {min(ts):7.1f} ms  max {max(ts):7.1f} ms  ({reps} repeats)',
              flush=True)


if __name__ == '__main__':
    main()
