"""The rollout sink at validation size: one seeded, device-resident rollouts dict of 32 scenes x 32 rollouts (64 agents each,
insertion off) scored (i) the per-rollout way - output_to_rollouts, compute_metric_features and compute_scenario_metrics per
rollout, 1,024 times - and (ii) by LongMetric.update_rollouts (batched features, one infgen_bundle_scores call, one host copy,
every scenario scored over all its rollouts).  Wall clock around a device synchronise, after a warm-up, the two ways
alternating; the medians and the ratio are those of the alternating samples (the fast way's back-to-back median is reported
next to them).  Prints one JSON line.

    python tools/bench_scoring.py [--scenes 32] [--rollouts 32] [--agents 64] [--steps 80] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infgen_amd.metrics import (LongMetric, compute_metric_features, compute_scenario_metrics,  # noqa: E402
                                get_scenario_id_int_tensor, output_to_rollouts)
from infgen_amd.metrics.scores import FIELDS  # noqa: E402


def make_dict(S, R, N, steps, seed, dev):
    """vehicles on three lanes at different speeds, every rollout its own noise; enter / exit states sprinkled in"""
    rng = np.random.default_rng(seed)
    T10, T2 = 11 + steps, (11 + steps) // 5
    n = S * N
    lane = rng.integers(0, 3, (n, 1, 1))
    s0, speed = rng.uniform(0, 300, (n, 1, 1)), rng.uniform(2, 15, (n, R, 1))
    t = np.arange(T10)[None, None] * 0.1
    s = s0 + speed * t
    off = (lane - 1) * 3.5 + rng.normal(0, 0.3, (n, R, 1))
    heading = 0.3 + rng.normal(0, 0.01, (n, R, T10))
    cx, cy = s * np.cos(0.3) - off * np.sin(0.3), s * np.sin(0.3) + off * np.cos(0.3)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    valid = rng.random((n, R, T10)) > 0.05
    valid[N - 1::N] = True                                        # the ego: last row of every scene
    state = rng.choice([0, 1, 1, 1, 1, 1, 2, 3], size=(n, R, T2)).astype(np.int64)
    ids = np.tile(np.arange(100, 100 + N), S)
    shape = np.concatenate([rng.uniform(4.0, 5.5, (n, 1, 1)), rng.uniform(1.8, 2.2, (n, 1, 1)), np.full((n, 1, 1), 1.6)], -1)
    traj = np.stack([cx, cy], -1)
    return dict(scenario_id=get_scenario_id_int_tensor(['s%d' % i for i in range(S)]), av_id=100 + N - 1,
                agent_id=torch.from_numpy(ids)[:, None].repeat(1, R).to(dev),
                agent_batch=torch.arange(S).repeat_interleave(N).to(dev), agent_count=[N] * S,
                pred_traj=f32(traj), pred_z=torch.zeros(n, R, T10, device=dev), pred_head=f32(heading),
                pred_shape=f32(np.broadcast_to(shape, (n, R, 3))), pred_type=torch.zeros(n, R, dtype=torch.long, device=dev),
                pred_state=torch.from_numpy(state).to(dev), pred_valid=torch.from_numpy(valid).to(dev),
                token_pos=f32(traj[:, :, ::5][:, :, :T2]), token_head=f32(heading[:, :, ::5][:, :, :T2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', type=int, default=32)
    ap.add_argument('--rollouts', type=int, default=32)
    ap.add_argument('--agents', type=int, default=64)
    ap.add_argument('--steps', type=int, default=80)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    d = make_dict(a.scenes, a.rollouts, a.agents, a.steps, 11, dev)
    g = torch.Generator().manual_seed(5)
    bins = dict(linear_speed=(0, 25, 10), linear_acceleration=(-12, 12, 11), angular_speed=(-0.628, 0.628, 11),
                angular_acceleration=(-3.14, 3.14, 11), distance_to_nearest_object=(-5, 40, 10), collision_indication=(-0.5, 0.5, 2),
                time_to_collision=(0, 5, 10), num_placement=(0, 10, 10), num_removement=(0, 10, 10),
                distance_placement=(0, 100, 10), distance_removement=(0, 100, 10))
    config = {k: dict(histogram=dict(min_val=float(lo), max_val=float(hi), num_bins=nb), metametric_weight=1.0 / len(FIELDS))
              for k, (lo, hi, nb) in bins.items()}
    logp = {k: torch.log_softmax(torch.randn(nb, generator=g), 0) for k, (_, _, nb) in bins.items()}
    plain = {k: v for k, v in d.items() if k != 'agent_count'}

    def per_rollout():
        lm = LongMetric(metrics_config=config, log_distributions=logp)
        for sr in output_to_rollouts(plain):
            for scene in sr.joint_scenes:
                lm.update(metrics=compute_scenario_metrics(config, logp, compute_metric_features(scene)))
        return lm

    batched_lm = LongMetric(metrics_config=config, log_distributions=logp)      # (its packed table is built once, like a run's)

    def batched():
        batched_lm.reset()
        batched_lm.update_rollouts(d)
        return batched_lm

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(2):
        batched()
    warm = LongMetric(metrics_config=config, log_distributions=logp)
    for scene in output_to_rollouts(plain)[0].joint_scenes[:4]:                  # warm-up of the per-rollout path: a few rollouts
        warm.update(metrics=compute_scenario_metrics(config, logp, compute_metric_features(scene)))
    t_old, t_new, t_alone = [], [], []
    for _ in range(a.repeats):
        t_old.append(timed(per_rollout))
        t_new.append(timed(batched))
    for _ in range(7):                                     # the fast arm once more back to back: reported apart, never mixed in
        t_alone.append(timed(batched))
    old, new = statistics.median(t_old), statistics.median(t_new)
    print(json.dumps({'metric': 'rollout sink, all rollouts of a validation batch scored', 'unit': 'ms',
                      'scenes': a.scenes, 'rollouts': a.rollouts, 'agents': a.agents, 'steps': a.steps,
                      'windows': (a.steps - 80) // 5 + 1, 'per_rollout_path_ms': old, 'update_rollouts_ms': new,
                      'speedup': old / new, 'update_rollouts_back_to_back_ms': statistics.median(t_alone),
                      'per_rollout_path_samples_ms': t_old, 'update_rollouts_samples_ms': t_new,
                      'update_rollouts_back_to_back_samples_ms': t_alone,
                      'note': 'the per-rollout path scores each of the scenes x rollouts rollouts alone (what validation_step '
                              'does for one of them); update_rollouts scores every scenario over all its rollouts; the medians '
                              'and the speedup are those of the alternating samples'}))


if __name__ == '__main__':
    main()
