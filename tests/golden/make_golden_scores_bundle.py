"""Golden vectors for the BUNDLE scoring of LongMetric: the REFERENCE's own output_to_rollouts and
compute_scenario_metrics_for_bundle (infgen/metrics/compute_metrics.py:360-463, :891-1103) with its own metric_config.textproto
on a seeded rollouts dict of 2 scenarios (12 and 7 agents) x 3 rollouts over 200 steps - the features of a scenario's rollouts
concatenated along the objects, windows and reductions over the concatenation.  The dict has an entering and an exiting agent,
an overlapping pair (collision) and an agent that is valid in one rollout only.  Logged distributions: those of
make_golden_scores.py.  Build container only.

    PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION=python python tests/golden/make_golden_scores_bundle.py [--out DIR]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_golden_scores as mgs  # noqa: E402  (installs the stand-ins, imports the reference, patches its third-party names)
from make_golden_metrics import make_platoon  # noqa: E402

cm = mgs.cm
FIELDS = mgs.FIELDS
NAME = 'scores_bundle_s2_r3_t200.npz'
SEED, AGENTS, N_ROLLOUT, STEPS = 7801, (12, 7), 3, 200
EGO_ID = 999                    # the reference hands ONE av_id to every scenario of a dict (:371-373, :448)


def scenario_arrays(seed, N, n_rollout, R):
    """one scenario: every rollout its own platoon (same agents, same shapes), ego = last row"""
    T10, T2 = 11 + R, (11 + R) // 5
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    per = []
    shape0 = None
    for r in range(n_rollout):
        b = make_platoon(seed + 10 * r, N, T10)
        rng = np.random.default_rng(seed + 10 * r + 1)
        valid = b['valid'].copy()
        valid[N - 1] = True                                          # the ego is always there
        valid[1, :60] = False                                        # agent 1 enters at step 60 ...
        valid[2, 120:] = False                                       # ... agent 2 leaves at step 120
        if r != 1:
            valid[3] = False                                         # agent 3 exists in rollout 1 only
        cx, cy = b['cx'].copy(), b['cy'].copy()
        if r == 0:                                                   # agent 5 drives into agent 4: overlapping boxes
            cx[5, 100:140] = cx[4, 100:140] + 1.0
            cy[5, 100:140] = cy[4, 100:140] + 0.3
            valid[4:6, 100:140] = True
        state = rng.choice([0, 1, 1, 1, 1, 1, 2, 3], size=(N, T2)).astype(np.int64)
        state[1, 12], state[2, 24] = 2, 3
        if shape0 is None:
            shape0 = np.stack([b['length'][:, 0], b['width'][:, 0], np.full(N, 1.6)], -1)
        per.append(dict(
            pred_traj=f32(np.stack([cx, cy], -1)), pred_z=torch.zeros(N, T10), pred_head=f32(b['heading']),
            pred_shape=f32(shape0), pred_type=torch.zeros(N, dtype=torch.long), pred_state=torch.from_numpy(state),
            pred_valid=torch.from_numpy(valid),
            token_pos=f32(np.stack([cx[:, ::5][:, :T2], cy[:, ::5][:, :T2]], -1)), token_head=f32(b['heading'][:, ::5][:, :T2]),
            agent_id=torch.cat([torch.arange(100, 100 + N - 1), torch.tensor([EGO_ID])])))
    return {k: torch.stack([p[k] for p in per], 1) for k in per[0]}


def rollouts_dict(seed=SEED, agents=AGENTS, n_rollout=N_ROLLOUT, R=STEPS):
    scen = [scenario_arrays(seed + 100 * s, N, n_rollout, R) for s, N in enumerate(agents)]
    out = {k: torch.cat([s[k] for s in scen]) for k in scen[0]}
    out.update(scenario_id=cm.get_scenario_id_int_tensor(['b%d' % (seed + s) for s in range(len(agents))]), av_id=EGO_ID,
               agent_batch=torch.repeat_interleave(torch.arange(len(agents)), torch.tensor(agents)))
    return out


def generate():
    from google.protobuf import text_format
    with open('/root/reference/infgen/metrics/metric_config.textproto') as f:
        config = text_format.Parse(f.read(), cm.long_metrics_pb2.SimAgentMetricsConfig())
    with torch.no_grad():
        lf = cm.compute_metric_features(cm.output_to_rollouts(mgs.rollouts_dict(7701, 16, 80))[0].joint_scenes[0])
        vals = dict(linear_speed=lf.linear_speed, linear_acceleration=lf.linear_acceleration, angular_speed=lf.angular_speed,
                    angular_acceleration=lf.angular_acceleration, distance_to_nearest_object=lf.distance_to_nearest_object,
                    collision_indication=torch.any(torch.where(lf.valid, lf.collision_per_step, False), dim=1, keepdim=True),
                    time_to_collision=lf.time_to_collision, num_placement=lf.num_placement.float(),
                    num_removement=lf.num_removement.float(), distance_placement=lf.distance_placement,
                    distance_removement=lf.distance_removement)
        dists = {k: cm._get_log_distributions(k, getattr(config, k), torch.nan_to_num(v, nan=0.0),
                                              'bernoulli' if k == 'collision_indication' else 'histogram')
                 for k, v in vals.items()}
        log_d = cm.LogDistributions(**dists)
        scen = rollouts_dict()
        bundles = cm.output_to_rollouts(scen)
        results = [cm.compute_scenario_metrics_for_bundle(config, log_d, None, sr) for sr in bundles]
    out = {'in_' + k: v.numpy() for k, v in scen.items() if torch.is_tensor(v)}
    out.update({'logp_' + k: d.logits.numpy()[0] for k, d in dists.items()})
    n_hit = 0
    for s, (metrics, long) in enumerate(results):
        for k in FIELDS:
            v = getattr(metrics, k + '_likelihood')
            assert v > 0, f'scenario {s}: {k} has no non-empty window (choose another seed)'
            out[f's{s}_m_{k}_likelihood'] = np.float32(v)
        out[f's{s}_metametric'] = np.float32(metrics.metametric)
        out[f's{s}_simulated_collision_rate'] = np.float32(metrics.simulated_collision_rate)
        n_hit += metrics.simulated_collision_rate > 0
        out.update({f's{s}_l_{k}': v.numpy() for k, v in long.items() if torch.is_tensor(v)})
    assert n_hit > 0, 'no collision in the fixture'
    pv = scen['pred_valid']
    assert bool((pv.any(2).sum(1) == 1).any()), 'no agent that is valid in one rollout only'
    cfgd = {}
    for k in FIELDS:
        fc = getattr(config, k)
        if fc.HasField('histogram'):
            h = fc.histogram
            cfgd[k] = [h.min_val, h.max_val, h.num_bins, h.additive_smoothing_pseudocount, fc.metametric_weight]
        else:
            cfgd[k] = [-0.5, 0.5, 2, fc.bernoulli.additive_smoothing_pseudocount, fc.metametric_weight]
    out.update(av_id=np.int64(scen['av_id']), config=np.array([cfgd[k] for k in FIELDS], np.float64), fields=np.array(FIELDS),
               n_scenario=np.int64(len(results)))
    return out, results


def main():
    dst = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else HERE
    out, results = generate()
    np.savez_compressed(os.path.join(dst, NAME), **out)
    for s, (metrics, long) in enumerate(results):
        print('scenario', s, 'metametric', metrics.metametric, 'collision rate', metrics.simulated_collision_rate)
        for k in FIELDS:
            print('  ', k, getattr(metrics, k + '_likelihood'), tuple(long[k + '_likelihood'].shape))


if __name__ == '__main__':
    main()
