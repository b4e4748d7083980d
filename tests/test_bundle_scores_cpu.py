"""Bundle semantics of the scoring, independent of the device: the oracle functions (oracle/metrics_oracle.py,
oracle/scores_oracle.py) applied to the features of ALL rollouts of a scenario concatenated along the objects reproduce the
REFERENCE's compute_scenario_metrics_for_bundle on a 2-scenario x 3-rollout dict (tests/golden/make_golden_scores_bundle.py ->
scores_bundle_s2_r3_t200.npz), to the bar tests/test_oracle_golden.py holds the single-rollout fixture to.  Where the reference
is present, the generator reproduces the fixture bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
FIXTURE = 'scores_bundle_s2_r3_t200.npz'
REFERENCE = '/root/reference'


def bundle_fixture():
    """-> (npz, rollouts dict, field names, cfg per field, logp per field)"""
    z = np.load(os.path.join(GOLDEN, FIXTURE))
    scen = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('in_')}
    scen['av_id'] = int(z['av_id'])
    fields = [str(f) for f in z['fields']]
    cfg = {f: z['config'][i].tolist() for i, f in enumerate(fields)}
    logp = {f: torch.from_numpy(z['logp_' + f]) for f in fields}
    return z, scen, fields, cfg, logp


def oracle_rollout_features(scen, s, r):
    """the feature dict of rollout ``r`` of scenario ``s`` by the oracle functions (as test_oracle_golden.py builds it)"""
    from oracle import metrics_oracle as mo, scores_oracle as so
    rows = torch.nonzero(scen['agent_batch'] == s)[:, 0]
    g = lambda k: scen[k][rows][:, r]
    x, y = g('pred_traj')[..., 0], g('pred_traj')[..., 1]
    N, T = x.shape
    hd, valid = g('pred_head'), g('pred_valid')
    ln, wd = g('pred_shape')[:, 0:1].expand(N, T), g('pred_shape')[:, 1:2].expand(N, T)
    every = torch.ones(N, dtype=torch.bool)
    feat = dict(valid=valid[:, 11:])
    for k, a in zip(so.KINEMATIC, mo.kinematic_features(x, y, torch.zeros_like(x), hd, 0.1)):
        feat[k] = a[:, 11:]
    d = mo.distance_to_nearest_object(x, y, ln, wd, hd, valid, every)[:, 11:]
    feat.update(distance_to_nearest_object=d, collision_per_step=d < 0,
                time_to_collision=mo.time_to_collision(x, y, ln, wd, hd, valid, every, 0.1)[:, 11:])
    tp = g('token_pos')
    pos3 = torch.cat([tp, torch.zeros(N, tp.shape[1], 1)], -1)
    ego = g('agent_id').tolist().index(scen['av_id'])
    nb, ne, db, de = mo.placement_features(pos3, g('pred_state'), ego)
    feat.update(num_placement=nb[None, 2:], num_removement=ne[None, 2:], distance_placement=db[:, 2:], distance_removement=de[:, 2:])
    return feat


def test_oracle_on_concatenated_rollouts_matches_reference_bundle():
    from oracle import scores_oracle as so
    z, scen, fields, cfg, logp = bundle_fixture()
    n_rollout = scen['pred_traj'].shape[1]
    assert int(z['n_scenario']) == 2 and n_rollout == 3
    for s in range(int(z['n_scenario'])):
        per = [oracle_rollout_features(scen, s, r) for r in range(n_rollout)]
        # THE bundle: objects of rollout 0, then 1, ... (reference compute_metrics.py:911-916); the counts are one row per rollout
        feat = {k: torch.cat([p[k] for p in per], 0) for k in per[0]}
        scal, long = so.scenario_scores(feat, logp, cfg)
        for f in fields:
            assert abs(scal[f] - float(z[f's{s}_m_{f}_likelihood'])) <= 1e-7, (s, f)
            assert torch.equal(long[f], torch.from_numpy(z[f's{s}_l_{f}_likelihood'])), (s, f)
        assert long['num_placement'].shape == (n_rollout, 25)
        assert abs(scal['metametric'] - float(z[f's{s}_metametric'])) <= 1e-6
        assert torch.equal(long['metametric'], torch.from_numpy(z[f's{s}_l_metametric']))
        assert abs(scal['simulated_collision_rate'] - float(z[f's{s}_simulated_collision_rate'])) <= 1e-7


def test_bundle_differs_from_its_first_rollout():
    """the fixture tells the bundle from what scoring rollout 0 alone gives (what validation_step does without
    score_all_rollouts)"""
    from oracle import scores_oracle as so
    z, scen, fields, cfg, logp = bundle_fixture()
    scal, _ = so.scenario_scores(oracle_rollout_features(scen, 0, 0), logp, cfg)
    assert max(abs(scal[f] - float(z[f's0_m_{f}_likelihood'])) for f in fields) > 1e-3


def test_fixture_has_what_it_promises():
    z, scen, fields, cfg, logp = bundle_fixture()
    valid = scen['pred_valid']
    assert bool((valid.any(2).sum(1) == 1).any()), 'an agent valid in one rollout only'
    assert sorted(torch.bincount(scen['agent_batch']).tolist()) == [7, 12]
    assert valid.shape[2] == 211
    assert any(float(z[f's{s}_simulated_collision_rate']) > 0 for s in range(2))
    assert all(float(z[f's{s}_m_{f}_likelihood']) > 0 for s in range(2) for f in fields)
    assert os.path.getsize(os.path.join(GOLDEN, FIXTURE)) < 1 << 20


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, 'infgen')), reason='needs /root/reference (build container only)')
def test_bundle_fixture_regenerates_bit_for_bit(tmp_path):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([REPO, env.get('PYTHONPATH', '')])
    env['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
    out = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_golden_scores_bundle.py'), '--out', str(tmp_path)],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    a, b = np.load(os.path.join(str(tmp_path), FIXTURE)), np.load(os.path.join(GOLDEN, FIXTURE))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), k
