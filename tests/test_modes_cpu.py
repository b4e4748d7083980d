"""CPU: the yardsticks of the mode selection and of minMultiADE / minMultiFDE.  tests/modes_ref.py (numpy, float64 distances, a
stable order) reproduces the fixtures the REFERENCE's batch_nms / new_batch_nms / minMultiFDE / minMultiADE produced
(tests/golden/make_golden_modes.py): indices and scores exactly, the float sums to 1e-12 relative; the generator regenerates
the fixtures bit for bit where the reference is present; the host-side argument checks raise before anything touches a device."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import modes_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
REFERENCE = '/root/reference'
FIXTURES = ['modes_nms.npz', 'modes_density.npz', 'modes_multi.npz']
NMS_CASES = ('b5_n33', 'b3_n64', 'b4_n6', 'b2_n2', 'b1_n1', 'b257_n16')
DENSITY_CASES = ('n33', 'n64', 'n33_k8')
MULTI_CASES = ('n1_m1_t1', 'n3_m6_t5', 'n300_m8_t5', 'n3_m8_t1', 'n300_m1_t5')


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


@pytest.mark.parametrize('name', NMS_CASES)
def test_restatement_equals_the_references_batch_nms(name):
    f = _load('modes_nms.npz')
    trajs, scores, thr, k = f[name + '_trajs'], f[name + '_scores'], float(f[name + '_thresh']), int(f[name + '_k'])
    assert len(R.near_threshold(trajs, thr)) == 0
    assert all(len(np.unique(r)) == len(r) for r in scores)
    t, s, i = R.select_modes(trajs, k, thr, scores=scores)
    assert np.array_equal(i, f[name + '_ret_idxs']) and i.min() >= 0
    assert np.array_equal(s, f[name + '_ret_scores'])
    assert np.array_equal(t, f[name + '_ret_trajs'])


@pytest.mark.parametrize('name', DENSITY_CASES)
def test_restatement_equals_the_references_new_batch_nms_up_to_the_cluster_member(name):
    f = _load('modes_density.npz')
    trajs, label, thr, k = f[name + '_trajs'], f[name + '_label'], float(f[name + '_thresh']), int(f[name + '_k'])
    assert len(R.near_threshold(trajs, thr)) == 0
    d = R.pair_dist(trajs)
    same = label[:, :, None] == label[:, None, :]
    assert d[same].max() < thr / 2 and d[~same].min() > 4 * thr
    sizes = [np.bincount(lab) for lab in label]
    assert all(len(np.unique(sz)) == len(sz) for sz in sizes)
    _, s, i = R.select_modes(trajs, k, thr)
    assert np.array_equal(s, f[name + '_ret_scores'])                          # exactly: float(count) / float(N)
    rows = np.arange(len(label))[:, None]
    assert np.array_equal(label[rows, i], label[rows, f[name + '_ret_idxs']])
    # by the definition the member is the cluster's lowest index not yet selected
    for b in range(len(label)):
        seen = set()
        for j in i[b]:
            members = [m for m in np.flatnonzero(label[b] == label[b, j]) if m not in seen]
            assert j == members[0]
            seen.add(int(j))


@pytest.mark.parametrize('name', MULTI_CASES)
def test_restatement_equals_the_references_multi_errors(name):
    f = _load('modes_multi.npz')
    pred, target, prob, valid = (f[f'{name}_{k}'] for k in ('pred', 'target', 'prob', 'valid'))
    G = int(f['max_guesses'])
    assert all(len(np.unique(r)) == len(r) for r in prob)
    for pr in (None, prob):
        for fe, ae in R.guess_errors(pred, target, pr, valid, G):
            assert len(np.unique(fe)) == len(fe) and len(np.unique(ae)) == len(ae)
    for with_prob in (0, 1):
        for keep in (0, 1):
            key = f'{name}_p{with_prob}_k{keep}'
            for crit in ('FDE', 'ADE'):
                a, fd, c = R.multi_traj_error(pred, target, prob if with_prob else None, valid, G, bool(keep), crit)
                tag = 'ade_' + crit.lower()
                assert c == int(f[f'{key}_{tag}_count']) == int(f[f'{key}_fde_count'])
                for got, want in ((a, float(f[f'{key}_{tag}_sum64'])), (fd, float(f[f'{key}_fde_sum64']))):
                    assert abs(got - want) <= 1e-12 * max(abs(want), 1e-300), (key, crit)
    if pred.shape[0] >= 3:                                # the row without a valid step is left out, the first-step-only row is kept
        assert not valid[1].any() and valid[2].sum() == 1 and valid[2, 0]
    with pytest.raises(ValueError, match='not a valid criterion'):
        R.multi_traj_error(pred, target, None, valid, G, True, 'XDE')


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, 'infgen')), reason='needs /root/reference (build container only)')
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    """the recipe of tests/test_golden_recipe_cpu.py: the generator runs in a scratch copy of tests/golden/ with the alias package
    importable, binds `infgen` to the reference anyway and rewrites the three files"""
    root = tmp_path / 'tree'
    (root / 'tests').mkdir(parents=True)
    shutil.copytree(GOLDEN, root / 'tests' / 'golden', ignore=shutil.ignore_patterns('__pycache__'))
    for f in FIXTURES:
        os.remove(root / 'tests' / 'golden' / f)
    for name in ('infgen_amd', 'oracle'):
        os.symlink(os.path.join(REPO, name), root / name)
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(REPO, 'compat'), REPO, env.get('PYTHONPATH', '')])
    env['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
    out = subprocess.run([sys.executable, str(root / 'tests' / 'golden' / 'make_golden_modes.py')], capture_output=True,
                         text=True, timeout=900, env=env, cwd=str(root))
    assert out.returncode == 0, out.stderr[-2000:]
    for f in FIXTURES:
        a, b = np.load(root / 'tests' / 'golden' / f, allow_pickle=False), _load(f)
        assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), (f, k)


def test_torch_form_of_batch_nms_equals_the_fixtures():
    """the timing comparison's torch helper computes what the reference computes (CPU tensors here)"""
    f = _load('modes_nms.npz')
    for name in ('b5_n33', 'b4_n6'):
        t, s, i = R.batch_nms_torch(torch.from_numpy(f[name + '_trajs']), torch.from_numpy(f[name + '_scores']),
                                    float(f[name + '_thresh']), int(f[name + '_k']))
        assert np.array_equal(i.numpy(), f[name + '_ret_idxs']) and np.array_equal(s.numpy(), f[name + '_ret_scores'])
        assert np.array_equal(t.numpy(), f[name + '_ret_trajs'])


def test_host_side_argument_checks():
    from infgen_amd import modes
    from infgen_amd._lib import InfgenHipError
    from infgen_amd.engine import RolloutEngine
    from infgen_amd.utils import metrics as M
    for copies, k, scores, word in ((1, 6, 'density', 'copies = 1'), (65, 6, 'density', 'copies = 65'), (32, 17, 'density', 'k = 17'),
                                    (4, 5, 'density', 'k = 5'), (32, 6, 'best', "'best'"), (32, 6, None, 'NoneType')):
        with pytest.raises(ValueError, match=word):
            modes.check_engine_args(copies, k, scores)
        # the engine's method makes these checks before it reads anything else of the engine
        with pytest.raises(ValueError, match=word):
            RolloutEngine.select_modes(types.SimpleNamespace(copies=copies), k=k, scores=scores)
    modes.check_engine_args(32, 6, 'logprob')
    modes.check_engine_args(2, 2, torch.zeros(1, 2))
    z = torch.zeros(2, 20, 3, 2)
    with pytest.raises(ValueError, match='k = 17'):
        modes.select_modes(z, k=17)
    with pytest.raises(ValueError, match='1..64'):
        modes.select_modes(torch.zeros(2, 65, 3, 2), k=6)
    with pytest.raises(ValueError, match='t_goal'):
        modes.select_modes(z, k=6, t_goal=3)
    with pytest.raises(ValueError, match='scores must be'):
        modes.select_modes(z, k=6, scores=torch.zeros(2, 19))
    with pytest.raises(InfgenHipError, match='GPU tensor'):
        modes.select_modes(z, k=6)                                       # no host implementation
    with pytest.raises(NotImplementedError, match='speed'):
        modes.batch_nms(z, torch.zeros(2, 20), 2.5, mode='speed')
    with pytest.raises(NotImplementedError, match='batch_nms_token'):
        modes.batch_nms_token(z, torch.zeros(2, 20), 2.5)
    with pytest.raises(ValueError, match='not a valid criterion'):
        M.minMultiADE().update(torch.zeros(3, 6, 5, 2), torch.zeros(3, 5, 2), min_criterion='XDE')
    with pytest.raises(InfgenHipError):
        M.minMultiFDE().update(torch.zeros(3, 6, 5, 2), torch.zeros(3, 5, 2))
    p = modes.mode_prob(torch.tensor([[3.0, 1.0, 0.0], [0.0, 0.0, 0.0]]), torch.tensor([[4, 2, -1], [1, 0, -1]]))
    assert torch.equal(p, torch.tensor([[0.75, 0.25, 0.0], [0.5, 0.5, 0.0]]))
    assert torch.equal(modes.mode_prob(torch.zeros(1, 3)), torch.zeros(1, 3))


def test_compat_alias_exports_the_new_names():
    code = ('import sys; sys.path[:0] = [%r, %r]\n'
            'from infgen.utils.metrics import minMultiADE, minMultiFDE\n'
            'from infgen.modes import batch_nms, new_batch_nms, select_modes\n'
            'import infgen_amd.utils.metrics as b, infgen_amd.modes as m\n'
            'assert minMultiADE is b.minMultiADE and minMultiFDE is b.minMultiFDE and batch_nms is m.batch_nms\nprint("SAME")\n'
            % (os.path.join(REPO, 'compat'), REPO))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'SAME' in out.stdout, out.stderr[-1500:]
