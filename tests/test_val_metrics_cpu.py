"""CPU: the validation-step metrics' yardsticks.  tests/val_metrics_ref.py (vectorised numpy, the closed form of the overlap count
included) reproduces the fixtures the REFERENCE's infgen/utils/metrics.py produced (tests/golden/make_golden_valmetrics.py): every
integer exactly, the float sums to 1e-12 relative; the generator regenerates the fixtures bit for bit where the reference is
present; ``infgen.utils.metrics`` resolves to ``infgen_amd.utils.metrics`` through compat/; CPU tensors are refused."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import val_metrics_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
REFERENCE = '/root/reference'
FIXTURES = ['valmetrics_state.npz', 'valmetrics_grid.npz', 'valmetrics_traj.npz', 'valmetrics_ce.npz']
CE_CASES = ('c4_r300', 'c4_r1', 'c2048_r300', 'c2048_r1', 'c4_allmasked')


def _load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def test_state_counters_exact():
    f = _load('valmetrics_state.npz')
    st = dict(zip(('invalid', 'valid', 'enter', 'exit'), f['state_token'].tolist()))
    for T in (18, 162):
        for n in ('n65', 'n7', 'n1'):
            lo, hi = f[f't{T}_{n}_rows']
            assert hi - lo == int(n[1:])
            s, m = f[f't{T}_state'][lo:hi], f[f't{T}_mask'][lo:hi]
            assert np.array_equal(R.state_accuracy(s, None, st), f[f't{T}_{n}_nomask']), (T, n)
            assert np.array_equal(R.state_accuracy(s, m, st), f[f't{T}_{n}_mask']), (T, n)


def test_grid_overlap_closed_form_exact():
    g = _load('valmetrics_grid.npz')
    args = (g['state'], g['grid'], 18, int(g['enter_state']), int(g['seed_size']))
    assert np.array_equal(R.grid_overlap(*args), g['out_one'])
    assert np.array_equal(R.grid_overlap(*args, ptr=g['ptr3']), g['out_groups'])
    assert g['out_one'][0, 1] == 1 and g['out_one'][0, 2] == 1 and g['out_one'][0, 3] == 2 and g['out_one'][2, 4] == 0
    assert g['out_one'][3, 5] == 1 and g['out_one'][3, 6] == 0              # n_insert == seed_size / seed_size - 1


def test_traj_sums():
    t = _load('valmetrics_traj.npz')
    for T in (5, 91):
        a, ca, f, cf = R.traj_error(t[f't{T}_pred'], t[f't{T}_target'], t[f't{T}_valid'])
        assert (ca, cf) == (int(t[f't{T}_ade_count']), int(t[f't{T}_fde_count']))
        assert abs(a - t[f't{T}_ade_sum']) <= 1e-12 * abs(t[f't{T}_ade_sum'])
        assert abs(f - t[f't{T}_fde_sum']) <= 1e-12 * abs(t[f't{T}_fde_sum'])


@pytest.mark.parametrize('name', CE_CASES)
def test_cross_entropy_sums(name):
    c = _load('valmetrics_ce.npz')
    x = R.expand_logits(c[name + '_a'], c[name + '_u'], c[name + '_b'], c[name + '_v'])
    w = c[name + '_weight'] if name + '_weight' in c.files else None
    sums = R.ce_sums(x, c[name + '_target'], c[name + '_mask'], w)
    assert np.allclose(sums, c[name + '_sums'], rtol=1e-12, atol=0)
    loss = R.ce_loss(x, c[name + '_target'], c[name + '_mask'], w, float(c[name + '_eps']))
    if name == 'c4_allmasked':
        assert np.isnan(loss) and np.isnan(c[name + '_loss'])
    else:
        assert abs(loss - c[name + '_loss']) <= 1e-12 * abs(c[name + '_loss'])
    if name == 'c2048_r300':
        assert x[0].max() - x[0].min() >= 150.0                          # the row spread over +-80


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, 'infgen')), reason='needs /root/reference (build container only)')
def test_fixtures_regenerate_bit_for_bit(tmp_path):
    """the recipe of tests/test_golden_recipe_cpu.py: the generator runs in a scratch copy of tests/golden/ with the alias package
    importable, binds `infgen` to the reference anyway and rewrites the four files"""
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
    out = subprocess.run([sys.executable, str(root / 'tests' / 'golden' / 'make_golden_valmetrics.py')], capture_output=True,
                         text=True, timeout=900, env=env, cwd=str(root))
    assert out.returncode == 0, out.stderr[-2000:]
    for f in FIXTURES:
        a, b = np.load(root / 'tests' / 'golden' / f, allow_pickle=False), _load(f)
        assert sorted(a.files) == sorted(b.files), set(a.files) ^ set(b.files)
        for k in a.files:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), (f, k)


def test_compat_alias_is_the_same_class():
    code = ('import sys; sys.path[:0] = [%r, %r]\n'
            'from infgen.utils.metrics import StateAccuracy, GridOverlapRate, NumInsertAccuracy, TokenCls, minADE, minFDE, AverageMeter\n'
            'import infgen.utils.metrics as a, infgen_amd.utils.metrics as b\n'
            'assert a is b and StateAccuracy is b.StateAccuracy and a.__all__ == ["minADE", "minFDE", "TokenCls", "StateAccuracy", '
            '"GridOverlapRate"]\nprint("SAME")\n' % (os.path.join(REPO, 'compat'), REPO))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'SAME' in out.stdout, out.stderr[-1500:]


def test_cpu_tensors_are_refused():
    from infgen_amd._lib import InfgenHipError
    from infgen_amd.utils import metrics as M
    st = R.STATE_TOKEN
    z = torch.zeros(3, 18, dtype=torch.long)
    with pytest.raises(InfgenHipError):
        M.StateAccuracy(state_token=st).update(state_idx=z)
    with pytest.raises(InfgenHipError):
        M.GridOverlapRate(num_step=18, state_token=st, seed_size=4).update(state_token=z, grid_index=z)
    with pytest.raises(InfgenHipError):
        M.minADE(max_guesses=1).update(pred=torch.zeros(3, 5, 2), target=torch.zeros(3, 5, 2), valid_mask=torch.ones(3, 5, dtype=torch.bool))
    with pytest.raises(InfgenHipError):
        M.TokenCls(max_guesses=1).update(pred=z[:, :1], target=z[:, 0], valid_mask=torch.ones(3, dtype=torch.bool))
    with pytest.raises(InfgenHipError):
        M.AverageMeter().update(torch.zeros(4))
    with pytest.raises(InfgenHipError):
        M.masked_cross_entropy(torch.zeros(3, 4), torch.zeros(3, dtype=torch.long), torch.ones(3, dtype=torch.bool))
