"""CPU: the reference's token-ablation models (configs/experiments/ablate_*_tokens.yaml) construct, carry the reference's
parameter tree per variant and pack; the generator of their golden rollouts reproduces the committed fixtures (build container
only, like test_golden_recipe_cpu.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, 'golden')
REFERENCE = '/root/reference'

# YAML fixture -> (variant of its state_dict, use_grid_token, use_head_token, use_state_token)
YAMLS = {'ablate_grid_tokens.yaml': ('grid', False, True, True),
         'ablate_head_tokens.yaml': ('head', True, False, True),
         # the configs write `disable_state_tokens`, both models read `disable_state_token`: from YAML the state ablation never
         # takes effect (kept as the reference has it)
         'ablate_state_tokens.yaml': (None, True, True, True),
         'ablate_state_and_grid_tokens.yaml': ('grid', False, True, True)}

# the fixtures of tests/golden/make_golden_ablation.py (tests/test_ablation_gpu.py rolls them out)
CASES = ('abl_grid_c1_a8_m128', 'abl_grid_ins_forced_a16_m256', 'abl_grid_ins_natural_a20_m256', 'abl_head_ins_forced_a16_m256',
         'abl_gridhead_ins_natural_a20_m256', 'abl_state_live_a16_m128')

VARIANT_FLAGS = {'grid': dict(use_grid_token=False), 'head': dict(use_head_token=False), 'state': dict(use_state_token=False),
                 'grid_head': dict(use_grid_token=False, use_head_token=False),
                 'state_grid': dict(use_grid_token=False, use_state_token=False)}


def _shapes(variant):
    """the reference's state_dict shapes of the full model (None) or of a variant"""
    from infgen_amd import synth
    with open(os.path.join(GOLDEN, 'state_dict_shapes.json')) as f:
        full = {k: tuple(v) for k, v in json.load(f).items()}
    if variant is None:
        return full
    with open(os.path.join(GOLDEN, 'state_dict_shapes_ablation.json')) as f:
        return synth.ablation_shapes(full, json.load(f)[variant])


def _model(yaml_name):
    from infgen_amd import synth
    from infgen_amd.model import InfGen
    from infgen_amd.utils.func import load_config_act
    cfg = load_config_act(os.path.join(GOLDEN, yaml_name))
    return InfGen(cfg.Model, map_token_traj=synth.make_map_vocab(), agent_tokens=synth.make_agent_vocab(2048))


@pytest.mark.parametrize('yaml_name', sorted(YAMLS))
def test_ablation_config_constructs_with_the_reference_parameter_tree(yaml_name):
    variant, grid, head, state = YAMLS[yaml_name]
    m = _model(yaml_name)
    ae = m.encoder.agent_encoder
    assert (m.use_grid_token, m.use_head_token, m.use_state_token) == (grid, head, state)
    assert (ae.use_grid_token, ae.use_head_token, ae.use_state_token) == (grid, head, state)
    assert m.val_close_loop and ae.num_recurrent_steps_val == 300
    if not grid:
        assert not m.predict_occ            # the model forces the occupancy heads off without the grid (reference infgen.py:63-64)
    got = {k[len('encoder.'):]: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith('encoder.')}
    assert got == _shapes(variant)


@pytest.mark.parametrize('variant', sorted(VARIANT_FLAGS))
def test_variant_modules_load_a_reference_checkpoint_strictly_and_pack(variant):
    """InfGenDecoder built with the variant's flags has the reference's keys and shapes; a checkpoint of them loads with
    strict=True and PackedWeights packs it (fusion_emb at K0 = 384 without the grid, the regression heads)"""
    from infgen_amd import engine, synth
    from infgen_amd.modules import Attr_Tokenizer, InfGenDecoder
    cfg = synth.standard_config()
    flags = VARIANT_FLAGS[variant]
    for k, v in flags.items():
        setattr(cfg, k, v)
    tok = Attr_Tokenizer(grid_range=cfg.grid_range, grid_interval=cfg.grid_interval, radius=cfg.pl2seed_radius,
                         angle_interval=cfg.angle_interval)
    dec = InfGenDecoder(decoder_type='agent_decoder', dataset='waymo', input_dim=2, hidden_dim=128, num_historical_steps=11,
                        pl2pl_radius=cfg.pl2pl_radius, time_span=cfg.time_span, pl2a_radius=cfg.pl2a_radius,
                        pl2seed_radius=cfg.pl2seed_radius, a2a_radius=cfg.a2a_radius, a2sa_radius=cfg.a2sa_radius,
                        pl2sa_radius=cfg.pl2sa_radius, num_freq_bands=64, num_map_layers=3, num_agent_layers=6, num_heads=8,
                        head_dim=16, dropout=0.1, map_token={'traj_src': torch.from_numpy(synth.make_map_vocab())},
                        token_size=2048, attr_tokenizer=tok, predict_motion=True, predict_state=True,
                        predict_occ=cfg.use_grid_token, state_token=cfg.state_token, seed_size=1, buffer_size=128,
                        num_recurrent_steps_val=80, **flags)
    shapes = _shapes(variant)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == shapes
    sd = synth.fill_state_dict(shapes, seed=1, rich=True, head_gain=64.0)
    full = dec.state_dict()
    dec.load_state_dict({k: torch.from_numpy(sd[k]) if k in sd else v for k, v in full.items()}, strict=True)
    w = engine.PackedWeights(sd, cfg, torch.device('cpu'))
    assert w.fusion_k0 == (384 if not cfg.use_grid_token else 512)
    assert ('seed_pos_rel_xy_predict_head' in w.heads) == (not cfg.use_grid_token)
    assert ('seed_pos_rel_token_predict_head' in w.heads) == cfg.use_grid_token
    assert ('seed_heading_rel_theta_predict_head' in w.heads) == (not cfg.use_head_token)
    # a pack of the other variant's config refuses these weights (fusion_emb's width says which model it is)
    other = synth.standard_config()
    other.use_grid_token = not cfg.use_grid_token
    with pytest.raises((ValueError, KeyError)):
        engine.PackedWeights(sd, other, torch.device('cpu'))


def test_forward_of_an_ablated_model_is_refused_by_name():
    """the teacher-forced forward implements the full-token model only: an ablated model says which flag, before any launch"""
    m = _model('ablate_head_tokens.yaml')
    with pytest.raises(NotImplementedError, match='use_head_token'):
        m(None)


def test_full_model_keeps_its_parameter_tree():
    from infgen_amd import synth
    cfg = synth.RolloutConfig()
    assert cfg.use_grid_token and cfg.use_head_token and cfg.use_state_token
    assert set(_shapes('grid')) - set(_shapes(None)) == {f'agent_encoder.seed_pos_rel_xy_predict_head.mlp.{i}.{p}'
                                                         for i in (0, 1, 3) for p in ('weight', 'bias')}


def test_abi_blocks_carry_the_switches_at_their_end():
    from infgen_amd import _lib
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT) == _lib.C.sizeof(_lib.Rollout)
    names = [f[0] for f in _lib.Rollout._fields_]
    assert names[-2:] == ['no_grid_token', 'no_state_token']
    names = [f[0] for f in _lib.Insertion._fields_]
    assert names[-4:] == ['head_pos_xy', 'head_heading_theta', 'no_grid_token', 'no_head_token']


def test_fixtures_are_strict_and_small():
    """every ablation fixture is free-running with a margin above the logits bar, and within the committed-file limit"""
    for name in CASES:
        path = os.path.join(GOLDEN, name + '.npz')
        assert os.path.getsize(path) <= 1 << 20, name
        z = np.load(path)
        assert z['margin'].min() > 1e-3, name


_needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, 'infgen')),
                                      reason='needs /root/reference (build container only)')


@_needs_reference
def test_ablation_generator_regenerates_bit_for_bit(tmp_path):
    """make_golden_ablation.py: the reference's own InfGenDecoder with the flags off; fixtures, shapes and YAML copies equal"""
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([os.path.join(REPO, 'compat'), REPO, env.get('PYTHONPATH', '')])
    env['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
    code = ('import sys, runpy, inspect; sys.argv = ["make_golden_ablation.py", "--out", %r]; '
            'runpy.run_path(%r, run_name="__main__"); '
            'from infgen.modules.agent_decoder import InfGenAgentDecoder as D; print("SRC", inspect.getsourcefile(D))'
            % (str(tmp_path), os.path.join(GOLDEN, 'make_golden_ablation.py')))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=1800, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    src = [ln for ln in out.stdout.splitlines() if ln.startswith('SRC ')][-1].split(' ', 1)[1]
    assert src.startswith(REFERENCE + '/'), src
    for f in sorted(os.listdir(tmp_path)):
        new, old = os.path.join(str(tmp_path), f), os.path.join(GOLDEN, f)
        if f.endswith('.npz'):
            a, b = np.load(new, allow_pickle=False), np.load(old, allow_pickle=False)
            assert sorted(a.files) == sorted(b.files), (f, set(a.files) ^ set(b.files))
            for k in a.files:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == 'f'), (f, k)
        elif f.endswith(('.json', '.yaml')):
            with open(new, 'rb') as x, open(old, 'rb') as y:
                assert x.read() == y.read(), f
    assert {f for f in os.listdir(tmp_path) if f.endswith('.npz')} == {c + '.npz' for c in CASES}
