"""GPU: the split mode of infgen_rollout_run - the batch as two phase-shifted halves on two streams of the
library's own - against the single-stream path in the same process.  Per scene a half runs the same kernels on the same rows,
so every comparison here is bit for bit (np.array_equal), and the edge totals are equal.

INFGEN_SPLIT_HALVES is read at every call of infgen_rollout_run: 0 = off, 2 = forced (any even S: the small shapes of this
file), so one process runs both legs.  infgen_split_stats counts the calls that took either path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import load_case, make_weights

pytestmark = pytest.mark.gpu

KNOB, OFFSET = 'INFGEN_SPLIT_HALVES', 'INFGEN_SPLIT_OFFSET'


@pytest.fixture(autouse=True)
def _knobs_restored():
    old = {k: os.environ.get(k) for k in (KNOB, OFFSET)}
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _stats():
    from infgen_amd import _lib
    a, b = C.c_int(0), C.c_int(0)
    _lib.check(_lib.load().infgen_split_stats(C.byref(a), C.byref(b)))
    return a.value, b.value


@pytest.fixture(scope='module')
def small():
    """4 scenes x 16 agents x 64 map tokens, R = 10 (two decode steps); scene 0 keeps ONE valid agent, scene 3 is full"""
    from infgen_amd import engine, synth
    cfg = synth.smart_config(num_recurrent_steps_val=10)
    vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    scenes = [synth.make_scene(synth.scene_seed(7, s), 16, 64, cfg, vocab=vocab, grid=grid, slip=0.3) for s in range(4)]
    uneven = [synth.make_scene(synth.scene_seed(7, 0), 1, 64, cfg, vocab=vocab, grid=grid, slip=0.3)] + scenes[1:]
    w = engine.PackedWeights(make_weights(seed=1, head_gain=64.0), cfg, torch.device('cuda:0'))
    return dict(cfg=cfg, vocab=vocab, map_vocab=map_vocab, grid=grid, scenes=scenes, uneven=uneven, w=w)


@pytest.fixture(scope='module')
def c1():
    from infgen_amd import engine
    c = load_case('c1_a8_m128')
    c['w'] = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    return c


def _engine(k, scenes, **kw):
    from infgen_amd import engine
    kw.setdefault('store_logits', True)
    kw.setdefault('token_logprob', True)
    kw.setdefault('use_graph', False)
    return engine.RolloutEngine(k['w'], scenes, k['vocab'], k['map_vocab'], k['grid'], **kw)


def _run(eng, mode, offset=None):
    """one rollout under INFGEN_SPLIT_HALVES = mode -> (outputs, edge totals, split calls, single-stream calls)"""
    os.environ[KNOB] = str(mode)
    if offset is None:
        os.environ.pop(OFFSET, None)
    else:
        os.environ[OFFSET] = str(offset)
    s0 = _stats()
    eng.rollout()
    outs, tot = eng.outputs(), eng.edge_totals()
    s1 = _stats()
    return outs, tot, s1[0] - s0[0], s1[1] - s0[1]


def _same(a, b):
    assert len(a) == len(b)
    for s, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        for key in x:
            if isinstance(x[key], np.ndarray):
                assert np.array_equal(x[key], y[key], equal_nan=x[key].dtype.kind == 'f'), f'scene {s}: {key}'
    need = {'next_token_idx', 'next_state_idx', 'pos_a', 'head_a', 'pred_traj', 'pred_head', 'logits', 'next_token_logprob'}
    assert need <= set(a[0]), sorted(need - set(a[0]))


def _pair(k, scenes, took_split, **kw):
    ref, tot_ref, n_split, n_single = _run(_engine(k, scenes, **kw), 0)
    assert (n_split, n_single) == (0, 1)
    out, tot, n_split, n_single = _run(_engine(k, scenes, **kw), 2)
    assert (n_split, n_single) == ((1, 0) if took_split else (0, 1))
    _same(out, ref)
    assert tot == tot_ref
    return ref


@pytest.mark.parametrize('which', ['even', 'uneven'])
def test_forced_split_equals_the_single_stream_path(small, which):
    _pair(small, small['scenes'] if which == 'even' else small['uneven'], True)


@pytest.mark.parametrize('n', [2, 4])
def test_forced_split_of_the_duplicated_fixture(c1, n):
    ref = _pair(c1, [c1['scene']] * n, True)
    assert np.array_equal(ref[0]['next_token_idx'], c1['z']['next_token_idx'])      # (and the fixture's own tokens)


@pytest.mark.parametrize('offset', [0, 1, 4, 18])
def test_every_phase_offset_gives_the_same_results(small, offset):
    ref, tot_ref, _, _ = _run(_engine(small, small['uneven']), 0)
    out, tot, n_split, _ = _run(_engine(small, small['uneven']), 2, offset)
    assert n_split == 1
    _same(out, ref)
    assert tot == tot_ref


def test_odd_batch_and_split_copy_group_keep_the_single_stream_path(small, c1):
    _pair(small, small['scenes'][:3], False)
    _pair(c1, [c1['scene']], False, copies=2)                 # S = 2, both slots copies of one scene: the middle is inside the group
    _pair(c1, [c1['scene']] * 2, True, copies=2)              # S = 4: the middle is the boundary between the two groups


def test_insertion_engine_is_left_alone():
    from infgen_amd import engine
    c = load_case('ins_forced_a16_m256')
    c['cfg'].disable_insertion = False
    c['w'] = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    legs = []
    for mode in (0, 2):
        eng = _engine(c, [c['scene'], c['scene']], token_logprob=False, live_state=c['meta']['live_state'], force_enter=True)
        assert eng.insertion
        outs, _, n_split, _ = _run(eng, mode)
        assert n_split == 0
        legs.append(outs)
    _same_keys = [k for k in legs[0][0] if isinstance(legs[0][0][k], np.ndarray)]
    for x, y in zip(*legs):
        for key in _same_keys:
            assert np.array_equal(x[key], y[key], equal_nan=x[key].dtype.kind == 'f'), key


def test_sampling_with_caller_uniforms(small):
    steps = small['cfg'].num_decode_steps
    u = np.random.default_rng(3).random((steps, 4, 16), dtype=np.float32)
    ref = _pair(small, small['uneven'], True, sample_k=5, sample_uniforms=u, sample_logprob=True)
    greedy, _, _, _ = _run(_engine(small, small['uneven']), 0)
    assert any(not np.array_equal(a['next_token_idx'], b['next_token_idx']) for a, b in zip(ref, greedy)), 'the draws never left the arg-max'


def test_two_rollouts_reload_and_a_third(small):
    a, b = small['scenes'], small['uneven'][:2] + small['scenes'][:2]
    ref_eng, eng = _engine(small, a), _engine(small, a)
    for k, scenes in enumerate((a, a, b)):
        if k == 2:
            ref_eng.reload(scenes)
            eng.reload(scenes)
        ref, tot_ref, _, _ = _run(ref_eng, 0)
        out, tot, n_split, _ = _run(eng, 2)
        assert n_split == 1
        _same(out, ref)
        assert tot == tot_ref


def test_captured_graph_takes_the_single_stream_path(small):
    ref, tot_ref, _, _ = _run(_engine(small, small['scenes']), 0)
    eng = _engine(small, small['scenes'], use_graph=True)
    out, tot, n_split, n_single = _run(eng, 2)               # the engine's first rollout runs eagerly (kernels load outside a capture)
    assert (n_split, n_single) == (1, 0)
    _same(out, ref)
    out, tot, n_split, n_single = _run(eng, 2)               # the second one is captured and replayed: one call, under capture
    assert (n_split, n_single) == (0, 1), 'the capture must not fork: no graph with parallel branches'
    assert eng._graph is not None
    _same(out, ref)
    assert tot == tot_ref
    out, tot, n_split, n_single = _run(eng, 2)               # a replay calls nothing
    assert (n_split, n_single) == (0, 0)
    _same(out, ref)
