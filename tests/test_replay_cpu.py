"""CPU: log replay (RolloutEngine(replay=...)) - marshalling of the row masks and plans into the engine's [S][T][A_cap] arrays
(row filter, copies, the global row order of a Batch), the errors of malformed masks / plans, and the C ABI's new field."""
import ctypes as C

import numpy as np
import pytest
import torch

from infgen_amd import scene_setup, synth


def _scenes():
    cfg = synth.standard_config()
    vocab = synth.make_agent_vocab(cfg.token_size)
    grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
    # the second scene has rows the filter of agent_decoder.py:1609 drops (invalid at the last history column)
    scenes = [synth.make_scene(900, 12, 64, cfg, vocab=vocab, grid=grid),
              synth.make_scene(8201, 30, 120, cfg, ego_last=True, edge_cases=True, vocab=vocab, grid=grid, slip=0.1)]
    filts = [np.asarray(sc['agent']['state_idx'])[:, cfg.hist_columns - 1] != 0 for sc in scenes]
    assert filts[0].all() and not filts[1].all()
    return cfg, scenes, filts


def _expect(scenes, filts, entries, cfg, a_cap, copies):
    """the plan arrays, written row by row"""
    T, hc, S = cfg.num_columns, cfg.hist_columns, len(scenes) * copies
    tt = np.full((S, T, a_cap), -1, np.int32); ts = np.zeros((S, T, a_cap), np.int32)
    tp = np.zeros((S, T, a_cap, 2), np.float32); th = np.zeros((S, T, a_cap), np.float32)
    rr = np.zeros((S, a_cap), np.uint8)
    for i, (sc, f, e) in enumerate(zip(scenes, filts, entries)):
        ag = sc['agent']
        if e is None:
            continue
        if isinstance(e, tuple):
            m, tok, st, pos, head = e
        else:
            m, tok, st, pos, head = e, ag['token_idx'], ag['state_idx'], ag['token_pos'], ag['token_heading']
        kept = np.nonzero(f)[0]
        for r, src in enumerate(kept):
            if not m[src]:
                continue
            for j in range(copies):
                s = i * copies + j
                rr[s, r] = 1
                tt[s, hc:, r] = np.asarray(tok)[src, hc:T]; ts[s, hc:, r] = np.asarray(st)[src, hc:T]
                tp[s, hc:, r] = np.asarray(pos)[src, hc:T]; th[s, hc:, r] = np.asarray(head)[src, hc:T]
    return dict(teacher_token=tt, teacher_state=ts, teacher_pos=tp, teacher_head=th, replay_row=rr)


@pytest.mark.parametrize('copies', [1, 2])
def test_masks_and_plans_reach_the_engine_layout(copies):
    cfg, scenes, filts = _scenes()
    T, hc, a_cap = cfg.num_columns, cfg.hist_columns, 32
    rng = np.random.default_rng(3)
    n1 = filts[1].shape[0]
    m1 = rng.random(n1) < 0.5
    m1[np.nonzero(~filts[1])[0][0]] = True                       # a flagged row that the filter drops
    m1[int(np.asarray(scenes[1]['agent']['av_index']).reshape(-1)[0])] = True
    explicit = (m1, rng.integers(0, cfg.token_size, (n1, T)), rng.integers(1, 4, (n1, T)),
                rng.standard_normal((n1, T, 2)).astype(np.float32), rng.standard_normal((n1, T)).astype(np.float32))
    m0 = np.zeros(12, bool); m0[[0, 5, 11]] = True
    for entries in ([m0, explicit], [None, m1], [m0, None]):
        mask, plan = scene_setup.stage_replay(scenes, filts, entries, T)
        assert mask.shape == (2, int(filts[1].sum())) and mask.dtype == torch.bool
        got = scene_setup.replay_arrays(mask, plan, hc, T, a_cap, copies)
        want = _expect(scenes, filts, entries, cfg, a_cap, copies)
        assert got.keys() == want.keys()
        for k, v in want.items():
            assert got[k].numpy().dtype == v.dtype and np.array_equal(got[k].numpy(), v), k
        # a kept row carries its flag: the flagged rows of scene 1 are the kept ones of its mask, in order
        if entries[1] is not None:
            assert got['replay_row'][copies].numpy()[:mask.shape[1]].astype(bool).tolist() == m1[filts[1]].tolist()
    # a plan of tokens and states only: no pose arrays (the stored pose is then the forced token's integration)
    mask, plan = scene_setup.stage_replay(scenes, filts, [None, explicit[:3]], T)
    got = scene_setup.replay_arrays(mask, plan, hc, T, a_cap, copies)
    assert set(got) == {'teacher_token', 'teacher_state', 'replay_row'}
    assert np.array_equal(got['teacher_token'].numpy(), _expect(scenes, filts, [None, explicit], cfg, a_cap, copies)['teacher_token'])


def test_public_forms_of_the_mask():
    """'ego' / one tensor over all rows / one tensor per scene, per scene and in the global row order of a Batch"""
    counts, av = [5, 3, 4], [4, 0, 2]
    ego = scene_setup.replay_rows('ego', counts, av)
    assert [m.tolist() for m in ego] == [[False] * 4 + [True], [True, False, False], [False, False, True, False]]
    flat = torch.tensor([1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1], dtype=torch.bool)
    per = scene_setup.replay_rows(flat, counts, av)
    assert [m.numel() for m in per] == counts and torch.equal(torch.cat(per), flat)
    assert all(torch.equal(a, b) for a, b in zip(scene_setup.replay_rows(list(per), counts, av), per))
    ptr = np.concatenate([[0], np.cumsum(counts)])
    av_global = torch.tensor(av) + torch.from_numpy(ptr[:-1])
    g = scene_setup.replay_global('ego', 12, av_global, 3)
    assert g.dtype == torch.bool and torch.equal(g, torch.cat(ego))
    assert torch.equal(scene_setup.replay_global(flat, 12, av_global, 3), flat)
    assert torch.equal(scene_setup.replay_global(list(per), 12, av_global, 3), flat)


def test_malformed_masks_and_plans_raise():
    cfg, scenes, filts = _scenes()
    T = cfg.num_columns
    with pytest.raises(ValueError, match='rows'):
        scene_setup.stage_replay(scenes, filts, [np.zeros(11, bool), None], T)                 # mask length != the scene's rows
    with pytest.raises(ValueError, match='rows'):
        scene_setup.replay_rows(torch.zeros(11, dtype=torch.bool), [5, 3, 4], [0, 0, 0])
    with pytest.raises(ValueError, match='rows'):
        scene_setup.replay_rows([torch.zeros(5, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), torch.zeros(4, dtype=torch.bool)],
                                [5, 3, 4], [0, 0, 0])
    with pytest.raises(ValueError, match='rows'):
        scene_setup.replay_global(torch.zeros(11, dtype=torch.bool), 12, torch.tensor([0, 5, 8]), 3)
    with pytest.raises(ValueError):
        scene_setup.replay_rows('all', [5], [0])
    m = np.ones(12, bool)
    st = np.ones((12, T), np.int64)
    with pytest.raises(ValueError, match='tokens'):
        scene_setup.stage_replay(scenes, filts, [(m, None, st), None], T)                      # a plan without tokens
    with pytest.raises(ValueError, match='token_idx'):
        scene_setup.check_plan(dict(state_idx=st))
    with pytest.raises(ValueError, match='together'):
        scene_setup.check_plan(dict(token_idx=st, state_idx=st, token_pos=np.zeros((12, T, 2))))
    with pytest.raises(ValueError, match='columns'):
        scene_setup.stage_replay(scenes, filts, [(m, st[:, :T - 1], st), None], T)             # a plan shorter than the rollout
    # poses: every plan of a batch carries them (the logged future does) or none
    m1 = np.zeros(filts[1].shape[0], bool); m1[-1] = True
    with pytest.raises(ValueError, match='poses'):
        scene_setup.stage_replay(scenes, filts, [(m, st, st), m1], T)


def test_rollout_struct_grew_by_the_flag_pointer():
    """_lib.Rollout against the library's own sizeof (the header's struct), the new field next to the teacher poses; a context
    that flags rows without a plan is refused before anything is launched"""
    from infgen_amd import _lib
    lib = _lib.load()
    assert lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT) == C.sizeof(_lib.Rollout)
    assert _lib.Rollout.replay_row.offset == _lib.Rollout.teacher_head.offset + C.sizeof(C.c_void_p)
    assert _lib.Rollout.map_scene.offset == _lib.Rollout.replay_row.offset + C.sizeof(C.c_void_p)
    assert _lib.BatchIngest.replay_row.offset == C.sizeof(_lib.BatchIngest) - C.sizeof(C.c_void_p)
    c = _lib.Rollout()
    c.S, c.A_cap, c.T, c.M_cap, c.W, c.ring, c.num_layers = 1, 32, 4, 32, 1, 2, 1
    flags = (C.c_ubyte * 32)()
    c.replay_row = C.addressof(flags)
    assert lib.infgen_rollout_validate(C.byref(c)) != 0
    assert b'replay_row' in lib.infgen_last_error()
