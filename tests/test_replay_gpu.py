"""GPU: log replay in the closed-loop rollout (RolloutEngine(replay=...), InfGenDecoder.inference(replay=...)): flagged rows
follow a plan - their logged future or an explicit one - and the others are generated around them.

The reference has no such mode; parity is defined against what the tree already pins: the all-row teacher path (bit for bit)
and the CPU oracle teacher-forced with all-row tokens and states (the tree's 1e-3 logits bar)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_case

pytestmark = pytest.mark.gpu

STATE = ('token', 'state', 'pos', 'head', 'gridtok')


@functools.lru_cache(maxsize=None)
def _case(name, insertion=False):
    from infgen_amd import engine
    c = load_case(name)
    c['cfg'].disable_insertion = not insertion
    c['w'] = engine.PackedWeights(c['sd'], c['cfg'], torch.device('cuda:0'))
    c['av'] = int(np.asarray(c['scene']['agent']['av_index']).reshape(-1)[0])
    return c


def _eng(c, scenes=None, run=True, **kw):
    from infgen_amd import engine
    eng = engine.RolloutEngine(c['w'], scenes if scenes is not None else [c['scene']], c['vocab'], c['map_vocab'], c['grid'],
                               store_logits=True, **kw)
    if run:
        eng.rollout()
    return eng


def _snap(eng, s=None, rows=None):
    """the stored columns and the logits of scene s (all scenes: None), cloned"""
    torch.cuda.synchronize()
    A_cap = eng.A_cap
    if s is None:
        return {**{k: getattr(eng, k).clone() for k in STATE}, 'logits': eng.logits.clone()}
    n = A_cap if rows is None else rows
    out = {k: getattr(eng, k)[s, :, :n].clone() for k in STATE}
    out['logits'] = eng.logits[:, s * A_cap:s * A_cap + n].clone()
    return out


def _same(a, b, what=''):
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (what, k)


def _mask(n, rows):
    m = np.zeros(n, bool)
    m[list(rows)] = True
    return m


def _mixed_plan(c):
    """rows {ego, 3, 5} follow the fixture's tokens rotated by one row - not what the model would emit - with valid states"""
    z = c['z']
    A = z['next_token_idx'].shape[0]
    flag = _mask(A, [c['av'], 3, 5])
    return flag, np.roll(z['next_token_idx'], 1, axis=0), np.ones_like(z['next_state_idx'])


def test_all_rows_flagged_is_the_teacher_path_and_none_is_the_free_rollout():
    c = _case('c1_a8_m128')
    z = c['z']
    A = z['next_token_idx'].shape[0]
    plan = (z['next_token_idx'], z['next_state_idx'])
    forced = _snap(_eng(c, teacher=[plan]))
    _same(_snap(_eng(c, replay=[(np.ones(A, bool),) + plan])), forced, 'all rows flagged')
    free = _snap(_eng(c))
    _same(_snap(_eng(c, replay=[np.zeros(A, bool)])), free, 'no row flagged')
    _same(_snap(_eng(c, replay=[None])), free, 'no entry')
    with pytest.raises(ValueError):
        _eng(c, run=False, teacher=[plan], replay=[np.ones(A, bool)])


def test_mixed_mask_against_the_teacher_path_and_the_oracle(torch_sd):
    from oracle import rollout_oracle as ro
    c = _case('c1_a8_m128')
    cfg, hc = c['cfg'], c['cfg'].hist_columns
    flag, ptok, pst = _mixed_plan(c)
    assert (ptok[flag][:, hc:] != c['z']['next_token_idx'][flag][:, hc:]).any()
    eng = _eng(c, replay=[(flag, ptok, pst)])
    o = eng.outputs()[0]
    # (a) the flagged rows store the plan
    assert np.array_equal(o['next_token_idx'][flag][:, hc:], ptok[flag][:, hc:])
    assert np.array_equal(o['next_state_idx'][flag][:, hc:], pst[flag][:, hc:])
    assert np.array_equal(o['replay_mask'], flag)
    assert (o['next_token_idx'][~flag][:, hc:] != c['z']['next_token_idx'][~flag][:, hc:]).any(), 'the others react'
    # (b) the run's own history through the all-row teacher path: every stored column and every step's logits again, bit for bit
    _same(_snap(_eng(c, teacher=[(o['next_token_idx'], o['next_state_idx'])])), _snap(eng), 'teacher path')
    # (c) the CPU oracle, teacher-forced with the same all-row tokens and states
    ref = ro.run_scene(torch_sd(c['sd']), c['scene'], cfg, c['vocab'], c['map_vocab'], c['grid'],
                       teacher=(o['next_token_idx'], o['next_state_idx']))
    lg = ref['logits'].numpy()
    err = float(np.abs(o['logits'] - lg).max())
    srt = np.sort(lg, axis=-1)
    margin = float((srt[..., -1] - srt[..., -2])[:, ~flag].min())
    print(f'mixed mask: max logits error {err:.2e}, smallest top-1 / top-2 margin of the oracle at generated rows {margin:.3f}')
    assert margin > 4e-3, 'a tie would decide: choose another plan (the sharpened head keeps the margins wide)'
    assert err <= 1e-3
    assert np.array_equal(lg.argmax(-1).T[~flag], o['next_token_idx'][~flag][:, hc:])


def test_explicit_poses_are_stored_and_seen_by_the_neighbours():
    c = _case('c1_a8_m128')
    cfg, hc, z = c['cfg'], c['cfg'].hist_columns, c['z']
    A = z['next_token_idx'].shape[0]
    flag = _mask(A, [c['av'], 3, 5])
    tok, st = z['next_token_idx'], np.ones_like(z['next_state_idx'])
    # the plan's poses: the free rollout's, moved by a fixed offset (80 m: out of the other agents' neighbourhood)
    pos = z['pos_a'].astype(np.float32) + np.asarray([80.0, -40.0], np.float32)
    head = z['head_a'].astype(np.float32) + np.float32(0.3)

    def stepwise(**kw):
        eng = _eng(c, run=False, **kw)
        eng.prologue()
        totals, acnt = [], []
        for t in range(cfg.num_decode_steps):
            eng.step(t)
            totals.append(eng.edge_totals())
            acnt.append(eng.edges['a']['cnt'][:A].clone())
        return eng, np.asarray(totals), torch.stack(acnt).cpu().numpy()
    eng, tot_p, acnt_p = stepwise(replay=[(flag, tok, st, pos, head)])
    o = eng.outputs()[0]
    assert np.array_equal(o['next_token_idx'][flag][:, hc:], tok[flag][:, hc:])
    assert np.array_equal(o['next_state_idx'][flag][:, hc:], st[flag][:, hc:])
    assert np.array_equal(o['pos_a'][flag][:, hc:], pos[flag][:, hc:]) and np.array_equal(o['head_a'][flag][:, hc:], head[flag][:, hc:])
    # the stored poses of the generated rows are their own integration, not the plan's
    assert not np.array_equal(o['pos_a'][~flag][:, hc:], pos[~flag][:, hc:])
    full = _eng(c, teacher=[(o['next_token_idx'], o['next_state_idx'], None, o['pos_a'], o['head_a'])])
    _same(_snap(full), _snap(eng), 'teacher path with poses')
    _, tot_0, acnt_0 = stepwise(replay=[(flag, tok, st)])
    assert (tot_p[:, 1] != tot_0[:, 1]).any() and (tot_p[:, 2] != tot_0[:, 2]).any(), (tot_p, tot_0)
    assert (acnt_p[:, ~flag] != acnt_0[:, ~flag]).any(), 'the generated rows see the replayed poses'


def _three(c):
    from infgen_amd import synth
    cfg = c['cfg']
    scenes = [c['scene']] + [synth.make_scene(synth.scene_seed(1, i), 8, 128, cfg, vocab=c['vocab'], grid=c['grid']) for i in (1, 2)]
    avs = [int(np.asarray(sc['agent']['av_index']).reshape(-1)[0]) for sc in scenes]
    masks = [np.zeros(8, bool), _mask(8, [avs[1]]), np.ones(8, bool)]
    return scenes, masks


def test_three_scene_batch_equals_single_scene_runs_on_every_path():
    from infgen_amd import engine
    from infgen_amd.modules.infgen_decoder import batch_datas, stack_datas
    from test_modules_gpu import _to_data
    c = _case('c1_a8_m128')
    dev = torch.device('cuda:0')
    scenes, masks = _three(c)
    single = [_snap(_eng(c, [sc], replay=[m]), 0) for sc, m in zip(scenes, masks)]
    assert not torch.equal(single[1]['token'], _snap(_eng(c, [scenes[1]]), 0)['token']), 'replaying the ego changes the scene'

    def check(eng, ref, what, copies=1):
        for s in range(len(ref) * copies):
            _same(_snap(eng, s), ref[s // copies], (what, s))
    host = _eng(c, scenes, replay=masks)
    check(host, single, 'host scenes')
    # a second reload with other masks: the same buffers, a new plan
    masks2 = [masks[2], masks[0], _mask(8, [0, 3])]
    single2 = [_snap(_eng(c, [sc], replay=[m]), 0) for sc, m in zip(scenes, masks2)]
    host.reload(scenes, replay=masks2)
    host.rollout()
    check(host, single2, 'reload with a new mask')
    _same(_snap(host), _snap(_eng(c, scenes, replay=masks2)), 'reload against a fresh engine')
    # stacked device tensors: the plan never visits the host
    datas = [_to_data(sc, dev) for sc in scenes]
    stk = stack_datas(datas, min_scenes=1)
    assert stk is not None and host.fits_device(stk)
    assert host.reload_device(stk, scenes, replay=torch.from_numpy(np.stack(masks)).to(dev))
    host.rollout()
    check(host, single, 'stacked device tensors')
    # a ragged Batch through the ingest kernel, the mask in the global row order
    b = batch_datas(datas)
    gmask = torch.from_numpy(np.concatenate(masks)).to(dev)
    eb = engine.RolloutEngine(c['w'], None, c['vocab'], c['map_vocab'], c['grid'], store_logits=True, batch=b, replay=gmask)
    eb.rollout()
    check(eb, single, 'ragged Batch')
    fresh = _eng(c, scenes, run=False, replay=masks)           # the ingest kernel's plan buffers against the host staging
    for k in ('teacher_token', 'teacher_state', 'teacher_pos', 'teacher_head', 'replay_row'):
        assert torch.equal(getattr(eb, k), getattr(fresh, k)), k
    outs = eb.outputs_batch()[0]
    assert outs['replay_mask'].dtype == torch.bool and np.array_equal(outs['replay_mask'].cpu().numpy(), np.concatenate(masks))
    eb.reload_batch(b, replay=torch.from_numpy(np.concatenate(masks2)).to(dev))
    eb.rollout()
    check(eb, single2, 'ragged Batch, reload')
    # copies = 2: every copy replays the same plan
    check(_eng(c, scenes, replay=masks, copies=2), single, 'host scenes, copies', copies=2)
    eb2 = engine.RolloutEngine(c['w'], None, c['vocab'], c['map_vocab'], c['grid'], store_logits=True, batch=b, replay=gmask, copies=2)
    eb2.rollout()
    check(eb2, single, 'ragged Batch, copies', copies=2)


def test_row_filter_and_explicit_plan_through_the_ingest_kernel():
    """a Batch with a row the filter drops before a flagged one, plan given explicitly (a planner's): the ingest kernel's plan
    buffers equal the host staging bit for bit, padding included"""
    from infgen_amd import engine
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_batch_inference_gpu import _ragged3
    from test_modules_gpu import _to_data
    c = _case('a24_m256_edge')
    cfg, dev = c['cfg'], torch.device('cuda:0')
    scenes = _ragged3(c)
    rng = np.random.default_rng(11)
    masks = [rng.random(np.asarray(sc['agent']['state_idx']).shape[0]) < 0.5 for sc in scenes]
    masks[0][:] = True                                      # (scene 0 has a filtered row: its flag is dropped with it)
    T = cfg.num_columns
    plans = [(m, rng.integers(0, cfg.token_size, (m.shape[0], T)), rng.integers(1, 3, (m.shape[0], T)),
              rng.standard_normal((m.shape[0], T, 2)).astype(np.float32), rng.standard_normal((m.shape[0], T)).astype(np.float32))
             for m in masks]
    b = batch_datas([_to_data(sc, dev) for sc in scenes])
    for copies in (1, 2):
        for host_rp, dev_rp in ((masks, torch.from_numpy(np.concatenate(masks)).to(dev)),
                                (plans, (torch.from_numpy(np.concatenate(masks)).to(dev),
                                         {k: torch.from_numpy(np.concatenate([p[i] for p in plans])).to(dev)
                                          for i, k in enumerate(('token_idx', 'state_idx', 'token_pos', 'token_heading'), start=1)}))):
            eb = engine.RolloutEngine(c['w'], None, c['vocab'], c['map_vocab'], c['grid'], batch=b, replay=dev_rp, copies=copies)
            eh = engine.RolloutEngine(c['w'], scenes, c['vocab'], c['map_vocab'], c['grid'], replay=host_rp, copies=copies,
                                      a_cap=eb.A_cap, m_cap=eb.M_cap)
            for k in ('teacher_token', 'teacher_state', 'teacher_pos', 'teacher_head', 'replay_row'):
                x, y = getattr(eb, k), getattr(eh, k)
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (k, copies)
            assert int(eb.replay_row.sum()) == copies * sum(int((m & (np.asarray(sc['agent']['state_idx'])[:, cfg.hist_columns - 1] != 0)).sum())
                                                             for m, sc in zip(masks, scenes))


def test_replayed_ego_outside_workgroup_zero():
    """k_integrate deals a scene's rows to several workgroups when the batch is small (csrc/api.hip integrate_groups: up to 128
    scenes, A_cap > 16 and a multiple of 16 -> 16 rows per workgroup).  A_cap = 32 is the smallest such layout: two workgroups.
    The ego sits in the second one and is replayed; the first one integrates the ego for itself and must use the replayed
    pose.  The switch is read from the environment once per process, so the one-group run is not available here: the grid
    cells are recomputed from the stored poses instead (attr_tokenizer.py:77-89).  A cell may differ from the recomputed one
    only where two cells are equidistant to float32 rounding: the engine's cell must be within 1e-4 m of the nearest."""
    from infgen_amd import synth
    c = _case('c1_a8_m128')
    cfg, hc = c['cfg'], c['cfg'].hist_columns
    scene = synth.make_scene(4242, 20, 128, cfg, ego_last=True, vocab=c['vocab'], grid=c['grid'])
    av = int(np.asarray(scene['agent']['av_index']).reshape(-1)[0])
    assert av >= 16
    eng = _eng(c, [scene], replay=[_mask(20, [av])], a_cap=32)
    assert eng.S <= 128 and eng.A_cap == 32 and eng.A_cap // 16 == 2
    o = eng.outputs()[0]
    A = o['pos_a'].shape[0]
    ego = int(o['ego_index'])
    assert ego >= 16 and o['replay_mask'][ego] and o['replay_mask'].sum() == 1
    logged = np.asarray(scene['agent']['token_pos'])[np.asarray(scene['agent']['state_idx'])[:, hc - 1] != 0]
    assert np.array_equal(o['pos_a'][ego, hc:], logged[ego, hc:])
    free = _eng(c, [scene], a_cap=32).outputs()[0]
    assert np.abs(free['pos_a'][ego, hc:] - o['pos_a'][ego, hc:]).max() > 1.0, 'the replayed ego is not where the generated one is'
    pos, head = torch.from_numpy(o['pos_a']).double(), torch.from_numpy(o['head_a']).double()
    grid = torch.from_numpy(np.asarray(c['grid'])).double()
    cells = eng.gridtok[0, :, :A].T.cpu().numpy()
    state = o['next_state_idx']
    checked = 0
    for col in range(hc, cfg.num_columns):
        phi = -(head[ego, col] - np.pi / 2)
        d = pos[:, col] - pos[ego, col]
        rx = d[:, 0] * torch.cos(phi) - d[:, 1] * torch.sin(phi)
        ry = d[:, 0] * torch.sin(phi) + d[:, 1] * torch.cos(phi)
        dist = torch.sqrt((rx[:, None] - grid[None, :, 0]) ** 2 + (ry[:, None] - grid[None, :, 1]) ** 2)     # [A, G]
        for a in range(A):
            if state[a, col] == 0:
                assert cells[a, col] == -1
                continue
            assert float(dist[a, cells[a, col]] - dist[a].min()) <= 1e-4, (col, a, int(cells[a, col]), int(dist[a].argmin()))
            checked += 1
    assert checked >= 16 * (cfg.num_columns - hc)


def test_insertion_on_with_replayed_initial_rows():
    c = _case('ins_forced_a16_m256', insertion=True)
    cfg, hc = c['cfg'], c['cfg'].hist_columns
    ag = c['scene']['agent']
    A0 = np.asarray(ag['state_idx']).shape[0]
    flag = _mask(A0, [c['av'], 2, 5])
    eng = _eng(c, replay=[flag], force_enter=True)
    o = eng.outputs()[0]
    A = o['pos_a'].shape[0]
    assert o['num_inserted'] > 0 and A == A0 + o['num_inserted']
    assert np.array_equal(o['replay_mask'][:A0], flag) and not o['replay_mask'][A0:].any()
    for key, src in (('next_token_idx', 'token_idx'), ('next_state_idx', 'state_idx'), ('pos_a', 'token_pos'), ('head_a', 'token_heading')):
        assert np.array_equal(o[key][:A0][flag][:, hc:], np.asarray(ag[src])[flag][:, hc:]), key
    free = _eng(c, force_enter=True).outputs()[0]
    assert not np.array_equal(free['next_token_idx'][:A0][flag][:, hc:], np.asarray(ag['token_idx'])[flag][:, hc:])
    full = _eng(c, teacher=[(o['next_token_idx'], o['next_state_idx'], None, o['pos_a'], o['head_a'])], force_enter=True,
                insert_headroom=eng.A_cap - A0)
    assert full.A_cap == eng.A_cap
    f = full.outputs()[0]
    assert f['pos_a'].shape[0] == A
    a, b = _snap(eng, 0, A), _snap(full, 0, A)
    for k in STATE:
        assert torch.equal(a[k], b[k]), k
    bos = eng.bos[0, :A].cpu().numpy()
    assert np.array_equal(bos, full.bos[0, :A].cpu().numpy())
    for t in range(cfg.num_decode_steps):          # (a row inserted at column bos holds logits from decode step bos - 1 on)
        n = A0 + int((bos[A0:] <= 1 + t).sum())
        assert torch.equal(a['logits'][t, :n], b['logits'][t, :n]), t


@pytest.mark.parametrize('mode', [True, 'all'])
def test_graph_capture_replays_the_current_plan(mode):
    c = _case('c1_a8_m128')
    flag, ptok, pst = _mixed_plan(c)
    scenes, masks = _three(c)
    eager = _snap(_eng(c, scenes, replay=masks))
    eng = _eng(c, scenes, run=False, replay=masks, use_graph=mode)
    for i in range(3):                               # eager warm-up, capture, replay
        eng.rollout()
        _same(_snap(eng), eager, (mode, i))
    assert (eng._wgraph if mode == 'all' else eng._graph) is not None
    # a new plan in the same buffers: contents change, pointers do not
    new = [(flag, ptok, pst, np.asarray(scenes[0]['agent']['token_pos']), np.asarray(scenes[0]['agent']['token_heading'])), masks[2], masks[1]]
    eager2 = _snap(_eng(c, scenes, replay=new))
    assert not torch.equal(eager2['token'], eager['token'])
    graph_before = eng._graph
    eng.reload(scenes, replay=new)
    for i in range(3):
        eng.rollout()
        _same(_snap(eng), eager2, (mode, 'reload', i))
    if mode is True:
        assert eng._graph is graph_before, 'the captured decode steps were replayed, not captured again'


def _integrated(vocab, atype, tok, pos, head):
    """the five 10 Hz poses of token ``tok`` integrated from (pos, head): reference agent_decoder.py:2168-2239"""
    ct = vocab[atype][tok][1:]                                        # (5, 4, 2)
    cs, sn = np.cos(np.float32(head)), np.sin(np.float32(head))
    x = ct[..., 0] * cs - ct[..., 1] * sn + pos[0]
    y = ct[..., 0] * sn + ct[..., 1] * cs + pos[1]
    return np.stack([x.mean(1), y.mean(1)], -1), np.arctan2(y[:, 0] - y[:, 3], x[:, 0] - x[:, 3])


def _check_ego_follows_the_log(c, scene, out, rows, ego):
    """rows: the slice of the scene's rows in ``out``; ego: the ego's row inside it"""
    cfg, hc, H = c['cfg'], c['cfg'].hist_columns, c['cfg'].num_historical_steps
    ag = scene['agent']
    keep = np.asarray(ag['state_idx'])[:, hc - 1] != 0
    av = int(np.asarray(ag['av_index']).reshape(-1)[0])
    assert ego == int(keep[:av].sum())
    g = lambda k: out[k][rows].cpu().numpy()
    mask = g('replay_mask')
    assert mask.dtype == np.bool_ and mask.shape[0] == g('pos_a').shape[0] == int(keep.sum())
    assert mask[ego] and mask.sum() == 1
    tok, st = np.asarray(ag['token_idx'])[av], np.asarray(ag['state_idx'])[av]
    pos, head = np.asarray(ag['token_pos'])[av], np.asarray(ag['token_heading'])[av]
    assert np.array_equal(g('next_token_idx')[ego, hc:], tok[hc:]) and np.array_equal(g('next_state_idx')[ego, hc:], st[hc:])
    assert np.array_equal(g('pos_a')[ego, hc:], pos[hc:]) and np.array_equal(g('head_a')[ego, hc:], head[hc:])
    vocab = np.stack([c['vocab'][k] for k in ('veh', 'ped', 'cyc')])
    atype = int(np.asarray(ag['type'])[av])
    pt, ph = g('pred_traj')[ego], g('pred_head')[ego]
    for t in range(cfg.num_decode_steps):
        # the logged token of column hc + t, integrated from the logged pose of the column before it
        xy, th = _integrated(vocab, atype, max(int(tok[hc + t]), 0), pos[hc + t - 1], head[hc + t - 1])
        assert np.abs(pt[H + 5 * t:H + 5 * t + 5] - xy).max() <= 1e-3 and np.abs(ph[H + 5 * t:H + 5 * t + 5] - th).max() <= 1e-4, t   # (the tree's pose bars)


def test_module_entry_replays_the_ego():
    from infgen_amd.modules.infgen_decoder import batch_datas
    from test_batch_inference_gpu import _dec, _ragged3
    from test_modules_gpu import _to_data
    dev = torch.device('cuda:0')
    c = _case('a24_m256_edge')
    dec = _dec(c)
    # one graph (a row is filtered before the ego: batch_size_a shrinks as without replay)
    d0, d1 = _to_data(c['scene'], dev), _to_data(c['scene'], dev)
    free = dec.inference(d0)
    out = dec.inference(d1, replay='ego')
    assert 'replay_mask' not in free and torch.equal(d0['batch_size_a'], d1['batch_size_a'])
    _check_ego_follows_the_log(c, c['scene'], out, slice(None), int(out['ego_index']))
    assert not torch.equal(out['next_token_idx'], free['next_token_idx'])
    # the same through an explicit mask tensor and through a plan that repeats the log
    ag = d1['agent']
    m = torch.zeros(ag['state_idx'].shape[0], dtype=torch.bool, device=dev)
    m[int(ag['av_index'].reshape(-1)[0])] = True
    again = dec.inference(_to_data(c['scene'], dev), replay=m,
                          replay_plan={k: ag[k] for k in ('token_idx', 'state_idx', 'token_pos', 'token_heading')})
    for k in ('next_token_idx', 'next_state_idx', 'pos_a', 'pred_traj', 'replay_mask'):
        assert torch.equal(again[k], out[k]), k
    with pytest.raises(ValueError):
        dec.inference(_to_data(c['scene'], dev), replay=m[:-1])
    with pytest.raises(ValueError):
        dec.inference(_to_data(c['scene'], dev), replay=m, replay_plan={'state_idx': ag['state_idx']})
    # a 3-graph Batch (one graph with a row filtered before its ego)
    scenes = _ragged3(c)
    b0, b1 = batch_datas([_to_data(sc, dev) for sc in scenes]), batch_datas([_to_data(sc, dev) for sc in scenes])
    dec.inference(b0)
    outb = dec.inference(b1, replay='ego')
    assert torch.equal(b0['batch_size_a'], b1['batch_size_a'])
    ptr = outb['agent_ptr'].tolist()
    for s, sc in enumerate(scenes):
        _check_ego_follows_the_log(c, sc, outb, slice(ptr[s], ptr[s + 1]), int(outb['ego_index'][s]) - ptr[s])
    # the per-scene list entry and n rollouts of one scene carry the key too
    lst = dec.inference_batch([_to_data(sc, dev) for sc in scenes], replay='ego')
    for s, r in enumerate(lst):
        assert torch.equal(r['replay_mask'], outb['replay_mask'][ptr[s]:ptr[s + 1]]), s
        assert torch.equal(r['next_token_idx'], outb['next_token_idx'][ptr[s]:ptr[s + 1]]), s
    two = dec.inference_rollouts(_to_data(c['scene'], dev), 2, replay='ego')
    assert len(two) == 2 and all(torch.equal(r['next_token_idx'], out['next_token_idx']) for r in two)
