"""GPU: the insertion rules ("INSERTION RULES" of include/infgen_hip.h).  Operator level: infgen_insert_cell_mask on
the named scenes of insert_rules_ref.gen_case against the float64 restatement - every bit exact outside the 1e-4 m band, which
the generator keeps nearly empty -, and infgen_insert_decide_mask on graph_ref's branch table plus the masks' own cases.  Engine
level: RolloutEngine(insert_rules=...) on small synthetic scenes."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import graph_ref as gr
import insert_rules_ref as ir
from conftest import REPO
from gpu_blocks import SENT_I, dev, device_block, guard_intact, guarded, lib_and_check
from test_insert_rules_cpu import FULL, SMALL, SUBSETS, subset

pytestmark = pytest.mark.gpu

_CASES = {}


def case(name):
    """the generated case and its float64 verdicts per rule subset, computed once and shared"""
    if name not in _CASES:
        st, shape, rules, c = ir.gen_case(FULL if name == 'G1961' else SMALL)
        ref = {sub: [ir.cell_verdicts(st, shape, subset(rules, sub), s, c) for s in range(st['S'])] for sub in SUBSETS}
        _CASES[name] = (st, shape, rules, c, ref)
    return _CASES[name]


def launch_mask(st, shape, rules, c, static_pass=0, static_bits=None, count_log=None):
    """infgen_insert_cell_mask on device copies -> (allowed words [S][W], count [S], live [S], the device inputs and their host originals)"""
    lib, check = lib_and_check()
    S, A_cap, T, G = st['S'], st['A_cap'], st['T'], st['grid_xy'].shape[0]
    W = ir.words_for(G)
    host = dict(pos=st['pos'], head=st['head'], state=st['state'], n_agents=st['n_agents'], av_index=st['av_index'], shape=shape,
                grid_xy=st['grid_xy'])
    for k in ('records', 'n_records', 'map_pos', 'map_type', 'n_map', 'zones', 'n_zones'):
        if rules[k] is not None:
            host[k] = rules[k]
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev()) for k, v in host.items()}
    P = lambda k: d[k].data_ptr() if k in d else None
    allowed, count, live = guarded(S * W, torch.int32), guarded(S, torch.int32), guarded(S, torch.int32)
    ko = (C.c_float * 3)(*rules['keepout']) if rules['keepout'] is not None else None
    lane = rules['near_lane'] or (0.0, ())
    dim = lambda k, ax: int(rules[k].shape[ax]) if rules[k] is not None else 0
    check(lib.infgen_insert_cell_mask(
        P('pos'), P('head'), P('state'), P('n_agents'), P('av_index'), P('shape'), S, A_cap, T, c, P('grid_xy'), G, ir.rule_bits(rules),
        ko, rules['clearance'] or 0.0, rules['edge_clearance'] or 0.0, lane[0], ir.lane_type_mask(lane[1]),
        P('records') if rules['edge_clearance'] is not None else None, P('n_records') if rules['edge_clearance'] is not None else None,
        dim('records', 1), P('map_pos') if rules['near_lane'] is not None else None,
        P('map_type') if rules['near_lane'] is not None else None, P('n_map') if rules['near_lane'] is not None else None,
        dim('map_pos', 1), P('zones') if rules['zones'] is not None else None, P('n_zones') if rules['zones'] is not None else None,
        dim('zones', 1), rules['copies'], static_pass, None if static_bits is None else static_bits.data_ptr(), allowed.data_ptr(), W,
        count.data_ptr(), live.data_ptr(), None if count_log is None else count_log.data_ptr(), 3, None), 'infgen_insert_cell_mask')
    torch.cuda.synchronize()
    assert guard_intact(allowed, S * W) and guard_intact(count, S) and guard_intact(live, S)
    for k, v in host.items():
        assert np.array_equal(d[k].cpu().numpy(), np.ascontiguousarray(v), equal_nan=True), f'{k} was written'
    words = allowed[:S * W].cpu().numpy().view(np.uint32).reshape(S, W)
    return words, count[:S].cpu().numpy(), live[:S].cpu().numpy()


@pytest.mark.parametrize('sub', SUBSETS, ids=['+'.join(s) if len(s) == 1 else 'all' for s in SUBSETS])
@pytest.mark.parametrize('name', ['G1961', 'small'])
def test_cell_mask_against_float64(name, sub):
    """the named scenes (0 live agents; A = A_cap = 33; an ego that is not row 0; ego heading at pi; a scene 1e4 m away; every cell
    banned; only allow-zones; void zones and radius -1 records; a row appended earlier in the step; copies = 2), each rule alone
    and all together.  ego_keepout bits exact; the distance rules exact outside the band, and the band holds at most 0.5 % of the
    cells of every scene by the reference alone; counts consistent with the bits and the states; bits >= G zero; guards intact,
    inputs unchanged (launch_mask); a second run gives identical bits."""
    st, shape, rules, c, ref = case(name)
    r = subset(rules, sub)
    G = st['grid_xy'].shape[0]
    words, count, live = launch_mask(st, shape, r, c)
    bits, clean = ir.unpack_bits(words, G)
    assert clean, 'a bit at a position >= G is set'
    worst = 0
    for s, v in enumerate(ref[sub]):
        band = v['margin'] < ir.BAND
        assert band.mean() <= ir.BAND_SHARE, (ir.SCENES[s], band.mean())
        if sub == ('keepout',):
            assert not band.any()
        wrong = (bits[s] != v['allowed']) & ~band
        worst = max(worst, int(band.sum()))
        assert not wrong.any(), (ir.SCENES[s], np.nonzero(wrong)[0][:8], v['margin'][wrong][:8])
        assert count[s] == bits[s].sum() and live[s] == v['live'] == ir.in_scene(st, s, c).sum(), ir.SCENES[s]
    print(f'{name} {sub}: allowed per scene {count.tolist()}, at most {worst} cells in the band')
    by = {n: i for i, n in enumerate(ir.SCENES)}
    if 'zones' in sub:
        assert count[by['all_banned']] == 0 and count[by['all_banned_copy']] == 0
    assert live[by['empty']] == 0 and live[by['full']] == st['A_cap'] - 1
    again = launch_mask(st, shape, r, c)
    assert np.array_equal(again[0], words) and np.array_equal(again[1], count) and np.array_equal(again[2], live)


def test_cell_mask_static_pass_and_count_log():
    """pass 1 stores the static bits and pass 2 reads them: with the same rows the three passes agree bit for bit; with a row that
    an earlier iteration appended, pass 2 bans its surroundings on top of the stored static bits, as a pass-0 launch does"""
    st, shape, rules, c, ref = case('G1961')
    S, G = st['S'], FULL.shape[0]
    W = ir.words_for(G)
    w0, c0, l0 = launch_mask(st, shape, rules, c)
    static, log = guarded(S * W, torch.int32), guarded(S * 3, torch.int32)
    w1, c1, l1 = launch_mask(st, shape, rules, c, 1, static, log)
    assert guard_intact(static, S * W) and guard_intact(log, S * 3)
    sb, clean = ir.unpack_bits(static[:S * W].cpu().numpy().view(np.uint32).reshape(S, W), G)
    assert clean and np.array_equal(w1, w0) and np.array_equal(c1, c0)
    lg = log[:S * 3].cpu().numpy().reshape(S, 3)
    assert np.array_equal(lg[:, 0], c0) and (lg[:, 1:] == SENT_I).all()
    for s, v in enumerate(ref[SUBSETS[-1]]):
        band = v['margin'] < ir.BAND
        assert np.array_equal(sb[s][~band], v['static'][~band])
    w2, c2, l2 = launch_mask(st, shape, rules, c, 2, static)
    assert np.array_equal(w2, w0) and np.array_equal(c2, c0) and np.array_equal(l2, l0)
    # the appended row leaves: pass 2 on the same static bits allows more cells of that scene, exactly what a fresh pass 0 allows
    s = ir.SCENES.index('appended_row')
    st2 = dict(st, state=st['state'].copy())
    st2['state'][s, c, 8] = 0
    w3, c3, l3 = launch_mask(st2, shape, rules, c, 2, static)
    w4, c4, l4 = launch_mask(st2, shape, rules, c)
    assert np.array_equal(w3, w4) and c3[s] >= c0[s] and l3[s] == l0[s] - 1
    assert np.array_equal(np.delete(w3, s, 0), np.delete(w0, s, 0))


def test_cell_mask_torch_op():
    from infgen_amd import torch_ops  # noqa: F401
    st, shape, rules, c, ref = case('small')
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev())
    S, A_cap = st['S'], st['A_cap']
    bits, count, live = torch.ops.infgen_hip.insert_cell_mask(
        t(st['pos']), t(st['head']), t(st['state']), t(st['n_agents']), t(st['av_index']), t(shape.reshape(S, A_cap, 3)), c,
        t(st['grid_xy']), keepout=list(rules['keepout']), clearance=rules['clearance'], edge_clearance=rules['edge_clearance'],
        records=t(rules['records']), n_records=t(rules['n_records']), lane_dist=rules['near_lane'][0],
        lane_types=list(rules['near_lane'][1]), map_pos=t(rules['map_pos']), map_type=t(rules['map_type']), n_map=t(rules['n_map']),
        zones=t(rules['zones']), n_zones=t(rules['n_zones']), copies=rules['copies'])
    words, cnt, lv = launch_mask(st, shape, rules, c)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), words) and np.array_equal(count.cpu().numpy(), cnt)
    assert np.array_equal(live.cpu().numpy(), lv)


# ------------------------------------------------------------------------------------------------ the decision under rules
STATE_KEYS = ('pos', 'head', 'state', 'token', 'grid', 'tmask', 'imask', 'catflag', 'type', 'bos', 'n_agents', 'pred_traj',
              'pred_head', 'pred_state')
EXTRA = ('argmax_banned', 'few_allowed_u0', 'few_allowed_partial', 'few_allowed_u1', 'no_allowed', 'banned_type', 'budget_reached',
         'budget_left')


def masked_case(sample_k, t, force_enter):
    """graph_ref's branch table with every cell allowed, every type allowed and no budget, followed by the masks' own scenes
    (copies of the 'enter_above' scene) -> (block, decisions, names, max_new, allowed [S][G], type_allowed, max_agents [S], live [S])"""
    G = FULL.shape[0]
    st0, dec0, names0, max_new = gr.gen_insert_decide(G, FULL, sample_k, t, force_enter)
    src = names0.index('enter_above')
    pick = [*range(len(names0)), *[src] * len(EXTRA)]
    st = gr.take_scenes(st0, pick)
    st['pred_traj'], st['pred_head'], st['pred_state'] = (
        np.concatenate([st0[k].reshape(st0['S'], st0['A_cap'], *st0[k].shape[1:])[pick]]).reshape(-1, *st0[k].shape[1:])
        for k in ('pred_traj', 'pred_head', 'pred_state'))
    dec = {k: v[pick].copy() for k, v in dec0.items()}
    names = names0 + list(EXTRA)
    S = len(names)
    allowed = np.ones((S, G), bool)
    max_agents, live = np.full(S, 1 << 20, np.int32), np.full(S, 5, np.int32)
    k = max(sample_k, 1)
    for s, name in enumerate(names):
        if name not in EXTRA:
            continue
        dec['occ'][s] = 0
        order = gr.topk_pick(dec['lg_pos'][s], 16, 0.0)[2]
        if name == 'argmax_banned':
            allowed[s, order[:3]] = False
            if sample_k > 1:                                # keep the draw clear of a boundary of the re-ranked list
                cand = np.nonzero(allowed[s])[0]
                for _ in range(100):
                    if gr.topk_pick(dec['lg_pos'][s][cand], k, dec['uniform'][s])[1] > gr.CDF_MARGIN:
                        break
                    dec['uniform'][s] = np.float32(np.random.default_rng(s).uniform(0, 1))
        elif name.startswith('few_allowed'):
            allowed[s] = False
            allowed[s, order[[1, 4]]] = True                 # two cells, fewer than insert_k = 16
            dec['lg_pos'][s, order[[1, 4]]] = 7.0            # equal logits: probabilities exactly 1 / 2, the lower index first
            dec['uniform'][s] = dict(few_allowed_u0=0.0, few_allowed_partial=0.5, few_allowed_u1=np.float32(1.0) - np.float32(2.0 ** -24))[name]
        elif name == 'no_allowed':
            allowed[s] = False
        elif name == 'banned_type':
            dec['lg_type'][s] = (0.25, 3.0, 1.0)
        elif name == 'budget_reached':
            max_agents[s], live[s] = 9, 9
        elif name == 'budget_left':
            max_agents[s], live[s] = 9, 8
    type_allowed = (1, 0, 1)
    for s in range(len(names0)):                            # the branch table's scenes must not feel the type ban: no pedestrian arg-max
        if np.argmax(dec['lg_type'][s]) == 1 or names[s].startswith('type_tie'):
            dec['lg_type'][s, 1] = -5.0
    return st, dec, names, max_new, allowed, type_allowed, max_agents, live


@pytest.mark.parametrize('sample_k,topk_entry,t,force_enter', gr.INSERT_DECIDE_CASES)
def test_insert_decide_mask_branch_table(sample_k, topk_entry, t, force_enter):
    """test_insert_decide_branch_table's scenes through infgen_insert_decide_mask, plus: the arg-max cells banned (the next best is
    taken); two allowed cells under insert_k = 16 with uniforms 0, 1 / 2 (a partial sum exactly) and 1 - 2^-24; no allowed cell (the
    "no cell" exit, nothing touched); a banned type with the largest logit; live == max_agents and live == max_agents - 1.
    Everything exact, positions within graph_ref.BAR_INS_POS."""
    lib, check = lib_and_check()
    st, dec, names, max_new, allowed, type_allowed, max_agents, live = masked_case(sample_k, t, force_enter)
    S, G, A_cap, c = st['S'], FULL.shape[0], st['A_cap'], 1 + t
    rst, rdec = gr.as_ref(st), gr.as_ref(dec)
    for s in range(S):
        ir.decide_mask_ref(rst, rdec, s, t, force_enter, max_new, sample_k, allowed[s], type_allowed, int(max_agents[s]), int(live[s]))
    b, ten = device_block(st)
    d = {k: torch.from_numpy(v.copy()).to(dev()) for k, v in dec.items()}
    al = torch.from_numpy(ir.pack_bits(allowed).view(np.int32)).to(dev())
    ma, lv = torch.from_numpy(max_agents).to(dev()), torch.from_numpy(live).to(dev())
    P = lambda k: d[k].data_ptr()
    check(lib.infgen_insert_decide_mask(C.byref(b), t, force_enter, max_new, P('lg_state'), P('lg_type'), P('shape'), P('lg_pos'),
                                        P('occ'), P('active'), P('n_new'), P('inserted'), P('new_row'), P('new_shape'), P('new_cell'),
                                        sample_k, P('uniform'), None, al.data_ptr(), ir.words_for(G), (C.c_int * 3)(*type_allowed),
                                        ma.data_ptr(), lv.data_ptr(), None), 'infgen_insert_decide_mask')
    torch.cuda.synchronize()
    got, gdec = {k: v.cpu().numpy() for k, v in ten.items()}, {k: v.cpu().numpy() for k, v in d.items()}
    for k in ('inserted', 'active', 'n_new', 'new_row', 'new_cell', 'new_shape'):
        assert np.array_equal(gdec[k], rdec[k]), (k, dict(zip(names, zip(gdec[k].tolist(), np.asarray(rdec[k]).tolist()))))
    for s, name in enumerate(names):
        if name not in EXTRA:
            assert (gdec['inserted'][s], gdec['active'][s]) == gr.insert_decide_expect(name, sample_k, force_enter), name
    for k in ('lg_state', 'lg_type', 'shape', 'occ', 'uniform', 'lg_pos'):
        assert np.array_equal(gdec[k], dec[k], equal_nan=True), k
    ins = np.asarray(rdec['inserted']) == 1
    tol = np.zeros(st['pos'].shape[:3], bool)
    ptol = np.zeros(st['pred_traj'].shape[:2], bool)
    for s in np.nonzero(ins)[0]:
        tol[s, c, rdec['new_row'][s] - s * A_cap] = True
        if t > 0:
            ptol[rdec['new_row'][s], (t - 1) * 5:(t - 1) * 5 + 5] = True
    for k in STATE_KEYS:
        g64 = got[k].astype(np.float64)
        m = tol if k == 'pos' else ptol if k == 'pred_traj' else np.zeros(g64.shape, bool)
        assert np.array_equal(g64[~m], np.asarray(rst[k], np.float64)[~m]), k
        if m.any():
            assert np.abs(g64[m] - rst[k][m]).max() <= gr.BAR_INS_POS, k
    by = {n: i for i, n in enumerate(names)}
    order = gr.topk_pick(dec['lg_pos'][by['argmax_banned']], 16, 0.0)[2]
    if sample_k == 1:
        assert gdec['new_cell'][by['argmax_banned']] == order[3]
    s = by['no_allowed']
    assert (gdec['inserted'][s], gdec['active'][s]) == (0, 0) and got['n_agents'][s] == st['n_agents'][s]
    two = np.nonzero(allowed[by['few_allowed_u0']])[0]
    want = (two[0], two[1], two[1]) if sample_k > 1 else (two[0],) * 3
    assert tuple(gdec['new_cell'][by[n]] for n in ('few_allowed_u0', 'few_allowed_partial', 'few_allowed_u1')) == want
    s = by['banned_type']
    assert gdec['inserted'][s] == 1 and got['type'][s, st['n_agents'][s]] == 2
    assert (gdec['inserted'][by['budget_reached']], gdec['active'][by['budget_reached']]) == (0, 0)
    assert gdec['inserted'][by['budget_left']] == 1


# ------------------------------------------------------------------------------------------------ the engine
_ENGINE = {}
BUFFERS = ('pos', 'head', 'state', 'token', 'gridtok', 'atype', 'n_agents', 'pred_traj', 'pred_head', 'pred_state')


def engine_parts():
    """4 synthetic scenes of 8 agents and 64 map tokens, 6 decode steps, insertion on: weights and scenes built once"""
    if not _ENGINE:
        from infgen_amd import engine, synth
        with open(os.path.join(REPO, 'tests', 'golden', 'state_dict_shapes.json')) as f:
            shapes = {k: tuple(v) for k, v in json.load(f).items()}
        cfg = synth.smart_config(num_recurrent_steps_val=30, disable_insertion=False)
        sd = synth.fill_state_dict(shapes, seed=3, rich=True, head_gain=64.0)
        vocab, map_vocab = synth.make_agent_vocab(cfg.token_size), synth.make_map_vocab()
        grid = synth.build_grid(cfg.grid_range, cfg.grid_interval, cfg.pl2seed_radius)
        scenes = [synth.make_scene(synth.scene_seed(7, i), 8, 64, cfg, vocab=vocab, grid=grid) for i in range(4)]
        w = engine.PackedWeights(sd, cfg, dev())
        _ENGINE.update(cfg=cfg, w=w, scenes=scenes, vocab=vocab, map_vocab=map_vocab, grid=grid, runs={})
    return _ENGINE


def run_engine(key=None, **kw):
    """a rollout of a fresh engine -> (engine, host copies of its state buffers); ``key``: cache the result under this name"""
    from infgen_amd import engine
    E = engine_parts()
    if key is not None and key in E['runs']:
        return E['runs'][key]
    kw.setdefault('force_enter', True)
    kw.setdefault('insert_headroom', 64)
    eng = engine.RolloutEngine(E['w'], E['scenes'], E['vocab'], E['map_vocab'], E['grid'], **kw)
    eng.rollout()
    torch.cuda.synchronize()
    out = (eng, {k: getattr(eng, k).cpu().numpy().copy() for k in BUFFERS}, [list(r) for r in eng.ins['inserted_rows']])
    if key is not None:
        E['runs'][key] = out
    return out


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in BUFFERS)


def engine_rules_ref(eng, bufs, conf):
    """the rule set of an engine in the restatement's terms, tables read back from the device"""
    r, k = eng.insert_rules, eng._ins_rules
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return ir.new_rules(
        keepout=r.ego_keepout, clearance=r.clearance, edge_clearance=r.edge_clearance, records=cpu(k.get('records')),
        n_records=cpu(k.get('n_records')), near_lane=r.near_lane, map_pos=cpu(eng.map_pos).reshape(eng.S0, eng.M_cap, 2),
        map_type=cpu(eng._map_cat[1]).reshape(eng.S0, eng.M_cap), n_map=cpu(eng.n_map), zones=cpu(k['zones']), n_zones=cpu(k['n_zones']),
        copies=eng.copies)


def check_inserted_cells(eng, bufs, rows, rules):
    """every appended row sat in a cell the restatement allows for the scene as it was at that step and iteration: the rows in
    front of it at the step's column (those appended earlier in the step at their final pose)"""
    S, A_cap, T = eng.S, eng.A_cap, eng.T
    st = dict(S=S, A_cap=A_cap, T=T, pos=bufs['pos'].reshape(S, T, A_cap, 2), head=bufs['head'].reshape(S, T, A_cap),
              state=bufs['state'].reshape(S, T, A_cap), av_index=eng.av.cpu().numpy(), grid_xy=eng.grid_xy.cpu().numpy().reshape(-1, 2))
    shape = eng._ins_rules['shape'].cpu().numpy()
    grid = bufs['gridtok'].reshape(S, T, A_cap)
    n = 0
    for s in range(S):
        for row, t in rows[s]:
            a, c = row - s * A_cap, 1 + t
            na = np.zeros(S, np.int32)
            na[s] = a
            v = ir.cell_verdicts(dict(st, n_agents=na), shape, rules, s, c)
            cell = grid[s, c, a]
            assert v['allowed'][cell] or v['margin'][cell] < ir.BAND, (s, row, t, cell)
            n += 1
    return n


def test_engine_without_rules_and_with_rules_that_ban_nothing():
    """insert_rules=None is the engine of today; a rule set that bans nothing (clearance 0, all types, no budget) runs the cell
    mask and the masked decision and gives bitwise the same buffers and the same appended rows"""
    _, plain, rows = run_engine('plain')
    _, none, rows_n = run_engine(insert_rules=None)
    eng, zero, rows_z = run_engine(insert_rules=dict(clearance=0.0, types=('veh', 'ped', 'cyc')))
    assert sum(map(len, rows)) >= 8, 'the fixture must insert'
    assert same(plain, none) and rows == rows_n
    assert same(plain, zero) and rows == rows_z
    G = eng.G
    cnt = eng.insert_allowed_count.cpu().numpy()
    assert (cnt[:, 0] == 0).all() and (cnt[:, 1:] == G).all()      # (no insertion at decode step 0)
    assert tuple(eng.insert_allowed.shape) == (eng.S, ir.words_for(G))


def test_engine_rules_hold_for_every_inserted_row():
    from infgen_amd import insertion_rules as rules_mod
    E = engine_parts()
    conf = dict(clearance=7.5004, ego_keepout=(5.0, 30.0, 4.0), edge_clearance=1.2503, types=('veh', 'cyc'), max_agents=14, per_step=3,
                zones=np.array([[0.0, 0.0, 1e4, 1], [0.0, 0.0, -1.0, 0]], np.float32))
    eng, bufs, rows = run_engine('ruled', insert_rules=conf)
    _, plain, rows_p = run_engine('plain')
    assert not same(plain, bufs)
    rules = engine_rules_ref(eng, bufs, conf)
    n = check_inserted_cells(eng, bufs, rows, rules)
    assert n >= 4, 'the fixture must insert under the rules'
    S, A_cap, T = eng.S, eng.A_cap, eng.T
    state = bufs['state'].reshape(S, T, A_cap)
    for s in range(S):
        per_step = {}
        for row, t in rows[s]:
            a = row - s * A_cap
            assert bufs['atype'].reshape(S, A_cap)[s, a] in (0, 2)
            per_step[t] = per_step.get(t, 0) + 1
            live = int((state[s, 1 + t, :a] != 0).sum())           # rows in the scene when this one was appended
            assert live < 14, (s, row, t, live)
        assert all(v <= 3 for v in per_step.values())
    cnt = eng.insert_allowed_count.cpu().numpy()
    assert (cnt[:, 1:] < eng.G).all() and (cnt[:, 1:] > 0).any()
    idx = rules_mod.cells_allowed_to_indices(eng.insert_allowed, eng.G)
    assert len(idx) == S and all((i < eng.G).all() for i in idx)


def test_engine_keepout_over_the_whole_disc_appends_nothing():
    eng, bufs, rows = run_engine(insert_rules=dict(ego_keepout=(80.0, 80.0, 80.0)))
    assert sum(map(len, rows)) == 0 and (bufs['n_agents'] == 8).all()
    assert (eng.insert_allowed_count.cpu().numpy() == 0).all()


def test_engine_sampled_cells_under_rules():
    E = engine_parts()
    iu = np.random.default_rng(5).random((E['cfg'].num_decode_steps, 10, 4)).astype(np.float32)
    conf = dict(clearance=7.5004, ego_keepout=(5.0, 30.0, 4.0))
    eng, bufs, rows = run_engine(insert_rules=conf, insert_k=5, insert_uniforms=iu)
    assert check_inserted_cells(eng, bufs, rows, engine_rules_ref(eng, bufs, conf)) >= 4
    _, zero, rows_z = run_engine(insert_rules=dict(clearance=0.0), insert_k=5, insert_uniforms=iu)
    _, plain, rows_p = run_engine(insert_k=5, insert_uniforms=iu)
    assert same(plain, zero) and rows_p == rows_z


def test_engine_set_insert_zones_changes_the_next_rollout_only():
    everywhere = np.array([[0.0, 0.0, 1e4, 1]], np.float32)
    eng, first, rows1 = run_engine(insert_rules=dict(zones=everywhere))
    _, plain, rows_p = run_engine('plain')
    assert same(first, plain) and rows1 == rows_p              # an allow zone over everything bans nothing
    eng.set_insert_zones(np.array([[0.0, 0.0, 1e4, 0]], np.float32))
    eng.rollout()
    torch.cuda.synchronize()
    assert sum(map(len, eng.ins['inserted_rows'])) == 0 and (eng.n_agents.cpu().numpy() == 8).all()
    eng.set_insert_zones(everywhere)
    eng.rollout()
    torch.cuda.synchronize()
    assert same({k: getattr(eng, k).cpu().numpy() for k in BUFFERS}, plain)
    with pytest.raises(ValueError):
        eng.set_insert_zones(np.zeros((3, 4), np.float32))      # another capacity


def test_engine_refusals():
    from infgen_amd import engine, synth
    E = engine_parts()
    build = lambda cfg, w, **kw: engine.RolloutEngine(w, E['scenes'], E['vocab'], E['map_vocab'], E['grid'], **kw)
    off = synth.smart_config(num_recurrent_steps_val=30, disable_insertion=True)
    with pytest.raises(ValueError, match='disable_insertion'):
        build(off, engine.PackedWeights(E['w'].sd, off, dev()), insert_rules=dict(clearance=1.0))
    with pytest.raises(ValueError, match='at least one'):
        build(E['cfg'], E['w'], insert_rules=dict(types=(0, 0, 0)))
    with pytest.raises(ValueError, match='per_step'):
        build(E['cfg'], E['w'], insert_rules=dict(per_step=11))
    from test_ablation_gpu import _load
    c = _load('abl_grid_ins_forced_a16_m256')
    cfg = c['cfg']
    assert not cfg.use_grid_token and not cfg.disable_insertion
    w = engine.PackedWeights(c['sd'], cfg, dev())
    with pytest.raises(ValueError, match='use_grid_token'):
        engine.RolloutEngine(w, [c['scene']], c['vocab'], c['map_vocab'], c['grid'], insert_rules=dict(clearance=1.0))
