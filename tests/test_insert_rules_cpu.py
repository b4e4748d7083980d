"""CPU: the insertion rules' restatement (tests/insert_rules_ref.py) on hand-computed cases, the decision under rules against
graph_ref.insert_decide_ref, the validation of infgen_amd.insertion_rules.InsertRules and of the C entries (which refuse before
any launch), and the bit-packing helpers."""
import ctypes as C
import math

import numpy as np
import pytest

import graph_ref as gr
import insert_rules_ref as ir
from infgen_amd import _lib, insertion_rules as rules_mod, synth

SMALL = synth.build_grid(30, 3, 15)
FULL = synth.build_grid()


def one_scene(rows, grid=SMALL, ego_head=math.pi / 2, ego=(0.0, 0.0)):
    """a block of one scene at column 1: row 0 the ego at ``ego`` heading ``ego_head`` (pi / 2: the ego frame is the world's, up
    to the translation), then ``rows`` = [(x, y, heading, length, width, state)]"""
    A_cap = 8
    st = gr.new_state(1, A_cap, 2, 4, G=grid.shape[0])
    st['grid_xy'] = np.asarray(grid, np.float32)
    shape = np.full((A_cap, 3), 0.1, np.float32)
    st['n_agents'][0] = 1 + len(rows)
    st['pos'][0, 1, 0], st['head'][0, 1, 0], st['state'][0, 1, 0] = ego, ego_head, 1
    shape[0] = (0.0, 0.0, 1.0)
    for j, (x, y, h, L, W, state) in enumerate(rows, 1):
        st['pos'][0, 1, j], st['head'][0, 1, j], st['state'][0, 1, j] = (x, y), h, state
        shape[j] = (L, W, 1.5)
    return st, shape


def cells(grid, ok):
    return {(float(x), float(y)) for x, y in np.asarray(grid)[np.asarray(ok)]}


def disc(grid, pred):
    return {(float(x), float(y)) for x, y in np.asarray(grid) if pred(float(x), float(y))}


def test_grids_are_exact_multiples_of_the_interval():
    for g in (SMALL, FULL):
        assert np.array_equal(g, np.round(g / 3.0) * 3.0) and g.dtype == np.float32
    assert FULL.shape[0] == 1961 and SMALL.shape[0] < 128


@pytest.mark.parametrize('f', [np.float32, np.float64])
def test_ego_keepout_by_hand(f):
    st, shape = one_scene([])
    v = ir.cell_verdicts(st, shape, ir.new_rules(keepout=(6.0, 12.0, 3.0)), 0, 1, f)
    assert cells(SMALL, ~v['allowed']) == disc(SMALL, lambda x, y: -6 <= y <= 12 and abs(x) <= 3)
    assert len(cells(SMALL, ~v['allowed'])) == 3 * 7 and v['live'] == 1 and np.isinf(v['margin']).all()
    # the ego turned by a quarter turn to the left (heading pi): the grid's +y is the world's -x, nothing else changes in the ego frame
    st, shape = one_scene([], ego_head=math.pi, ego=(500.0, -20.0))
    v2 = ir.cell_verdicts(st, shape, ir.new_rules(keepout=(6.0, 12.0, 3.0)), 0, 1, f)
    assert np.array_equal(v2['allowed'], v['allowed'])


@pytest.mark.parametrize('f', [np.float32, np.float64])
def test_clearance_by_hand(f):
    # a 4 x 2 box at (9, 0) along +x, clearance 2.5: the lattice points within 2.5 m of the rectangle [7, 11] x [-1, 1]
    rows = [(9.0, 0.0, 0.0, 4.0, 2.0, 1), (-9.0, -9.0, 0.0, 4.0, 2.0, 0)]          # the second row left the scene: no obstacle
    st, shape = one_scene(rows)
    shape[0] = (0.0, 0.0, 1.0)                                                    # the ego is a point here: its own ban is the disc
    v = ir.cell_verdicts(st, shape, ir.new_rules(clearance=2.5), 0, 1, f)
    want = disc(SMALL, lambda x, y: math.hypot(max(abs(x - 9) - 2, 0), max(abs(y) - 1, 0)) < 2.5 or math.hypot(x, y) < 2.5)
    assert cells(SMALL, ~v['allowed']) == want == {(6.0, 0.0), (9.0, 0.0), (12.0, 0.0), (9.0, 3.0), (9.0, -3.0), (12.0, 3.0), (6.0, 3.0),
                                                   (12.0, -3.0), (6.0, -3.0), (0.0, 0.0)}
    assert v['live'] == 2 and v['static'].all()
    # the same box turned by 90 degrees: [8, 10] x [-2, 2]
    st['head'][0, 1, 1] = np.float32(math.pi / 2)
    v = ir.cell_verdicts(st, shape, ir.new_rules(clearance=2.5), 0, 1, f)
    assert cells(SMALL, ~v['allowed']) == disc(SMALL, lambda x, y: math.hypot(max(abs(x - 9) - 1, 0), max(abs(y) - 2, 0)) < 2.5
                                               or math.hypot(x, y) < 2.5)
    # clearance 0 bans nothing, not even a cell inside a box
    assert ir.cell_verdicts(st, shape, ir.new_rules(clearance=0.0), 0, 1, f)['allowed'].all()


@pytest.mark.parametrize('f', [np.float32, np.float64])
def test_edge_clearance_by_hand(f):
    rec = ir.segment_records([(-3.0, 6.0, 3.0, 6.0), (0.0, -9.0, 0.0, -9.0)])[None]          # the second: zero length, radius -1
    assert rec[0, 1, 7] == -1 and tuple(rec[0, 0]) == (-3.0, 6.0, 3.0, 0.0, 1.0, 0.0, 3.0, 3.0)
    st, shape = one_scene([])
    r = ir.new_rules(edge_clearance=1.0, records=rec, n_records=np.array([2], np.int32))
    v = ir.cell_verdicts(st, shape, r, 0, 1, f)
    assert cells(SMALL, ~v['allowed']) == {(-3.0, 6.0), (0.0, 6.0), (3.0, 6.0)}
    r = ir.new_rules(edge_clearance=3.5, records=rec, n_records=np.array([2], np.int32))
    v = ir.cell_verdicts(st, shape, r, 0, 1, f)
    assert cells(SMALL, ~v['allowed']) == disc(SMALL, lambda x, y: math.hypot(max(abs(x) - 3, 0), y - 6) < 3.5)
    r['n_records'] = np.array([0], np.int32)
    assert ir.cell_verdicts(st, shape, r, 0, 1, f)['allowed'].all()


@pytest.mark.parametrize('f', [np.float32, np.float64])
def test_near_lane_by_hand(f):
    st, shape = one_scene([])
    mp = np.array([[[0.0, 0.0], [9.0, 9.0], [-9.0, 0.0], [0.0, -9.0]]], np.float32)
    mt = np.array([[1, 12, 2, 1]], np.int64)                # the EDGE token is no lane; the fourth token is beyond n_map
    r = ir.new_rules(near_lane=(4.0, (1, 2)), map_pos=mp, map_type=mt, n_map=np.array([3], np.int32))
    v = ir.cell_verdicts(st, shape, r, 0, 1, f)
    near = lambda x, y, cx, cy: math.hypot(x - cx, y - cy) <= 4.0
    assert cells(SMALL, v['allowed']) == disc(SMALL, lambda x, y: near(x, y, 0, 0) or near(x, y, -9, 0))
    assert len(cells(SMALL, v['allowed'])) == 10
    r['n_map'] = np.array([0], np.int32)                    # no lane token at all: nothing is allowed
    assert not ir.cell_verdicts(st, shape, r, 0, 1, f)['allowed'].any()


@pytest.mark.parametrize('f', [np.float32, np.float64])
def test_zones_by_hand(f):
    st, shape = one_scene([], ego=(100.0, 50.0))
    inside = lambda x, y, cx, cy, rr: math.hypot(x - cx, y - cy) <= rr
    z = np.array([[[106.0, 50.0, 4.0, 0], [100.0, 59.0, -1.0, 0], [100.0, 41.0, np.inf, 1]]], np.float32)
    r = ir.new_rules(zones=z, n_zones=np.array([3], np.int32))
    v = ir.cell_verdicts(st, shape, r, 0, 1, f)             # one ban zone; a void ban zone and a void allow zone change nothing
    assert cells(SMALL, ~v['allowed']) == disc(SMALL, lambda x, y: inside(x, y, 6, 0, 4)) == {(6.0, 0.0), (3.0, 0.0), (9.0, 0.0), (6.0, 3.0),
                                                                                             (6.0, -3.0)}
    z[0, 2] = (100.0, 44.0, 7.0, 1)                         # now a live allow zone: only its inside is left, minus the ban zone
    z[0, 1] = (109.0, 50.0, 3.5, 1)
    v = ir.cell_verdicts(st, shape, ir.new_rules(zones=z, n_zones=np.array([3], np.int32)), 0, 1, f)
    assert cells(SMALL, v['allowed']) == disc(SMALL, lambda x, y: (inside(x, y, 0, -6, 7) or inside(x, y, 9, 0, 3.5))
                                              and not inside(x, y, 6, 0, 4))
    v = ir.cell_verdicts(st, shape, ir.new_rules(zones=z, n_zones=np.array([1], np.int32)), 0, 1, f)
    assert cells(SMALL, ~v['allowed']) == disc(SMALL, lambda x, y: inside(x, y, 6, 0, 4))      # beyond n_zones: not read


def test_static_and_dynamic_parts_and_copies():
    st, shape, rules, c = ir.gen_case(SMALL)
    by = {n: i for i, n in enumerate(ir.SCENES)}
    for s in range(st['S']):
        v = ir.cell_verdicts(st, shape, rules, s, c)
        no_clear = dict(rules, clearance=None)
        assert np.array_equal(ir.cell_verdicts(st, shape, no_clear, s, c)['allowed'], v['static'])
        assert not (v['allowed'] & ~v['static']).any()
    assert not ir.cell_verdicts(st, shape, rules, by['all_banned'], c)['allowed'].any()
    assert ir.cell_verdicts(st, shape, rules, by['empty'], c)['live'] == 0
    assert ir.cell_verdicts(st, shape, rules, by['full'], c)['live'] == st['A_cap'] - 1       # (row 1 left the scene)
    # the appended row counts: without it more cells are allowed
    st, shape, rules, c = ir.gen_case(FULL)
    s = by['appended_row']
    only = ir.new_rules(clearance=rules['clearance'])
    with_row = ir.cell_verdicts(st, shape, only, s, c)['allowed']
    st2 = dict(st, state=st['state'].copy())
    st2['state'][s, c, 8] = 0
    without = ir.cell_verdicts(st2, shape, only, s, c)['allowed']
    assert (without & ~with_row).any() and not (with_row & ~without).any()


@pytest.mark.parametrize('grid', [FULL, SMALL], ids=['G1961', 'small'])
def test_generated_cases_keep_the_band_nearly_empty_and_float32_agrees_outside_it(grid):
    st, shape, rules, c = ir.gen_case(grid)
    for sub in SUBSETS:
        r = subset(rules, sub)
        for s in range(st['S']):
            v64, v32 = ir.cell_verdicts(st, shape, r, s, c), ir.cell_verdicts(st, shape, r, s, c, np.float32)
            band = v64['margin'] < ir.BAND
            assert band.mean() <= ir.BAND_SHARE, (sub, ir.SCENES[s], band.mean())
            assert np.array_equal(v64['allowed'][~band], v32['allowed'][~band]) and v64['live'] == v32['live']


SUBSETS = (('keepout',), ('clearance',), ('edge_clearance',), ('near_lane',), ('zones',),
           ('keepout', 'clearance', 'edge_clearance', 'near_lane', 'zones'))


def subset(rules, on):
    return dict(rules, **{k: None for k in ('keepout', 'clearance', 'edge_clearance', 'near_lane', 'zones') if k not in on})


# ------------------------------------------------------------------------------------------------ the decision under rules
@pytest.mark.parametrize('sample_k,topk_entry,t,force_enter', gr.INSERT_DECIDE_CASES)
def test_decision_with_nothing_ruled_is_the_plain_decision(sample_k, topk_entry, t, force_enter):
    G = FULL.shape[0]
    st, dec, names, max_new = gr.gen_insert_decide(G, FULL, sample_k, t, force_enter)
    a, ad = gr.as_ref(st), gr.as_ref(dec)
    b, bd = gr.as_ref(st), gr.as_ref(dec)
    for s in range(st['S']):
        gr.insert_decide_ref(a, ad, s, t, force_enter, max_new, sample_k=sample_k)
        ir.decide_mask_ref(b, bd, s, t, force_enter, max_new, sample_k, np.ones(G, bool), (1, 1, 1))
    for k, v in a.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, b[k], equal_nan=True), k
    for k, v in ad.items():
        assert np.array_equal(v, bd[k], equal_nan=True), k


def test_decision_under_rules_by_hand():
    G = FULL.shape[0]
    st, dec, names, max_new = gr.gen_insert_decide(G, FULL, 1, 2, 0)
    s = names.index('enter_above')
    order = gr.topk_pick(dec['lg_pos'][s], 3, 0.0)[2]
    dec['occ'][s] = 0
    allowed = np.ones(G, bool)
    allowed[order[0]] = False                                # the arg-max cell banned: the next best is taken
    b, bd = gr.as_ref(st), gr.as_ref(dec)
    ir.decide_mask_ref(b, bd, s, 2, 0, max_new, 1, allowed, (1, 1, 1))
    assert bd['inserted'][s] == 1 and bd['new_cell'][s] == order[1]
    b, bd = gr.as_ref(st), gr.as_ref(dec)                    # no allowed cell: the "no cell" exit, nothing touched
    ir.decide_mask_ref(b, bd, s, 2, 0, max_new, 1, np.zeros(G, bool), (1, 1, 1))
    assert (bd['inserted'][s], bd['active'][s]) == (0, 0) and b['n_agents'][s] == st['n_agents'][s]
    assert np.array_equal(b['state'], st['state'])
    dec['lg_type'][s] = (0.5, 3.0, 1.0)                      # the pedestrian logit is the largest, pedestrians are banned
    b, bd = gr.as_ref(st), gr.as_ref(dec)
    ir.decide_mask_ref(b, bd, s, 2, 0, max_new, 1, allowed, (1, 0, 1))
    assert b['type'][s, st['n_agents'][s]] == 2
    for live, want in ((7, 0), (6, 1)):                      # live == max_agents stops the scene, live == max_agents - 1 does not
        b, bd = gr.as_ref(st), gr.as_ref(dec)
        ir.decide_mask_ref(b, bd, s, 2, 1, max_new, 1, allowed, (1, 1, 1), max_agents=7, live=live)
        assert (bd['inserted'][s], bd['active'][s]) == (want, want)
    # fewer allowed cells than insert_k: the draw is over those alone, for every uniform
    few = np.zeros(G, bool)
    few[order[:2]] = True
    for u, want in ((0.0, order[0]), (np.float32(1.0) - np.float32(2.0 ** -24), order[1])):
        b, bd = gr.as_ref(st), gr.as_ref(dec)
        bd['uniform'][s] = u
        ir.decide_mask_ref(b, bd, s, 2, 0, max_new, 16, few, (1, 1, 1))
        assert bd['inserted'][s] == 1 and bd['new_cell'][s] == want


# ------------------------------------------------------------------------------------------------ validation
def test_insert_rules_from_config():
    R = rules_mod.InsertRules
    assert R.from_config(None) is None and R.from_config(False) is None
    r = R.from_config(dict(clearance=10, ego_keepout=(5, 40, 4), edge_clearance=1.5, near_lane=dict(dist=6.0, types=[15, 0, 1]),
                           types=('veh', 'cyc'), max_agents=48, per_step=3))
    assert (r.clearance, r.ego_keepout, r.edge_clearance, r.near_lane) == (10.0, (5.0, 40.0, 4.0), 1.5, (6.0, (0, 1, 15)))
    assert r.types == (1, 0, 1) and int(r.max_agents) == 48 and r.per_step == 3
    assert r.rule_bits == ir.KEEPOUT | ir.CLEARANCE | ir.EDGES | ir.LANES and r.lane_type_mask == (1 << 15) | 3
    assert R.from_config({}).rule_bits == 0 and R.from_config({}).types == (1, 1, 1) and R.from_config({}).per_step == 10
    z = R.from_config(dict(zones=np.array([[0, 0, 5, 0], [1, 1, -1, 1]], np.float32)), n_scenes=3).zones
    assert z[0].shape == (3, 2, 4) and z[1].tolist() == [2, 2, 2]


@pytest.mark.parametrize('conf,match', [
    (dict(clearance=-1.0), 'clearance'), (dict(clearance=float('nan')), 'clearance'), (dict(clearance=float('inf')), 'clearance'),
    (dict(edge_clearance=-0.5), 'edge_clearance'), (dict(edge_clearance='2'), 'edge_clearance'),
    (dict(ego_keepout=(1, 2)), 'ego_keepout'), (dict(ego_keepout=(1, -2, 3)), 'ego_keepout'),
    (dict(near_lane=5.0), 'near_lane'), (dict(near_lane=dict(dist=-1, types=[1])), 'near_lane dist'),
    (dict(near_lane=dict(dist=1, types=[])), 'near_lane types'), (dict(near_lane=dict(dist=1, types=[40])), 'near_lane types'),
    (dict(types=(0, 0, 0)), 'at least one'), (dict(types=()), 'types'), (dict(types=('car',)), 'unknown agent types'),
    (dict(per_step=0), 'per_step'), (dict(per_step=11), 'per_step'), (dict(per_step=2.5), 'per_step'),
    (dict(max_agents=-1), 'max_agents'), (dict(max_agents=[1, 2, 3]), 'max_agents'), (dict(max_agents=1.5), 'max_agents'),
    (dict(zones=np.zeros((2, 3, 4))), 'zones cover'), (dict(zones=np.zeros((4, 3))), 'zones must be'),
    (dict(zones=np.array([[0, 0, 1, 2]])), 'mode'), (dict(zones=np.array([[np.nan, 0, 1, 0]])), 'finite'),
    (dict(zones=(np.zeros((4, 3, 4)), np.array([1, 2, 3, 4]))), 'n_zones'),
    (dict(radius=3), 'unknown keys'), ([1, 2], 'insert_rules takes'),
])
def test_insert_rules_refusals(conf, match):
    with pytest.raises(ValueError, match=match):
        rules_mod.InsertRules.from_config(conf, n_scenes=4, n_slots=8)


def test_device_tables_on_the_host():
    r = rules_mod.InsertRules.from_config(dict(zones=np.zeros((2, 4), np.float32), max_agents=5), n_scenes=2, n_slots=4)
    t = rules_mod.device_tables(r, 4, 2, 32, 1961, 6)
    assert t['W'] == 64 and tuple(t['allowed'].shape) == (4, 64) and tuple(t['count_log'].shape) == (4, 6)
    assert t['max_agents'].tolist() == [5] * 4 and tuple(t['zones'].shape) == (2, 2, 4) and tuple(t['shape'].shape) == (128, 3)
    with pytest.raises(ValueError, match='cells'):
        rules_mod.device_tables(r, 4, 2, 32, 8193, 6)


def test_c_entries_refuse_before_any_launch():
    """every refusal of infgen_insert_cell_mask / infgen_insert_decide_mask comes with a message and launches nothing, so it is
    testable without a device (the pointers are never followed)"""
    lib = _lib.load()
    for sym in ('infgen_insert_cell_mask', 'infgen_insert_decide_mask', 'infgen_insert_seed_rules'):
        assert sym in _lib.SYMBOLS and hasattr(lib, sym)
    buf = (C.c_float * 64)()
    a = C.addressof(buf) // 16 * 16 + 16                                  # an aligned non-NULL stand-in
    ko = (C.c_float * 3)(1, 2, 3)
    G, W = 1961, 64

    def call(**kw):
        d = dict(S=4, A_cap=32, T=3, c=1, G=G, rules=0, keepout=None, clearance=0.0, edge=0.0, lane=0.0, records=None, map_pos=None,
                 zones=None, copies=1, static_pass=0, static_bits=None, allowed=a, words=W)
        d.update(kw)
        rc = lib.infgen_insert_cell_mask(a, a, a, a, a, a, d['S'], d['A_cap'], d['T'], d['c'], a, d['G'], d['rules'], d['keepout'],
                                         d['clearance'], d['edge'], d['lane'], 0, d['records'], d['records'], 8, d['map_pos'],
                                         d['map_pos'], d['map_pos'], 8, d['zones'], d['zones'], 2, d['copies'], d['static_pass'],
                                         d['static_bits'], d['allowed'], d['words'], a, a, None, 0, None)
        return rc, (lib.infgen_last_error() or b'').decode()
    for kw, msg in ((dict(rules=2, clearance=-1.0), 'finite and >= 0'), (dict(rules=4, edge=float('nan'), records=a), 'finite and >= 0'),
                    (dict(rules=8, lane=float('inf'), map_pos=a), 'finite and >= 0'), (dict(rules=1, keepout=(C.c_float * 3)(1, -2, 3)), 'finite'),
                    (dict(copies=0), 'copies'), (dict(copies=3), 'copies'), (dict(G=0), 'G must be'), (dict(G=9000, words=284), 'G must be'),
                    (dict(words=62), 'words'), (dict(c=3), 'column'), (dict(A_cap=2048), 'A_cap'), (dict(static_pass=3), 'static_pass'),
                    (dict(static_pass=1), 'static_bits'), (dict(rules=4), 'road-record'), (dict(rules=8), 'map_pos'),
                    (dict(rules=16), 'zone table'), (dict(rules=1), 'three floats'), (dict(rules=32), 'unknown rule'),
                    (dict(allowed=a + 4), '16-byte'), (dict(rules=16, zones=a + 8), '16-byte'), (dict(allowed=None), 'needs allowed')):
        rc, err = call(**kw)
        assert rc != 0 and msg in err, (kw, rc, err)
    r = _lib.Rollout()
    r.no_grid_token = 1
    ty = (C.c_int * 3)(1, 1, 1)
    args = (C.byref(r), 0, 0, 10, a, a, a, a, a, a, a, a, a, a, a, 1, None, None)
    assert lib.infgen_insert_decide_mask(*args, a, W, ty, None, None, None) != 0       # (an empty context, and no grid token)
    assert lib.infgen_last_error()


# ------------------------------------------------------------------------------------------------ bit packing
@pytest.mark.parametrize('grid', [FULL, SMALL], ids=['G1961', 'small'])
def test_bit_packing_round_trip(grid):
    G = grid.shape[0]
    W = rules_mod.words_for(G)
    assert W == ir.words_for(G) and W % 4 == 0 and 32 * W >= G > 32 * (W - 4)
    if G == 1961:
        assert W == 64 and G - 61 * 32 == 9                 # the tail word carries 9 valid bits, two padding words follow
    rng = np.random.default_rng(G)
    ok = rng.integers(0, 2, (3, G)).astype(bool)
    ok[0], ok[1] = True, False
    words = ir.pack_bits(ok)
    assert words.shape == (3, W) and words.dtype == np.uint32
    back, clean = ir.unpack_bits(words, G)
    assert clean and np.array_equal(back, ok)
    assert words[0, (G - 1) // 32] == (1 << ((G - 1) % 32 + 1)) - 1 and not words[0, (G - 1) // 32 + 1:].any()
    idx = rules_mod.cells_allowed_to_indices(words.view(np.int32), G)
    assert [i.tolist() for i in idx] == [np.nonzero(r)[0].tolist() for r in ok]
    assert np.array_equal(rules_mod.cells_allowed_to_indices(words[2], G), np.nonzero(ok[2])[0])
    assert np.array_equal(rules_mod.indices_to_cells_allowed(np.nonzero(ok[2])[0], G), words[2])
    dirty = words.copy()
    dirty[:, -1] |= np.uint32(1 << 31)                       # a bit beyond G is ignored by the reader and reported by unpack_bits
    assert not ir.unpack_bits(dirty, G)[1]
    assert np.array_equal(rules_mod.cells_allowed_to_indices(dirty[2], G), np.nonzero(ok[2])[0])
    with pytest.raises(ValueError):
        rules_mod.indices_to_cells_allowed([G], G)
