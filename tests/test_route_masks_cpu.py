"""Route-following decoding without a GPU: the two restatements of tests/route_ref.py against each other on the inputs
the GPU tests use, the host-side helpers and the argument checks of the Python and C entries."""
import ctypes as C

import numpy as np
import pytest

import route_ref as rr

NEAR_CAP = 0.005         # of the tokens in ruled rows: a condition the cases are chosen to meet, not a measurement


@pytest.mark.parametrize('with_base', [False, True], ids=['all', 'base'])
@pytest.mark.parametrize('name', list(rr.CASES))
def test_float32_and_float64_agree_outside_near_tokens_and_few_tokens_are_near(name, with_base):
    K = rr.CASES[name]['token_size']
    for pace in rr.PACES:
        r32, r64 = rr.case_reference(name, with_base, pace, False), rr.case_reference(name, with_base, pace, True)
        ruled, near = r64['ruled'], r64['near']
        assert np.array_equal(ruled, r32['ruled']) and np.array_equal(r32['progress'][:, 3], r64['progress'][:, 3])
        assert not r64['row_open'].any(), 'no row-level decision (finished, gmax > 0) is within the band'
        assert not ((r32['pre'] != r64['pre']) & ~near).any()
        assert not near[~ruled].any() and near.sum() <= NEAR_CAP * ruled.sum() * K, (pace, int(near.sum()), int(ruled.sum()) * K)
        assert ((r64['count'] > 0) & (r64['count'] < r64['base'].sum(axis=1)))[ruled].any(), 'the rule bans tokens'
        tol = 8 * 2.0 ** -23 * (r64['scale'] + r64['progress'][:, 2])
        assert (np.abs(r32['progress'][:, :3] - r64['progress'][:, :3]).max(axis=1) <= tol).all()


def test_the_cases_hold_what_they_are_meant_to():
    case = rr.make_case('k2048_a32_p32', True)
    n, routes = case['n_points'], case['routes']
    assert n[0, 1] == 0 and n[0, 2] == 1 and n[1, 2] == 5 and np.isnan(routes[0, 4]).any()
    rec, total = rr.records(routes, n, np.float64)
    assert total[0, 1] == 0 and total[0, 2] == 0
    dead = rec[0, 3, :, 4] < 0
    assert dead[16 - 1] and not dead[0] and not dead[-1], 'a dead segment in the middle'
    assert (rec[0, 4, -2:, 4] < 0).all() and rec[0, 4, 0, 4] > 0, 'the NaN waypoint kills the two segments that touch it'
    assert rec[0, 3, 16, 5] == rec[0, 3, 14, 5] + rec[0, 3, 14, 4], 'cum does not advance over a dead segment'
    r = rr.case_reference('k2048_a32_p32', True, 0.0, True)
    pr = r['progress'].reshape(4, 32, 4)
    assert abs(pr[2, 0, 1] - 3 * rr.CORRIDOR) < 0.5 and r['ruled'].reshape(4, 32)[2, 0], 'the row 3 corridors off its route'
    assert r['pre'].reshape(4, 32, -1)[2, 0].any() or r['count'].reshape(4, 32)[2, 0] == 0
    assert (pr[2:, 1, 3] == 2).all(), 'the row past total - finish'
    assert (pr[2:, 3, 3] == 0).all() and (case['atype'][2:, 3] == 1).all(), 'the type switched off'
    assert (pr[1, 20:, 3] == 0).all() and pr[0, 7, 3] == 0, 'padding rows and the row that is not in the scene'
    assert (r['count'] == 0).any(), 'the static base empties some row: the fallback'
    # the U-turn: a token that ends beside the far leg is nearer to it, but lies far ahead along the route - it is on-route
    # (back only bans what lies behind), and the row's own s0 is on the near leg
    assert pr[2, 2, 0] < 20.0


def test_routes_from_logged_on_a_hand_written_case():
    from infgen_amd import constraints
    pos = np.zeros((1, 3, 6, 2), np.float32)
    pos[0, 0, :, 0] = [0, 1, 1, 2, 3, 4]                   # a repeated point
    pos[0, 1, :, 1] = [5, 5, 5, 5, 5, 5]                   # a parked agent: one point, no route
    pos[0, 2, :, 0] = [0, 2, 4, 6, 8, 10]
    st = np.ones((1, 3, 6), np.int64)
    st[0, 0, 3] = 0                                        # invalid at column 3: left out
    routes, n = constraints.routes_from_logged(dict(token_pos=pos, state_idx=st), points=4)
    assert routes.shape == (1, 3, 4, 2) and routes.dtype == np.float32 and n.tolist() == [[4, 1, 4]]
    assert routes[0, 0, :, 0].tolist() == [0, 1, 3, 4] and routes[0, 2, :, 0].tolist() == [0, 2, 4, 6], 'truncated to `points`'
    routes, n = constraints.routes_from_logged(dict(token_pos=pos, state_idx=st), stride=2, start=1)
    assert n.tolist() == [[2, 1, 3]] and routes[0, 2, :3, 0].tolist() == [2, 6, 10] and routes[0, 0, :2, 0].tolist() == [1, 4]
    scene = dict(agent=dict(token_pos=pos[0], state_idx=st[0]))
    again, m = constraints.routes_from_logged([scene, scene], stride=2, start=1)
    assert again.shape[0] == 2 and np.array_equal(again[1], routes[0]) and np.array_equal(m[0], n[0])
    with pytest.raises(ValueError):
        constraints.routes_from_logged(scene, stride=0)


def test_the_python_argument_checks_raise():
    from infgen_amd import constraints
    ok = dict(routes=np.zeros((2, 3, 4, 2), np.float32), n_points=np.zeros((2, 3), np.int32))
    conf = constraints.check_follow_routes(ok, n_scenes=2, a_cap=32)
    assert (conf['corridor'], conf['back'], conf['pace'], conf['finish'], conf['types']) == (2.0, 0.5, 0.0, 1.0, (1, 0, 1))
    assert constraints.check_follow_routes(False) is None and constraints.check_follow_routes(None) is None
    assert constraints.route_key(None) is None and constraints.route_key(conf) == (2.0, 0.5, 0.0, 1.0, (1, 0, 1))
    nan = float('nan')
    for bad in (True, dict(ok, corridor=-1), dict(ok, corridor=nan), dict(ok, back=-1), dict(ok, finish=float('inf')), dict(ok, pace=1.5),
                dict(ok, pace=-0.1), dict(ok, pace=nan), dict(ok, types='veh'), dict(ok, types=(3,)), dict(ok, margin=1.0),
                dict(routes=ok['routes']), dict(ok, routes=np.zeros((2, 3, 1, 2))), dict(ok, routes=np.zeros((2, 3, 33, 2))),
                dict(ok, routes=np.zeros((2, 3, 4, 3))), dict(ok, n_points=np.zeros((2, 4), np.int32)),
                dict(ok, n_points=np.full((2, 3), 5)), dict(ok, n_points=np.full((2, 3), -1)), dict(ok, n_points=np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            constraints.check_follow_routes(bad, n_scenes=2, a_cap=32)
    with pytest.raises(ValueError):
        constraints.check_follow_routes(ok, n_scenes=3, a_cap=32)
    with pytest.raises(ValueError):
        constraints.check_follow_routes(ok, n_scenes=2, a_cap=2)
    with pytest.raises(ValueError):
        constraints.route_buffers(1, 32, 32, 4, 48)


def test_the_c_entries_refuse_on_the_host_and_attach_to_handles_only():
    """the checks that come before any launch, on a machine without a device: NULL tables, the ranges of the scalars, alignment, and
    the handle lookup of the attach entry (a handle without a route configuration is what every engine without follow_routes has:
    attaching nothing to it succeeds and changes nothing)"""
    from infgen_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p += (-p) % 16
    types = (C.c_int * 3)(1, 0, 1)
    h = lib.infgen_token_mask_create(None, 0, None, None, None)
    assert h >= 1
    good = dict(bits=p, ident=p, shape=p, end=p, rec=p, total=p, P=4, copies=1, corridor=2.0, back=0.5, pace=0.0, finish=1.0, types=types,
                count=None, progress=None)
    assert lib.infgen_token_mask_route(h, *good.values()) == 0
    for over, word in ((dict(corridor=-1.0), 'corridor'), (dict(back=float('nan')), 'back'), (dict(finish=-2.0), 'finish'),
                       (dict(pace=1.01), 'pace'), (dict(P=1), 'P must be'), (dict(P=33), 'P must be'), (dict(copies=0), 'copies'),
                       (dict(shape=None), 'shape'), (dict(end=None), 'end-pose'), (dict(rec=None), 'record'), (dict(total=None), 'record'),
                       (dict(types=None), 'type switch'), (dict(ident=None), 'identity'), (dict(rec=p + 4), 'aligned'),
                       (dict(progress=p + 8), 'aligned')):
        assert lib.infgen_token_mask_route(h, *dict(good, **over).values()) != 0, over
        assert word in lib.infgen_last_error().decode() and 'route mask' in lib.infgen_last_error().decode(), over
    assert lib.infgen_token_mask_route(h, None, *list(good.values())[1:]) == 0, 'NULL bits detach'
    for bad_handle in (0, -3, h + 100):
        assert lib.infgen_token_mask_route(bad_handle, *good.values()) != 0
    assert lib.infgen_token_mask_destroy(h) == 0
    assert lib.infgen_token_mask_route(h, *good.values()) != 0, 'a destroyed handle'
    assert lib.infgen_route_records(None, p, 1, 1, 4, p, p, None) != 0 and lib.infgen_route_records(p, p, 1, 1, 40, p, p, None) != 0
    assert lib.infgen_route_records(p, p, 1, 1, 4, p + 4, p, None) != 0 and lib.infgen_route_records(p, p, 1, 2000, 4, p, p, None) != 0
    assert lib.infgen_route_mask(p, p, p, p, None, p, p, 1, 1, 4, 1, p, 64, p, p, 4, 1, 2.0, 0.5, 2.0, 1.0, types, None, 0, None, None, p, None,
                                 None, None) != 0 and 'pace' in lib.infgen_last_error().decode()


class _Mask(C.Structure):
    _fields_ = [('bits', C.c_void_p), ('n_sets', C.c_int), ('mask_row', C.c_void_p), ('mask_type', C.c_int * 3), ('type', C.c_void_p)]


class _Coll(C.Structure):
    _fields_ = [('bits', C.c_void_p), ('ident', C.c_void_p), ('shape', C.c_void_p), ('end_pose', C.c_void_p), ('predict', C.c_int),
                ('margin', C.c_float), ('count', C.c_void_p)]


class _Road(C.Structure):
    _fields_ = [('bits', C.c_void_p), ('ident', C.c_void_p), ('shape', C.c_void_p), ('end_pose', C.c_void_p), ('paths', C.c_void_p),
                ('records', C.c_void_p), ('n_records', C.c_void_p), ('rec_cap', C.c_int), ('copies', C.c_int), ('sweep', C.c_int),
                ('margin', C.c_float), ('types', C.c_int * 3), ('count', C.c_void_p)]


class _Score(C.Structure):
    _fields_ = [('out', C.c_void_p), ('steps', C.c_int), ('row', C.c_void_p), ('shape', C.c_void_p), ('records', C.c_void_p),
                ('n_records', C.c_void_p), ('rec_cap', C.c_int), ('copies', C.c_int), ('sweep', C.c_int), ('margin', C.c_float),
                ('types', C.c_int * 3), ('dt', C.c_float)]


class _Route(C.Structure):
    _fields_ = [('bits', C.c_void_p), ('ident', C.c_void_p), ('shape', C.c_void_p), ('end_pose', C.c_void_p), ('records', C.c_void_p),
                ('total', C.c_void_p), ('P', C.c_int), ('copies', C.c_int), ('corridor', C.c_float), ('back', C.c_float),
                ('pace', C.c_float), ('finish', C.c_float), ('types', C.c_int * 3), ('count', C.c_void_p), ('progress', C.c_void_p)]


class _ParentRiders(C.Structure):      # the step-rider block as it was before the route rider
    _fields_ = [('mask', _Mask), ('coll', _Coll), ('road', _Road), ('score', _Score)]


class _Riders(C.Structure):
    _fields_ = _ParentRiders._fields_ + [('route', _Route)]


def test_without_routes_the_rider_block_is_the_parents_bytes():
    """the library's own step-rider block of a handle (infgen_token_mask_riders), byte for byte: without a route configuration its
    front is what the block was before the route rider - no handle, a bare handle, a handle with collision, road and scores
    attached - and the rest is the empty route configuration; attaching routes changes those last bytes only"""
    from infgen_amd import _lib
    lib = _lib.load()
    arena = (C.c_float * 256)()
    p = C.addressof(arena)
    p += (-p) % 32
    types = (C.c_int * 3)(1, 0, 1)
    size = C.sizeof(_Riders)

    def block(h):
        buf = (C.c_ubyte * size)()
        assert lib.infgen_token_mask_riders(h, None, 2048, buf, size) == size, lib.infgen_last_error()
        return bytes(buf)

    def expect(**parts):
        e = _Riders()
        e.mask.mask_type[:] = [-1, -1, -1]
        e.coll.predict = 1
        e.road.copies = e.road.sweep = e.score.copies = e.score.sweep = e.route.copies = 1
        e.score.dt, e.route.P = 0.5, 2
        for name, vals in parts.items():
            for k, v in vals.items():
                setattr(getattr(e, name), k, v)
        return bytes(e)

    front = C.sizeof(_ParentRiders)
    assert _Riders.route.offset == front, 'the route configuration follows the four of before'
    none = expect()
    assert block(0) == none
    small = (C.c_ubyte * 8)()
    assert lib.infgen_token_mask_riders(0, None, 2048, small, 8) < 0
    h = lib.infgen_token_mask_create(None, 0, None, None, None)
    try:
        assert block(h) == none
        assert lib.infgen_token_mask_collision(h, p, p + 16, p + 32, p + 48, 0, 0.25, p + 64) == 0
        assert lib.infgen_token_mask_road(h, p + 80, p + 96, p + 112, p + 128, p + 144, p + 160, p + 176, 7, 1, 0, 0.5, types, p + 192) == 0
        assert lib.infgen_token_mask_score(h, p + 224, 10, p + 256, p + 288, p + 320, p + 352, 7, 1, 1, 0.1, types, 0.5) == 0
        f3 = lambda v: (C.c_int * 3)(*v)
        rest = dict(coll=dict(bits=p, ident=p + 16, shape=p + 32, end_pose=p + 48, predict=0, margin=0.25, count=p + 64),
                    road=dict(bits=p + 80, ident=p + 96, shape=p + 112, end_pose=p + 128, paths=p + 144, records=p + 160, n_records=p + 176,
                              rec_cap=7, copies=1, sweep=0, margin=0.5, types=f3((1, 0, 1)), count=p + 192),
                    score=dict(out=p + 224, steps=10, row=p + 256, shape=p + 288, records=p + 320, n_records=p + 352, rec_cap=7, copies=1,
                               sweep=1, margin=0.1, types=f3((1, 0, 1)), dt=0.5))
        without = block(h)
        assert without == expect(**rest)
        assert without[front:] == none[front:], 'no route configuration: the empty one'
        assert lib.infgen_token_mask_route(h, p + 384, p + 400, p + 416, p + 432, p + 448, p + 480, 8, 2, 2.0, 0.5, 0.25, 1.0, types, p + 496,
                                           p + 512) == 0
        routed = block(h)
        assert routed[:front] == without[:front], 'attaching routes leaves the four configurations of before alone'
        assert routed == expect(route=dict(bits=p + 384, ident=p + 400, shape=p + 416, end_pose=p + 432, records=p + 448, total=p + 480, P=8,
                                           copies=2, corridor=2.0, back=0.5, pace=0.25, finish=1.0, types=f3((1, 0, 1)), count=p + 496,
                                           progress=p + 512), **rest)
        assert lib.infgen_token_mask_route(h, None, None, None, None, None, None, 2, 1, 0.0, 0.0, 0.0, 0.0, None, None, None) == 0
        assert block(h) == without, 'detached: the bytes of before'
    finally:
        assert lib.infgen_token_mask_destroy(h) == 0


def test_decoder_attribute_reaches_the_engine_arguments_and_key():
    import types
    from infgen_amd.modules.infgen_decoder import InfGenDecoder
    dec = types.SimpleNamespace(sample_temperature=1.0, sample_top_p=1.0, insert_temperature=1.0, insert_top_p=1.0,
                                token_constraints=None, avoid_collisions=False, follow_routes=False)
    off = InfGenDecoder._sampling_kw(dec, 2, 3)
    conf = dict(routes=np.zeros((2, 3, 4, 2), np.float32), n_points=np.zeros((2, 3), np.int32), pace=0.5)
    dec.follow_routes = conf
    ctor, live, key = InfGenDecoder._sampling_kw(dec, 2, 3)
    assert 'follow_routes' not in off[0] and ctor['follow_routes'] is conf and live['follow_routes'] is conf and key != off[2]
    dec.follow_routes = dict(conf, routes=np.zeros((2, 3, 5, 2), np.float32))
    assert InfGenDecoder._sampling_kw(dec, 2, 3)[2] != key, 'P is part of the engine key'
    dec.follow_routes = dict(conf, pace=2.0)
    with pytest.raises(ValueError, match='pace'):
        InfGenDecoder._sampling_kw(dec, 2, 3)
    with pytest.raises(ValueError, match='scenes'):
        dec.follow_routes = conf
        InfGenDecoder._sampling_kw(dec, 3, 1)


def test_the_u_turn_exercises_the_first_minimum():
    """on the U-turn route some token ends nearer to the far leg than to the leg the row drives on - its arc position jumps ahead by
    more than the turn - and some token's two nearest segments are the two legs"""
    case = rr.make_case('k2048_a32_p32', False)
    rec, total = rr.records(case['routes'], case['n_points'], np.float64)
    s, i, c = 2, 2, case['c']
    segs, _ = rr._frame(rec[1, i], case['pos'][s, c, i, 0], case['pos'][s, c, i, 1], case['head'][s, c, i], np.float64)
    assert len(segs) == 4
    centre = rr.end_centres(case['vocab'], np.float64)[int(case['atype'][s, i])]
    sk, best, idx, S_all, D_all = rr._project(centre[:, 0], centre[:, 1], segs, np.float64)
    s0 = rr._project(np.zeros(1), np.zeros(1), segs, np.float64)[0][0]
    assert (idx == 3).any() and (sk[idx == 3] - s0 > 20.0).all(), 'a token whose nearest segment is the far leg'
    order = np.argsort(D_all, axis=0)
    legs = ((order[0] == 0) & (order[1] == 3)) | ((order[0] == 3) & (order[1] == 0))
    assert legs.any(), 'a token whose two nearest segments are the two legs'
