"""CPU: the IDM commands - anchors of the numpy restatement tests/idm_ref.py worked out by hand, the conditions the
shared operator cases must meet (so that the GPU test cannot pass on cases that exercise nothing), the platoon scenario on the
restatement alone, and the parameter and ABI checks."""
import numpy as np
import pytest

import idm_ref as ir
import route_ref as rr


def _solo(lateral=0.0, at=30.0, speed=0.0, length=100.0, **over):
    """one controlled vehicle on a straight route along +x that starts at route_ref.ORIGIN"""
    pts = np.stack([rr.ORIGIN, rr.ORIGIN + [length, 0.0]]).astype(np.float32)
    pos = np.zeros((1, 2, 1, 2), np.float32)
    pos[0, 1, 0] = rr.ORIGIN + [at, lateral]
    pos[0, 0, 0] = rr.ORIGIN + [at - speed * 0.5, lateral]
    case = dict(S=1, A=1, P=2, copies=1, T=2, c=1, pos=pos, head=np.zeros((1, 2, 1), np.float32), state=np.ones((1, 2, 1), np.int32),
                n_agents=np.array([1], np.int32), atype=np.zeros((1, 1), np.int32), ctl=np.ones((1, 1), np.uint8),
                shape=np.array([[[4.0, 2.0, 1.5]]], np.float32), routes=pts[None, None], n_points=np.array([[2]], np.int32))
    case.update(over)
    return case


# ------------------------------------------------------------------------------------------ anchors, by hand
def test_law_anchors():
    par = ir.params()
    assert ir.law(0.0, 0.0, np.inf, 15.0, False, par)[0] == par['a_max']                   # free road, standing: full acceleration
    assert ir.law(15.0, 0.0, np.inf, 15.0, False, par)[0] == 0.0                           # at the desired speed: none
    assert ir.law(0.0, 0.0, par['s_min'], 15.0, True, par)[0] == 0.0                       # standing s_min behind a standing lead
    assert ir.law(15.0, 0.0, 1.0, 15.0, True, par)[0] == -par['b_max']                     # the clamp
    acc, v1, adv, q, r = ir.law(10.0, 10.0, 17.0, 15.0, True, par)                         # sstar = 2 + 15 = 17 = gap: q = 1
    assert q == 1.0 and acc == pytest.approx(1.5 * (1 - (10 / 15) ** 4 - 1.0)) and v1 == 10.0 + acc * 0.5
    assert adv == pytest.approx(0.5 * (10.0 + v1) * 0.5)


def test_route_end_is_a_standing_candidate():
    case = _solo(at=30.0, speed=4.0)
    on, off = ir.reference(case, ir.params(), np.float64), ir.reference(case, ir.params(stop_at_end=0), np.float64)
    assert on['lead'][0] == -2 and on['state'][0, 3] == pytest.approx(100.0 - 30.0 - 2.0, abs=1e-3)
    assert off['lead'][0] == -1 and off['state'][0, 3] == np.inf and off['state'][0, 4] == pytest.approx(1.5 * (1 - (4 / 15) ** 4), abs=1e-6)
    assert on['state'][0, 2] == pytest.approx(4.0, abs=1e-3) and on['state'][0, 7] == 1
    # the end wins only if it is strictly nearer than the best agent: a standing agent 10 m ahead leads
    two = _solo(at=30.0, speed=4.0)
    two.update(A=2, pos=np.concatenate([two['pos'], two['pos'] + np.float32([10.0, 0.0])], 2), head=np.zeros((1, 2, 2), np.float32),
               state=np.ones((1, 2, 2), np.int32), n_agents=np.array([2], np.int32), atype=np.zeros((1, 2), np.int32),
               ctl=np.array([[1, 0]], np.uint8), shape=np.tile(two['shape'], (1, 2, 1)), routes=np.tile(two['routes'], (1, 2, 1, 1)),
               n_points=np.array([[2, 2]], np.int32))
    r = ir.reference(two, ir.params(), np.float64)
    assert r['lead'][0] == 1 and r['state'][0, 3] == pytest.approx(10.0 - 4.0, abs=1e-3)
    assert r['state'][0, 2] == pytest.approx(4.0, abs=1e-3)                                 # vl = 4: the agent moved with the row
    assert not r['ruled'][1] and r['lead'][1] == -1 and not r['state'][1].any() and np.isnan(r['pose'][1]).all()


def test_target_lies_on_the_polyline_or_keeps_the_offset():
    for keep, want in ((0.0, 0.0), (1.0, 0.7), (0.5, 0.35)):
        r = ir.reference(_solo(lateral=0.7, speed=6.0), ir.params(keep=keep), np.float64)
        x, y, h = r['pose'][0]
        assert r['state'][0, 1] == pytest.approx(0.7, abs=1e-3)                             # e0: left of the route is positive
        assert y - rr.ORIGIN[1] == pytest.approx(want, abs=1e-3) and h == 0.0
        assert x - rr.ORIGIN[0] == pytest.approx(r['state'][0, 6], abs=1e-3) and r['state'][0, 6] > 30.0


def test_stand_still_fill_and_feed():
    case = ir.platoon_case()
    r = ir.reference(case, ir.params(), np.float64)
    assert list(r['ruled']) == [False, True, True, True] and np.isnan(r['pose'][0]).all()
    nxt = ir.platoon_feed(case, r['pose'], r['ruled'])
    c = case['c']
    assert np.array_equal(nxt['pos'][0, c, 0], case['pos'][0, c, 0]) and np.array_equal(nxt['pos'][0, c - 1], case['pos'][0, c])
    assert np.allclose(nxt['pos'][0, c, 1:], r['pose'][1:, :2], atol=1e-3)


# ------------------------------------------------------------------------------------------ the conditions on the shared cases
@pytest.mark.parametrize('name', list(ir.CASES))
def test_cases_exercise_every_kind_of_row(name):
    case = ir.make_case(name)
    S, A, c = case['S'], case['A'], case['c']
    leads = set()
    for variant in ir.VARIANTS:
        r32, r64 = ir.case_reference(name, variant, False), ir.case_reference(name, variant, True)
        ruled, lead = r64['ruled'], r64['lead']
        assert np.array_equal(ruled, r32['ruled'])
        leads |= set(np.minimum(lead[ruled], 0).tolist())
        assert (lead[ruled] >= 0).any() and (lead[ruled] == (-2 if ir.VARIANTS[variant][0] else -1)).any(), variant
        out = r64['near'] | r64['ill']                     # what the GPU test may leave out of a comparison: under one cap
        assert out.sum() <= 0.1 * ruled.sum(), (variant, int(out.sum()), int(ruled.sum()))
        assert not out[~ruled].any() and not (r64['ambiguous'] & ~r64['near']).any()
        # unruled rows of each kind
        types = ir.VARIANTS[variant][2]
        ctl, live = case['ctl'].reshape(-1) != 0, (case['state'][:, c] != 0).reshape(-1)
        inside = (np.arange(A)[None] < case['n_agents'][:, None]).reshape(-1)
        routed = np.repeat(rr.records(case['routes'], case['n_points'])[1], case['copies'], axis=0).reshape(-1) > 0
        on = np.array(types)[np.clip(case['atype'], 0, 2)].reshape(-1) != 0
        for what, kind in (('not controlled', ~ctl & inside & live & routed & on), ('not live', ctl & inside & ~live & routed & on),
                           ('type off', ctl & inside & live & routed & ~on), ('no route', ctl & inside & live & ~routed & on),
                           ('padding', ~inside)):
            assert kind.any() and not ruled[kind].any(), (variant, what)
        assert np.array_equal(ruled, ctl & inside & live & routed & on)
    assert leads == {0, -1, -2}                                                            # lead >= 0, -1 and -2 over the variants
    # the placements: leaders that stand, that are not live at c - 1, that are faster than their follower
    r = ir.case_reference(name, 'stop', True)
    led = r['lead'][r['ruled'] & (r['lead'] >= 0)]
    rows = np.flatnonzero(r['ruled'] & (r['lead'] >= 0))
    scene = rows // A
    assert (case['state'][scene, c - 1, led] == 0).any(), 'a lead that is not live at c - 1'
    if A > 5:
        moved = np.abs(case['pos'][scene, c, led] - case['pos'][scene, c - 1, led]).sum(-1)
        assert (moved[case['state'][scene, c - 1, led] != 0] > 1.0).any() and (moved == 0).any(), 'a moving and a standing lead'
    if name == 'a70_p32':
        assert (r['lead'] >= 64).any(), 'a lead found in the second trip of the 64-lane walk'
        assert (rr.records(case['routes'], case['n_points'])[0][..., 4] < 0).any() and set(case['n_points'].reshape(-1)) >= {0, 1}


# ------------------------------------------------------------------------------------------ the platoon scenario
def _platoon(dt):
    case, par, log = ir.platoon_case(), ir.params(), []
    for _ in range(ir.PLATOON['steps']):
        r = ir.reference(case, par, dt)
        log.append(r['state'][1:, :4].astype(np.float64))
        case = ir.platoon_feed(case, r['pose'], r['ruled'])
    return np.array(log), case


def check_platoon(log):
    """the properties of the scenario on a log [steps][3 rows][s0, e0, v, gap]; the GPU test asks the same of the device's run"""
    gap, v = log[..., 3], log[..., 2]
    assert gap.min() >= 0.0, gap.min()
    assert (np.diff(v[25:], axis=0) <= 1e-6).all() and (v[-1] <= 0.05).all(), v[-1]
    assert ((gap[-1] >= 1.9) & (gap[-1] <= 2.1)).all(), gap[-1]


def test_platoon_comes_to_rest_behind_the_standing_row():
    """three rows at 8 m/s, 20 m apart, behind a row standing at 140 m of a 150 m route; 40 steps of 0.5 s, every target fed back as
    the next pose.  Bands: the final gaps in [1.9, 2.1] m (s_min = 2 m), the final speeds <= 0.05 m/s, the speeds never rise after
    step 25.  The float64 trajectory itself: least gap ever 1.9584 m (the final gap of the first follower), final gaps 1.9584,
    1.9722, 1.9757 m, final speeds 0, 0, 0.0022 m/s, largest speeds 9.30, 9.03, 8.86 m/s."""
    for dt in (np.float64, np.float32):
        log, case = _platoon(dt)
        check_platoon(log)
    assert np.array_equal(case['pos'][0, 1, 0], ir.platoon_case()['pos'][0, 1, 0])          # the standing row never moved
    assert log[0, :, 2] == pytest.approx(8.0, abs=1e-2) and log[:, :, 2].max() < 9.5


# ------------------------------------------------------------------------------------------ parameters and the ABI
def test_check_idm_defaults_and_refusals():
    from infgen_amd import constraints, controllers
    d = controllers.check_idm()
    assert d == dict(dt=constraints.STEP_SECONDS, v0=(15.0, 1.5, 6.0), headway=1.5, s_min=2.0, a_max=1.5, b_comf=2.0, b_max=6.0,
                     lateral=0.5, keep=0.5, types=(1, 0, 1), stop_at_end=1)
    assert {k: d[k] for k in ir.DEFAULTS} == {k: (float(v) if np.isscalar(v) and k != 'stop_at_end' else v) for k, v in ir.DEFAULTS.items()}
    assert controllers.check_idm(dict(types=('ped',), stop_at_end=False, keep=1, v0=[1, 2, 3])) == dict(d, types=(0, 1, 0), stop_at_end=0,
                                                                                                       keep=1.0, v0=(1.0, 2.0, 3.0))
    assert controllers.check_idm(dict(types=(1, 1, 0)))['types'] == (1, 1, 0)
    nan, inf = float('nan'), float('inf')
    bad = [dict(dt=0), dict(dt=-1), dict(dt=nan), dict(dt=inf), dict(a_max=0), dict(b_comf=0), dict(b_max=-1), dict(b_max=inf),
           dict(v0=(15, 0, 6)), dict(v0=(15, 1)), dict(v0=(15, nan, 6)), dict(v0=5.0), dict(headway=-0.1), dict(s_min=-1), dict(s_min=nan),
           dict(lateral=-0.5), dict(lateral=inf), dict(keep=-0.1), dict(keep=1.1), dict(keep=nan), dict(types=('car',)), dict(types='veh'),
           dict(types=(1, 0)), dict(stop_at_end='yes'), dict(stop_at_end=2), dict(speed=3), dict(dt='0.5'), dict(a_max=True)]
    for p in bad:
        with pytest.raises(ValueError, match='idm'):
            controllers.check_idm(p)
    with pytest.raises(ValueError, match='idm'):
        controllers.check_idm([1, 2])


def test_binding_has_the_entry():
    import ctypes as C
    from infgen_amd import _lib
    assert 'infgen_idm_command' in _lib.SYMBOLS
    res, args = _lib.SYMBOLS['infgen_idm_command']
    p, i, f = C.c_void_p, C.c_int, C.c_float
    assert res is i and args == [p] * 7 + [i] * 4 + [p, p, i, i, p, f, p] + [f] * 7 + [p, i, p, p, p, p]
    assert hasattr(_lib.load(), 'infgen_idm_command')
