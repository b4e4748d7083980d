"""Collision-aware decoding without a GPU: the float64 restatement against a brute-force polygon test, the band of the shared
operator-level cases, and the host-side refusals."""
import numpy as np
import pytest

import collision_ref as cr


def _pair(ca, ha, ea, cb, hb, eb):
    sep = float(cr.sat_sep(ca, ha, ea, cb, hb, eb))
    brute = cr.polygons_overlap_brute(cr.box_corners(ca, ha, ea), cr.box_corners(cb, hb, eb))
    return sep, brute


Q = np.pi / 4
PAIRS = {
    # name: (boxes, overlap?)
    'touching edge to edge': (([0, 0], 0.0, [2, 1], [4, 0], 0.0, [2, 1]), False),
    'just inside': (([0, 0], 0.0, [2, 1], [3.999, 0], 0.0, [2, 1]), True),
    'nested': (([0, 0], 0.3, [5, 4], [0.5, 0.2], 1.1, [1, 0.5]), True),
    'identical': (([1, 1], 0.2, [2, 1], [1, 1], 0.2, [2, 1]), True),
    'cross': (([0, 0], 0.0, [4, 0.5], [0, 0], np.pi / 2, [4, 0.5]), True),
    'rotated 45 corner in': (([0, 0], 0.0, [2, 2], [3.3, 0], Q, [1, 1]), True),
    'rotated 45 corner out': (([0, 0], 0.0, [2, 2], [3.5, 0], Q, [1, 1]), False),
    # disjoint on ONE axis only: the axes of the first box both see an overlap of the projections, an axis of the second separates
    'one axis only': (([0, 0], 0.0, [2, 2], [3.1, 3.1], -Q, [3, 0.5]), False),
    'one axis only, closer': (([0, 0], 0.0, [2, 2], [2.2, 2.2], -Q, [3, 0.5]), True),
}


@pytest.mark.parametrize('name', list(PAIRS))
def test_axis_test_agrees_with_brute_force_polygons(name):
    boxes, want = PAIRS[name]
    sep, brute = _pair(*boxes)
    assert brute == want, (name, 'the brute-force check itself')
    assert (sep < 0) == want, (name, sep)
    if name == 'touching edge to edge':
        assert sep == 0.0
    if name.startswith('one axis only') and not want:
        ca, ha, ea, cb, hb, eb = boxes
        d = np.asarray(cb, float) - np.asarray(ca, float)
        r_b = eb[0] * abs(np.cos(hb)) + eb[1] * abs(np.sin(hb))     # the second box's reach along the first's x axis (= y axis at 45 deg)
        assert abs(d[0]) < ea[0] + r_b and abs(d[1]) < ea[1] + r_b, 'both axes of the first box see overlapping projections'


def test_axis_test_agrees_with_brute_force_on_random_pairs():
    rng = np.random.default_rng(5)
    n_over = 0
    for _ in range(300):
        a = (rng.uniform(-3, 3, 2), rng.uniform(-np.pi, np.pi), rng.uniform(0.4, 3, 2))
        b = (rng.uniform(-3, 3, 2), rng.uniform(-np.pi, np.pi), rng.uniform(0.4, 3, 2))
        sep, brute = _pair(*a, *b)
        if abs(sep) > 1e-9:
            assert (sep < 0) == brute, (a, b, sep)
        n_over += brute
    assert 30 < n_over < 270


@pytest.fixture(scope='module')
def vocabs():
    from infgen_amd import synth
    full = synth.make_agent_vocab(2048)
    return {2048: full, 64: cr.thin_vocab(full, 64)}


@pytest.mark.parametrize('name', list(cr.CASES))
def test_shared_cases_meet_the_band_and_exercise_every_branch(name, vocabs):
    """the seeds: at most 0.1 % of a case's (live row, token) pairs lie inside the 1e-4 m band, no row's fallback decision hangs on a
    pair inside it, the boxed-in row falls back, rows absent at c - 1 and at c exist, some row keeps a proper subset"""
    case = cr.make_case(name, vocabs[cr.CASES[name]['token_size']])
    ref = cr.case_reference(case)
    A, K = case['A'], case['token_size']
    live = ref['live']
    in_band = (ref['min_abs_sep'] <= cr.BAND) & live[:, None]
    assert in_band.sum() <= 1e-3 * live.sum() * K, (int(in_band.sum()), int(live.sum()) * K)
    # emptiness never depends on the band: a row is empty whatever its band pairs do, or keeps a token outside the band
    sure = ref['pre'] & ~in_band
    maybe_empty = (sure.sum(axis=1) == 0) & ((ref['pre'] | (in_band & ref['base'])).sum(axis=1) > 0)
    assert not maybe_empty.any()
    boxed = cr.BOXED_SCENE * A + cr.BOXED_ROW
    assert live[boxed] and ref['count'][boxed] == 0 and np.array_equal(ref['allowed'][boxed], ref['base'][boxed])
    assert not live[2 * A:3 * A].any() and live[A] and not live[A + 1:2 * A].any()
    if case.get('dense'):
        assert live[:A].all() and cr.reachable(case).max() > cr.LIST, 'some row\'s list overflows: a further pass over the tokens'
    else:
        assert not live[2]
    assert np.array_equal(ref['allowed'][A], ref['base'][A]), 'a scene of one agent has no obstacle'
    proper = live & (ref['count'] > 0) & (ref['count'] < ref['base'].sum(axis=1))
    assert proper.sum() >= 1, 'some rows lose tokens without falling back'
    if case['predict']:
        other = cr.reference(case['pos'], case['head'], case['state'], case['n_agents'], case['atype'], case['shape'], case['vocab'],
                             case['c'], 0, case['margin'], case['base_rows'])
        assert not np.array_equal(other['pre'], ref['pre']), 'the extrapolation changes a set'


def test_larger_margin_never_allows_more(vocabs):
    case = cr.make_case('k64_a33_p0_m0_base', vocabs[64])
    a = cr.case_reference(case)
    b = cr.case_reference(dict(case, margin=0.5))
    assert not (b['pre'] & ~a['pre']).any() and (a['pre'] & ~b['pre']).any()


# ------------------------------------------------------------------------------------------ host-side refusals, no launch
@pytest.mark.parametrize('bad', [dict(margin=-0.1), dict(margin=float('nan')), dict(margin=float('inf')), dict(margin='1'),
                                 dict(predict=2), dict(predict=-1), dict(predict='yes'), dict(speed=1.0), 3, 'on'])
def test_bad_configurations_are_refused_on_the_host(bad):
    from infgen_amd import constraints
    with pytest.raises(ValueError, match='avoid_collisions'):
        constraints.check_avoid_collisions(bad)


def test_no_shapes_is_refused_and_good_values_pass():
    from infgen_amd import constraints
    with pytest.raises(ValueError, match='shape'):
        constraints.check_avoid_collisions(True, has_shape=False)
    assert constraints.check_avoid_collisions(False, has_shape=False) is None
    assert constraints.check_avoid_collisions(None) is None
    assert constraints.check_avoid_collisions(True) == dict(margin=0.0, predict=1)
    assert constraints.check_avoid_collisions(dict(margin=0.5, predict=False)) == dict(margin=0.5, predict=0)


def test_off_builds_no_buffers_and_on_builds_static_ones():
    from infgen_amd import constraints
    assert constraints.collision_buffers(constraints.check_avoid_collisions(False), 64, 2048) is None
    b = constraints.collision_buffers(constraints.check_avoid_collisions(True), 64, 2048)
    assert tuple(b['bits'].shape) == (64, 64) and tuple(b['allowed'].shape) == (64,) and tuple(b['shape'].shape) == (64, 3)
    assert b['ident'].tolist() == list(range(64)) and int(b['bits'].view(-1)[0]) == -1
    with pytest.raises(ValueError, match='token_size'):
        constraints.collision_buffers(dict(margin=0.0, predict=1), 64, 48)


def test_library_refuses_bad_arguments_before_any_launch():
    """the C entries check margin / predict / shapes / sizes first: no device memory is touched, so this runs without a GPU"""
    from infgen_amd import _lib
    lib = _lib.load()
    ok = dict(pos=16, head=16, state=16, n_agents=16, first_new=None, type=16, shape=16, S=1, A_cap=8, T=4, c=1, end_pose=16,
              token_size=64, predict=1, margin=0.0, mask_bits=None, mask_n_sets=0, mask_row=None, mask_type=None, out_bits=16,
              out_count=None, stream=None)

    def call(**kw):
        return lib.infgen_collision_mask(*dict(ok, **kw).values())
    for kw, text in ((dict(margin=-1.0), 'margin'), (dict(margin=float('nan')), 'margin'), (dict(predict=2), 'predict'),
                     (dict(shape=None), 'shape'), (dict(A_cap=4096), 'A_cap'),
                     (dict(token_size=48), 'token_size'), (dict(out_bits=8), 'aligned'), (dict(c=4), 'column')):
        assert call(**kw) != 0, kw
        assert text in lib.infgen_last_error().decode(), (kw, lib.infgen_last_error())
    h = lib.infgen_token_mask_create(None, 0, None, None, None)
    assert h >= 1
    try:
        assert lib.infgen_token_mask_collision(h, 16, 16, 16, 16, 1, -0.5, None) != 0 and b'margin' in lib.infgen_last_error()
        assert lib.infgen_token_mask_collision(h, 16, 16, 16, 16, 3, 0.0, None) != 0 and b'predict' in lib.infgen_last_error()
        assert lib.infgen_token_mask_collision(h, 16, 16, None, 16, 1, 0.0, None) != 0 and b'shape' in lib.infgen_last_error()
        assert lib.infgen_token_mask_collision(h, 16, 16, 16, 16, 1, 0.5, None) == 0
        assert lib.infgen_token_mask_collision(h, None, None, None, None, 1, 0.0, None) == 0      # detach
        assert lib.infgen_token_mask_collision(h + 1000, 16, 16, 16, 16, 1, 0.0, None) != 0
    finally:
        assert lib.infgen_token_mask_destroy(h) == 0


def test_decoder_attribute_reaches_the_engine_arguments_and_key():
    import types
    from infgen_amd.modules.infgen_decoder import InfGenDecoder
    dec = types.SimpleNamespace(sample_temperature=1.0, sample_top_p=1.0, insert_temperature=1.0, insert_top_p=1.0,
                                token_constraints=None, avoid_collisions=False)
    off = InfGenDecoder._sampling_kw(dec, 1, 1)
    dec.avoid_collisions = dict(margin=0.25)
    on = InfGenDecoder._sampling_kw(dec, 1, 1)
    assert 'avoid_collisions' not in off[0] and on[0]['avoid_collisions'] == dict(margin=0.25, predict=1) and on[2] != off[2]
    dec.avoid_collisions = dict(margin=-1)
    with pytest.raises(ValueError, match='margin'):
        InfGenDecoder._sampling_kw(dec, 1, 1)
