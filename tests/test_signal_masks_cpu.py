"""Signal-aware decoding without a GPU: the two restatements of tests/signal_ref.py against each other on the inputs the
GPU tests use, the host-side helpers and the argument checks of the Python and C entries."""
import ctypes as C

import numpy as np
import pytest

import signal_ref as sr

NEAR_CAP = 0.02          # of the (row, token) pairs of a case: a condition the cases are chosen to meet, not a measurement


@pytest.mark.parametrize('with_base', [False, True], ids=['all', 'base'])
@pytest.mark.parametrize('name', list(sr.CASES))
def test_float32_and_float64_agree_outside_near_tokens_and_few_tokens_are_near(name, with_base):
    K = sr.CASES[name]['token_size']
    rows = sr.S_CASE * sr.A_CASE
    for t in sr.STEPS:
        r32, r64 = sr.case_reference(name, with_base, t, False), sr.case_reference(name, with_base, t, True)
        ruled, near = r64['ruled'], r64['near']
        assert np.array_equal(ruled, r32['ruled']) and np.array_equal(r64['governed'], r32['governed'])
        assert not r64['row_open'].any() and not r64['info_open'].any(), 'no row-level decision is within the band'
        assert not ((r32['pre'] != r64['pre']) & ~near).any()
        assert not near[~ruled].any() and near.sum() <= NEAR_CAP * rows * K, (t, int(near.sum()), rows * K)
        assert np.array_equal(r32['info'][:, 1:], r64['info'][:, 1:]), 'line and flag'
        tol = 8 * 2.0 ** -23 * r64['scale']
        assert (np.abs(r32['info'][:, 0] - r64['info'][:, 0]) <= tol).all()


@pytest.mark.parametrize('name', list(sr.CASES))
def test_the_cases_hold_what_they_are_meant_to(name):
    case = sr.make_case(name, True)
    A, K = sr.A_CASE, case['token_size']
    rec = sr.records(case['lines'], case['n_lines'], np.float64)
    assert (rec[0, :, 4] < 0).all() and (rec[1, 0, 4] > 0) and (rec[1, 1:, 4] < 0).all(), 'n_lines 0 and 1'
    assert (rec[2, [7, 21, 40], 4] < 0).all() and (rec[2, :, 4] > 0).sum() == 61, 'three dead records among 64'
    assert np.array_equal(rec[2, 7], sr.DEAD) and (case['phase'][2][:, [7, 21, 40]] != 0).all(), 'dead and closed'
    r = {t: sr.case_reference(name, True, t, True) for t in sr.STEPS}
    r0 = r[0]
    info, ruled, cnt, base = r0['info'].reshape(6, A, 4), r0['ruled'].reshape(6, A), r0['count'].reshape(6, A), r0['base'].reshape(6, A, K)
    size = base.sum(axis=2)
    assert ruled[:2].all() and (info[:2, :, 1] == -1).all() and (cnt[:2] == size[:2]).all(), 'no line: ruled rows keep their base'
    assert info[2, 0, 1] == 0 and abs(info[2, 0, 0] - 2.5) < 1e-3 and info[2, 0, 2] == 2 and 0 < cnt[2, 0] < size[2, 0], 'in front'
    for row, what in ((1, 'astride'), (2, 'past'), (3, 'facing against')):
        assert ruled[2, row] and info[2, row, 1] == -1 and info[2, row, 2] == 1 and cnt[2, row] == size[2, row], what
    assert info[2, 4, 1] == -1 and r0['governed'].reshape(6, A)[2, 4] and 0 < cnt[2, 4] < size[2, 4], 'beside the line: the lateral test'
    assert not ruled[3, 0] and not ruled[3, 1] and (info[3, :2, 2] == 0).all(), 'a pedestrian, an invalid row'
    assert cnt[3, 2] == 0 and np.array_equal(r0['allowed'][sr.FALLBACK_ROW], r0['base'][sr.FALLBACK_ROW]), 'the fallback'
    assert ruled[3, 3] and cnt[3, 3] < size[3, 3]
    fn = sr.case_reference(name, True, 0, True, True)
    assert not fn['ruled'].reshape(6, A)[3, 3:].any() and (fn['count'].reshape(6, A)[3, 3:] == size[3, 3:]).all(), '>= first_new'
    assert (info[5, 1:3, 1] != 7).all() and (info[5, 1:3, 1] != 21).all(), 'a dead record governs nobody'
    banned = [int((~x['pre'] & x['base']).sum()) for x in r.values()]
    assert banned[0] > 0 and banned[1] > 0 and (r[0]['pre'] != r[1]['pre']).any(), 'phase rows 0 and 1 differ'
    assert (r[2]['count'].reshape(6, A)[2:4] == size[2:4]).all(), 'phase row 2 opens the one line'
    for key in ('pre', 'allowed', 'count', 'info'):
        assert np.array_equal(r[4][key], r[1][key]), 't = 4 wraps to the row of t = 1'
    assert (r0['pre'] & r0['base']).any() and (~r0['pre'] & r0['base']).any(), 'allowed and banned tokens both exist'


def test_signal_phase_on_hand_written_schedules():
    from infgen_amd import constraints
    ph = constraints.signal_phase(3, 6, [0, 4, 2], [3, 2, 2])
    assert ph.dtype == np.uint8 and ph.shape == (6, 3)
    assert ph[:, 0].tolist() == [1, 1, 1, 0, 0, 0] and ph[:, 1].tolist() == [1, 1, 0, 0, 1, 1] and ph[:, 2].tolist() == [0] * 6
    assert constraints.signal_phase(2, 4, 0, 2, offset=[0, 1])[:, 1].tolist() == [1, 0, 0, 1]
    assert constraints.signal_phase(1, 5, 0, 5)[:, 0].tolist() == [1] * 5
    for bad in (dict(n_lines=0, period=4, red_from=0, red_to=1), dict(n_lines=1, period=0, red_from=0, red_to=0),
                dict(n_lines=1, period=4, red_from=-1, red_to=1), dict(n_lines=1, period=4, red_from=0, red_to=5),
                dict(n_lines=1, period=4, red_from=0.5, red_to=1)):
        with pytest.raises(ValueError):
            constraints.signal_phase(**bad)


def test_stop_lines_from_map_on_a_hand_written_map():
    from infgen_amd import constraints
    scene = {'map_polygon': {'light_type': np.array([1, 0, 2, 0], np.uint8)},
             'pt_token': {'position': np.array([[9., 9.], [10., 0.], [20., 0.], [0., 5.], [30., 30.], [1., 1.]], np.float32),
                          'orientation': np.array([0.3, 0.0, 0.0, np.pi / 2, 1.0, 2.0], np.float32)},
             'pt_token__to__map_polygon': {'edge_index': np.array([[0, 2, 1, 3, 4, 5], [0, 1, 1, 3, 2, 3]])}}
    lines, n, phase = constraints.stop_lines_from_map(scene, half_width=2.0)
    assert lines.shape == (1, 2, 4) and lines.dtype == np.float32 and n.tolist() == [2] and phase.tolist() == [[[1, 1]]]
    assert np.allclose(lines[0, 0], [10, 2, 10, -2], atol=1e-6), 'polygon 1: its first token is 1, heading +x: a is to its left'
    assert np.allclose(lines[0, 1], [-2, 5, 2, 5], atol=1e-6), 'polygon 3: token 3, heading +y'
    both, n2, ph2 = constraints.stop_lines_from_map([scene, scene], states=(0, 2))
    assert both.shape == (2, 3, 4) and n2.tolist() == [3, 3] and ph2.shape == (2, 1, 3)
    key = dict(scene)
    key[('pt_token', 'to', 'map_polygon')] = key.pop('pt_token__to__map_polygon')
    assert np.array_equal(constraints.stop_lines_from_map(key, half_width=2.0)[0], lines)
    none, n0, ph0 = constraints.stop_lines_from_map(scene, states=(3,))
    assert none.shape == (1, 1, 4) and n0.tolist() == [0] and ph0.tolist() == [[[0]]]
    with pytest.raises(ValueError):
        constraints.stop_lines_from_map(scene, half_width=0.0)
    # the record of such a line points along the token's orientation
    rec = sr.records(lines, n, np.float64)
    assert np.allclose(rec[0, 0, 2:4], [1, 0], atol=1e-6) and np.allclose(rec[0, 1, 2:4], [0, 1], atol=1e-6)


def test_the_python_argument_checks_raise():
    from infgen_amd import constraints
    ok = dict(lines=np.zeros((2, 5, 4), np.float32), phase=np.zeros((2, 3, 5), np.uint8))
    conf = constraints.check_obey_signals(ok, n_scenes=2)
    assert (conf['setback'], conf['align'], conf['types']) == (0.5, 0.5, (1, 0, 1)) and conf['n_lines'].tolist() == [5, 5]
    assert constraints.check_obey_signals(False) is None and constraints.check_obey_signals(None) is None
    assert constraints.signal_key(None) is None and constraints.signal_key(conf) == (0.5, 0.5, (1, 0, 1), 5, 3)
    assert constraints.check_obey_signals(dict(ok, phase=np.ones((2, 5), bool)), n_scenes=2)['phase'].shape == (2, 1, 5)
    nan = float('nan')
    for bad in (True, dict(ok, setback=-1), dict(ok, setback=nan), dict(ok, setback=float('inf')), dict(ok, align=1.5), dict(ok, align=-1.1),
                dict(ok, align=nan), dict(ok, types='veh'), dict(ok, types=(3,)), dict(ok, margin=1.0), dict(lines=ok['lines']),
                dict(phase=ok['phase']), dict(ok, lines=np.zeros((2, 0, 4))), dict(ok, lines=np.zeros((2, 65, 4))),
                dict(ok, lines=np.zeros((2, 5, 3))), dict(ok, n_lines=np.zeros(3, np.int32)), dict(ok, n_lines=np.full(2, 6)),
                dict(ok, n_lines=np.full(2, -1)), dict(ok, n_lines=np.zeros(2)), dict(ok, phase=np.zeros((2, 3, 4), np.uint8)),
                dict(ok, phase=np.zeros((1, 3, 5), np.uint8)), dict(ok, phase=np.zeros((2, 0, 5), np.uint8)),
                dict(ok, phase=np.zeros((2, 3, 5), np.float32))):
        with pytest.raises(ValueError):
            constraints.check_obey_signals(bad, n_scenes=2)
    with pytest.raises(ValueError):
        constraints.check_obey_signals(ok, n_scenes=3)
    with pytest.raises(ValueError):
        constraints.check_obey_signals(ok, has_shape=False, n_scenes=2)
    with pytest.raises(ValueError):
        constraints.signal_buffers(1, 32, 4, 1, 48)


class _Signal(C.Structure):
    _fields_ = [('bits', C.c_void_p), ('ident', C.c_void_p), ('shape', C.c_void_p), ('end_pose', C.c_void_p), ('records', C.c_void_p),
                ('phase', C.c_void_p), ('n_phase', C.c_int), ('K', C.c_int), ('copies', C.c_int), ('setback', C.c_float),
                ('align', C.c_float), ('types', C.c_int * 3), ('count', C.c_void_p), ('info', C.c_void_p)]


def _arena():
    buf = (C.c_float * 256)()
    p = C.addressof(buf)
    return buf, p + (-p) % 32


def test_the_c_entries_refuse_on_the_host_and_attach_get_detach_on_a_handle():
    """the checks that come before any launch, on a machine without a device, and infgen_token_mask_signal_get's "none / attached /
    detached" bytes"""
    from infgen_amd import _lib
    lib = _lib.load()
    keep, p = _arena()
    types = (C.c_int * 3)(1, 0, 1)
    size = C.sizeof(_Signal)

    def got(h):
        buf = (C.c_ubyte * size)()
        assert lib.infgen_token_mask_signal_get(h, buf, size) == size, lib.infgen_last_error()
        return bytes(buf)

    none = _Signal()
    none.n_phase = none.K = none.copies = 1
    assert got(0) == bytes(none)
    assert lib.infgen_token_mask_signal_get(0, (C.c_ubyte * 8)(), 8) < 0 and lib.infgen_token_mask_signal_get(0, None, size) < 0
    h = lib.infgen_token_mask_create(None, 0, None, None, None)
    assert h >= 1
    try:
        assert got(h) == bytes(none)
        good = dict(bits=p, ident=p + 16, shape=p + 32, end=p + 48, rec=p + 64, phase=p + 81, n_phase=3, K=7, copies=2, setback=0.75,
                    align=0.25, types=types, count=p + 96, info=p + 112)
        assert lib.infgen_token_mask_signal(h, *good.values()) == 0, lib.infgen_last_error()
        want = _Signal(p, p + 16, p + 32, p + 48, p + 64, p + 81, 3, 7, 2, 0.75, 0.25, (C.c_int * 3)(1, 0, 1), p + 96, p + 112)
        assert got(h) == bytes(want), 'attached'
        for over, word in ((dict(setback=-1.0), 'setback'), (dict(setback=float('nan')), 'setback'), (dict(setback=float('inf')), 'setback'),
                           (dict(align=1.5), 'align'), (dict(align=-1.01), 'align'), (dict(align=float('nan')), 'align'),
                           (dict(K=0), 'K must be'), (dict(K=65), 'K must be'), (dict(n_phase=0), 'n_phase'), (dict(copies=0), 'copies'),
                           (dict(shape=None), 'shape'), (dict(end=None), 'end-pose'), (dict(rec=None), 'record'), (dict(phase=None), 'phase'),
                           (dict(types=None), 'type switch'), (dict(ident=None), 'identity'), (dict(rec=p + 4), 'aligned'),
                           (dict(info=p + 8), 'aligned'), (dict(bits=p + 4), 'aligned')):
            assert lib.infgen_token_mask_signal(h, *dict(good, **over).values()) != 0, over
            msg = lib.infgen_last_error().decode()
            assert word in msg and 'signal mask' in msg, (over, msg)
        assert got(h) == bytes(want), 'a refused attach changes nothing'
        assert lib.infgen_token_mask_signal(h, None, *list(good.values())[1:]) == 0, 'NULL bits detach'
        assert got(h) == bytes(none), 'detached'
        for bad_handle in (0, -3, h + 100):
            assert lib.infgen_token_mask_signal(bad_handle, *good.values()) != 0
        assert lib.infgen_token_mask_signal_get(h + 100, (C.c_ubyte * size)(), size) < 0
    finally:
        assert lib.infgen_token_mask_destroy(h) == 0
    assert lib.infgen_token_mask_signal(h, *good.values()) != 0, 'a destroyed handle'
    # the record builder and the stand-alone operator
    assert lib.infgen_signal_records(None, p, 1, 4, p, None) != 0 and lib.infgen_signal_records(p, p, 1, 65, p, None) != 0
    assert lib.infgen_signal_records(p, p, 1, 0, p, None) != 0 and lib.infgen_signal_records(p, p, 1, 4, p + 4, None) != 0
    assert lib.infgen_signal_records(p + 4, p, 1, 4, p, None) != 0 and lib.infgen_signal_records(p, p, 0, 4, p, None) != 0
    op = dict(pos=p, head=p, state=p, n_agents=p, first_new=None, type=p, shape=p, S=2, A_cap=1, T=4, c=1, end=p, token_size=64, rec=p,
              phase=p, n_phase=1, K=4, t=0, copies=1, setback=0.5, align=0.5, types=types, mask_bits=None, mask_n_sets=0, mask_row=None,
              mask_type=None, out_bits=p, out_count=None, out_info=None, stream=None)
    for over, word in ((dict(t=-1), 'step t'), (dict(copies=3), 'multiple of copies'), (dict(token_size=48), 'token_size'),
                       (dict(token_size=4128), 'token_size'), (dict(A_cap=1025), 'INFGEN_Q_MAX_AGENTS'), (dict(K=65), 'K must be'),
                       (dict(n_phase=0), 'n_phase'), (dict(setback=-0.5), 'setback'), (dict(align=2.0), 'align'), (dict(out_bits=None), 'output'),
                       (dict(c=4), 'column'), (dict(pos=None), 'scene array'), (dict(out_info=p + 4), 'aligned')):
        assert lib.infgen_signal_mask(*dict(op, **over).values()) != 0, over
        msg = lib.infgen_last_error().decode()
        assert msg.startswith('infgen_signal_mask: signal mask:') and word in msg, (over, msg)


def test_the_rider_block_keeps_the_parents_bytes_with_signals_attached():
    """infgen_token_mask_riders, the entry tests/test_route_masks_cpu.py pins: the same size and the same bytes whether or not a
    signal configuration is attached"""
    from test_route_masks_cpu import _Riders
    from infgen_amd import _lib
    lib = _lib.load()
    keep, p = _arena()
    types = (C.c_int * 3)(1, 0, 1)
    size = C.sizeof(_Riders)

    def block(h):
        buf = (C.c_ubyte * (size + 64))(*([0xA5] * (size + 64)))
        assert lib.infgen_token_mask_riders(h, None, 2048, buf, size) == size, lib.infgen_last_error()
        assert bytes(buf)[size:] == bytes([0xA5] * 64), 'nothing is written behind the five configurations'
        return bytes(buf)[:size]

    h = lib.infgen_token_mask_create(None, 0, None, None, None)
    try:
        assert lib.infgen_token_mask_route(h, p + 384, p + 400, p + 416, p + 432, p + 448, p + 480, 8, 2, 2.0, 0.5, 0.25, 1.0, types, p + 496,
                                           p + 512) == 0
        before = block(h)
        assert before != block(0)
        assert lib.infgen_token_mask_signal(h, p, p + 16, p + 32, p + 48, p + 64, p + 80, 3, 7, 2, 0.75, 0.25, types, p + 96, p + 112) == 0
        assert block(h) == before
        assert lib.infgen_token_mask_signal(h, None, None, None, None, None, None, 1, 1, 1, 0.0, 0.0, None, None, None) == 0
        assert block(h) == before
    finally:
        assert lib.infgen_token_mask_destroy(h) == 0


def test_decoder_attribute_reaches_the_engine_arguments_and_key():
    import types
    from infgen_amd.modules.infgen_decoder import InfGenDecoder
    dec = types.SimpleNamespace(sample_temperature=1.0, sample_top_p=1.0, insert_temperature=1.0, insert_top_p=1.0,
                                token_constraints=None, avoid_collisions=False)
    off = InfGenDecoder._sampling_kw(dec, 2, 3)
    dec.obey_signals = False
    assert InfGenDecoder._sampling_kw(dec, 2, 3)[2] == off[2], 'off: the key of a decoder without the attribute'
    conf = dict(lines=np.zeros((2, 5, 4), np.float32), phase=np.zeros((2, 3, 5), np.uint8), setback=1.0)
    dec.obey_signals = conf
    ctor, live, key = InfGenDecoder._sampling_kw(dec, 2, 3)
    assert 'obey_signals' not in off[0] and ctor['obey_signals'] is conf and live['obey_signals'] is conf and key != off[2]
    dec.obey_signals = dict(conf, phase=np.zeros((2, 4, 5), np.uint8))
    assert InfGenDecoder._sampling_kw(dec, 2, 3)[2] != key, 'n_phase is part of the engine key'
    dec.obey_signals = dict(conf, align=2.0)
    with pytest.raises(ValueError, match='align'):
        InfGenDecoder._sampling_kw(dec, 2, 3)
    with pytest.raises(ValueError, match='scenes'):
        dec.obey_signals = conf
        InfGenDecoder._sampling_kw(dec, 3, 1)
