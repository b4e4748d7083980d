"""The engine's bookkeeping for the step riders (collision, road, score, route and signal configurations on the token-mask handle),
pinned in one place: which ``infgen_token_mask_*`` entries a ``reload`` calls, when a captured graph is dropped, how long the handle
lives, the road / scores ordering case and the threading of the step keywords through the three reload entries.  What each rider
computes is the business of its own test file; this one only watches the calls, on the smallest engine there is (c1_a8_m128, one
scene, one copy)."""
import numpy as np
import pytest
import torch

from conftest import load_case
from rider_helpers import _make, _weights

pytestmark = pytest.mark.gpu

CREATE, DESTROY = 'infgen_token_mask_create', 'infgen_token_mask_destroy'
# per rider keyword: the library's attach entry, the arguments that detach it (behind the handle), the engine's registration attribute
ATTACH = dict(
    avoid_collisions=('infgen_token_mask_collision', (None, None, None, None, 1, 0.0, None), '_coll_reg'),
    stay_on_road=('infgen_token_mask_road', (None, None, None, None, None, None, None, 0, 1, 1, 0.0, None, None), '_road_reg'),
    step_scores=('infgen_token_mask_score', (None, 0, None, None, None, None, 0, 1, 1, 0.0, None, 0.5), '_score_reg'),
    follow_routes=('infgen_token_mask_route', (None, None, None, None, None, None, 2, 1, 0.0, 0.0, 0.0, 0.0, None, None, None), '_route_reg'),
    obey_signals=('infgen_token_mask_signal', (None, None, None, None, None, None, 1, 1, 1, 0.0, 0.0, None, None, None), '_signal_reg'))
STEP_KEYWORDS = ('token_masks', 'token_mask_type', 'token_mask_row') + tuple(ATTACH)


class _Recorder:
    """``eng.lib`` with the ``infgen_token_mask_*`` calls written down: every attribute is the library's own"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('infgen_token_mask_'):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded

    def names(self):
        return [name for name, _ in self.calls]


@pytest.fixture(scope='module')
def case():
    from infgen_amd import constraints
    c = load_case('c1_a8_m128')
    routes, n = constraints.routes_from_logged(c['scene'], start=c['cfg'].hist_columns - 1)
    lines = np.array([[[10.0, 2.0, 10.0, -2.0], [30.0, 2.0, 30.0, -2.0]]], np.float32)
    on = dict(avoid_collisions=True, stay_on_road=True, step_scores=True, follow_routes=dict(routes=routes, n_points=n),
              obey_signals=dict(lines=lines, phase=np.ones((1, 2, 2), np.uint8)))
    # one scalar of the key changed: the value, and the scalar as the attach call carries it
    changed = dict(avoid_collisions=(dict(margin=0.5), 0.5), stay_on_road=(dict(margin=0.5), 0.5), step_scores=(dict(road_margin=0.75), 0.75),
                   follow_routes=(dict(on['follow_routes'], corridor=1.5), 1.5), obey_signals=(dict(on['obey_signals'], setback=1.25), 1.25))
    return dict(c=c, w=_weights(c), scenes=[c['scene']], on=on, changed=changed)


def _engine(case, **kw):
    eng = _make(case['c'], case['w'], **kw)
    eng.lib = _Recorder(eng.lib)
    return eng


def _capture(eng):
    """a rollout, and more until the decode steps replay from a captured graph (an engine's first rollout runs eagerly) -> the
    calls they made"""
    del eng.lib.calls[:]
    for _ in range(3):
        eng.rollout()
        if eng._graph is not None:
            break
    assert eng._graph is not None
    return eng.lib.names()


def _reload(eng, case, **kw):
    """``reload(scenes, **kw)`` on an engine that holds a captured graph -> (the recorded calls, was the graph dropped)"""
    assert eng._graph is not None
    del eng.lib.calls[:]
    eng.reload(case['scenes'], **kw)
    return list(eng.lib.calls), eng._graph is None


def _road_table(eng):
    return None if eng.road_records is None else (eng.road_records.data_ptr(), eng._road_cap)


@pytest.mark.parametrize('name', list(ATTACH))
def test_off_on_same_changed_off_none(case, name):
    entry, off, reg = ATTACH[name]
    on, (changed, scalar) = case['on'][name], case['changed'][name]
    eng = _engine(case, use_graph=True)
    assert _capture(eng) == [] and eng._ctx.token_mask == 0 and eng._mask_handle == 0

    def recapture():
        """the rollouts in between attach nothing - but the road table's riders again where the prologue grew the table"""
        table = _road_table(eng)
        calls = _capture(eng)
        assert calls == ([entry] if getattr(eng, name) is not None and _road_table(eng) != table else []), calls

    # off on an engine that has nothing on: nothing happens, and no handle comes into being
    calls, dropped = _reload(eng, case, **{name: False})
    assert calls == [] and not dropped and getattr(eng, name) is None
    recapture()
    assert eng._ctx.token_mask == 0 and eng._mask_handle == 0
    # on: the handle is created (without a table) and the rider attached to it; the graph goes
    calls, dropped = _reload(eng, case, **{name: on})
    assert [n for n, _ in calls] == [CREATE, entry] and dropped and getattr(eng, name) is not None
    h = eng._mask_handle
    assert h >= 1 and eng._ctx.token_mask == h and calls[1][1][0] == h and calls[1][1][1:] != off
    assert all((getattr(eng, r) is not None) == (r == reg) for _, _, r in ATTACH.values())
    recapture()
    # the same value again: nothing is attached; only the signals, whose every upload rewrites tables a graph would replay over,
    # drop the graph
    calls, dropped = _reload(eng, case, **{name: on})
    assert calls == [] and dropped == (name == 'obey_signals'), (calls, dropped)
    recapture()
    # no value at all: kept, also by the signals (nothing is uploaded)
    calls, dropped = _reload(eng, case)
    assert calls == [] and not dropped and getattr(eng, name) is not None
    recapture()
    # one scalar changed: attached again with the new value
    calls, dropped = _reload(eng, case, **{name: changed})
    assert [n for n, _ in calls] == [entry] and dropped
    assert calls[0][1][0] == h and any(isinstance(a, float) and a == scalar for a in calls[0][1])
    recapture()
    # off: the one call, with the "off" arguments; the handle stays in the context
    calls, dropped = _reload(eng, case, **{name: False})
    assert [n for n, _ in calls] == [entry] and calls[0][1] == (h,) + off and dropped
    assert getattr(eng, name) is None and getattr(eng, reg) is None and eng._ctx.token_mask == h == eng._mask_handle
    if name in ('avoid_collisions', 'stay_on_road'):         # their buffers stay (static addresses) ...
        k = eng._coll if name == 'avoid_collisions' else eng._road
        bits = eng.collision_bits if name == 'avoid_collisions' else eng.road_bits
        assert k is not None and bits is k['bits']
    elif name == 'step_scores':
        assert eng.step_score is not None and eng.score_row is not None and eng._score_arg is None
    elif name == 'follow_routes':                            # ... routes and signals leave nothing readable
        assert eng._route is None and eng.route_bits is None and eng.route_allowed is None and eng.route_progress is None
    else:
        assert eng._signal is None and eng.signal_bits is None and eng.signal_allowed is None and eng.signal_info is None
    recapture()
    # None: off stays off
    calls, dropped = _reload(eng, case, **{name: None})
    assert calls == [] and not dropped and getattr(eng, name) is None
    recapture()
    assert eng._ctx.token_mask == h


def test_handle_life_and_attaching_every_live_rider_again(case):
    entries = [e for e, _, _ in ATTACH.values()]
    regs = [r for _, _, r in ATTACH.values()]
    # nothing ever on: no handle, and applying or dropping is nothing
    bare = _engine(case)
    bare.rollout()
    bare._drop_mask_handle()
    bare._apply_token_masks()
    assert bare.lib.calls == [] and bare._ctx.token_mask == 0 and bare._mask_handle == 0
    # all five on from the constructor: created and attached in the engine's one order when the context is built
    eng = _engine(case, **case['on'])
    assert eng.lib.calls == [] and eng._ctx is None, 'nothing is registered before there is a context'
    eng.rollout()
    h = eng._mask_handle
    assert h >= 1 and eng._ctx.token_mask == h
    assert eng.lib.names() == [CREATE] + entries, eng.lib.names()
    assert all(args[0] == h for n, args in eng.lib.calls if n != CREATE)
    del eng.lib.calls[:]
    eng._apply_token_masks()
    assert eng.lib.calls == [], 'no registration changed'
    eng._drop_mask_handle()
    assert eng.lib.calls == [(DESTROY, (h,))] and eng._mask_handle == 0 and eng._ctx.token_mask == 0
    assert eng._mask_reg is None and all(getattr(eng, r) is None for r in regs)
    del eng.lib.calls[:]
    eng._apply_token_masks()
    assert eng.lib.names() == [CREATE] + entries
    h2 = eng._mask_handle
    assert h2 >= 1 and eng._ctx.token_mask == h2 and all(args[0] == h2 for n, args in eng.lib.calls if n != CREATE)
    assert all(args[1:] != ATTACH[k][1] for k in ATTACH for n, args in eng.lib.calls if n == ATTACH[k][0])
    assert all(getattr(eng, r) is not None for r in regs)
    eng.rollout()
    # all off in one reload: one "off" call each, the handle stays
    del eng.lib.calls[:]
    eng.reload(case['scenes'], **{k: False for k in ATTACH})
    assert sorted(eng.lib.calls) == sorted((e, (h2,) + off) for e, off, _ in ATTACH.values())
    assert eng._ctx.token_mask == h2 and all(getattr(eng, r) is None for r in regs)


def test_scores_are_resolved_around_the_road(case):
    """``_load_riders``' ordering case.  The parent commit does NOT leave the configuration as it was when the scores conflict with
    a road that the same call changes: the new road is stored (and drives the table) before the scores are checked against it.
    That is what is pinned here; a conflict with a road the call leaves alone changes neither."""
    eng = _engine(case, use_graph=True, stay_on_road=dict(detail=2), step_scores=True)
    _capture(eng)
    assert eng.stay_on_road['detail'] == 2 and eng.step_scores['detail'] == 2
    # road's detail changes, the scores follow it: scores that name nothing, and scores that name the new detail
    eng.reload(case['scenes'], stay_on_road=dict(detail=5), step_scores=True)
    assert eng.stay_on_road['detail'] == 5 and eng.step_scores['detail'] == 5 and eng._score_arg is True and eng._graph is None
    _capture(eng)
    eng.reload(case['scenes'], stay_on_road=dict(detail=10), step_scores=dict(detail=10))
    assert eng.stay_on_road['detail'] == 10 and eng.step_scores['detail'] == 10 and eng._score_arg == dict(detail=10)
    _capture(eng)
    # scores alone that conflict with the road that is there: refused, both configurations as they were, the argument recorded
    road, scores = dict(eng.stay_on_road), dict(eng.step_scores)
    del eng.lib.calls[:]
    with pytest.raises(ValueError, match=r"^step_scores: detail 5 conflicts with stay_on_road's 10: the engine keeps one road table$"):
        eng.reload(case['scenes'], step_scores=dict(detail=5))
    assert eng.stay_on_road == road and eng.step_scores == scores and eng._score_arg == dict(detail=5)
    assert eng.lib.calls == [] and eng._graph is not None
    # a road change with scores that conflict with the NEW road: refused when road re-checks the scores' recorded argument - the
    # new road is already the engine's by then, the scores are the old ones, nothing was attached
    with pytest.raises(ValueError, match=r"^step_scores: detail 10 conflicts with stay_on_road's 5: the engine keeps one road table$"):
        eng.reload(case['scenes'], stay_on_road=dict(detail=5), step_scores=dict(detail=10))
    assert eng.stay_on_road['detail'] == 5 and eng.step_scores == scores and eng._score_arg == dict(detail=10)
    assert eng.lib.calls == [] and eng._graph is None and eng._road_dirty
    # scores that go are gone before road is resolved: no re-check against the new road
    eng.reload(case['scenes'], stay_on_road=dict(detail=2), step_scores=False)
    assert eng.stay_on_road['detail'] == 2 and eng.step_scores is None and eng._score_arg is None
    eng.rollout()


def test_every_reload_entry_threads_the_eight_step_keywords(case):
    from infgen_amd import constraints, engine
    from infgen_amd.modules.infgen_decoder import batch_datas, stack_datas
    from test_modules_gpu import _to_data
    c, w, scenes = case['c'], case['w'], case['scenes']
    datas = [_to_data(c['scene'], torch.device('cuda:0'))]
    stk, b = stack_datas(datas, min_scenes=1), batch_datas(datas)
    tm = constraints.TokenMasks(np.ones((1, c['cfg'].token_size), bool))
    kw = dict(case['on'], token_masks=tm, token_mask_type=[0, -1, -1], token_mask_row=np.full((1, 8), -1))
    assert set(kw) == set(STEP_KEYWORDS)
    host = _engine(case)
    ragged = engine.RolloutEngine(w, None, c['vocab'], c['map_vocab'], c['grid'], batch=b)
    ragged.lib = _Recorder(ragged.lib)
    assert host.fits_device(stk)
    entries = (('reload', host, lambda **k: host.reload(scenes, **k)),
               ('reload_device', host, lambda **k: host.reload_device(stk, scenes, **k)),
               ('reload_batch', ragged, lambda **k: ragged.reload_batch(b, **k)))
    for what, eng, call in entries:
        eng.rollout()
        del eng.lib.calls[:]
        assert call(**kw) is not False, what
        assert eng.token_masks is tm and eng.token_mask_type == [0, -1, -1] and all(getattr(eng, k) is not None for k in ATTACH), what
        # the static mask first, then the riders in the order the engine resolves them: collisions, road, scores, routes, signals
        assert eng.lib.names() == [CREATE] + [e for e, _, _ in ATTACH.values()], (what, eng.lib.names())
        eng.rollout()
        with pytest.raises(TypeError):
            call(obey_signal=False)
        del eng.lib.calls[:]
        assert call(**{k: None for k in STEP_KEYWORDS}) is not False and eng.lib.calls == [], what
        assert all(getattr(eng, k) is not None for k in ATTACH), what
        eng.reload(scenes, **{k: False for k in ATTACH}) if eng is host else eng.reload_batch(b, **{k: False for k in ATTACH})
        eng._drop_mask_handle()
