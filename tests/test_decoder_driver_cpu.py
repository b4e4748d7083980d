"""CPU: the steps of InfGenDecoder's rollout driver that the list entry and the Batch entry share (modules/infgen_decoder.py:
_draw_uniforms, _engine_key, _cached_engine, _rollout_or_yield) with stub engines - no weights, no device, no library."""
import pytest
import torch

from infgen_amd import synth
from infgen_amd.engine import InsertionHeadroomError
from infgen_amd.modules import infgen_decoder as idec


class _Engine:
    """records what the driver asks of an engine"""

    def __init__(self, A_cap=32, fits=(), device_ok=True, fail=0, name='e'):
        self.A_cap, self.hosts, self.name = A_cap, [dict(A=16), dict(A=12)], name
        self._fits, self._device_ok, self._fail = set(fits), device_ok, fail
        self.calls = []

    def fits(self, *a):
        self.calls.append('fits')
        return 'host' in self._fits

    def fits_device(self, *a):
        self.calls.append('fits_device')
        return 'device' in self._fits

    def reload(self, *a):
        self.calls.append('reload')

    def reload_device(self, *a):
        self.calls.append('reload_device')
        return self._device_ok

    def rollout(self):
        self.calls.append('rollout')
        if self._fail:
            self._fail -= 1
            raise InsertionHeadroomError('out of rows', needed=1)


_LIST = [(lambda e: e.fits_device(), lambda e: e.reload_device()), (lambda e: e.fits(), lambda e: e.reload())]


def _never():
    raise AssertionError('an engine was built')


@pytest.mark.parametrize('fits, device_ok, calls', [
    (('device', 'host'), True, ['fits_device', 'reload_device']),                       # the device reload is preferred
    (('device', 'host'), False, ['fits_device', 'reload_device', 'fits', 'reload']),   # ... and falls through when it declines
    (('host',), True, ['fits_device', 'fits', 'reload'])])
def test_cache_step_reloads_in_order_of_preference(fits, device_ok, calls):
    eng = _Engine(fits=fits, device_ok=device_ok)
    engines = {'k': eng}
    assert idec._cached_engine(engines, 'k', _LIST, _never) is eng
    assert eng.calls == calls and engines == {'k': eng}


def test_cache_step_builds_and_evicts_the_oldest():
    old, kept, new = _Engine(name='old'), _Engine(name='kept'), _Engine(name='new')
    engines = {'a': old, 'b': kept}
    assert idec._cached_engine(engines, 'c', _LIST, lambda: new) is new
    assert list(engines.items()) == [('b', kept), ('c', new)] and old.calls == kept.calls == []
    # a held engine that fits no attempt is replaced under its own key; with one other entry nothing is evicted
    engines = {'a': old}
    assert idec._cached_engine(engines, 'b', _LIST, lambda: kept) is kept and list(engines) == ['a', 'b']
    assert idec._cached_engine(engines, 'a', _LIST, lambda: new) is new and engines['a'] is new
    assert old.calls == ['fits_device', 'fits']


def _finish(gen):
    try:
        yielded = next(gen)
    except StopIteration as e:
        return None, e.value
    return yielded, gen


def test_retry_step_rebuilds_with_twice_the_rows_under_the_same_key():
    first, second = _Engine(A_cap=32, fail=1), _Engine(A_cap=64)
    asked = []

    def make(headroom=None):
        asked.append(headroom)
        return second
    engines = {'k': first, 'other': object()}
    # amax is the caller's value (19), not the stub's hosts' (16)
    yielded, eng = _finish(idec._rollout_or_yield(engines, 'k', first, make, 19, 1024))
    assert yielded is None and eng is second and engines['k'] is second and len(engines) == 2
    assert asked == [min(2 * 32, 1024) - 19] and first.calls == ['rollout'] and second.calls == ['rollout']
    # the doubled rows are capped by the limit
    asked.clear()
    first = _Engine(A_cap=48, fail=1)
    _finish(idec._rollout_or_yield({}, 'k', first, make, 19, 80))
    assert asked == [80 - 19]


def test_retry_step_reraises_at_the_limit():
    eng = _Engine(A_cap=64, fail=1)
    with pytest.raises(InsertionHeadroomError):
        _finish(idec._rollout_or_yield({'k': eng}, 'k', eng, _never, 16, 64))
    assert eng.calls == ['rollout']


def test_retry_step_yields_the_engine_of_a_session():
    eng = _Engine(fail=1)
    yielded, gen = _finish(idec._rollout_or_yield({'k': eng}, 'k', eng, _never, 16, 1024, session=True))
    assert yielded is eng and eng.calls == []
    with pytest.raises(StopIteration) as stop:
        next(gen)
    assert stop.value.value is eng and eng.calls == []


def test_uniforms_follow_torchs_stream():
    cfg = synth.standard_config()
    cfg.disable_insertion = False
    steps, S, ucols = cfg.num_decode_steps, 6, 40
    torch.manual_seed(11)
    su, iu = idec._draw_uniforms(cfg, 5, 3, S, ucols)
    torch.manual_seed(11)
    want_s, want_i = torch.rand(steps, S, ucols), torch.rand(steps, 10, S)
    assert su.shape == (steps, S, ucols) and iu.shape == (steps, 10, S)
    assert (su == want_s.numpy()).all() and (iu == want_i.numpy()).all()
    # the insert draw alone; nothing without insertion; a caller's uniforms are kept and nothing is drawn for them
    torch.manual_seed(11)
    su, iu = idec._draw_uniforms(cfg, 1, 3, S, ucols)
    torch.manual_seed(11)
    assert su is None and (iu == torch.rand(steps, 10, S).numpy()).all()
    cfg.disable_insertion = True
    assert idec._draw_uniforms(cfg, 1, 3, S, ucols) == (None, None)
    state = torch.get_rng_state()
    mine = want_s.numpy()
    su, iu = idec._draw_uniforms(cfg, 5, 1, S, ucols, sample_uniforms=mine)
    assert su is mine and iu is None
    assert idec._draw_uniforms(cfg, 1, 1, S, ucols) == (None, None)
    assert torch.equal(torch.get_rng_state(), state)


_FACTS = dict(graphs=False, scenes=4, tables=b'tables', disable_insertion=False, steps=80, sample_k=5, insert_k=1, debug=False,
              copies=1, replay=False, token_logprob=False, sample_logprob=False, sampling=(1.0, 1.0), single=False, map_only=False,
              own_map=True, seed_outputs=False)


@pytest.mark.parametrize('fact, other', [('copies', 3), ('replay', True), ('token_logprob', True), ('sample_logprob', True),
                                         ('sampling', (0.5, 1.0)), ('map_only', True), ('graphs', True)])
def test_engine_key_tells_every_fact_apart(fact, other):
    assert idec._engine_key(**_FACTS) == idec._engine_key(**dict(_FACTS))
    assert idec._engine_key(**_FACTS) != idec._engine_key(**dict(_FACTS, **{fact: other}))


def test_batch_engines_are_found_by_their_tag():
    assert idec._engine_key(**dict(_FACTS, graphs=True))[0] == 'graphs' != idec._engine_key(**_FACTS)[0]
