"""k_observe_rows (include/infgen_hip.h, "observations") against the numpy restatement of tests/observe_ref.py.

Exactly equal to the float32 restatement: the indices, the counts and every field that is a copy or a flag.  Rotated values against
the float64 evaluation of the same float32 inputs, inside bars that follow from the definition - every difference, product and sum
rounds by at most half an ulp, cosf / sinf are good to 2 ulp, and the whole is doubled:
    x', y'            8 * 2^-23 * (|dx| + |dy|), dx, dy the float32-formed differences
    velocities        the same bar of the displacement, over dt
    cos D, sin D      8 * 2^-23
    yaw rate          8 * 2^-23 * 2 pi / dt (the wrap's intermediates are at most 2 pi in magnitude; its constants are the nearest
                      floats of pi and 2 pi, 9e-8 and 1.8e-7 from them)
The largest measured ratio to its bar is printed; only the bar is asserted.
"""
import functools

import numpy as np
import pytest
import torch

import observe_ref as R

pytestmark = pytest.mark.gpu

EPS = 8 * 2.0 ** -23
DEV = 'cuda:0'


def _launch(case, **over):
    import infgen_amd.torch_ops  # noqa: F401
    k = dict(case, **over)
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    out = torch.ops.infgen_hip.observe_rows(t(k['pos']), t(k['head']), t(k['state']), t(k['n_agents']), t(k['type']), t(k['shape']),
                                            k['c'], k['dt'], t(k['map_pos']), t(k['map_orient']), t(k['map_type']), t(k['n_map']),
                                            k['copies'], t(k['rows']), k['K'], float(k['radius']), k['Km'], float(k['map_radius']))
    torch.cuda.synchronize()
    return dict(zip(('self_feat', 'nbr_feat', 'nbr_index', 'nbr_count', 'map_feat', 'map_index', 'map_count'), (o.cpu().numpy() for o in out)))


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.evaluate(R.CASES[name])


def _ratio(got, want, bar):
    """max |got - want| / bar over the entries with a positive bar; entries with bar 0 must be exact"""
    err = np.abs(got.astype(np.float64) - want)
    assert (err[bar == 0] == 0).all()
    return float((err[bar > 0] / bar[bar > 0]).max()) if (bar > 0).any() else 0.0


def _check(got, ref, dt, what):
    for k in ('nbr_index', 'nbr_count', 'map_index', 'map_count'):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k)
    # copies and flags, exactly: live, length, width, type, has-previous; the 1.0 marks; the zeros of unused entries and dead rows
    assert np.array_equal(got['self_feat'][:, [0, 4, 5, 6, 7]], ref['self_feat32'][:, [0, 4, 5, 6, 7]]), what
    assert np.array_equal(got['nbr_feat'][..., 6:], ref['nbr_feat32'][..., 6:]) and np.array_equal(got['map_feat'][..., 4:], ref['map_feat32'][..., 4:]), what
    assert (got['nbr_feat'][got['nbr_index'] < 0] == 0).all() and (got['map_feat'][got['map_index'] < 0] == 0).all(), what
    dead = got['self_feat'][:, 0] == 0
    assert (got['self_feat'][dead] == 0).all() and (got['nbr_index'][dead] == -1).all() and (got['map_index'][dead] == -1).all(), what
    assert (got['self_feat'][got['self_feat'][:, 7] == 0][:, 1:4] == 0).all(), what
    ns, ms, ss = ref['nbr_scale'], ref['map_scale'], ref['self_scale']
    one = lambda a: np.where(a, EPS, 0.0)
    ratios = dict(
        nbr_xy=_ratio(got['nbr_feat'][..., 0:2], ref['nbr_feat'][..., 0:2], EPS * ns[..., :1].repeat(2, -1)),
        nbr_cs=_ratio(got['nbr_feat'][..., 2:4], ref['nbr_feat'][..., 2:4], one(ref['nbr_index'] >= 0)[..., None].repeat(2, -1)),
        nbr_v=_ratio(got['nbr_feat'][..., 4:6], ref['nbr_feat'][..., 4:6], EPS * ns[..., 1:].repeat(2, -1) / dt),
        map_xy=_ratio(got['map_feat'][..., 0:2], ref['map_feat'][..., 0:2], EPS * ms[..., None].repeat(2, -1)),
        map_cs=_ratio(got['map_feat'][..., 2:4], ref['map_feat'][..., 2:4], one(ref['map_index'] >= 0)[..., None].repeat(2, -1)),
        self_v=_ratio(got['self_feat'][:, 1:3], ref['self_feat'][:, 1:3], EPS * ss[:, None].repeat(2, -1) / dt),
        self_yaw=_ratio(got['self_feat'][:, 3], ref['self_feat'][:, 3], np.where(ref['self_feat'][:, 7] > 0, EPS * 2 * np.pi / dt, 0.0)))
    print(f'{what}: largest error / bar ' + ', '.join(f'{k} {v:.3f}' for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (what, ratios)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_against_the_restatement(name):
    case = R.CASES[name]
    got = _launch(case)
    _check(got, _ref(name), case['dt'], name)
    again = _launch(case)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), (name, k, 'two launches differ')


def test_without_a_map_and_with_a_device_row_list_of_another_dtype():
    case = R.CASES['rows']
    ref = _ref('rows_km0')
    got = _launch(case, map_pos=None, map_orient=None, map_type=None, n_map=None, Km=0, rows=case['rows'].astype(np.int64))
    for k in ('self_feat', 'nbr_feat', 'nbr_index', 'nbr_count'):
        assert np.array_equal(got[k], _launch(R.CASES['rows_km0'])[k]), k
    assert got['map_feat'].shape == (len(case['rows']), 0, 6) and (got['map_count'] == 0).all() and ref['map_count'].max() > 0


def test_refusals():
    import ctypes as C
    from infgen_amd import _lib
    lib = _lib.load()
    S, T, A, M, N, K, Km = 2, 3, 8, 16, 16, 4, 4
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    scene = dict(pos=z(S, T, A, 2), head=z(S, T, A), state=z(S, T, A, dt=torch.int32), n_agents=z(S, dt=torch.int32),
                 type=z(S * A, dt=torch.int32), shape=z(S * A, 3))
    maps = dict(map_pos=z(S, M, 2), map_orient=z(S, M), map_type=z(S, M, dt=torch.int64), n_map=z(S, dt=torch.int32))
    outs = dict(self_feat=z(N + 1, 8), nbr_feat=z(N, K, 10), nbr_index=z(N, K, dt=torch.int32), nbr_count=z(N, dt=torch.int32),
                map_feat=z(N, Km, 6), map_index=z(N, Km, dt=torch.int32), map_count=z(N, dt=torch.int32))

    def call(**kw):
        a = dict(S=S, A_cap=A, T=T, c=1, dt=0.5, M_cap=M, copies=1, obs_row=None, N=N, K=K, radius=10.0, Km=Km, map_radius=10.0)
        a.update({k: v.data_ptr() for k, v in {**scene, **maps, **outs}.items()})
        a.update(kw)
        rc = lib.infgen_observe_rows(a['pos'], a['head'], a['state'], a['n_agents'], a['type'], a['shape'], a['S'], a['A_cap'], a['T'],
                                     a['c'], a['dt'], a['map_pos'], a['map_orient'], a['map_type'], a['n_map'], a['M_cap'], a['copies'],
                                     a['obs_row'], a['N'], a['K'], a['radius'], a['Km'], a['map_radius'], a['self_feat'], a['nbr_feat'],
                                     a['nbr_index'], a['nbr_count'], a['map_feat'], a['map_index'], a['map_count'], None)
        return rc, (lib.infgen_last_error() or b'').decode()

    assert call()[0] == 0
    for kw, msg in ((dict(c=T), 'column outside'), (dict(c=-1), 'column outside'), (dict(K=65), 'K and Km must be in'),
                    (dict(Km=-1), 'K and Km must be in'), (dict(dt=0.0), 'dt must be finite and > 0'),
                    (dict(dt=float('inf')), 'dt must be finite and > 0'), (dict(radius=-1.0), 'radius must be >= 0'),
                    (dict(map_radius=float('nan')), 'radius must be >= 0'), (dict(copies=0), 'copies must be at least 1'),
                    (dict(S=3, copies=2), 'multiple of copies'), (dict(self_feat=None), 'self_feat'),
                    (dict(nbr_index=None), 'K > 0 needs'), (dict(map_count=None), 'Km > 0 needs'), (dict(map_orient=None), 'needs the map arrays'),
                    (dict(self_feat=outs['self_feat'].data_ptr() + 8), '16-byte aligned'),
                    (dict(map_index=outs['map_index'].data_ptr() + 4), '16-byte aligned'),
                    (dict(A_cap=2048), 'INFGEN_Q_MAX_AGENTS'), (dict(N=N - 1), 'N must be S \\* A_cap'), (dict(N=-1, obs_row=scene['type'].data_ptr()), 'never negative')):
        rc, err = call(**kw)
        assert rc != 0 and __import__('re').search(msg, err), (kw, rc, err)
    # K = 0 and Km = 0 take NULL for what they do not write
    assert call(K=0, nbr_feat=None, nbr_index=None, nbr_count=None)[0] == 0
    assert call(Km=0, map_feat=None, map_index=None, map_count=None, map_pos=None, map_orient=None, map_type=None, n_map=None)[0] == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the session
def _session_run(observe_agent):
    from test_replay_gpu import _case, _eng, _mask, _snap
    c = _case('c1_a8_m128')
    hc, av, A = c['cfg'].hist_columns, c['av'], 8
    free = _eng(c)
    ego_tok = free.token[0, :, av].clone()
    eng = _eng(c, run=False, replay=[_mask(A, [av, 3])])
    ses = eng.session()
    seen = []
    while not ses.done:
        if observe_agent:
            o = ses.observe(frame='agent', rows='controlled', neighbors=4, map_tokens=8)
            seen.append({k: o[k].clone() for k in ('self_feat', 'nbr_index', 'map_index')})
        ses.command(tokens=ego_tok[hc + ses.t].reshape(1))          # (row 3, controlled too, takes token 0)
        ses.advance()
    return eng, ses, _snap(eng), seen


def test_session_observation():
    from test_replay_gpu import _case, _eng, _mask, _same
    c = _case('c1_a8_m128')
    hc, av, A = c['cfg'].hist_columns, c['av'], 8
    eng = _eng(c, run=False, replay=[_mask(A, [av, 3])])
    ses = eng.session()
    before = ses.observe()
    ptrs = {k: v.data_ptr() for k, v in before.items() if isinstance(v, torch.Tensor)}
    world = ses.observe(frame='world')
    assert set(world) == set(before) == {'pos', 'head', 'state', 'token', 'type', 'shape', 'n_agents', 'ego_index', 'controlled', 'column'}
    assert {k: v.data_ptr() for k, v in world.items() if isinstance(v, torch.Tensor) and k != 'controlled'} == \
        {k: p for k, p in ptrs.items() if k != 'controlled'}
    for k in ('pos', 'head', 'state', 'token'):
        assert before[k].data_ptr() == getattr(eng, k)[:, hc - 1].data_ptr()
    tok = eng.token[0, hc - 1, av].reshape(1).clone()
    for _ in range(2):
        ses.command(tokens=tok)
        ses.advance()
    o = ses.observe(frame='agent', rows='controlled', neighbors=4, map_tokens=8)
    assert set(o) == set(before) | {'self_feat', 'nbr_feat', 'nbr_index', 'nbr_count', 'map_feat', 'map_index', 'map_count', 'obs_row'}
    col = hc - 1 + 2
    assert o['column'] == col and o['obs_row'].dtype == torch.int32 and o['obs_row'].tolist() == sorted({av, 3})
    again = ses.observe(frame='agent', rows='controlled', neighbors=4, map_tokens=8)
    assert again['nbr_feat'].data_ptr() == o['nbr_feat'].data_ptr() and again['obs_row'].data_ptr() == o['obs_row'].data_ptr()
    # ... equals the operator on cloned engine buffers
    import infgen_amd.torch_ops  # noqa: F401
    from infgen_amd import constraints
    cl = lambda x: x.clone()
    op = torch.ops.infgen_hip.observe_rows(cl(eng.pos), cl(eng.head), cl(eng.state), cl(eng.n_agents), cl(eng.atype), cl(eng._shape10), col,
                                           constraints.STEP_SECONDS, cl(eng.map_pos), cl(eng.map_orient), cl(eng._map_cat[1]), cl(eng.n_map),
                                           eng.copies, cl(o['obs_row']), 4, None, 8, None)
    keys = ('self_feat', 'nbr_feat', 'nbr_index', 'nbr_count', 'map_feat', 'map_index', 'map_count')
    for k, v in zip(keys, op):
        assert torch.equal(o[k], v), k
    # ... and the restatement
    g = lambda x: x.cpu().numpy()
    case = dict(pos=g(eng.pos), head=g(eng.head), state=g(eng.state), n_agents=g(eng.n_agents), type=g(eng.atype), shape=g(eng._shape10),
                map_pos=g(eng.map_pos), map_orient=g(eng.map_orient), map_type=g(eng._map_cat[1]), n_map=g(eng.n_map), copies=eng.copies,
                c=col, dt=constraints.STEP_SECONDS, rows=g(o['obs_row']), K=4, radius=np.inf, Km=8, map_radius=np.inf)
    got = {k: g(o[k]) for k in keys}
    _check(got, R.evaluate(case), case['dt'], 'session')
    assert got['self_feat'][:, 0].all() and (got['nbr_index'] >= 0).any() and (got['map_index'] >= 0).all()
    allrows = ses.observe(frame='agent', rows='all', neighbors=2)
    assert allrows['self_feat'].shape == (eng.S * eng.A_cap, 8) and allrows['map_feat'].shape == (eng.S * eng.A_cap, 0, 6)
    assert torch.equal(allrows['self_feat'][o['obs_row'].long()], o['self_feat'])


def test_observing_changes_nothing():
    eng_a, ses_a, snap_a, seen = _session_run(True)
    eng_b, ses_b, snap_b, _ = _session_run(False)
    from test_replay_gpu import _same
    _same(snap_a, snap_b, 'a session that observes in the agent frame against one that does not')
    assert len(seen) == ses_a.steps and not torch.equal(seen[0]['self_feat'], seen[-1]['self_feat'])
