"""Constrained decoding: per-row allowed-token sets for the motion-token heads (the token mask of
include/infgen_hip.h).

A ``TokenMasks`` is a mask table: ``n_sets`` sets of ``token_size`` bits, bit ``c`` set = token ``c`` allowed, packed into
``token_size / 32`` little-endian uint32 words per set.  Which set a row takes is the caller's selection (per agent type, per row);
the table itself knows nothing about rows.  Everything here runs on the host at construction: the table is a few KB.
"""
from __future__ import annotations

from typing import Mapping, Optional, Sequence, Union

import numpy as np

TYPE_NAMES = ('veh', 'ped', 'cyc')        # the row types 0, 1, 2 (engine.py stacks the vocabulary in this order)
RULES = ('max_speed', 'min_speed', 'no_reverse', 'max_yaw_rate')
STEP_SECONDS = 0.5                        # one motion token spans 0.5 s (six contours, 0.1 s apart)


def pack_bits(allowed: np.ndarray) -> np.ndarray:
    """bool [n_sets][token_size] -> uint32 [n_sets][token_size / 32], bit c % 32 of word c / 32 = allowed[c]"""
    allowed = np.asarray(allowed)
    if allowed.ndim != 2 or allowed.dtype != np.bool_:
        raise ValueError('token masks are boolean arrays [n_sets][token_size]')
    if allowed.shape[1] == 0 or allowed.shape[1] % 32:
        raise ValueError(f'token masks: token_size {allowed.shape[1]} is not a positive multiple of 32')
    b = allowed.reshape(allowed.shape[0], -1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_bits(words: np.ndarray) -> np.ndarray:
    """the inverse of ``pack_bits``"""
    words = np.asarray(words, dtype=np.uint32)
    return ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.bool_).reshape(words.shape[0], -1)


def token_kinematics(vocab: Union[Mapping[str, np.ndarray], np.ndarray]):
    """the motion vocabulary -> (speed [3][token_size] m/s along the agent's heading, negative = backwards; |speed| [3][token_size];
    yaw rate [3][token_size] rad/s).  Per type and token the vocabulary holds six contours of four corners (front-left, front-right,
    rear-right, rear-left) in the agent frame; the last contour's centre is the displacement over the 0.5 s step and its heading
    (rear-left -> front-left) the yaw change"""
    v = np.stack([vocab[k] for k in TYPE_NAMES]) if isinstance(vocab, Mapping) else np.asarray(vocab)
    if v.ndim != 5 or v.shape[0] != 3 or v.shape[2:] != (6, 4, 2):
        raise ValueError(f'the motion vocabulary is [3][token_size][6][4][2], not {v.shape}')
    last = v[:, :, -1].astype(np.float64)                    # [3][token_size][4][2]
    centre = last.mean(axis=2)
    yaw = np.arctan2(last[:, :, 0, 1] - last[:, :, 3, 1], last[:, :, 0, 0] - last[:, :, 3, 0])
    return centre[..., 0] / STEP_SECONDS, np.hypot(centre[..., 0], centre[..., 1]) / STEP_SECONDS, yaw / STEP_SECONDS


class TokenMasks:
    """a mask table (see the module's text).  ``TokenMasks(allowed)`` takes boolean arrays [n_sets][token_size];
    ``TokenMasks.from_vocab(vocab, rules)`` derives one set per agent type from the motion vocabulary.  ``names[i]`` says what set i
    is (for error messages); ``type_sets`` is the per-type selection ``from_vocab`` produced ([-1, -1, -1] otherwise)"""

    def __init__(self, allowed, names: Optional[Sequence[str]] = None, type_sets: Sequence[int] = (-1, -1, -1)):
        allowed = np.asarray(allowed)
        if allowed.ndim == 1:
            allowed = allowed[None]
        self.words = pack_bits(allowed)                       # (raises on a wrong shape or width)
        self.n_sets, self.token_size = int(allowed.shape[0]), int(allowed.shape[1])
        self.names = [f'set {i}' for i in range(self.n_sets)] if names is None else list(names)
        if len(self.names) != self.n_sets:
            raise ValueError('token masks: one name per set')
        for i in np.flatnonzero(~allowed.any(axis=1)):
            raise ValueError(f'token masks: {self.names[i]} allows no token')
        self.type_sets = check_type_selectors(type_sets, self.n_sets)
        self._bits = {}

    @property
    def allowed(self) -> np.ndarray:
        return unpack_bits(self.words)

    @property
    def bits(self):
        """the packed table as a torch.uint32 tensor [n_sets][token_size / 32] (host memory)"""
        import torch
        return torch.from_numpy(self.words.view(np.int32).copy()).view(torch.uint32)

    def key(self):
        """a hashable identity of the table and its per-type selection (engine caches)"""
        return (self.n_sets, self.token_size, self.words.tobytes(), tuple(self.type_sets))

    @classmethod
    def from_vocab(cls, vocab, rules: Mapping) -> 'TokenMasks':
        """one set per constrained agent type.  ``rules`` maps rule names (``max_speed`` / ``min_speed`` in m/s on the displacement's
        length, ``no_reverse`` (bool: no token whose displacement points backwards), ``max_yaw_rate`` in rad/s on the yaw change's
        magnitude) to values for every type, or type names (``'veh'``, ``'ped'``, ``'cyc'``) to such rule mappings:
        ``{'max_speed': 15.0}``, ``{'veh': {'no_reverse': True}, 'ped': {'max_speed': 2.0}}``.  A type without rules gets no set
        (``type_sets`` -1).  A rule that leaves a type without a token raises ValueError naming both."""
        fwd, speed, yaw = token_kinematics(vocab)
        per_type = {t: {} for t in TYPE_NAMES}
        for k, val in rules.items():
            if k in TYPE_NAMES:
                if not isinstance(val, Mapping):
                    raise ValueError(f'token masks: rules[{k!r}] must map rule names to values')
                per_type[k].update(val)
            elif k in RULES:
                for t in TYPE_NAMES:
                    per_type[t].setdefault(k, val)
            else:
                raise ValueError(f'token masks: unknown rule or type {k!r} (rules: {", ".join(RULES)}; types: {", ".join(TYPE_NAMES)})')
        sets, names, type_sets = [], [], [-1, -1, -1]
        for ti, t in enumerate(TYPE_NAMES):
            if not per_type[t]:
                continue
            ok = np.ones(fwd.shape[1], dtype=np.bool_)
            for rule, val in per_type[t].items():
                if rule not in RULES:
                    raise ValueError(f'token masks: unknown rule {rule!r} for type {t!r}')
                if rule == 'max_speed':
                    ok &= speed[ti] <= float(val)
                elif rule == 'min_speed':
                    ok &= speed[ti] >= float(val)
                elif rule == 'no_reverse':
                    ok &= (fwd[ti] >= 0.0) | (not val)
                else:
                    ok &= np.abs(yaw[ti]) <= float(val)
                if not ok.any():
                    raise ValueError(f'token masks: no {t!r} token is left after rule {rule!r} = {val!r}')
            type_sets[ti] = len(sets)
            sets.append(ok)
            names.append(f'type {t!r} ({", ".join(per_type[t])})')
        if not sets:
            raise ValueError('token masks: no rule given')
        return cls(np.stack(sets), names, type_sets)


def check_type_selectors(sel, n_sets: int):
    """host-side per-type selection -> [int, int, int], each -1 (unconstrained) or a set of the table"""
    sel = [int(v) for v in sel]
    if len(sel) != 3:
        raise ValueError('token_mask_type takes three set indices (vehicle, pedestrian, cyclist; -1: unconstrained)')
    for v in sel:
        if v < -1 or v >= n_sets:
            raise ValueError(f'token_mask_type {v} is outside the table\'s {n_sets} sets (-1: unconstrained)')
    return sel


def check_row_selectors(sel: np.ndarray, n_sets: int) -> np.ndarray:
    """host-side per-row selection -> int32 array, each entry -1 (the row's type decides) or a set of the table"""
    sel = np.asarray(sel)
    if sel.dtype.kind not in 'iu':
        raise ValueError('token_mask_row holds integer set indices')
    if sel.size and (int(sel.min()) < -1 or int(sel.max()) >= n_sets):
        raise ValueError(f'token_mask_row has entries outside -1 .. {n_sets - 1}')
    return sel.astype(np.int32)


# ---------------------------------------------------------------------------------------- what the step riders' checks share
def _check_metres(what: str, key: str, v) -> float:
    if isinstance(v, (bool, str)) or not np.isscalar(v) or not np.isfinite(v) or v < 0:
        raise ValueError(f'{what}: {key} must be a finite number of metres >= 0 (got {v!r})')
    return float(v)


def _check_switch(what: str, key: str, v) -> int:
    if isinstance(v, str) or not np.isscalar(v) or v not in (0, 1, False, True):
        raise ValueError(f'{what}: {key} must be 0 or 1 (got {v!r})')
    return int(v)


def _check_within(what: str, key: str, v, lo, hi) -> float:
    if isinstance(v, (bool, str)) or not np.isscalar(v) or not lo <= v <= hi:
        raise ValueError(f'{what}: {key} must be a number in [{lo}, {hi}] (got {v!r})')
    return float(v)


def _row_buffers(what: str, rows: int, token_size: int, device):
    """every per-step mask kernel's own, ``rows`` = S * A_cap: ``bits`` [rows][token_size / 32] int32 (the sets of the step that just
    ran), ``allowed`` [rows] int32 (their sizes before the empty-set fallback), ``ident`` [rows] int32 (row i is set i), ``shape`` [rows][3]"""
    import torch
    if token_size % 32 or token_size > 4096:
        raise ValueError(f'{what}: token_size {token_size} must be a multiple of 32, at most 4096')
    return dict(bits=torch.full((rows, token_size // 32), -1, dtype=torch.int32, device=device),
                allowed=torch.full((rows,), token_size, dtype=torch.int32, device=device),
                ident=torch.arange(rows, dtype=torch.int32, device=device),
                shape=torch.zeros(rows, 3, dtype=torch.float32, device=device))


# ---------------------------------------------------------------------------------------- collision-aware decoding
def check_avoid_collisions(avoid, has_shape: bool = True):
    """``avoid_collisions`` as the engine takes it -> None (off) or dict(margin=float, predict=0 | 1).  False / None: off; True: the
    defaults (margin 0 m, constant-velocity obstacles); a mapping with the keys ``margin`` (metres, finite, >= 0) and / or ``predict``
    (0 or 1 / False or True).  Everything is checked here, on the host, before any launch."""
    if avoid is None or avoid is False:
        return None
    if avoid is True:
        avoid = {}
    if not isinstance(avoid, Mapping):
        raise ValueError('avoid_collisions takes False, True or dict(margin=, predict=)')
    unknown = set(avoid) - {'margin', 'predict'}
    if unknown:
        raise ValueError(f'avoid_collisions: unknown keys {sorted(unknown)} (margin, predict)')
    margin = _check_metres('avoid_collisions', 'margin', avoid.get('margin', 0.0))
    predict = _check_switch('avoid_collisions', 'predict', avoid.get('predict', 1))
    if not has_shape:
        raise ValueError('avoid_collisions needs the rows\' shapes: this engine has no shape array')
    return dict(margin=margin, predict=predict)


def collision_key(conf):
    """the hashable form of a checked avoid_collisions configuration: both of its values are launch arguments"""
    return None if conf is None else (conf['margin'], conf['predict'])


def collision_buffers(conf, rows: int, token_size: int, device='cpu'):
    """the static buffers of collision-aware decoding for ``rows`` = S * A_cap rows, or None when ``conf`` (``check_avoid_collisions``)
    is off: the four of ``_row_buffers`` - ``bits``, ``allowed``, ``ident``, ``shape``"""
    return None if conf is None else _row_buffers('avoid_collisions', rows, token_size, device)


# ---------------------------------------------------------------------------------------- road-aware decoding
ROAD_DETAILS = (1, 2, 5, 10)              # chords per EDGE map token: the polyline's points 0, 10 / detail, ..., 10


def _road_types(types, what: str = 'stay_on_road') -> tuple:
    """``types`` of stay_on_road -> the three-entry switch (vehicle, pedestrian, cyclist) of 0 / 1"""
    if isinstance(types, (str, bytes)) or not isinstance(types, (Sequence, set, frozenset, np.ndarray)):
        raise ValueError(f'{what}: types is a collection of agent types, names {TYPE_NAMES} or 0 .. 2 (got {types!r})')
    on = [0, 0, 0]
    for t in types:
        if isinstance(t, str) and t in TYPE_NAMES:
            on[TYPE_NAMES.index(t)] = 1
        elif not isinstance(t, (bool, str)) and np.isscalar(t) and t in (0, 1, 2):
            on[int(t)] = 1
        else:
            raise ValueError(f'{what}: unknown agent type {t!r} (names {TYPE_NAMES} or 0 .. 2)')
    return tuple(on)


def _road_segments(segments, what: str = 'stay_on_road'):
    """``segments`` of stay_on_road -> (float32 [S0][E][4], int32 [S0]): an array [S0][E][4] (every segment used) or one array
    [E_s][4] = (x0, y0, x1, y1) per distinct scene, world coordinates.  Non-finite and zero-length segments are allowed: the
    definition makes them no obstacle"""
    if isinstance(segments, np.ndarray) and segments.ndim == 3:
        segments = list(segments)
    if isinstance(segments, (str, bytes)) or not isinstance(segments, Sequence) or len(segments) == 0:
        raise ValueError(f'{what}: segments is an array [S0][E][4] or one array [E][4] per distinct scene')
    per = []
    for s, seg in enumerate(segments):
        a = np.asarray(seg)
        if a.size == 0:
            a = np.zeros((0, 4), np.float32)
        if a.ndim != 2 or a.shape[1] != 4 or a.dtype.kind not in 'fiu':
            raise ValueError(f'{what}: segments[{s}] must be numbers [E][4] = (x0, y0, x1, y1), got shape {a.shape}')
        per.append(a.astype(np.float32))
    E = max(1, max(a.shape[0] for a in per))
    out = np.zeros((len(per), E, 4), np.float32)
    for s, a in enumerate(per):
        out[s, :a.shape[0]] = a
    return out, np.array([a.shape[0] for a in per], np.int32)


def check_stay_on_road(stay, has_shape: bool = True, n_scenes: Optional[int] = None, what: str = 'stay_on_road',
                       margin_key: str = 'margin'):
    """``stay_on_road`` as the engine takes it -> None (off) or dict(margin=float, sweep=0 | 1, detail=1 | 2 | 5 | 10, types=(veh, ped,
    cyc) switches, segments=None | (float32 [S0][E][4], int32 [S0])).  False / None: off; True: the defaults (margin 0 m, the path
    rectangle on, two chords per EDGE map token, vehicles and cyclists, segments from the map); a mapping with any of those keys.
    ``what`` / ``margin_key``: the argument's name in the messages and the key the margin comes under (``check_step_scores``).
    ``n_scenes``: the number of distinct scenes explicit segments must cover.  Everything is checked here, on the host, before any
    launch."""
    if stay is None or stay is False:
        return None
    if stay is True:
        stay = {}
    if not isinstance(stay, Mapping):
        raise ValueError(f'{what} takes False, True or dict({margin_key}=, sweep=, detail=, types=, segments=)')
    unknown = set(stay) - {margin_key, 'sweep', 'detail', 'types', 'segments'}
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)} ({margin_key}, sweep, detail, types, segments)')
    margin = _check_metres(what, margin_key, stay.get(margin_key, 0.0))
    sweep, detail = _check_switch(what, 'sweep', stay.get('sweep', 1)), stay.get('detail', 2)
    if isinstance(detail, (bool, str)) or not np.isscalar(detail) or detail not in ROAD_DETAILS:
        raise ValueError(f'{what}: detail must be one of {ROAD_DETAILS} (got {detail!r})')
    types = _road_types(stay.get('types', ('veh', 'cyc')), what)
    segments = stay.get('segments')
    if segments is not None:
        if isinstance(segments, tuple) and len(segments) == 2 and np.asarray(segments[1]).ndim == 1 and np.asarray(segments[0]).ndim == 3:
            seg, n = np.ascontiguousarray(segments[0], np.float32), np.asarray(segments[1])      # (a value this function returned)
            if seg.shape[2] != 4 or n.shape[0] != seg.shape[0] or n.dtype.kind not in 'iu' or (n < 0).any() or (n > seg.shape[1]).any():
                raise ValueError(f'{what}: segments as (array [S0][E][4], counts [S0]) with 0 <= counts <= E')
            segments = (seg, n.astype(np.int32))
        else:
            segments = _road_segments(segments, what)
        if n_scenes is not None and segments[0].shape[0] != n_scenes:
            raise ValueError(f'{what}: segments cover {segments[0].shape[0]} scenes, the batch has {n_scenes} distinct scenes')
    if not has_shape:
        raise ValueError(f'{what} needs the rows\' shapes: this engine has no shape array')
    return dict(margin=margin, sweep=sweep, detail=int(detail), types=types, segments=segments)


def road_key(conf):
    """the hashable part of a checked configuration that decides the launches' arguments (the segments are contents)"""
    return None if conf is None else (conf['margin'], conf['sweep'], conf['detail'], conf['types'], conf['segments'] is not None)


def road_buffers(conf, rows: int, token_size: int, device='cpu'):
    """the static per-row buffers of road-aware decoding for ``rows`` = S * A_cap rows, or None when ``conf`` (``check_stay_on_road``)
    is off: the four of ``collision_buffers`` - ``bits``, ``allowed``, ``ident``, ``shape`` - for the road kernel's own sets.  (The
    record table is the engine's: it is sized from a count of the map's EDGE tokens.)"""
    return None if conf is None else _row_buffers('stay_on_road', rows, token_size, device)


# ---------------------------------------------------------------------------------------- step scores
def check_step_scores(scores, has_shape: bool = True, n_scenes: Optional[int] = None, stay_on_road=None):
    """``step_scores`` as the engine takes it -> None (off) or dict(road_margin=float, sweep=0 | 1, types=(veh, ped, cyc) switches,
    detail=1 | 2 | 5 | 10, segments=None | (float32 [S0][E][4], int32 [S0]), dt=float).  False / None: off; True: the defaults
    (margin 0 m, the path rectangle on, vehicles and cyclists, two chords per EDGE map token, segments from the map, 0.5 s per
    step); a mapping with any of those keys.  ``stay_on_road``: the engine's CHECKED road configuration (``check_stay_on_road``) or
    None - the engine keeps one road table, so with road-aware decoding on the scores read that table: ``detail`` / ``segments``
    left out are taken from it, and ones that differ from it raise.  Everything is checked here, on the host, before any launch."""
    if scores is None or scores is False:
        return None
    if scores is True:
        scores = {}
    if not isinstance(scores, Mapping):
        raise ValueError('step_scores takes False, True or dict(road_margin=, sweep=, types=, detail=, segments=, dt=)')
    unknown = set(scores) - {'road_margin', 'sweep', 'types', 'detail', 'segments', 'dt'}
    if unknown:
        raise ValueError(f'step_scores: unknown keys {sorted(unknown)} (road_margin, sweep, types, detail, segments, dt)')
    dt = scores.get('dt', STEP_SECONDS)
    if isinstance(dt, (bool, str)) or not np.isscalar(dt) or not np.isfinite(dt) or dt <= 0:
        raise ValueError(f'step_scores: dt must be a finite number of seconds > 0 (got {dt!r})')
    road = dict(road_margin=scores.get('road_margin', 0.0), sweep=scores.get('sweep', 1), types=scores.get('types', ('veh', 'cyc')))
    for k in ('detail', 'segments'):
        if scores.get(k) is not None:
            road[k] = scores[k]
        elif stay_on_road is not None:
            road[k] = stay_on_road[k]
    road = check_stay_on_road(road, has_shape=has_shape, n_scenes=n_scenes, what='step_scores', margin_key='road_margin')
    if stay_on_road is not None:
        if road['detail'] != stay_on_road['detail']:
            raise ValueError(f'step_scores: detail {road["detail"]} conflicts with stay_on_road\'s {stay_on_road["detail"]}: the engine '
                             'keeps one road table')
        a, b = road['segments'], stay_on_road['segments']
        if (a is None) != (b is None) or (a is not None and not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))):
            raise ValueError('step_scores: segments conflict with stay_on_road\'s: the engine keeps one road table')
    return dict(road_margin=road['margin'], sweep=road['sweep'], types=road['types'], detail=road['detail'], segments=road['segments'],
                dt=float(dt))


def score_key(conf):
    """the hashable part of a checked step_scores configuration that decides the launches' arguments"""
    return None if conf is None else (conf['road_margin'], conf['sweep'], conf['types'], conf['detail'], conf['segments'] is not None,
                                      conf['dt'])


# ---------------------------------------------------------------------------------------- route-following decoding
ROUTE_MAX_POINTS = 32                     # RT_MAX_POINTS of csrc/kernels.h


def route_arrays(routes, n_points, n_scenes: Optional[int] = None, a_cap: Optional[int] = None, what: str = 'follow_routes'):
    """``routes`` [S0][A][P][2] world-coordinate waypoints and ``n_points`` [S0][A] as the engine takes them -> (float32, int32)
    arrays, checked: 2 <= P <= 32, 0 <= n_points <= P, one entry per distinct scene, A within the engine's rows.  Non-finite and
    repeated waypoints are allowed: the definition makes their segments dead"""
    r, n = np.asarray(routes), np.asarray(n_points)
    if r.ndim != 4 or r.shape[3] != 2 or r.dtype.kind not in 'fiu':
        raise ValueError(f'{what}: routes are numbers [S0][A][P][2], got shape {r.shape}')
    if not 2 <= r.shape[2] <= ROUTE_MAX_POINTS:
        raise ValueError(f'{what}: P = {r.shape[2]} waypoints per route, must be 2 .. {ROUTE_MAX_POINTS} (window longer paths)')
    if n.shape != r.shape[:2] or n.dtype.kind not in 'iu':
        raise ValueError(f'{what}: n_points holds integers [S0][A] = {r.shape[:2]}, got shape {n.shape}')
    if n.size and (int(n.min()) < 0 or int(n.max()) > r.shape[2]):
        raise ValueError(f'{what}: n_points has entries outside 0 .. P = {r.shape[2]}')
    if n_scenes is not None and r.shape[0] != n_scenes:
        raise ValueError(f'{what}: routes cover {r.shape[0]} scenes, the batch has {n_scenes} distinct scenes')
    if a_cap is not None and r.shape[1] > a_cap:
        raise ValueError(f'{what}: routes for {r.shape[1]} rows, the engine has {a_cap} per scene')
    return np.ascontiguousarray(r, np.float32), np.ascontiguousarray(n, np.int32)


def check_follow_routes(follow, n_scenes: Optional[int] = None, a_cap: Optional[int] = None):
    """``follow_routes`` as the engine takes it -> None (off) or dict(routes=float32 [S0][A][P][2], n_points=int32 [S0][A],
    corridor=, back=, pace=, finish= floats, types=(veh, ped, cyc) switches).  False / None: off; a mapping with ``routes`` and
    ``n_points`` and any of ``corridor`` (2 m), ``back`` (0.5 m), ``pace`` (0: off), ``finish`` (1 m), ``types`` (vehicles and
    cyclists).  Everything is checked here, on the host, before any launch."""
    if follow is None or follow is False:
        return None
    what = 'follow_routes'
    if not isinstance(follow, Mapping):
        raise ValueError(f'{what} takes False or dict(routes=, n_points=, corridor=, back=, pace=, finish=, types=)')
    unknown = set(follow) - {'routes', 'n_points', 'corridor', 'back', 'pace', 'finish', 'types'}
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)} (routes, n_points, corridor, back, pace, finish, types)')
    if follow.get('routes') is None or follow.get('n_points') is None:
        raise ValueError(f'{what} needs routes [S0][A][P][2] and n_points [S0][A]')
    out = {}
    for key, dflt in (('corridor', 2.0), ('back', 0.5), ('finish', 1.0)):
        out[key] = _check_metres(what, key, follow.get(key, dflt))
    out['pace'] = _check_within(what, 'pace', follow.get('pace', 0.0), 0, 1)
    out['types'] = _road_types(follow.get('types', ('veh', 'cyc')), what)
    out['routes'], out['n_points'] = route_arrays(follow['routes'], follow['n_points'], n_scenes, a_cap, what)
    return out


def route_key(conf):
    """the hashable part of a checked follow_routes configuration that decides the launches' arguments (the routes are contents)"""
    return None if conf is None else (conf['corridor'], conf['back'], conf['pace'], conf['finish'], conf['types'])


def route_buffers(n_scenes: int, rows: int, a_cap: int, P: int, token_size: int, device='cpu'):
    """the static buffers of route-following decoding: the four of ``collision_buffers`` - ``bits``, ``allowed``, ``ident``,
    ``shape`` (the row skeleton reads it, the rule does not: it stays zero) -, ``progress`` [rows][4], and per distinct scene
    ``routes`` [S0][A_cap][P][2], ``n_points`` [S0][A_cap], ``records`` [S0][A_cap][P - 1][8], ``total`` [S0][A_cap]"""
    import torch
    k = _row_buffers('follow_routes', rows, token_size, device)
    k.update(P=P, progress=torch.zeros(rows, 4, device=device), routes=torch.zeros(n_scenes, a_cap, P, 2, device=device),
             n_points=torch.zeros(n_scenes, a_cap, dtype=torch.int32, device=device),
             records=torch.zeros(n_scenes, a_cap, P - 1, 8, device=device), total=torch.zeros(n_scenes, a_cap, device=device))
    return k


# ---------------------------------------------------------------------------------------- signal-aware decoding
SIGNAL_MAX_LINES = 64                     # SG_MAX_LINES of csrc/kernels.h
LIGHT_STOP, LIGHT_GO, LIGHT_CAUTION, LIGHT_UNKNOWN = 0, 1, 2, 3      # map_polygon.light_type


def signal_lines(lines, n_lines=None, n_scenes: Optional[int] = None, what: str = 'obey_signals'):
    """``lines`` [S0][K][4] = (ax, ay, bx, by) world coordinates - a the left and b the right end as the traffic the line stops sees
    them - and ``n_lines`` [S0] (None: every line) -> (float32, int32) arrays, checked: 1 <= K <= 64, 0 <= n_lines <= K, one entry
    per distinct scene.  Non-finite and zero-length lines are allowed: the definition makes their records dead"""
    a = np.asarray(lines)
    if a.ndim != 3 or a.shape[2] != 4 or a.dtype.kind not in 'fiu':
        raise ValueError(f'{what}: lines are numbers [S0][K][4] = (ax, ay, bx, by), got shape {a.shape}')
    if not 1 <= a.shape[1] <= SIGNAL_MAX_LINES:
        raise ValueError(f'{what}: K = {a.shape[1]} lines per scene, must be 1 .. {SIGNAL_MAX_LINES}')
    n = np.full(a.shape[0], a.shape[1], np.int32) if n_lines is None else np.asarray(n_lines)
    if n.shape != a.shape[:1] or n.dtype.kind not in 'iu':
        raise ValueError(f'{what}: n_lines holds integers [S0] = {a.shape[:1]}, got shape {n.shape}')
    if n.size and (int(n.min()) < 0 or int(n.max()) > a.shape[1]):
        raise ValueError(f'{what}: n_lines has entries outside 0 .. K = {a.shape[1]}')
    if n_scenes is not None and a.shape[0] != n_scenes:
        raise ValueError(f'{what}: lines cover {a.shape[0]} scenes, the batch has {n_scenes} distinct scenes')
    return np.ascontiguousarray(a, np.float32), np.ascontiguousarray(n, np.int32)


def signal_phase_table(phase, n_scenes: int, K: int, what: str = 'obey_signals'):
    """``phase`` [S0][n_phase][K] (or [S0][K]: one row) -> uint8, non-zero = closed; checked against the lines' [S0][K]"""
    p = np.asarray(phase)
    if p.ndim == 2:
        p = p[:, None]
    if p.ndim != 3 or p.dtype.kind not in 'biu' or p.shape[1] < 1:
        raise ValueError(f'{what}: phase holds bytes [S0][n_phase >= 1][K] (non-zero: closed), got shape {p.shape} of {p.dtype}')
    if p.shape[0] != n_scenes or p.shape[2] != K:
        raise ValueError(f'{what}: phase {p.shape} does not fit the lines\' [S0 = {n_scenes}][n_phase][K = {K}]')
    return np.ascontiguousarray(p != 0, np.uint8)


def check_obey_signals(obey, has_shape: bool = True, n_scenes: Optional[int] = None):
    """``obey_signals`` as the engine takes it -> None (off) or dict(lines=float32 [S0][K][4], n_lines=int32 [S0], phase=uint8
    [S0][n_phase][K], setback=, align= floats, types=(veh, ped, cyc) switches).  False / None: off; a mapping with ``lines`` and
    ``phase`` and any of ``n_lines`` (every line), ``setback`` (0.5 m), ``align`` (0.5: the cosine a row's heading must make with a
    line's direction of travel to be stopped by it), ``types`` (vehicles and cyclists).  Everything is checked here, on the host,
    before any launch."""
    if obey is None or obey is False:
        return None
    what = 'obey_signals'
    if not isinstance(obey, Mapping):
        raise ValueError(f'{what} takes False or dict(lines=, n_lines=, phase=, setback=, align=, types=)')
    unknown = set(obey) - {'lines', 'n_lines', 'phase', 'setback', 'align', 'types'}
    if unknown:
        raise ValueError(f'{what}: unknown keys {sorted(unknown)} (lines, n_lines, phase, setback, align, types)')
    if obey.get('lines') is None or obey.get('phase') is None:
        raise ValueError(f'{what} needs lines [S0][K][4] and phase [S0][n_phase][K]')
    setback = _check_metres(what, 'setback', obey.get('setback', 0.5))
    align = _check_within(what, 'align', obey.get('align', 0.5), -1, 1)
    out = dict(setback=setback, align=align, types=_road_types(obey.get('types', ('veh', 'cyc')), what))
    out['lines'], out['n_lines'] = signal_lines(obey['lines'], obey.get('n_lines'), n_scenes, what)
    out['phase'] = signal_phase_table(obey['phase'], out['lines'].shape[0], out['lines'].shape[1], what)
    if not has_shape:
        raise ValueError(f'{what} needs the rows\' shapes: this engine has no shape array')
    return out


def signal_key(conf):
    """the hashable part of a checked obey_signals configuration that decides the launches' arguments (lines and phase bytes are
    contents; the table's extents K and n_phase are arguments - an engine keeps them in place of the arrays it has uploaded)"""
    if conf is None:
        return None
    K = conf['K'] if 'K' in conf else int(conf['lines'].shape[1])
    n_phase = conf['n_phase'] if 'n_phase' in conf else int(conf['phase'].shape[1])
    return (conf['setback'], conf['align'], conf['types'], K, n_phase)


def signal_buffers(n_scenes: int, rows: int, K: int, n_phase: int, token_size: int, device='cpu'):
    """the static buffers of signal-aware decoding: the four of ``collision_buffers`` - ``bits``, ``allowed``, ``ident``, ``shape`` -,
    ``info`` [rows][4], and per distinct scene ``lines`` [S0][K][4], ``n_lines`` [S0], ``records`` [S0][K][8], ``phase``
    [S0][n_phase][K] bytes"""
    import torch
    k = _row_buffers('obey_signals', rows, token_size, device)
    info = torch.zeros(rows, 4, device=device)
    info[:, 1] = -1.0
    k.update(K=K, n_phase=n_phase, info=info, lines=torch.zeros(n_scenes, K, 4, device=device),
             n_lines=torch.zeros(n_scenes, dtype=torch.int32, device=device), records=torch.zeros(n_scenes, K, 8, device=device),
             phase=torch.zeros(n_scenes, n_phase, K, dtype=torch.uint8, device=device))
    return k


def signal_phase(n_lines: int, period: int, red_from, red_to, offset=0):
    """a cyclic phase table [period][n_lines] (uint8, 1 = closed) from per-line schedules: line j is closed at the steps t with
    red_from[j] <= (t + offset[j]) mod period < red_to[j]; red_from > red_to wraps around the cycle's end, red_from == red_to is
    never closed.  ``red_from`` / ``red_to`` / ``offset``: scalars or [n_lines] integers in 0 .. period.  numpy, host only; stack one
    table per distinct scene for ``obey_signals['phase']``."""
    if n_lines < 1 or period < 1:
        raise ValueError('signal_phase: n_lines and period must be at least 1')
    lo, hi, off = (np.broadcast_to(np.asarray(v), (n_lines,)) for v in (red_from, red_to, offset))
    if any(v.dtype.kind not in 'iu' for v in (lo, hi, off)):
        raise ValueError('signal_phase: red_from, red_to and offset are integers (decode steps)')
    if (lo < 0).any() or (lo > period).any() or (hi < 0).any() or (hi > period).any():
        raise ValueError(f'signal_phase: red_from and red_to must lie in 0 .. period = {period}')
    at = (np.arange(period)[:, None] + off[None]) % period
    plain = (at >= lo[None]) & (at < hi[None])
    wrapped = (at >= lo[None]) | (at < hi[None])
    return np.where((lo <= hi)[None], plain, wrapped).astype(np.uint8)


def stop_lines_from_map(data_or_staged, states=(LIGHT_STOP,), half_width: float = 1.8):
    """one stop line per map polygon whose ``light_type`` is in ``states`` (WOMD codes: 0 STOP, 1 GO, 2 CAUTION, 3 unknown - the caller
    decides which close a line).  ``data_or_staged``: a scene (``map_polygon.light_type`` [P], ``pt_token.position`` [M][>= 2],
    ``pt_token.orientation`` [M] and ``pt_token__to__map_polygon`` - or ``('pt_token', 'to', 'map_polygon')`` - ``['edge_index']`` [2][M],
    map token -> polygon) or a sequence of scenes.  The
    line is centred on the polygon's FIRST map token - the smallest token index mapped to it -, perpendicular to that token's
    orientation, and spans +- ``half_width`` metres: a = centre + half_width * left, b = centre - half_width * left.
    -> lines float32 [S][K][4], n_lines int32 [S], phase uint8 [S][1][K] with those lines closed (K: the largest scene's count, at
    least 1; more than 64 raises).  Pure host code."""
    if not np.isscalar(half_width) or not np.isfinite(half_width) or half_width <= 0:
        raise ValueError('stop_lines_from_map: half_width must be a finite number of metres > 0')
    datas = [data_or_staged] if isinstance(data_or_staged, Mapping) else list(data_or_staged)
    per = []
    for d in datas:
        light = np.asarray(d['map_polygon']['light_type']).reshape(-1)
        pos = np.asarray(d['pt_token']['position'], np.float64)[:, :2]
        ori = np.asarray(d['pt_token']['orientation'], np.float64).reshape(-1)
        key = ('pt_token', 'to', 'map_polygon')
        edge = np.asarray(d[key if key in d else 'pt_token__to__map_polygon']['edge_index'])
        first = {}
        for tok, poly in zip(edge[0].tolist(), edge[1].tolist()):
            first[poly] = min(tok, first.get(poly, tok))
        out = []
        for poly in range(light.shape[0]):
            if int(light[poly]) in states and poly in first:
                m, th = pos[first[poly]], ori[first[poly]]
                left = np.array([-np.sin(th), np.cos(th)])
                out.append(np.concatenate([m + half_width * left, m - half_width * left]))
        per.append(np.array(out, np.float64).reshape(-1, 4))
    K = max(1, max(a.shape[0] for a in per))
    if K > SIGNAL_MAX_LINES:
        raise ValueError(f'stop_lines_from_map: a scene has {K} such polygons, more than {SIGNAL_MAX_LINES} lines (choose among them)')
    lines, n_lines = np.zeros((len(per), K, 4), np.float32), np.zeros(len(per), np.int32)
    phase = np.zeros((len(per), 1, K), np.uint8)
    for s, a in enumerate(per):
        lines[s, :a.shape[0]], n_lines[s], phase[s, 0, :a.shape[0]] = a, a.shape[0], 1
    return lines, n_lines, phase


def routes_from_logged(data_or_staged, stride: int = 1, start: int = 0, points: int = ROUTE_MAX_POINTS):
    """every agent's logged positions as its route: "follow your own log".  ``data_or_staged``: a scene (its ``agent`` holds
    ``token_pos`` [A][T0][2] and ``state_idx`` [A][T0]), a sequence of scenes, or a mapping of stacked ``token_pos`` [S][A][T0][2] /
    ``state_idx`` [S][A][T0].  From column ``start`` on every ``stride``-th column where the agent is valid (state != 0) is a
    waypoint; a point equal to the one before it is dropped, and the route is cut after ``points`` waypoints.
    -> routes float32 [S][A][points][2], n_points int32 [S][A] (A: the largest scene's rows).  Pure host code."""
    if stride < 1 or start < 0 or not 2 <= points <= ROUTE_MAX_POINTS:
        raise ValueError(f'routes_from_logged: stride >= 1, start >= 0 and 2 <= points <= {ROUTE_MAX_POINTS}')
    if isinstance(data_or_staged, Mapping) and 'token_pos' in data_or_staged:
        pos, st = np.asarray(data_or_staged['token_pos']), np.asarray(data_or_staged['state_idx'])
        scenes = [(pos[s], st[s]) for s in range(pos.shape[0])]
    else:
        datas = [data_or_staged] if isinstance(data_or_staged, Mapping) else list(data_or_staged)
        scenes = [(np.asarray(d['agent']['token_pos']), np.asarray(d['agent']['state_idx'])) for d in datas]
    A = max(p.shape[0] for p, _ in scenes)
    routes, n_points = np.zeros((len(scenes), A, points, 2), np.float32), np.zeros((len(scenes), A), np.int32)
    for s, (pos, st) in enumerate(scenes):
        for i in range(pos.shape[0]):
            n = 0
            for col in range(start, pos.shape[1], stride):
                p = pos[i, col, :2].astype(np.float32)
                if st[i, col] == 0 or n == points or (n and np.array_equal(p, routes[s, i, n - 1])):
                    continue
                routes[s, i, n] = p
                n += 1
            n_points[s, i] = n
    return routes, n_points
