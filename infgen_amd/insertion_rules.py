"""Insertion rules ("INSERTION RULES" of include/infgen_hip.h): where, what and how many agents the insertion
sub-loop may append.  ``InsertRules`` is the checked form of ``RolloutEngine(insert_rules=dict(...))``; the helpers build the device
tables and read the bit tables back.  Pure Python / torch: nothing here needs the library or a GPU, so every refusal is testable
on the host."""
from __future__ import annotations

import dataclasses
import math
from typing import Mapping, Optional, Tuple

import numpy as np
import torch

KEEPOUT, CLEARANCE, EDGES, LANES, ZONES = 1, 2, 4, 8, 16       # INFGEN_IM_* of include/infgen_hip.h
MAX_CELLS = 8192
MAX_PER_STEP = 10
TYPE_NAMES = ('veh', 'ped', 'cyc')
KEYS = ('clearance', 'ego_keepout', 'edge_clearance', 'near_lane', 'zones', 'types', 'max_agents', 'per_step')


def words_for(G: int) -> int:
    """32-bit words of one scene's cell set: ceil(G / 32) rounded up to a multiple of 4 (16-byte rows)"""
    return (int(G) + 127) // 128 * 4


def _distance(v, name):
    if isinstance(v, (bool, str)) or not np.isscalar(v) or not math.isfinite(v) or v < 0:
        raise ValueError(f'insert_rules: {name} must be a finite number of metres >= 0 (got {v!r})')
    return float(v)


def _types(types):
    """'veh' / 'ped' / 'cyc' names or three 0 / 1 switches -> (veh, ped, cyc) ints"""
    if isinstance(types, str):
        types = (types,)
    types = tuple(types)
    if types and all(isinstance(t, str) for t in types):
        unknown = set(types) - set(TYPE_NAMES)
        if unknown:
            raise ValueError(f'insert_rules: unknown agent types {sorted(unknown)} ({", ".join(TYPE_NAMES)})')
        out = tuple(int(n in types) for n in TYPE_NAMES)
    elif len(types) == 3 and all(t in (0, 1, False, True) for t in types):
        out = tuple(int(bool(t)) for t in types)
    else:
        raise ValueError(f'insert_rules: types takes names of {TYPE_NAMES} or three 0 / 1 switches (got {types!r})')
    if not any(out):
        raise ValueError('insert_rules: types must allow at least one agent type')
    return out


def check_zones(zones, n_zones=None, n_scenes: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """zones as (float32 [S0][Z][4] = (x, y, r, mode), int32 [S0]): one [Z][4] array is every scene's; n_zones None: all Z.  A zone
    with a radius that is not finite or <= 0 is void (the kernel skips it); a mode other than 0 / 1 is refused here."""
    z = np.asarray(zones, np.float32)
    if z.ndim == 2:
        z = np.broadcast_to(z[None], ((n_scenes or 1),) + z.shape)
    if z.ndim != 3 or z.shape[2] != 4:
        raise ValueError(f'insert_rules: zones must be [S0][Z][4] = (x, y, r, mode) (got shape {z.shape})')
    if n_scenes is not None and z.shape[0] != n_scenes:
        raise ValueError(f'insert_rules: zones cover {z.shape[0]} scenes, the engine has {n_scenes} distinct ones')
    n = np.full(z.shape[0], z.shape[1], np.int32) if n_zones is None else np.asarray(n_zones)
    if n.shape != (z.shape[0],) or n.dtype.kind not in 'iu' or (n < 0).any() or (n > z.shape[1]).any():
        raise ValueError('insert_rules: n_zones must be [S0] integers with 0 <= n_zones <= Z')
    if not np.isfinite(z[..., :2]).all():
        raise ValueError('insert_rules: zone centres must be finite')
    if not np.isin(z[..., 3], (0.0, 1.0)).all():
        raise ValueError('insert_rules: a zone\'s mode is 0 (ban inside) or 1 (allow only inside)')
    return np.ascontiguousarray(z, np.float32), n.astype(np.int32)


@dataclasses.dataclass(frozen=True)
class InsertRules:
    """the checked rule set.  None switches a rule off; ``types`` are (veh, ped, cyc) switches; ``max_agents`` None, an int or an
    int array [S]; ``zones`` (float32 [S0][Z][4], int32 [S0]) or None."""
    clearance: Optional[float] = None
    ego_keepout: Optional[Tuple[float, float, float]] = None
    edge_clearance: Optional[float] = None
    near_lane: Optional[Tuple[float, Tuple[int, ...]]] = None
    zones: Optional[Tuple[np.ndarray, np.ndarray]] = None
    types: Tuple[int, int, int] = (1, 1, 1)
    max_agents: Optional[np.ndarray] = None
    per_step: int = MAX_PER_STEP

    @classmethod
    def from_config(cls, conf, n_scenes: Optional[int] = None, n_slots: Optional[int] = None) -> Optional['InsertRules']:
        """``insert_rules`` as the engine takes it -> InsertRules, or None for None / False.  ``n_scenes``: distinct scenes the zone
        table must cover; ``n_slots``: scene slots a per-scene ``max_agents`` must cover.  Everything is checked here, before any
        launch."""
        if conf is None or conf is False:
            return None
        if isinstance(conf, cls):
            return conf
        if not isinstance(conf, Mapping):
            raise ValueError(f'insert_rules takes None or dict({", ".join(k + "=" for k in KEYS)})')
        unknown = set(conf) - set(KEYS)
        if unknown:
            raise ValueError(f'insert_rules: unknown keys {sorted(unknown)} ({", ".join(KEYS)})')
        kw = {}
        if conf.get('clearance') is not None:
            kw['clearance'] = _distance(conf['clearance'], 'clearance')
        if conf.get('edge_clearance') is not None:
            kw['edge_clearance'] = _distance(conf['edge_clearance'], 'edge_clearance')
        ko = conf.get('ego_keepout')
        if ko is not None:
            if isinstance(ko, str) or not hasattr(ko, '__len__') or len(ko) != 3:
                raise ValueError(f'insert_rules: ego_keepout takes (back, front, half_width) in metres (got {ko!r})')
            kw['ego_keepout'] = tuple(_distance(v, f'ego_keepout[{i}]') for i, v in enumerate(ko))
        nl = conf.get('near_lane')
        if nl is not None:
            if not isinstance(nl, Mapping) or set(nl) != {'dist', 'types'}:
                raise ValueError('insert_rules: near_lane takes dict(dist=, types=) with the map-token types that count as lanes')
            lt = tuple(nl['types']) if not np.isscalar(nl['types']) else (nl['types'],)
            if not lt or any(isinstance(t, (bool, str)) or int(t) != t or not 0 <= int(t) < 32 for t in lt):
                raise ValueError(f'insert_rules: near_lane types must be map-token types in 0..31 (got {nl["types"]!r})')
            kw['near_lane'] = (_distance(nl['dist'], 'near_lane dist'), tuple(sorted({int(t) for t in lt})))
        if conf.get('zones') is not None:
            zz = conf['zones']
            kw['zones'] = check_zones(*zz, n_scenes=n_scenes) if isinstance(zz, tuple) and len(zz) == 2 else check_zones(zz, None, n_scenes)
        if conf.get('types') is not None:
            kw['types'] = _types(conf['types'])
        ma = conf.get('max_agents')
        if ma is not None:
            a = np.asarray(ma)
            if a.dtype.kind not in 'iu' or a.ndim > 1 or (a < 0).any() or (a.ndim == 1 and n_slots is not None and a.shape[0] != n_slots):
                raise ValueError(f'insert_rules: max_agents takes an integer >= 0 or one per scene slot (got {ma!r})')
            kw['max_agents'] = a.astype(np.int32)
        ps = conf.get('per_step', MAX_PER_STEP)
        if isinstance(ps, bool) or not isinstance(ps, (int, np.integer)) or not 1 <= ps <= MAX_PER_STEP:
            raise ValueError(f'insert_rules: per_step must be an integer in 1..{MAX_PER_STEP} (got {ps!r})')
        kw['per_step'] = int(ps)
        return cls(**kw)

    @property
    def rule_bits(self) -> int:
        return (KEEPOUT * (self.ego_keepout is not None) | CLEARANCE * (self.clearance is not None)
                | EDGES * (self.edge_clearance is not None) | LANES * (self.near_lane is not None) | ZONES * (self.zones is not None))

    @property
    def lane_type_mask(self) -> int:
        return sum(1 << t for t in self.near_lane[1]) if self.near_lane is not None else 0


def device_tables(rules: InsertRules, S: int, S0: int, A_cap: int, G: int, steps: int, device='cpu'):
    """the device buffers of a rule set for S scene slots over S0 distinct scenes: ``allowed`` / ``static`` uint32-as-int32 [S][W],
    ``count`` / ``live`` int32 [S], ``count_log`` int32 [S][steps], ``shape`` float32 [S * A_cap][3], ``max_agents`` int32 [S] or
    None, ``zones`` float32 [S0][Z][4] / ``n_zones`` int32 [S0] or None"""
    if G < 1 or G > MAX_CELLS:
        raise ValueError(f'insert_rules: the grid has {G} cells, the cell masks take 1..{MAX_CELLS}')
    W = words_for(G)
    i32 = lambda *sh: torch.zeros(*sh, dtype=torch.int32, device=device)
    t = dict(W=W, allowed=i32(S, W), static=i32(S, W), count=i32(S), live=i32(S), count_log=i32(S, max(steps, 1)),
             shape=torch.zeros(S * A_cap, 3, device=device), max_agents=None, zones=None, n_zones=None)
    if rules.max_agents is not None:
        t['max_agents'] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(rules.max_agents, (S,)))).to(device)
    if rules.zones is not None:
        z, n = rules.zones
        if z.shape[0] != S0:
            raise ValueError(f'insert_rules: zones cover {z.shape[0]} scenes, the engine has {S0} distinct ones')
        t['zones'], t['n_zones'] = torch.from_numpy(z).to(device), torch.from_numpy(n).to(device)
    return t


def cells_allowed_to_indices(bits, G: int):
    """a bit table [..., W] (torch or numpy, int32 / uint32 words) -> for one set the sorted cell indices, for a stack of sets a
    list of them; bits at positions >= G are ignored"""
    w = bits.detach().cpu().numpy() if isinstance(bits, torch.Tensor) else np.asarray(bits)
    w = w.view(np.uint32) if w.dtype == np.int32 else w.astype(np.uint32)
    on = ((w[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool).reshape(w.shape[:-1] + (-1,))[..., :G]
    if on.ndim == 1:
        return np.nonzero(on)[0]
    return [np.nonzero(r)[0] for r in on.reshape(-1, on.shape[-1])]


def indices_to_cells_allowed(cells, G: int) -> np.ndarray:
    """sorted or unsorted cell indices -> one uint32 set of words_for(G) words"""
    on = np.zeros(32 * words_for(G), bool)
    c = np.asarray(cells, np.int64)
    if c.size and (c.min() < 0 or c.max() >= G):
        raise ValueError(f'cell indices must lie in 0..{G - 1}')
    on[c] = True
    return (on.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
