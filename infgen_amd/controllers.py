"""Rule-based controlled agents ("IDM commands" of include/infgen_hip.h): what ``torch.ops.infgen_hip.idm_command``,
``RolloutEngine.idm_command`` and ``ClosedLoopSession.command_idm`` share - the parameter checks (plain Python, no GPU), the output
buffers and the one call of ``infgen_idm_command``, whose scalar and host-array arguments are marshalled here."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Mapping, Optional

from . import _lib, constraints

TYPE_NAMES = ('veh', 'ped', 'cyc')
DEFAULTS = dict(dt=constraints.STEP_SECONDS, v0=(15.0, 1.5, 6.0), headway=1.5, s_min=2.0, a_max=1.5, b_comf=2.0, b_max=6.0,
                lateral=0.5, keep=0.5, types=('veh', 'cyc'), stop_at_end=True)


def _number(what, v):
    if isinstance(v, (bool, str)) or not isinstance(v, (int, float)) and not hasattr(v, '__float__'):
        raise ValueError(f'idm: {what} must be a number (got {v!r})')
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f'idm: {what} must be finite (got {v!r})')
    return v


def check_idm(params: Optional[Mapping] = None) -> Dict:
    """the IDM parameters as the library takes them -> dict(dt, v0 = (veh, ped, cyc) m/s, headway s, s_min m, a_max, b_comf, b_max
    m/s^2, lateral m, keep in [0, 1], types = (veh, ped, cyc) switches, stop_at_end 0 / 1).  ``params``: any of those keys (``types``
    as names or three switches); what is missing takes ``DEFAULTS``.  Everything the library refuses is a ``ValueError`` here."""
    params = {} if params is None else params
    if not isinstance(params, Mapping):
        raise ValueError('idm takes dict(dt=, v0=, headway=, s_min=, a_max=, b_comf=, b_max=, lateral=, keep=, types=, stop_at_end=)')
    unknown = set(params) - set(DEFAULTS)
    if unknown:
        raise ValueError(f'idm: unknown keys {sorted(unknown)} ({", ".join(DEFAULTS)})')
    p = dict(DEFAULTS)
    p.update(params)
    out = {}
    for key in ('dt', 'a_max', 'b_comf', 'b_max'):
        out[key] = _number(key, p[key])
        if out[key] <= 0:
            raise ValueError(f'idm: {key} must be > 0 (got {p[key]!r})')
    for key in ('headway', 's_min', 'lateral'):
        out[key] = _number(key, p[key])
        if out[key] < 0:
            raise ValueError(f'idm: {key} must be >= 0 (got {p[key]!r})')
    out['keep'] = _number('keep', p['keep'])
    if not 0 <= out['keep'] <= 1:
        raise ValueError(f'idm: keep must be in [0, 1] (got {p["keep"]!r})')
    v0 = p['v0']
    if isinstance(v0, (str, bytes)) or not hasattr(v0, '__len__') or len(v0) != 3:
        raise ValueError(f'idm: v0 has three entries, m/s for vehicles, pedestrians and cyclists (got {v0!r})')
    out['v0'] = tuple(_number('v0', v) for v in v0)
    if min(out['v0']) <= 0:
        raise ValueError(f'idm: every v0 must be > 0 (got {v0!r})')
    types = p['types']
    if isinstance(types, str) or not hasattr(types, '__len__'):
        raise ValueError(f"idm: types is a list of names from {TYPE_NAMES} or three switches (got {types!r})")
    if all(isinstance(t, str) for t in types):
        bad = [t for t in types if t not in TYPE_NAMES]
        if bad:
            raise ValueError(f'idm: unknown agent types {bad} ({", ".join(TYPE_NAMES)})')
        out['types'] = tuple(int(n in types) for n in TYPE_NAMES)
    elif len(types) == 3 and not any(isinstance(t, str) for t in types):
        out['types'] = tuple(int(bool(t)) for t in types)
    else:
        raise ValueError(f"idm: types is a list of names from {TYPE_NAMES} or three switches (got {types!r})")
    if isinstance(p['stop_at_end'], str) or p['stop_at_end'] not in (0, 1, False, True):
        raise ValueError(f'idm: stop_at_end is a switch (got {p["stop_at_end"]!r})')
    out['stop_at_end'] = int(bool(p['stop_at_end']))
    return out


def idm_buffers(S: int, A_cap: int, device, out: Optional[Dict] = None) -> Dict:
    """``state`` [S * A_cap, 8] float32 = s0, e0, v, gap, acc, v1, s1, flag and ``lead`` [S * A_cap] int32 - new ones, or those of
    an earlier result ``out`` (checked for shape, dtype and device)"""
    import torch
    want = dict(state=((S * A_cap, 8), torch.float32), lead=((S * A_cap,), torch.int32))
    if out is None:
        return {k: torch.zeros(shape, dtype=dt, device=device) for k, (shape, dt) in want.items()}
    res = {}
    for k, (shape, dt) in want.items():
        t = out.get(k)
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or t.device != torch.device(device) \
                or not t.is_contiguous():
            raise ValueError(f'idm: out[{k!r}] must be a contiguous {dt} tensor of shape {shape} on {device}')
        res[k] = t
    return res


def launch(lib, stream, pos, head, state, n_agents, type, shape, ctl_row, c, records, total, copies, v_des, conf, cmd_pose, out) -> None:
    """one ``infgen_idm_command`` that writes the ruled rows of ``cmd_pose`` and the tensors of ``out``; every tensor is what the
    library reads (contiguous, fp32 / int32, ``ctl_row`` uint8) - the callers see to that; ``conf``: a result of ``check_idm``"""
    P = _lib.ptr
    S, T, A = (int(v) for v in pos.shape[:3])
    _lib.check(lib.infgen_idm_command(
        P(pos), P(head), P(state), P(n_agents), P(type), P(shape), P(ctl_row), S, A, T, int(c), P(records), P(total),
        int(records.shape[2]) + 1, int(copies), P(v_des), conf['dt'], (C.c_float * 3)(*conf['v0']), conf['headway'], conf['s_min'],
        conf['a_max'], conf['b_comf'], conf['b_max'], conf['lateral'], conf['keep'], (C.c_int * 3)(*conf['types']),
        conf['stop_at_end'], P(cmd_pose), P(out['state']), P(out['lead']), stream), 'infgen_idm_command')
