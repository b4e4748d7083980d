"""Snapshots ("snapshots" of include/infgen_hip.h): a rollout's decode state saved outside the engine and put back.

    snap = eng.snapshot(t)                 # every slot's state as of the boundary in front of decode step t, on the device
    eng.run(t, t + 4)                      # look ahead ...
    eng.restore(snap)                      # ... and be at step t again, bit for bit
    eng.restore(snap, index)               # slot s := entry index[s] (-1: keep); one entry may go to several slots of its group

A ``Snapshot`` is a device buffer of ENTRIES - one per saved slot, ``stride`` bytes each, holding what ``RolloutEngine.branch``
copies between slots (stored columns, the K / V rings, the pending raw feature, ``pred_*``, the logs of the steps that ran, the
step-score block) - plus one ``head`` row per entry, {slot, copy group, t, valid}, that the restore kernel checks.  An entry is
dominated by the rings: about ``2 * layers * ring * A_cap * 512`` bytes per slot.  Save fewer slots (``slots=``) or reuse one
buffer (``out=``) where a batch is large.  No function here reads the device."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib


class Snapshot:
    """``buf`` uint8 [capacity, stride] and ``head`` int32 [capacity, 4] on the device; ``n`` entries taken at decode step ``t``
    (``n == 0``: an empty buffer made by ``RolloutEngine.snapshot_buffer``); ``slots`` int32 [n] on the device, ``slots_host`` the
    same as a numpy array where the caller named them on the host (None after a device ``slots=``); ``signature`` / ``generation``:
    the engine layout and the batch the entries belong to (``restore`` refuses any other)."""

    def __init__(self, buf: torch.Tensor, head: torch.Tensor, signature, generation: int):
        self.buf, self.head, self.signature, self.generation = buf, head, signature, generation
        self.t, self.n, self.slots, self.slots_host = 0, 0, None, None

    @property
    def capacity(self) -> int:
        return int(self.buf.shape[0])

    @property
    def stride(self) -> int:
        return int(self.buf.shape[1])

    @property
    def nbytes(self) -> int:
        return self.buf.numel()


def signature(eng):
    """what has to agree between the engine a snapshot was taken from and the one it goes back to"""
    return (eng._snap_token, eng.S, eng.S0, eng.copies, eng.A_cap, eng.T, entry_bytes(eng, eng.cfg.num_decode_steps))


def entry_bytes(eng, t: int) -> int:
    """``infgen_snapshot_bytes`` of the engine's context: the bytes of one entry at decode step ``t`` (host only)"""
    n = C.c_longlong(0)
    _lib.check(eng.lib.infgen_snapshot_bytes(C.byref(eng._ctx), int(t), C.byref(n)), 'infgen_snapshot_bytes')
    return int(n.value)


def allocate(eng, n: int, t: Optional[int] = None) -> Snapshot:
    """an empty ``Snapshot`` of ``n`` entries with room for step ``t`` (None: for any step)"""
    stride = entry_bytes(eng, eng.cfg.num_decode_steps if t is None else t)
    buf = torch.empty(max(int(n), 1), stride, dtype=torch.uint8, device=eng.device)
    head = torch.zeros(max(int(n), 1), 4, dtype=torch.int32, device=eng.device)
    return Snapshot(buf, head, signature(eng), eng._reload_gen)


def check_slots(slots, S: int) -> np.ndarray:
    """a HOST list of slots -> int32 [n]; ValueError naming the first entry outside 0 .. S - 1"""
    s = np.asarray(slots)
    if s.size == 0:
        raise ValueError('slots names no slot')
    if s.dtype.kind not in 'iu':
        raise ValueError('slots holds integer slot indices')
    if s.ndim != 1:
        raise ValueError(f'slots: expected a list of slot indices, got shape {tuple(s.shape)}')
    if s.size > 65535:
        raise ValueError('slots: at most 65535 entries')
    for e, q in enumerate(s.tolist()):
        if not 0 <= q < S:
            raise ValueError(f'slots[{e}] = {q} is outside 0 .. {S - 1}')
    return s.astype(np.int32)


def check_index(index, S: int, n: int, copies: int, slots_host=None) -> np.ndarray:
    """a HOST restore index [S] (or [S0, copies]) -> int32 [S]; ValueError naming the first entry that is neither -1 nor an entry of
    the snapshot, or (where the saved slots are known on the host) an entry of another copy group"""
    x = np.asarray(index)
    if x.dtype.kind not in 'iu':
        raise ValueError('index holds integer entry indices')
    if x.shape not in ((S,), (S // max(copies, 1), copies)):
        raise ValueError(f'index: expected shape {(S,)}, got {tuple(x.shape)}')
    x = x.reshape(-1).astype(np.int64)
    for s in range(S):
        e = int(x[s])
        if e == -1:
            continue
        if not 0 <= e < n:
            raise ValueError(f'index[{s}] = {e} is neither -1 nor an entry 0 .. {n - 1}')
        if slots_host is not None and int(slots_host[e]) // copies != s // copies:
            raise ValueError(f'index[{s}] = {e} is the entry of slot {int(slots_host[e])}, a slot of another copy group '
                             f'(scene {int(slots_host[e]) // copies}, not {s // copies})')
    return x.astype(np.int32)


def identity_index(snap: Snapshot, S: int) -> torch.Tensor:
    """the index that puts every saved slot back onto itself, built on the device from the head: entries that are not valid (a
    slot out of range at the save) go nowhere"""
    head = snap.head[:snap.n]
    dev = head.device
    slot = torch.where(head[:, 3] != 0, head[:, 0], torch.full_like(head[:, 0], S)).clamp_(0, S).long()
    index = torch.full((S + 1,), -1, dtype=torch.int32, device=dev)
    index[slot] = torch.arange(snap.n, dtype=torch.int32, device=dev)
    return index[:S].contiguous()
