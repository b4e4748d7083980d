"""CPU: snapshots ("snapshots" of include/infgen_hip.h) - infgen_snapshot_bytes against the layout restated in
tests/snapshot_ref.py, the host-side argument checks of RolloutEngine.snapshot / restore, the refusals of the two entries that launch
nothing, and the prototypes in the header and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import snapshot_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, W, RING, R, TS, L = 10, 4, 5, 5, 96, 3
STEPS = T - 2


def _bytes(lib, r, t):
    """infgen_snapshot_bytes: the entry's bytes, or the negative code"""
    n = C.c_longlong(-1)
    rc = lib.infgen_snapshot_bytes(C.byref(r), t, C.byref(n))
    return rc if rc else n.value


def _context(A_cap, logits=True, S=6):
    """an InfgenRollout whose pointers are made-up addresses: the entries under test here never dereference them"""
    from infgen_amd import _lib
    r = _lib.Rollout()
    r.S, r.A_cap, r.T, r.W, r.ring, r.R, r.token_size, r.num_layers = S, A_cap, T, W, RING, R, TS, L
    addr = 0x10000
    for name in ref.SCENE_ARRAYS + ('bos', 'X', 'pred_traj', 'pred_head', 'pred_state', 'token_logprob', 'sample_logprob'):
        setattr(r, name, addr)
        addr += 0x10000
    for l in range(L):
        r.ringK[l], r.ringV[l] = addr, addr + 0x10000
        addr += 0x20000
    if logits:
        r.logits, r.store_logits = addr, 1
    else:
        r.logits_scratch = addr
    return r


@pytest.mark.parametrize('A_cap', (32, 96))
@pytest.mark.parametrize('logits', (True, False))
def test_snapshot_bytes_equals_the_restated_layout_and_is_monotone(A_cap, logits):
    from infgen_amd import _lib
    lib = _lib.load()
    r = _context(A_cap, logits)
    got = {}
    for t in (0, 3, STEPS):
        got[t] = _bytes(lib, r, t)
        assert got[t] == ref.entry_bytes(A_cap, T, RING, L, R, TS, t, logits=logits), t
        assert got[t] % 16 == 0
    every = [_bytes(lib, r, t) for t in range(STEPS + 1)]
    assert all(a < b for a, b in zip(every, every[1:])), 'monotone in t: the logs grow by one block per step'
    # the rings dominate: 2 * layers * ring * A_cap * 512 bytes
    assert got[0] > 2 * L * RING * A_cap * 512 > got[0] // 2
    # absent buffers take no room
    r.token_logprob = r.sample_logprob = None
    assert _bytes(lib, r, 3) == ref.entry_bytes(A_cap, T, RING, L, R, TS, 3, logits=logits, token_logprob=False,
                                                                         sample_logprob=False)
    # a block that is no multiple of 16 is padded to the boundary (the library's own layouts never are: validate wants A_cap % 32)
    assert ref.align16(5) == 16 and ref.entry_bytes(1, 3, 2, 1, 1, 1, 1) % 16 == 0
    for t in (-1, STEPS + 1):
        assert _bytes(lib, r, t) < 0 and b't must be' in lib.infgen_last_error()
    r.first_new = 0x10000
    assert _bytes(lib, r, 0) < 0 and b'insertion' in lib.infgen_last_error()


def test_refusals_that_launch_nothing():
    from infgen_amd import _lib
    lib = _lib.load()
    r = _context(32)
    need = _bytes(lib, r, 3)
    sel = (C.c_int * 6)(0, 1, 2, 3, 4, 5)
    head = (C.c_int * 24)()
    buf, ok = 0x7000000, need + 16

    def save(t=3, slots=sel, n=2, snap=buf, stride=ok, hd=head):
        return lib.infgen_snapshot_scenes(C.byref(r), t, slots, n, snap, stride, hd, None, None)

    def load(t=3, index=sel, snap=buf, stride=ok, hd=head, n=2):
        return lib.infgen_restore_scenes(C.byref(r), t, index, snap, stride, hd, n, None, None)

    for call in (save, load):
        for t in (-1, STEPS + 1):
            assert call(t=t) < 0 and b't must be' in lib.infgen_last_error()
        assert call(snap=None) < 0 and b'null' in lib.infgen_last_error()
        assert call(hd=None) < 0 and b'null' in lib.infgen_last_error()
        assert call(stride=need - 16) < 0 and b'infgen_snapshot_bytes' in lib.infgen_last_error()
        assert call(stride=need + 8) < 0 and b'multiple of 16' in lib.infgen_last_error()
        assert call(snap=buf + 8) < 0 and b'16-byte aligned' in lib.infgen_last_error()
        assert call(n=-1) < 0 and call(n=65536) < 0
    assert save(slots=None) < 0 and b'null' in lib.infgen_last_error()
    assert load(index=None) < 0 and b'null' in lib.infgen_last_error()
    # a stride that fits step 3 does not fit the last step
    assert save(t=STEPS, stride=need) < 0 and b'infgen_snapshot_bytes' in lib.infgen_last_error()
    r.first_new = C.addressof(sel)
    for call in (save, load):
        assert call() < 0 and b'insertion' in lib.infgen_last_error()
    assert lib.infgen_snapshot_scenes(None, 0, sel, 2, buf, ok, head, None, None) < 0


def test_host_side_checks_of_slots_and_index():
    from infgen_amd import snapshots
    assert snapshots.check_slots([4, 1], 6).tolist() == [4, 1] and snapshots.check_slots([4, 1], 6).dtype == np.int32
    with pytest.raises(ValueError, match='no slot'):
        snapshots.check_slots([], 6)
    with pytest.raises(ValueError, match=r'slots\[1\] = 6 is outside 0 \.\. 5'):
        snapshots.check_slots([0, 6], 6)
    with pytest.raises(ValueError, match=r'slots\[0\] = -1'):
        snapshots.check_slots([-1], 6)
    with pytest.raises(ValueError, match='integer'):
        snapshots.check_slots([0.5], 6)
    with pytest.raises(ValueError, match='shape'):
        snapshots.check_slots([[0, 1]], 6)
    # index: S = 6 as two groups of three, entries of slots [4, 1]
    slots = np.asarray([4, 1])
    good = [1, 1, -1, 0, 0, -1]
    assert snapshots.check_index(good, 6, 2, 3, slots).tolist() == good
    assert snapshots.check_index(np.asarray(good).reshape(2, 3), 6, 2, 3, slots).tolist() == good
    with pytest.raises(ValueError, match=r'index\[2\] = 2 is neither -1 nor an entry 0 \.\. 1'):
        snapshots.check_index([1, 1, 2, 0, 0, -1], 6, 2, 3, slots)
    with pytest.raises(ValueError, match=r'index\[0\] = -2'):
        snapshots.check_index([-2, 1, -1, 0, 0, -1], 6, 2, 3, slots)
    with pytest.raises(ValueError, match=r'index\[3\] = 1 is the entry of slot 1, a slot of another copy group'):
        snapshots.check_index([1, 1, -1, 1, 0, -1], 6, 2, 3, slots)
    assert snapshots.check_index([1, 1, -1, 1, 0, -1], 6, 2, 3, None).tolist() == [1, 1, -1, 1, 0, -1]      # slots unknown on the host
    with pytest.raises(ValueError, match='shape'):
        snapshots.check_index([0, 1], 6, 2, 3, slots)
    with pytest.raises(ValueError, match='integer'):
        snapshots.check_index([0.0] * 6, 6, 2, 3, slots)
    # the restatement of the kernel's checks agrees on the same vectors
    head, bad = ref.head_rows([4, 1], 6, [0, 0, 0, 1, 1, 1], 3)
    assert bad == 0 and head.tolist() == [[4, 1, 3, 1], [1, 0, 3, 1]]
    assert ref.effective_index(good, head, 6, [0, 0, 0, 1, 1, 1], 3) == (good, 0)
    assert ref.effective_index([1, 1, 2, 1, 0, -2], head, 6, [0, 0, 0, 1, 1, 1], 3) == ([1, 1, -1, -1, 0, -1], 3)
    assert ref.effective_index(good, head, 6, [0, 0, 0, 1, 1, 1], 4) == ([-1] * 6, 4)
    assert ref.head_rows([4, 6, -1], 6, None, 0)[0].tolist() == [[4, 4, 0, 1], [6, -1, 0, 0], [-1, -1, 0, 0]]


def test_header_and_binding_declare_the_entries_and_the_context_is_unchanged():
    from infgen_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    m = re.search(r'int infgen_snapshot_bytes\(([^;]*)\);', hdr)
    assert m and 'const InfgenRollout* r' in m.group(1) and 'int t' in m.group(1) and 'long long* bytes' in m.group(1)
    m = re.search(r'int infgen_snapshot_scenes\(([^;]*)\);', hdr)
    assert m, 'include/infgen_hip.h declares infgen_snapshot_scenes'
    for name in ('const InfgenRollout* r', 'int t', 'const int* slots', 'int n', 'void* snap', 'long long entry_stride', 'int* head',
                 'int* n_bad', 'void* stream'):
        assert name in m.group(1), name
    m = re.search(r'int infgen_restore_scenes\(([^;]*)\);', hdr)
    assert m, 'include/infgen_hip.h declares infgen_restore_scenes'
    for name in ('const InfgenRollout* r', 'int t', 'const int* index', 'const void* snap', 'long long entry_stride',
                 'const int* head', 'int n', 'int* n_bad', 'void* stream'):
        assert name in m.group(1), name
    section = hdr[hdr.index('snapshots: SNAPSHOTS'):hdr.index('int infgen_snapshot_bytes(')]
    assert 'scenario insertion' in section and '16-byte' in section
    assert 'snapshots' in hdr[hdr.index('branching rollouts: BRANCHING'):hdr.index('int infgen_branch_scenes(')]
    lib = _lib.load()
    assert _lib.SYMBOLS['infgen_snapshot_bytes'] == (C.c_int, [C.POINTER(_lib.Rollout), C.c_int, C.c_void_p])
    assert lib.infgen_snapshot_bytes(C.byref(_lib.Rollout()), 0, None) < 0
    P, i, ll = C.c_void_p, C.c_int, C.c_longlong
    assert _lib.SYMBOLS['infgen_snapshot_scenes'] == (i, [C.POINTER(_lib.Rollout), i, P, i, P, ll, P, P, P])
    assert _lib.SYMBOLS['infgen_restore_scenes'] == (i, [C.POINTER(_lib.Rollout), i, P, P, ll, P, i, P, P])
    assert lib.infgen_snapshot_scenes.argtypes == _lib.SYMBOLS['infgen_snapshot_scenes'][1]
    # no new struct member, no new option, no new kernel id
    assert C.sizeof(_lib.Rollout) == 1272 == lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT)
    assert _lib.OPTIONS_VALUE_BYTES == 48 and _lib.HEADER.consts['INFGEN_KID_COUNT'] == 11
