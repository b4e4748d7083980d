"""CPU: the parent-vector contract of branching rollouts (tests/branch_ref.py restates infgen_resample_parents and the resamplers of
infgen_amd/branching.py), the host-side validation of ``RolloutEngine.branch`` and the C boundary of the two entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import branch_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = ((1, 1), (3, 2), (2, 33), (1, 1024), (4, 7))


def _ancestors(rng, S0, copies, kind):
    S = S0 * copies
    base = np.repeat(np.arange(S0) * copies, copies)
    if kind == 'random':
        return base + rng.integers(0, copies, S)
    if kind == 'same':
        return base + copies // 2
    if kind == 'identity':
        return np.arange(S)
    a = base + rng.integers(0, copies, S)          # 'outside': some entries below 0, beyond S, or in a neighbouring group
    a[::3] = -1
    a[1::5] = S + 4
    if S0 > 1:
        a[2::7] = (a[2::7] + copies) % S
    return a


@pytest.mark.parametrize('S0,copies', SHAPES)
@pytest.mark.parametrize('kind', ('random', 'same', 'identity', 'outside'))
def test_resampled_parents_are_valid_and_keep_the_multiset(S0, copies, kind):
    rng = np.random.default_rng(S0 * 131 + copies)
    anc = _ancestors(rng, S0, copies, kind)
    parent = ref.resample_parents(anc, copies)
    clean = ref.sanitise(anc, copies)
    assert ref.bad_entries(parent, copies) == []                                  # in range, own group, sources fixed points
    assert (parent[parent] == parent).all()
    for g0 in range(0, S0 * copies, copies):
        assert sorted(parent[g0:g0 + copies]) == sorted(clean[g0:g0 + copies])    # the group's multiset of ancestors
    named = np.unique(clean)
    assert (parent[named] == named).all()                                         # a named slot keeps itself
    if kind == 'identity':
        assert (parent == np.arange(S0 * copies)).all()
    if kind == 'same' and copies > 1:
        assert (parent == clean).all()
    assert (ref.resample_parents(anc, copies) == parent).all()                    # deterministic


def test_resamplers_give_valid_ancestors():
    rng = np.random.default_rng(5)
    w = rng.integers(1, 9, (3, 8)).astype(np.float64)
    u = np.asarray([0.31, 0.77, 0.05])
    anc = ref.systematic_ancestors(np.log(w), u)
    for g in range(3):
        cnt = np.bincount(anc[g] - g * 8, minlength=8)
        exp = 8 * w[g] / w[g].sum()
        assert (cnt >= np.floor(exp)).all() and (cnt <= np.ceil(exp)).all(), (cnt, exp)
    score = rng.integers(0, 4, (3, 8)).astype(np.float64)                         # many ties: the lower slot ranks first
    for keep in (1, 3, 8):
        kb = ref.keep_best(score, keep)
        assert ref.bad_entries(kb.reshape(-1), 8) == []
        for g in range(3):
            kept = np.flatnonzero(kb[g] == g * 8 + np.arange(8))
            assert len(kept) == keep
            assert score[g][kept].min() >= np.delete(score[g], kept).max(initial=-np.inf)
            assert (np.bincount(kb[g] - g * 8, minlength=8)[kept] >= 1 + (8 - keep) // keep).all()      # round-robin


def test_host_parents_are_checked_without_a_device():
    from infgen_amd import branching
    ok = branching.check_parent([0, 0, 2, 3, 3, 3], 2, 3)
    assert ok.dtype == np.int32 and ok.tolist() == [0, 0, 2, 3, 3, 3]
    assert branching.check_parent(np.asarray([[0, 0, 2], [3, 3, 3]]), 2, 3).tolist() == [0, 0, 2, 3, 3, 3]
    for bad, word in (([0, -1, 2, 3, 4, 5], r'parent\[1\] = -1'), ([0, 1, 6, 3, 4, 5], r'parent\[2\] = 6'),
                      ([0, 1, 2, 1, 4, 5], r'parent\[3\] = 1 .*another copy group'),
                      ([0, 0, 1, 3, 4, 5], r'parent\[2\] = 1 .*fixed point')):
        with pytest.raises(ValueError, match=word):
            branching.check_parent(bad, 2, 3)
        assert ref.bad_entries(bad, 3), bad
    with pytest.raises(ValueError, match='integer'):
        branching.check_parent([0.0, 1.0], 1, 2)
    with pytest.raises(ValueError, match='shape'):
        branching.check_parent([0, 1, 2], 2, 3)
    with pytest.raises(ValueError, match='another copy group'):
        branching.check_parent([1, 1], 2, 1)              # copies == 1: every scene is its own group


def test_header_and_binding_declare_both_entries_and_the_context_is_unchanged():
    from infgen_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'infgen_hip.h')).read()
    m = re.search(r'int infgen_branch_scenes\(([^;]*)\);', hdr)
    assert m, 'include/infgen_hip.h declares infgen_branch_scenes'
    for name in ('const InfgenRollout* r', 'int t', 'const int* parent', 'int* n_bad', 'void* stream'):
        assert name in m.group(1), name
    m = re.search(r'int infgen_resample_parents\(([^;]*)\);', hdr)
    assert m, 'include/infgen_hip.h declares infgen_resample_parents'
    for name in ('const int* ancestor', 'int S0', 'int copies', 'int* parent', 'void* stream'):
        assert name in m.group(1), name
    assert 'scenario insertion' in hdr[hdr.index('branching rollouts: BRANCHING'):hdr.index('int infgen_branch_scenes(')]
    lib = _lib.load()
    assert len(lib.infgen_branch_scenes.argtypes) == 5 and len(lib.infgen_resample_parents.argtypes) == 5
    # no new struct, no new member, no new kernel id
    assert C.sizeof(_lib.Rollout) == 1272 == lib.infgen_layout_query(_lib.Q_SIZEOF_ROLLOUT)
    assert _lib.HEADER.consts['INFGEN_KID_COUNT'] == 11
    # refusals that launch nothing (this runs without a GPU)
    r = _lib.Rollout()
    r.S, r.A_cap, r.T, r.W, r.ring, r.R, r.token_size, r.num_layers = 2, 32, 6, 4, 5, 5, 64, 1
    one = (C.c_int * 2)(0, 1)
    assert lib.infgen_branch_scenes(C.byref(r), 0, None, None, None) != 0 and b'parent' in lib.infgen_last_error()
    assert lib.infgen_branch_scenes(C.byref(r), 5, one, None, None) != 0 and b't must be' in lib.infgen_last_error()
    assert lib.infgen_branch_scenes(C.byref(r), -1, one, None, None) != 0 and b't must be' in lib.infgen_last_error()
    r.first_new = C.addressof(one)
    assert lib.infgen_branch_scenes(C.byref(r), 0, one, None, None) != 0 and b'insertion' in lib.infgen_last_error()
    assert lib.infgen_resample_parents(one, 1, 1025, one, None) != 0 and b'1024' in lib.infgen_last_error()
    assert lib.infgen_resample_parents(None, 1, 2, one, None) != 0
