"""CPU: the ABI of the map-token head (infgen_map_token_head): the ctypes binding agrees with the header, the torch op has a
shape function, and the pack the kernel reads is the MLPLayer pack with the split section at the offsets the kernel uses."""
import os
import re

import numpy as np

from conftest import REPO, make_weights


def test_binding_argtypes_match_the_header():
    from infgen_amd import _lib
    with open(os.path.join(REPO, 'include', 'infgen_hip.h')) as f:
        hdr = f.read()
    m = re.search(r'\bint infgen_map_token_head\(([^)]*)\);', hdr)
    assert m, 'infgen_map_token_head missing from include/infgen_hip.h'
    args = [a.strip() for a in m.group(1).split(',')]
    res, types = _lib.SYMBOLS['infgen_map_token_head']
    assert res is _lib._i and len(types) == len(args) == 10
    for a, t in zip(args, types):
        assert t is (_lib._p if '*' in a else _lib._i), a


def test_fake_kernel_gives_the_output_shapes():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import infgen_amd.torch_ops  # noqa: F401
    with FakeTensorMode():
        x = torch.empty(50, 128)
        lg, top = torch.ops.infgen_hip.map_token_head(x, torch.empty(7, dtype=torch.int32), torch.empty(10))
    assert tuple(lg.shape) == (7, 1024) and lg.dtype == torch.float32
    assert tuple(top.shape) == (7, 10) and top.dtype == torch.int64


def test_pack_layout_the_kernel_reads():
    from infgen_amd import packing
    sd = make_weights()
    p = packing.pack_mlp_layer(sd, 'map_encoder.token_predict_head')
    W3, N = 16768, 1024
    oh = W3 + 128 * N + N                                   # k_map_head_h: split section (16 floats, then the quarters)
    assert p.size == oh + 16 + (1 + N // 128) * 4 * 8 * 2 * 64 * 8 // 2
    assert np.array_equal(p[16384:16512], sd['map_encoder.token_predict_head.mlp.0.bias'])
    assert np.array_equal(p[W3 + 128 * N:W3 + 128 * N + N], sd['map_encoder.token_predict_head.mlp.3.bias'])
    # the bf16-operand pack rounds the same weights (hi plane only) and keeps the fp32 planes
    with packing.operand_bits(8):
        q = packing.pack_mlp_layer(sd, 'map_encoder.token_predict_head')
    assert q.size == p.size and np.array_equal(q[:oh + 16], p[:oh + 16])


FIXTURES = ('maphead_a8_m128', 'maphead_a32_m512', 'maphead_batch3')


def test_reference_logit_gaps_leave_the_top10_decidable():
    """precondition of the top-10 rule of tests/test_map_head_gpu.py: in the reference's own logits, adjacent gaps under 1e-4
    among each row's 11 largest are at most 1 % of the pairs"""
    from conftest import GOLDEN
    for name in FIXTURES:
        z = np.load(os.path.join(GOLDEN, name + '.npz'))
        top11 = -np.sort(-z['logits'], axis=1)[:, :11]
        share = float((np.diff(-top11, axis=1) < 1e-4).mean())
        print(f'{name}: {100 * share:.2f} % of adjacent top-11 gaps under 1e-4')
        assert share <= 0.01, name
        # the stored top-10 is the descending order of the stored logits
        lg = z['logits']
        assert np.all(np.diff(np.take_along_axis(lg, z['top_idx'][z['logit_rows']], 1), axis=1) <= 0)


def test_generator_regenerates_the_fixtures(tmp_path):
    """tests/golden/make_golden_maphead.py reproduces the committed fixtures bit for bit from the reference"""
    import subprocess
    import sys
    import pytest
    from conftest import GOLDEN
    if not os.path.isdir('/root/reference/infgen'):
        pytest.skip('the reference checkout is not on this machine')
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_golden_maphead.py'), '--out', str(tmp_path)],
                       capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stderr[-2000:]
    for name in FIXTURES:
        a, b = np.load(os.path.join(GOLDEN, name + '.npz')), np.load(str(tmp_path / (name + '.npz')))
        assert sorted(a.files) == sorted(b.files), name
        for k in a.files:
            assert np.array_equal(a[k], b[k]), (name, k)
