"""CPU: the host-side pieces of bench.py - the scene pool builds the serial scenes, --dump-outputs writes a seeded, bounded
sample of what the engines return, and a step count below one is refused before any device work."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_scene_pool_builds_the_serial_scenes():
    import bench
    from infgen_amd import synth
    cfg = synth.standard_config(disable_insertion=True, num_recurrent_steps_val=80)
    idx = list(range(5, 69))                            # 64 scenes: the pool's threshold
    pooled = bench.build_scenes(cfg, idx, 16, 128, procs=2)[0]
    serial = bench.build_scenes(cfg, idx, 16, 128)[0]
    assert len(pooled) == len(serial) == len(idx)
    assert all(_same(a, b) for a, b in zip(pooled, serial))


class _Engine:
    """what dump_outputs reads of a RolloutEngine: A_cap, hosts and outputs_device() (lazy per-scene dicts)"""

    def __init__(self, S, A, seed):
        g = torch.Generator().manual_seed(seed)
        self.A_cap, self.hosts, self.S, self.A = A, [dict(A=A)] * S, S, A
        self.pos = torch.randn(S, A, 18, 2, generator=g)
        self.tok = torch.randint(0, 2048, (S, A, 18), generator=g)
        self.traj = torch.randn(S, A, 91, 2, generator=g)
        self.x_pt = torch.randn(S * 1024, 128, generator=g)           # (per map token: not scaled by the agent rows)

    def outputs_device(self):
        from infgen_amd.engine import LazyOut
        outs = []
        for s in range(self.S):
            o = LazyOut(dict(ego_index=self.A - 1, num_inserted=0),
                        dict(pos_a=lambda s=s: self.pos[s], next_token_idx=lambda s=s: self.tok[s],
                             pred_valid=lambda s=s: self.pos[s, :, :, 0] > 0, pred_traj=lambda s=s: self.traj[s],
                             agent_id=lambda s=s: torch.arange(self.A), x_pt=lambda s=s: self.x_pt[s * 1024:(s + 1) * 1024]))
            o['agent_labels'] = [[None] * 18 for _ in range(self.A)]
            outs.append(o)
        return outs


@pytest.mark.parametrize('scenes', [3, 1024])
def test_dump_outputs_is_a_seeded_bounded_sample(tmp_path, scenes):
    import bench
    engines = lambda: [_Engine(scenes // 2, 64, 0), _Engine(scenes - scenes // 2, 64, 1)]
    bench.dump_outputs(str(tmp_path / 'a'), engines())
    bench.dump_outputs(str(tmp_path / 'b'), engines())
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert files == ['agent_id.npy', 'ego_index.npy', 'next_token_idx.npy', 'num_inserted.npy', 'pos_a.npy', 'pred_traj.npy',
                     'pred_valid.npy', 'scene_index.npy', 'x_pt.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= 64_000_000
    load = lambda d, f: np.load(tmp_path / d / f)
    for f in files:
        assert load('a', f).dtype in (np.float32, np.float64), f
        assert np.array_equal(load('a', f), load('b', f)), f
    idx = load('a', 'scene_index.npy')
    assert np.all(np.diff(idx) > 0) and idx.min() >= 0 and idx.max() < scenes
    assert len(idx) == scenes if scenes == 3 else 0 < len(idx) < scenes
    assert load('a', 'pos_a.npy').shape == (64 * len(idx), 18, 2)
    # the rows of the first sampled scene are that scene's outputs, integers exactly
    s = int(idx[0])
    e, r = (engines()[0], s) if s < scenes // 2 else (engines()[1], s - scenes // 2)
    assert np.array_equal(load('a', 'pos_a.npy')[:64], e.pos[r].numpy())
    assert np.array_equal(load('a', 'next_token_idx.npy')[:64], e.tok[r].numpy().astype(np.float64))


def test_steps_below_one_are_refused():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and '--steps must be >= 1' in out.stderr
