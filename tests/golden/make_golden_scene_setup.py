"""SHA-256 digests of everything the host scene setup leaves (tests/golden/scene_setup_digests.json): every entry of
RolloutEngine._SCENE_ARRAYS, the four map-token category arrays and every entry of _epi_from_hosts(), for
  ragged     the 16 ragged scenes of test_ingest_equals_host_setup (5 filtered rows: the filter and the ego shift),
  ragged_x3  the same scenes with copies = 3,
  uniform    the one-shape scenes of the boundary tests (40 agents, 200 map tokens, no filtered row).
The fixture was written at the commit BEFORE the three Python scene setups were merged into infgen_amd/scene_setup.py
(the `legacy` branch of scene_arrays below, which only runs there); tests/test_scene_setup_cpu.py recomputes the digests
through the current code.  No GPU, no reference project: synth is deterministic.

    python tests/golden/make_golden_scene_setup.py
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from conftest import load_case  # noqa: E402

FIXTURE = os.path.join(HERE, 'scene_setup_digests.json')
MAP_CAT = ('map_tok', 'map_type', 'map_pl', 'map_light')


def blank_engine(cfg, n_scenes, copies=1, a_cap=64, m_cap=320):
    """a RolloutEngine without device state: what the host setup reads, nothing else"""
    from infgen_amd.engine import RolloutEngine
    e = RolloutEngine.__new__(RolloutEngine)
    e.cfg, e.T, e.hc, e.R, e.device = cfg, cfg.num_columns, cfg.hist_columns, cfg.num_recurrent_steps_val, torch.device('cpu')
    e.copies, e.S0, e.S, e.A_cap, e.M_cap = copies, n_scenes, n_scenes * copies, a_cap, m_cap
    return e


def scene_arrays(e, scenes):
    """set ``e`` up from host scenes (e.scenes, e.hosts) and return the padded arrays its device buffers are loaded from"""
    e.scenes = scenes
    if hasattr(e, '_setup_scenes_stacked'):                    # legacy: the commit that wrote the fixture
        e._stacked = None
        e.hosts = e._replicate(e._setup_scenes(scenes))
        return e._map_side(e._scene_arrays(e.hosts))
    hosts, batch = e._setup_scenes(scenes)
    e.hosts = e._replicate(hosts)
    return e._scene_arrays(batch)


def inputs():
    """name -> (cfg, scenes, copies)"""
    from infgen_amd import synth
    c = load_case('a24_m256_edge')
    cfg = c['cfg']
    rng = np.random.default_rng(5)
    ragged = [synth.make_scene(8200 + i, int(rng.integers(9, 41)), int(rng.integers(60, 300)), cfg, ego_last=bool(i % 3),
                               edge_cases=bool(i % 2), vocab=c['vocab'], grid=c['grid'], slip=0.1) for i in range(16)]
    assert sum(int((sc['agent']['state_idx'][:, cfg.hist_columns - 1] == 0).sum()) for sc in ragged) == 5
    std = synth.standard_config()
    vocab = synth.make_agent_vocab(std.token_size)
    grid = synth.build_grid(std.grid_range, std.grid_interval, std.pl2seed_radius)
    uniform = [synth.make_scene(900 + i, 40, 200, std, ego_last=(i % 2 == 0), edge_cases=(i % 3 == 0), vocab=vocab, grid=grid)
               for i in range(12)]
    uniform = [sc for sc in uniform if (np.asarray(sc['agent']['state_idx'])[:, std.hist_columns - 1] != 0).all()]
    assert len(uniform) >= 8
    return {'ragged': (cfg, ragged, 1), 'ragged_x3': (cfg, ragged, 3), 'uniform': (std, uniform, 1)}


def digest(x):
    x = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return dict(sha256=hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest(), dtype=str(x.dtype), shape=list(x.shape))


def compute():
    from infgen_amd.engine import RolloutEngine
    out = {}
    for name, (cfg, scenes, copies) in inputs().items():
        e = blank_engine(cfg, len(scenes), copies)
        arr = scene_arrays(e, scenes)
        d = {k: digest(arr[k]) for k in RolloutEngine._SCENE_ARRAYS + MAP_CAT}
        d.update({'epi.' + k: digest(v) for k, v in e._epi_from_hosts().items()})
        d['gt_len'] = digest(np.asarray(e._gt_len, np.int64))
        out[name] = d
    return out


if __name__ == '__main__':
    res = compute()
    with open(FIXTURE, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print({k: len(v) for k, v in res.items()})
