"""CPU: the scene setup (infgen_amd/scene_setup.py through RolloutEngine._setup_scenes / _scene_arrays / _epi_from_hosts)
leaves, byte for byte, what the three separate Python setups left before they were merged: SHA-256 digests recorded at
that commit (tests/golden/make_golden_scene_setup.py) for a ragged batch with filtered rows, the same batch with three
copies per scene, and a one-shape batch."""
import importlib.util
import json
import os

from conftest import GOLDEN


def test_scene_setup_reproduces_the_recorded_digests():
    spec = importlib.util.spec_from_file_location('make_golden_scene_setup', os.path.join(GOLDEN, 'make_golden_scene_setup.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(gen.FIXTURE) as f:
        want = json.load(f)
    got = gen.compute()
    assert set(got) == set(want) == {'ragged', 'ragged_x3', 'uniform'}
    for name in want:
        assert set(got[name]) == set(want[name]) and len(want[name]) == 32, name
        for k, w in want[name].items():
            assert got[name][k] == w, (name, k, got[name][k], w)          # digest, dtype and shape
