"""Every host path into the sampler gives the bits it gave in front of the host refactor.

tools/profile/sampler_paths.py runs the paths -- ``sampling`` unseeded and seeded in both modes, alone and packed; pinned ``hold`` /
``renoise`` and guided free / pinned with their trajectories and traces; the proximal tail at B = 1 and packed; ``repack``;
``sample_ensemble`` / ``repack_ensemble`` with recombination and the buried surface; ``mutate``; ``sample_sharded`` rehearsed with
two ranks, seeded and with fixed masks; ``sample_from`` -- on synthetic complexes of 20 to 48 rows.
tests/golden/r22_sampler_paths.json holds the sha256 of each path's tensors as the parent commit computed them on the MI355X, twice
with equal results: every path is bit-reproducible there, so the comparison is equality.
"""
import importlib.util
import json
import os

import pytest

from .conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("sampler_paths", os.path.join(ROOT, "tools", "profile", "sampler_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_path_has_the_parents_bits(tool):
    with open(os.path.join(ROOT, "tests", "golden", "r22_sampler_paths.json")) as f:
        want = json.load(f)["paths"]
    got = tool.digests(tool.compute("cuda:0"))
    for k in sorted(set(want) | set(got)):
        print(f"{k}: {'equal' if got.get(k) == want.get(k) else 'DIFFERENT'}")
    assert set(got) == set(want)
    assert {k for k in want if got[k] != want[k]} == set()
