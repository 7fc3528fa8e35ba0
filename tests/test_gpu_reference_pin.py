"""Reference -> kernel without the oracle in between: tests/golden/ref/*.npz hold what the reference's OWN text computes
(oracle/_ref/libref.so, recorded by tools/make_reference_pin_fixtures.py on a machine that has the reference tree; data only).
librt_hip_v1.so -- the product under numeric contract v1, the contract the reference's expressions are compiled under -- must
return the recorded closest hits (t, triangle, u, v) bit for bit from rt_query_closest over the recorded tree, and
scene_init_gpu on the recorded triangles must return the recorded node and triangle bytes.  Those bytes are the REFERENCE's
scene_init for quad, spheres and tower (asserted through the fixture's `builder` field).  For soup513 the reference stops at
its own assertion (deviation D7), so that fixture's tree is the library's CPU builder's: its builder half compares
scene_init_gpu with rt_scene_build.c, NOT with the reference, and only its hits (the reference's traversal over that tree) are
the reference's.  u and v are compared after
-0.0 -> +0.0 (the recording reads them out of a sum that loses the sign of a zero, oracle/ref_harness.c).
tests/test_gpu_contracts.py and tests/test_oracle_contracts.py tie contract v1 to the contract the product ships;
tests/test_reference_pin.py checks on the CPU that the fixtures are still what libref.so produces.  Own process (RT_LIB_PATH)."""
import glob
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref", "*.npz")))

_results = {}


def _replay():
    if not _results:
        lib = os.path.join(ROOT, "raytracing_c_amd", "librt_hip_v1.so")
        if not os.path.exists(lib):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "raytracing_c_amd", "csrc"), "v1"], stdout=subprocess.DEVNULL)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_refpin_worker.py")] + FIXTURES, text=True,
                           capture_output=True, env=dict(os.environ, RT_LIB_PATH=lib), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.strip(), r.stderr[-2000:]
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                j = json.loads(line)
                _results[j["fixture"]] = j
    return _results


def test_fixture_set():
    assert [os.path.basename(f) for f in FIXTURES] == ["quad.npz", "soup513.npz", "spheres.npz", "tower.npz"]


@pytest.mark.parametrize("name", ["quad", "spheres", "tower", "soup513"])
def test_gpu_builder_returns_the_recorded_bytes(name):
    j = _replay().get(name + ".npz")
    assert j is not None, "the worker stopped at an earlier fixture: " + str([v["error"] for v in _replay().values()])
    assert j["error"] is None, j["error"]
    assert j["builder"] == ("library" if name == "soup513" else "reference"), "see the module docstring: whose bytes the fixture holds"
    assert j["head_equal"], "depth / node count / slot count differ"
    assert j["build_equal"] == [True] * 5, dict(zip(("nodes", "coordinates", "records", "materials", "populated"), j["build_equal"]))


@pytest.mark.parametrize("name", ["spheres", "tower", "soup513"])
def test_gpu_closest_hit_returns_the_recorded_hits(name):
    """(quad has depth 0: the reference cannot traverse it, the fixture holds no rays)"""
    j = _replay().get(name + ".npz")
    assert j is not None, "the worker stopped at an earlier fixture: " + str([v["error"] for v in _replay().values()])
    assert j["error"] is None, j["error"]
    assert j["rays"] >= 4000 and 400 <= j["hits"] <= j["rays"] - 400
    assert j["t_equal"] and j["triangle_equal"] and j["uv_equal"], f"{j['mismatches']} of {j['rays']} rays differ"
