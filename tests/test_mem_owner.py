"""The owners of device memory, pinned memory and events (raytracing_c_amd/csrc/rt_mem.h) against a stand-in HIP runtime
(tests/c/hip_stub), under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone CPU program, no GPU and no ROCm needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_owners_free_once_grow_in_order_and_count_exactly(tmp_path):
    exe = str(tmp_path / "mem_owner")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "tests", "c", "hip_stub"), os.path.join(ROOT, "tests", "c", "mem_owner.cpp"), "-o", exe]
    subprocess.check_call(cmd)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(" ok") == 5, r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr


def test_host_units_call_the_runtime_allocator_only_through_the_owners():
    """hipMalloc / hipFree / hipHostMalloc / hipHostFree / hipEventCreate* / hipEventDestroy occur in rt_mem.h and nowhere else in
    the host units: a buffer that is not an owner's cannot be forgotten in a free list, because there is none."""
    import glob
    import re
    csrc = os.path.join(ROOT, "raytracing_c_amd", "csrc")
    units = sorted(glob.glob(os.path.join(csrc, "*.cpp"))) + [os.path.join(csrc, "rt_host.h")]
    assert len(units) == 12, units
    pat = re.compile(r"\bhip(Malloc|Free|HostMalloc|HostFree)\s*\(|\bhipEvent(Create|Destroy)")
    hits = [f"{os.path.basename(u)}:{i + 1}" for u in units for i, line in enumerate(open(u)) if pat.search(line)]
    assert hits == [], hits
