"""The host backend's bb_playout_values(_pos) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
(tests/native/playout_values_sanitize.cpp, its own main) compiled together with csrc/bb_host.cpp and run as a process of
its own, the way tests/test_plan2_values_sanitize.py runs its entry points.  Rows, combos, stream ids and every output
sit in heap buffers of exactly the size the call may touch; all nine outputs are held to the definition restated over
the existing entry points, each output is asked for alone, and the handle form is held to the _pos form."""
import os
import shutil
import subprocess

import pytest

from runtime.build import CSRC, HOST_SOURCES
from runtime.lib import REPO_DIR

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1",
       "-fopenmp", "-ffp-contract=off"]


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("san_playout_values") / "playout_values_sanitize")
    subprocess.run(["g++", *SAN, "-std=c++17", f"-I{os.path.join(REPO_DIR, 'include')}",
                    os.path.join(REPO_DIR, "tests", "native", "playout_values_sanitize.cpp"),
                    *[os.path.join(CSRC, s) for s in HOST_SOURCES], "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("threads", ["4", "1"])
def test_playout_values_under_asan_ubsan(sanitized_driver, threads):
    env = dict(os.environ, OMP_NUM_THREADS=threads,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sanitized_driver], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "playout values under sanitizers: 7 boards at depth 1-3, consistent" in r.stdout
