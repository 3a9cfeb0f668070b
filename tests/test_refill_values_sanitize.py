"""The host backend's bb_refill_values(_pos) and bb_play_plan_pos under AddressSanitizer + UndefinedBehaviorSanitizer:
a stand-alone program (tests/native/refill_values_sanitize.cpp, its own main) compiled together with
csrc/bb_host.cpp and run as a process of its own, the way tests/test_refill_census_sanitize.py runs the census.  The
output buffers hold exactly n * deals (n) elements, each output is NULL in turn, and the hands, attempts and depth-2
values of the fixed case are held to a table in the program."""
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
    exe = str(tmp_path_factory.mktemp("san_refill_values") / "refill_values_sanitize")
    subprocess.run(["g++", *SAN, "-std=c++17", f"-I{os.path.join(REPO_DIR, 'include')}",
                    os.path.join(REPO_DIR, "tests", "native", "refill_values_sanitize.cpp"),
                    *[os.path.join(CSRC, s) for s in HOST_SOURCES], "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("threads", ["4", "1"])
def test_refill_values_under_asan_ubsan(sanitized_driver, threads):
    env = dict(os.environ, OMP_NUM_THREADS=threads,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sanitized_driver], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "hands equal the table" in r.stdout
