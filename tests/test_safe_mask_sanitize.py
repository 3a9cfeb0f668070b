"""The host backend's bb_safe_mask under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
(tests/native/safe_mask_sanitize.cpp, its own main) compiled together with csrc/bb_host.cpp, run as a process of its
own, the way tests/test_plan_values_sanitize.py runs bb_plan_values.  Played and crafted positions and a crowded
random set go through both modes into exactly sized buffers, stateless and through the handle, and are held to
bb_plan_values' safe words and legal set; any sanitizer report aborts it."""
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
    exe = str(tmp_path_factory.mktemp("san_safe_mask") / "safe_mask_sanitize")
    subprocess.run(["g++", *SAN, "-std=c++17", f"-I{os.path.join(REPO_DIR, 'include')}",
                    os.path.join(REPO_DIR, "tests", "native", "safe_mask_sanitize.cpp"),
                    *[os.path.join(CSRC, s) for s in HOST_SOURCES], "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("threads", ["4", "1"])
def test_safe_mask_under_asan_ubsan(sanitized_driver, threads):
    env = dict(os.environ, OMP_NUM_THREADS=threads,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sanitized_driver], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "both modes equal bb_plan_values" in r.stdout
