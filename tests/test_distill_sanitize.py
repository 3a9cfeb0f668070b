"""The host backend's bb_snapshot_combo under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
(tests/native/distill_sanitize.cpp, its own main) compiled together with csrc/bb_host.cpp and run as a process of
its own, the way tests/test_safe_mask_sanitize.py runs bb_safe_mask.  Played games' combo columns are copied into
exactly sized buffers after every step and held to bb_get_state's; any sanitizer report aborts it."""
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
    exe = str(tmp_path_factory.mktemp("san_distill") / "distill_sanitize")
    subprocess.run(["g++", *SAN, "-std=c++17", f"-I{os.path.join(REPO_DIR, 'include')}",
                    os.path.join(REPO_DIR, "tests", "native", "distill_sanitize.cpp"),
                    *[os.path.join(CSRC, s) for s in HOST_SOURCES], "-o", exe], check=True)
    return exe


def test_snapshot_combo_under_asan_ubsan(sanitized_driver):
    env = dict(os.environ, OMP_NUM_THREADS="4",
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sanitized_driver], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-4000:]
    assert "equal bb_get_state" in r.stdout
