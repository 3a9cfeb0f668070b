"""select_bit (csrc/bb_device.h) on the host: a stand-alone program (tests/native/select_bit_check.cpp, its own
main) holds the header's host form equal to the six-level routine it replaced, for every k in 0..69 over 2^20
random words of each of five density classes, 0 and the 64 single-bit words.  Built host-only, once plain and
once with -fsanitize=undefined (the shift and extract widths), and run as a process of its own; nothing is
loaded into Python and no GPU is used.  bb_device.h includes the HIP runtime header, so the compiler is the
library's own (runtime/build.py) in its host-only mode; the device pass and the host pass read the same
function, whose two forms differ in the one line that takes the low t bits."""
import os
import subprocess

import pytest

from runtime.build import _hipcc
from runtime.lib import REPO_DIR

SRC = os.path.join(REPO_DIR, "tests", "native", "select_bit_check.cpp")
BASE = ["--cuda-host-only", "-O2", "-std=c++17", "-pthread", f"-I{os.path.join(REPO_DIR, 'include')}"]
BUILDS = {
    "plain": [],
    "ubsan": ["-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"],
}


@pytest.mark.parametrize("build", list(BUILDS))
def test_select_bit_equals_six_level_form(tmp_path, build):
    exe = str(tmp_path / f"select_bit_check_{build}")
    subprocess.run([_hipcc(), *BASE, *BUILDS[build], SRC, "-o", exe], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "select_bit equals the six-level form: 367006150 (x, k) pairs, 1048576 words per class" in r.stdout
    assert "runtime error" not in r.stderr
