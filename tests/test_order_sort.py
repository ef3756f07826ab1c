"""The processing-order sort under the project's own launcher (groot_amd/csrc/hip/order_sort.hpp) as a stand-alone program:
tools/order_sort_check.hip includes the header alone, is compiled for gfx950 and run as a child process.  It compares perm with
std::stable_sort on (key >> begin_bit) & mask for

  sizes      2 049; 4 095 / 4 096 / 4 097 (one onesweep tile of 256 x 16 items and its neighbours); 8 193; 3 x 4 096 + 1; 100 000
  keys       all equal; all 0xFFFFFFFF; two values; random 24-bit with a tenth 0xFFFFFFFF, which come last when every sorted bit counts
  bits       begin_bit 2, end_bit 8, 9, 10, 16, 17, 18, 26: one, two and three iterations, whole and partial last digits

-- 7 x 4 x 7 = 196 sorts through ONE scratch block whose only fills are the driver's own (at allocation, and one behind each sort) -- and then
100 000 -> 4 097 -> 100 000 items through a fresh block that grew once: the case a clear sized for the wrong batch gets wrong.  The program
also checks that the inputs are untouched, that nothing is written behind the outputs and that the block's state is all zero at the end."""
import os
import subprocess

import pytest

from test_batch_history import need_gpu  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tools", "order_sort_check.hip")
HDR = os.path.join(REPO, "groot_amd", "csrc", "hip", "order_sort.hpp")


def _program(tmp_path):
    """build/order_sort_check when it is newer than its two sources (a tree that was built beforehand), else a fresh build"""
    exe = os.path.join(REPO, "build", "order_sort_check")
    if os.path.exists(exe) and os.path.getmtime(exe) >= max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        return exe
    exe = str(tmp_path / "order_sort_check")
    hipcc = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-Wno-pass-failed", "-I" + os.path.dirname(HDR), "-o", exe, SRC],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_order_sort_against_stable_sort(need_gpu, tmp_path):
    r = subprocess.run([_program(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.splitlines()[-1] == "order_sort_check: 199 cases, 0 failed", r.stdout[-2000:]
