"""The host folds of the rescue family's collect (groot_amd/csrc/hip/rescue_fold.hpp: bitmap rows into ID lists, the log into the host map
of assigned coverage) at their edges: tools/rescue_fold_check.cpp, a stand-alone program whose expected values are written out by hand,
built and run on the CPU under AddressSanitizer + UBSan."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_folds_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rescue_fold_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "groot_amd", "csrc", "hip"), "-o", exe,
                           os.path.join(REPO, "tools", "rescue_fold_check.cpp")])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "rescue_fold_check: ok" and not p.stderr, (p.returncode, p.stdout, p.stderr)
