"""The block kernels' level indices (yoda_layout.h kb_level_lo, kb_level_hi) against the
sequential searches they replace.

tools/check_k2_bounds.cpp is a stand-alone program: it includes yoda_layout.h as the host side of
libyoda does.  Tables of 4 (exhaustive), 32 and 64 strictly increasing levels from 0 to
0xFFFFFFFF, every bound at a level, one below, one above, 0 and 0xFFFFFFFF, and 10^6 random
bounds.  Built with AddressSanitizer and UBSan as an ordinary executable (an out-of-range shift
in a mask helper fails the run)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_level_indices_match_sequential_search(tmp_path):
    exe = str(tmp_path / "check_k2_bounds")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_k2_bounds.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_k2_bounds ok" in out.stdout, out.stdout
