"""The block K2's window helper (yoda_layout.h window_bits) against a bit-by-bit reference.

tools/check_k2_window.cpp is a stand-alone program: it includes yoda_layout.h as the host side of
libyoda does, keeps each block-list row in a heap buffer of exactly row_words words and walks
chunks of every start shift / length / row size the K2 meets.  Built here with AddressSanitizer
and UBSan as an ordinary executable, so a read of the word after a row (another wave's words, or
the seeds, on the device) or an out-of-range shift fails the run."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_window_bits_matches_reference(tmp_path):
    exe = str(tmp_path / "check_k2_window")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_k2_window.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_k2_window ok" in out.stdout, out.stdout
