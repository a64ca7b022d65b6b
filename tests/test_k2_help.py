"""Two host/device pieces of the block K2 (yoda_layout.h): argmax_fold, the one fold that merges
K2's partial results across chunks (k_reduce2, k_reduce2_finalize), and k2_claim_pick, the walk's
choice of the next block of a window.  The check program also runs the pick as the claim step of
a protocol that no kernel uses yet and that lives in the program only (an atomic AND on a window
word that several threads share).

tools/check_k2_help.cpp is a stand-alone program: it includes yoda_layout.h as the host side of
libyoda does.  The fold on states that include empty, a score of 0, equal scores with different
indices and scores near 2^52: commutative, associative, and folding any partition of a node list
equals the sequential argmax with its ties and lowest index.  The claim protocol with a
std::atomic<uint64_t> word and four threads over random list, hot and prune masks: every listed,
unpruned bit claimed exactly once, no dropped bit claimed afterwards, no claim outside the word.
Built with AddressSanitizer and UBSan as an ordinary executable."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_fold_and_claim_protocol(tmp_path):
    exe = str(tmp_path / "check_k2_help")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_k2_help.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_k2_help ok" in out.stdout, out.stdout
