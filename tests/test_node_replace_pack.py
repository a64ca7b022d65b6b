"""pack_node packing another node over a node's rows, as yoda_replace_nodes does.

tools/check_node_replace.cpp is a stand-alone program, built here with AddressSanitizer and UBSan
as an ordinary executable: every row sits in a heap buffer of exactly its size; a node of a cards
is packed, then a node of b cards and other GPU models into the same buffers (every pair 0..K x
0..K, K = 1..16, all three record paths), and the rows and returned flags must be those of a pack
into zeroed buffers."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_pack_over_another_node(tmp_path):
    exe = str(tmp_path / "check_node_replace")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_node_replace.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_node_replace ok" in out.stdout, out.stdout
