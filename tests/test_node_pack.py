"""The per-node packer shared by yoda_upload_nodes and yoda_update_node_cards (yoda_node_pack.h
pack_node) on random nodes.

tools/check_node_pack.cpp is a stand-alone program: it includes the packer header as the host side
of libyoda does, keeps every row in a heap buffer of exactly its size and packs nodes of K = 1, 2,
4, 8, 16 with 0..K cards, mixed models, unhealthy cards, equal frees and more than four clocks.
Built here with AddressSanitizer and UBSan as an ordinary executable, so a word written past a
row fails the run; a row that keeps a word of the node's older state (hfs past a fallen healthy
count, a ch entry, a change bit) differs from the pack into zeroed buffers."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_pack_node_rows(tmp_path):
    exe = str(tmp_path / "check_node_pack")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(ROCM, "include"), "-o", exe,
                    os.path.join(REPO, "tools", "check_node_pack.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_node_pack ok" in out.stdout, out.stdout


def test_greedy_session_host_check(tmp_path):
    """tools/check_greedy_session.cpp: the host-only greedy session (yoda_greedy_session.cpp, no
    HIP header), built with AddressSanitizer and UBSan as an ordinary executable and driven on
    random small clusters -- zero-total nodes, Allocate wrapping past 2^64 mid-window, lists
    shorter than the feasible counts, refreshes -- against a plain sequential loop."""
    exe = str(tmp_path / "check_greedy_session")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(REPO, "tools", "check_greedy_session.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "check_greedy_session ok" in out.stdout, out.stdout
