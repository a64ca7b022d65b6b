#!/usr/bin/env python3
"""One line per kernel of a built object, for comparing two builds (no GPU needed):

    python3 tools/kernel_listing.py [yoda_kernels.o] > listing.txt

the demangled name, VGPR / AGPR / SGPR counts, spills, LDS bytes, code bytes and a SHA-256
prefix of the kernel's instruction bytes, sorted by name.  Two builds hold the same kernel when
the whole line matches.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs as kr  # noqa: E402


def strip_params(name):
    """`void k<..., (yoda::Path)0>(args)` -> `void k<..., (yoda::Path)0>`."""
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i] if name[i] == "(" else name
    return name


def main():
    obj = sys.argv[1] if len(sys.argv) > 1 else kr.OBJ
    with tempfile.TemporaryDirectory() as t:
        co = os.path.join(t, "k.co")
        kr.code_object(obj, co)
        run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout
        meta = {r["symbol"][:-3]: r for r in kr.kernels(run(f"{kr.L}/llvm-readelf", "--notes", co))
                if r.get("symbol", "").endswith(".kd")}
        # .text: its address and file offset (the kernels' symbols are addresses)
        m = re.search(r"\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)",
                      run(f"{kr.L}/llvm-readelf", "-S", "-W", co))
        addr, off = int(m.group(1), 16), int(m.group(2), 16)
        blob = open(co, "rb").read()
        rows, seen = [], set()
        for line in run(f"{kr.L}/llvm-readelf", "--symbols", "-W", co).splitlines():
            f = line.split()
            if len(f) == 8 and f[3] == "FUNC" and f[7] in meta and f[7] not in seen:
                seen.add(f[7])  # (.dynsym and .symtab both list it)
                v, size = int(f[1], 16), int(f[2])
                code = blob[off + v - addr:off + v - addr + size]
                rows.append((f[7], size, hashlib.sha256(code).hexdigest()[:16]))
        filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
        names = run(filt, *[r[0] for r in rows]).splitlines() if filt else [r[0] for r in rows]
        out = []
        for (sym, size, h), name in zip(rows, names):
            r = meta[sym]
            name = re.sub(r"^void ", "", strip_params(name))
            out.append(f"{name}  vgpr {r.get('vgpr_count')} agpr {r.get('agpr_count')}"
                       f" sgpr {r.get('sgpr_count')} vspill {r.get('vgpr_spill_count')}"
                       f" sspill {r.get('sgpr_spill_count')}"
                       f" lds {r.get('group_segment_fixed_size')} bytes {size} sha {h}")
        print("\n".join(sorted(out)))
        print(f"# {len(out)} kernels", file=sys.stderr)


if __name__ == "__main__":
    main()
