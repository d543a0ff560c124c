"""Per-kernel resource usage of a built libuuo_hip.so, from the gfx950 code object's AMDGPU metadata notes.

    python tools/kernel_resources.py LIB.so                 # table: kernel, VGPRs, SGPRs, scratch, LDS
    python tools/kernel_resources.py BASE.so NEW.so         # every kernel of BASE must keep its four figures and its bytes in NEW

The comparison is how a change that adds kernel instantiations shows it left the existing ones alone (exit 1 otherwise).  The
bytes are a hash of the kernel's own stretch of .text (its symbol's value and size), so a kernel that moved to another
translation unit or to another place in its own is still compared instruction for instruction.
Needs llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm installation (ROCM_PATH, default /opt/rocm); no GPU.
"""
from __future__ import annotations

import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def code_objects(lib: str, tmp: str) -> list:
    """The gfx950 code objects of `lib`: its .hip_fatbin section holds one offload bundle per translation unit."""
    fatbin = os.path.join(tmp, "fatbin")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fatbin, lib,
                           os.path.join(tmp, "stripped")])
    data = open(fatbin, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)]
    out = []
    for i, st in enumerate(starts):
        chunk = os.path.join(tmp, "bundle%d" % i)
        with open(chunk, "wb") as fh:
            fh.write(data[st:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = os.path.join(tmp, "gfx950_%d.co" % i)
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--input=" + chunk, "--output=" + co,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle"])
        out.append(co)
    return out


def text_hashes(co: str) -> dict:
    """{function symbol: sha256 of its bytes in .text} of one code object, from its section and symbol tables alone."""
    readelf = os.path.join(LLVM, "llvm-readelf")
    sec = re.search(r"^\s*\[\s*(\d+)\] \.text\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ",
                    subprocess.check_output([readelf, "-S", "-W", co], text=True), re.M)
    ndx, addr, off = sec.group(1), int(sec.group(2), 16), int(sec.group(3), 16)
    data = open(co, "rb").read()
    out = {}
    for line in subprocess.check_output([readelf, "--symbols", "-W", co], text=True).splitlines():
        t = line.split()  # Num: Value Size Type Bind Vis Ndx Name
        if len(t) == 8 and t[3] == "FUNC" and t[6] == ndx:
            at = off + int(t[1], 16) - addr
            out[t[7]] = hashlib.sha256(data[at:at + int(t[2])]).hexdigest()[:16]
            RAW[(co, t[7])] = data[at:at + int(t[2])]
    return out


RAW = {}  # (code object, symbol) -> the bytes hashed above, kept to describe a difference


def byte_difference(k: str) -> str:
    """How the two versions of kernel `k` differ: the 32-bit words that do, and their differences when all are the same (a
    kernel that only moved relative to a global it addresses differs by its displacement in those words, and nowhere else)."""
    a, b = [v for (co, name), v in RAW.items() if name == k][:2]  # (in the order read: BASE, then NEW)
    if len(a) != len(b):
        return "%d -> %d bytes" % (len(a), len(b))
    words = [i for i in range(0, len(a), 4) if a[i:i + 4] != b[i:i + 4]]
    deltas = {int.from_bytes(b[i:i + 4], "little", signed=True) - int.from_bytes(a[i:i + 4], "little", signed=True) for i in words}
    return "%d of %d words differ%s" % (len(words), len(a) // 4, ", all by %d" % deltas.pop() if len(deltas) == 1 else "")


def resources(lib: str) -> dict:
    """{kernel name: {field: value}} of every kernel of `lib`'s gfx950 code objects; the entry "bytes" is the hash of its code."""
    with tempfile.TemporaryDirectory() as tmp:
        cos = code_objects(lib, tmp)
        notes = "".join(subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True) for co in cos)
        hashes = {}
        for co in cos:
            hashes.update(text_hashes(co))
    # amdhsa.kernels: every kernel is a list entry "  - .key: value" whose own keys sit at indent 4 (its arguments nest deeper)
    kernels, block = {}, None
    for line in notes.splitlines():
        m = re.match(r"^(  - |    )(\.[a-z_]+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            block = {}
        if block is None:
            continue
        block[m.group(2)] = m.group(3)
        if ".name" in block and all(f in block for f in FIELDS):
            kernels[block[".name"]] = {f: int(block[f]) for f in FIELDS}
            kernels[block[".name"]]["bytes"] = hashes.get(block[".name"])
    return kernels


def main(argv) -> int:
    if len(argv) == 1:
        for k, v in sorted(resources(argv[0]).items()):
            print("%-40s %4d VGPR %4d SGPR %6d B scratch %6d B LDS" % (k, *(v.get(f, -1) for f in FIELDS)))
        return 0
    if len(argv) != 2:
        print(__doc__)
        return 2
    base, new = resources(argv[0]), resources(argv[1])
    bad = 0
    for k, v in sorted(base.items()):
        w = new.get(k)
        if w != v:
            bad += 1
            print("CHANGED %s: %s -> %s" % (k, v, w))
            if w and {f: v[f] for f in FIELDS} == {f: w[f] for f in FIELDS}:
                print("        bytes only: %s" % byte_difference(k))
    for k in sorted(set(new) - set(base)):
        print("new     %-36s %s" % (k, " ".join("%s=%d" % (f, new[k][f]) for f in FIELDS if f in new[k])))
    print("%d kernels compared, %d changed, %d new" % (len(base), bad, len(set(new) - set(base))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
