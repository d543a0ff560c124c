"""Per-kernel resource usage of a built libuuo_hip.so, from the gfx950 code object's AMDGPU metadata notes.

    python tools/kernel_resources.py LIB.so                 # table: kernel, VGPRs, SGPRs, scratch, LDS
    python tools/kernel_resources.py BASE.so NEW.so         # every kernel of BASE must keep its four figures in NEW

The comparison is how a change that adds kernel instantiations shows it left the existing ones alone (exit 1 otherwise).
Needs llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm installation (ROCM_PATH, default /opt/rocm); no GPU.
"""
from __future__ import annotations

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


def resources(lib: str) -> dict:
    """{kernel name: {field: value}} of every kernel of `lib`'s gfx950 code object."""
    with tempfile.TemporaryDirectory() as tmp:
        notes = "".join(subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
                        for co in code_objects(lib, tmp))
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
    for k in sorted(set(new) - set(base)):
        print("new     %-36s %s" % (k, " ".join("%s=%d" % (f, new[k][f]) for f in FIELDS if f in new[k])))
    print("%d kernels compared, %d changed, %d new" % (len(base), bad, len(set(new) - set(base))))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
