"""DEV TOOL: the register and scratch figures of every kernel in a built libart.so, from the
code objects' own metadata (the AMDGPU notes of each gfx950 ELF inside .hip_fatbin).

    python tools/kernel_resources.py [LIB] [--filter SUBSTR] > profiles/NAME.txt

One line per kernel: demangled name, vgpr_count, agpr_count, sgpr_count, vgpr_spill_count,
private_segment_fixed_size (scratch bytes per lane), group_segment_fixed_size (LDS bytes)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    """Every device ELF bundled into `lib` (one uncompressed offload bundle per translation unit)."""
    with tempfile.TemporaryDirectory() as d:
        fat = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "x")],
                       check=True)
        blob = open(fat, "rb").read()
    out, at = [], blob.find(MAGIC)
    while at >= 0:
        n = int.from_bytes(blob[at + 24:at + 32], "little")
        p = at + 32
        for _ in range(n):
            off, size, tl = (int.from_bytes(blob[p + 8 * i:p + 8 * i + 8], "little") for i in range(3))
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "amdgcn" in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + 1)
    return out


def kernels(lib):
    rows = []
    for elf in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(elf)
            f.flush()
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f.name], check=True, capture_output=True,
                                   text=True).stdout
        for blk in re.split(r"\n\s+- ", notes):
            m = re.search(r"\.name:\s+(\S+)", blk)
            if not m or ".vgpr_count" not in blk:
                continue
            g = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) if re.search(rf"\.{k}:\s+(\d+)", blk) else 0  # noqa: E731
            rows.append((m.group(1), g("vgpr_count"), g("agpr_count"), g("sgpr_count"), g("vgpr_spill_count"),
                         g("private_segment_fixed_size"), g("group_segment_fixed_size")))
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True,
                           text=True, check=True).stdout.split("\n")
    return sorted((n,) + r[1:] for n, r in zip(names, rows))


if __name__ == "__main__":
    args = sys.argv[1:]
    flt = ""
    if "--filter" in args:
        flt = args.pop(args.index("--filter") + 1)
        args.remove("--filter")
    here = os.path.dirname(os.path.abspath(__file__))
    lib = args[0] if args else os.path.join(here, "..", "adiabatic_raytracer_amd", "lib", "libart.so")
    print("# kernel | vgpr | agpr | sgpr | vgpr_spill | private_segment_fixed_size | group_segment_fixed_size")
    for r in kernels(lib):
        if flt in r[0]:
            print(" | ".join(str(v) for v in r))
