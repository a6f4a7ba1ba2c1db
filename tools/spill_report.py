"""DEV TOOL: where the integrators read and write spilled scalars, for a built libart.so.

    python tools/spill_report.py [LIB] [--filter SUBSTR] > profiles/NAME.txt

Per propagate_kernel / tail_kernel instantiation of both kernel units:
  * from the code object's metadata: VGPRs, SGPR spill slots, spilled VGPRs, scratch bytes per lane;
  * from llvm-objdump of the code object: the instructions of every region of the main loop -- all, VALU,
    FP64 VALU, v_readlane, v_writelane, scratch accesses, scalar loads.
The main loop is the widest backward branch's span. Its regions, in address order, are cut at the s_setprio
marks and at the first and last instruction of every loop nested directly in it; a region that is such a loop
is named "loop", and the one between the two priority marks with the most FP64 is the stage-slot loop
("slot loop"). Regions are address ranges: a block the compiler laid out elsewhere counts where it lies.
Addresses are left out, so two builds' reports diff line by line. The last lines repeat, one line per
instantiation, what a change must not make worse (spilled VGPRs, scratch bytes, the slot loop's scalar loads,
the lane reads outside the slot loop) and check what must hold for each: a slot loop without lane traffic
and scratch access, at most 256 VGPRs at 2 waves/SIMD. Runs on the CPU (it only reads the library)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as KR  # noqa: E402

LLVM = KR.LLVM
COLS = ("instr", "valu", "f64", "readlane", "writelane", "scratch", "s_load")
INSN = re.compile(r"^\t(\S+)\s*(.*?)\s*// ([0-9A-F]+):")
TARGET = re.compile(r"<[^>]*\+0x([0-9a-f]+)>\s*$")


def classify(mn):
    return (1, int(mn.startswith("v_") and not mn.startswith(("v_readlane", "v_writelane", "v_readfirstlane"))),
            int(mn.startswith("v_") and "_f64" in mn), int(mn.startswith("v_readlane")),
            int(mn.startswith("v_writelane")), int(mn.startswith("scratch_")),
            int(mn.startswith(("s_load_", "s_buffer_load_"))))


def disassemble(elf):
    """{mangled name: [(address, mnemonic, branch target or None)]} of one code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(elf)
        f.flush()
        text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", f.name], check=True,
                              capture_output=True, text=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f.name], check=True, capture_output=True,
                               text=True).stdout
    funcs, cur, base = {}, None, 0
    for line in text.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            base, cur = int(m.group(1), 16), funcs.setdefault(m.group(2), [])
            continue
        m = INSN.match(line)
        if m and cur is not None:
            t = TARGET.search(line) if m.group(1).startswith(("s_cbranch", "s_branch")) else None
            cur.append((int(m.group(3), 16), m.group(1), base + int(t.group(1), 16) if t else None))
    meta = {}
    for blk in re.split(r"\n\s+- ", notes):
        m = re.search(r"\.name:\s+(\S+)", blk)
        if m and ".vgpr_count" in blk:
            g = lambda k: int(x.group(1)) if (x := re.search(rf"\.{k}:\s+(\d+)", blk)) else 0  # noqa: E731
            meta[m.group(1)] = {k: g(k) for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count",
                                                  "private_segment_fixed_size")}
    return funcs, meta


def regions(ins):
    """[(name, first index, last index)] of the main loop of one kernel, and the index range of the loop."""
    at = {a: i for i, (a, _, _) in enumerate(ins)}
    back = [(at[t], i) for i, (a, _, t) in enumerate(ins) if t in at and t <= a]
    if not back:
        return [], None
    main = max(back, key=lambda l: l[1] - l[0])
    # a span with a priority mark inside is no nested loop: the main loop has several latches (one skips the
    # refill of a drained wave), and the marks' else-blocks, laid out at its end, jump back as well
    loops = sorted(l for l in set(back) if not any(ins[i][1] == "s_setprio" for i in range(l[0], l[1] + 1)))
    inner = [l for l in loops if main[0] <= l[0] and l[1] <= main[1] and l != main]
    # loops nested directly in the main loop; back edges onto one header are one loop
    top = []
    for l in sorted(inner, key=lambda l: (l[0], -l[1])):
        if top and l[0] <= top[-1][1]:
            top[-1] = (top[-1][0], max(top[-1][1], l[1]))
        else:
            top.append(l)
    prio = [i for i in range(main[0], main[1] + 1) if ins[i][1] == "s_setprio"]
    marks = []  # the two groups of priority marks (each an if/else pair a few instructions apart)
    for i in prio:
        if not marks or i - marks[-1][-1] > 8:
            marks.append([i])
        else:
            marks[-1].append(i)
    cuts = {main[0], main[1] + 1}
    for l in top:
        cuts |= {l[0], l[1] + 1}
    for g in marks:
        cuts.add(g[-1] + 1)
    cuts = sorted(cuts)
    out = []
    for a, b in zip(cuts, cuts[1:]):
        out.append(["loop" if (a, b - 1) in top else "code", a, b - 1])
    if len(marks) >= 2:
        lo, hi = marks[0][-1], marks[1][0]
        between = [r for r in out if r[0] == "loop" and lo < r[1] and r[2] < hi]
        if between:
            max(between, key=lambda r: sum(classify(ins[i][1])[2] for i in range(r[1], r[2] + 1)))[0] = "slot loop"
        for r in out:
            if r[0] == "code":
                r[0] = ("code before the low-priority mark (refill)" if r[2] <= lo else
                        "code before the slot loop (step size)" if r[2] < hi and not any(
                            q[0] == "slot loop" and q[1] < r[1] for q in out) else
                        "code up to the high-priority mark" if r[2] <= hi else "code after the slot loop")
    return [tuple(r) for r in out], main


def report(lib, flt=""):
    rows, bad, summary = [], [], []
    for elf in KR.code_objects(lib):
        funcs, meta = disassemble(elf)
        for name in sorted(funcs):
            if not re.match(r"_ZN3art(16propagate|11tail)_kernel", name) or name not in meta:
                continue
            rows.append((name, funcs[name], meta[name]))
    names = subprocess.run(["c++filt", "-p"], input="\n".join(r[0] for r in rows), capture_output=True, text=True,
                           check=True).stdout.split("\n")
    for dn, (name, ins, m) in sorted(zip(names, rows)):
        if flt not in dn:
            continue
        print(f"== {dn}")
        print(f"   vgpr {m['vgpr_count']} | sgpr spill slots {m['sgpr_spill_count']} | vgpr spills {m['vgpr_spill_count']}"
              f" | scratch bytes {m['private_segment_fixed_size']}")
        regs, main = regions(ins)
        if main is None:
            continue
        tot_out, slot, step = [0] * len(COLS), None, None
        print("   region | " + " | ".join(COLS))
        for rn, a, b in regs:
            c = [sum(x) for x in zip(*(classify(ins[i][1]) for i in range(a, b + 1)))]
            print(f"   {rn} | " + " | ".join(str(v) for v in c))
            if rn == "slot loop":
                slot = c
                if c[3] or c[4] or c[5]:
                    bad.append(f"{dn}: slot loop has readlane {c[3]} writelane {c[4]} scratch {c[5]}")
            else:
                tot_out = [x + y for x, y in zip(tot_out, c)]
                if "step size" in rn:
                    step = c
        print("   main loop outside the slot loop | " + " | ".join(str(v) for v in tot_out))
        wps = re.search(r"propagate_kernel<\d+, \d+, \w+, \d+, (\d+)", dn)  # (the tail kernel: 1 wave/SIMD)
        if wps and wps.group(1) == "2" and m["vgpr_count"] > 256:
            bad.append(f"{dn}: {m['vgpr_count']} VGPRs")
        summary.append(f"   {dn} | {m['vgpr_count']} | {m['sgpr_spill_count']} | {m['vgpr_spill_count']} | "
                       f"{m['private_segment_fixed_size']} | {slot[6] if slot else '-'} | {step[3] if step else '-'} | "
                       f"{tot_out[3]} | {tot_out[4]}")
    print("== summary")
    print("   kernel | vgpr | sgpr spill slots | vgpr spills | scratch bytes | slot loop s_load | step size readlane | "
          "readlane outside the slot loop | writelane outside the slot loop")
    print("\n".join(summary))
    print("== checks")
    print("\n".join("   FAIL " + b for b in bad) if bad else "   every slot loop is free of lane traffic and scratch access; no 2-waves/SIMD integrator above 256 VGPRs")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    flt = ""
    if "--filter" in args:
        flt = args.pop(args.index("--filter") + 1)
        args.remove("--filter")
    here = os.path.dirname(os.path.abspath(__file__))
    sys.exit(report(args[0] if args else os.path.join(here, "..", "adiabatic_raytracer_amd", "lib", "libart.so"), flt))
