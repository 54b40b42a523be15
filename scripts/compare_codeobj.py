#!/usr/bin/env python3
"""Do two builds of libcholmi.so hold the same instructions for the update kernels?
python scripts/compare_codeobj.py OTHER/libcholmi.so [THIS/libcholmi.so] [name prefix ...]
python scripts/compare_codeobj.py --all OTHER/libcholmi.so [THIS/libcholmi.so]

Disassembles the gfx950 code object of kernels.hip in both libraries (tests/codeobj.py: disassemble) and compares,
kernel by kernel, the instruction text of every kernel whose name holds one of the prefixes (default: k_trail_update_w8,
k_syr2k_w8, k_ldl_update_w8, k_update_ptrs_w8), then of every other kernel of that code object.  OTHER is typically a
build of the parent commit (git worktree add ../parent HEAD~1; make -C ../parent/dense_linear_app_amd/csrc).  Exit
status 1 when an update kernel differs.  For each of those it prints, other build first: instructions, VGPRs, LDS and
scratch, whether the opcode multiset is equal, and whether the sequence of MFMA / LDS / global-memory / barrier /
waitcnt opcodes is.  Kernels are matched without their parameter lists (the mangled name cut at "EEv": templates
in a namespace, as all of this library's are), so a dropped parameter keeps a kernel's identity.  In EVERY kernel the
literal of the instruction behind s_getpc_b64 is left out of the comparison: it is the distance to a data symbol and
moves whenever any kernel of the code object changes size.  No GPU needed.

--all: every kernel of every code object of the library (one per .hip file, in link order; tests/codeobj.py:
device_elfs), one line each: identical / differs / only in one build, with instructions, VGPRs, LDS and scratch, other
build first.  A kernel is matched by name wherever it lies, so one that moved to another file keeps its identity.
Exit status 1 when a kernel gains scratch or its VGPR allocation crosses an occupancy step: the waves a SIMD of
gfx950 holds, min(8, 512 // VGPRs)."""
import os, re, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj

args = sys.argv[1:]
if not args:
    sys.exit(__doc__)
libs = [a for a in args if a.endswith(".so")]
if len(libs) == 1:
    libs.append(os.path.join(ROOT, "dense_linear_app_amd", "libcholmi.so"))
prefixes = [a for a in args if not a.endswith(".so")] or ["k_trail_update_w8", "k_syr2k_w8", "k_ldl_update_w8",
                                                         "k_update_ptrs_w8"]
def by_kernel(d):  # mangled names up to the parameter list
    out = {k.split("EEv")[0]: v for k, v in d.items()}
    assert len(out) == len(d)
    return out
def rel(v):  # the literal behind s_getpc_b64 is a distance to data: it moves when any kernel's size does
    return [re.sub(r"0x\w+$", "<rel>", i) if j and v[j - 1].startswith("s_getpc") else i for j, i in enumerate(v)]
def whole(path):  # {kernel: (code object, instructions, resources)} over every code object
    out = {}
    for n, elf in enumerate(codeobj.device_elfs(path)):
        res = by_kernel(codeobj.kernel_resources(path, elf))
        for k, v in by_kernel(codeobj.disassemble(path, elf=elf)).items():
            if k in res:
                assert k not in out, k
                out[k] = (n, rel(v), res[k])
    return out
if "--all" in args:
    a, b = whole(libs[0]), whole(libs[1])
    bad = same = 0
    show = lambda e: f"{len(e[1])} instructions, {e[2]['vgprs']} VGPRs, {e[2]['lds']} LDS, {e[2]['scratch']} scratch"
    for k in sorted(set(a) | set(b), key=lambda k: (b.get(k) or a[k])[0]):
        ea, eb = a.get(k), b.get(k)
        if ea and eb and ea[1] == eb[1] and ea[2] == eb[2]:
            same += 1
            print(f"[{eb[0]:2d}] identical  {k}: {show(eb)}")
        elif ea and eb:
            waves = lambda e: min(8, 512 // e[2]["vgprs"])
            worse = eb[2]["scratch"] > ea[2]["scratch"] or waves(eb) != waves(ea)
            bad += worse
            print(f"[{eb[0]:2d}] differs    {k}: {show(ea)} -> {show(eb)}" + ("  <-- scratch / occupancy" if worse else ""))
        else:
            print(f"[{(ea or eb)[0]:2d}] only in {'other' if ea else 'this '} {k}: {show(ea or eb)}")
    print(f"{len(set(a) | set(b))} kernels, {same} identical, {bad} with more scratch or another occupancy step")
    sys.exit(1 if bad else 0)
a, b = ({k: rel(v) for k, v in by_kernel(codeobj.disassemble(p)).items()} for p in libs[:2])
ra, rb = (by_kernel(codeobj.kernel_resources(p)) for p in libs[:2])
ops = lambda ins: [i.split()[0] for i in ins]
mem = lambda ins: [o for o in ops(ins) if re.match(r"v_mfma|ds_|global_|s_barrier|s_waitcnt", o)]
upd = sorted(k for k in a if any(p in k for p in prefixes))
diff = [k for k in upd if a[k] != b.get(k)]
rest = [k for k in a if k not in upd and a[k] != b.get(k)]
print(f"update kernels: {len(upd)}, {sum(len(a[k]) for k in upd)} instructions, {len(upd) - len(diff)} identical")
for k in diff:
    print("  differs:", k)
    if k in b:
        res = ", ".join(f"{r} {ra[k][r]} -> {rb[k][r]}" for r in ("vgprs", "lds", "scratch"))
        eq = lambda f: "equal" if f(a[k]) == f(b[k]) else "differs"
        print(f"    instructions {len(a[k])} -> {len(b[k])}, {res}, opcode multiset {eq(lambda i: sorted(ops(i)))}, "
              f"memory / MFMA / barrier / waitcnt sequence {eq(mem)}")
print(f"other kernels of the code object: {len(a) - len(upd)}, {len(rest)} differ, names {'equal' if set(a) == set(b) else 'differ'}")
sys.exit(1 if diff or not upd else 0)
