#!/usr/bin/env python3
"""Do two builds of libcholmi.so hold the same instructions for the update kernels?
python scripts/compare_codeobj.py OTHER/libcholmi.so [THIS/libcholmi.so] [name prefix ...]

Disassembles the gfx950 code object of kernels.hip in both libraries (tests/codeobj.py: disassemble) and compares,
kernel by kernel, the instruction text of every kernel whose name holds one of the prefixes (default: k_trail_update_w8,
k_syr2k_w8, k_ldl_update_w8, k_update_ptrs_w8), then of every other kernel of that code object.  OTHER is typically a
build of the parent commit (git worktree add ../parent HEAD~1; make -C ../parent/dense_linear_app_amd/csrc).  Exit
status 1 when an update kernel differs.  For each of those it prints, other build first: instructions, VGPRs, LDS and
scratch, whether the opcode multiset is equal, and whether the sequence of MFMA / LDS / global-memory / barrier /
waitcnt opcodes is.  Kernels are matched without their parameter lists (the mangled name cut at "EEv": templates
in a namespace, as all of this library's are), so a dropped parameter keeps a kernel's identity.  In EVERY kernel the
literal of the instruction behind s_getpc_b64 is left out of the comparison: it is the distance to a data symbol and
moves whenever any kernel of the code object changes size.  No GPU needed."""
import os, re, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import codeobj

args = sys.argv[1:]
if not args:
    sys.exit(__doc__)
libs = [a for a in args if a.endswith(".so")]
prefixes = [a for a in args if not a.endswith(".so")] or ["k_trail_update_w8", "k_syr2k_w8", "k_ldl_update_w8",
                                                         "k_update_ptrs_w8"]
if len(libs) == 1:
    libs.append(os.path.join(ROOT, "dense_linear_app_amd", "libcholmi.so"))
def by_kernel(d):  # mangled names up to the parameter list
    out = {k.split("EEv")[0]: v for k, v in d.items()}
    assert len(out) == len(d)
    return out
def rel(v):  # the literal behind s_getpc_b64 is a distance to data: it moves when any kernel's size does
    return [re.sub(r"0x\w+$", "<rel>", i) if j and v[j - 1].startswith("s_getpc") else i for j, i in enumerate(v)]
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
