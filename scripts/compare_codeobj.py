#!/usr/bin/env python3
"""Do two builds of libcholmi.so hold the same instructions for the update kernels?
python scripts/compare_codeobj.py OTHER/libcholmi.so [THIS/libcholmi.so] [name prefix ...]

Disassembles the gfx950 code object of kernels.hip in both libraries (tests/codeobj.py: disassemble) and compares,
kernel by kernel, the instruction text of every kernel whose name holds one of the prefixes (default: k_trail_update_w8,
k_syr2k_w8, k_ldl_update_w8, k_update_ptrs_w8), then of every other kernel of that code object.  OTHER is typically a
build of the parent commit (git worktree add ../parent HEAD~1; make -C ../parent/dense_linear_app_amd/csrc).  Exit
status 1 when an update kernel differs.  No GPU needed."""
import os, sys
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
a, b = (codeobj.disassemble(p) for p in libs[:2])
upd = sorted(k for k in a if any(p in k for p in prefixes))
diff = [k for k in upd if a[k] != b.get(k)]
rest = [k for k in a if k not in upd and a[k] != b.get(k)]
print(f"update kernels: {len(upd)}, {sum(len(a[k]) for k in upd)} instructions, {len(upd) - len(diff)} identical")
for k in diff:
    print("  differs:", k)
print(f"other kernels of the code object: {len(a) - len(upd)}, {len(rest)} differ, names {'equal' if set(a) == set(b) else 'differ'}")
sys.exit(1 if diff or not upd else 0)
