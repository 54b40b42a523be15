#!/usr/bin/env python3
"""Do two builds of libcholmi.so return the same bits from the routines that work from a factor or a stored triangle?
python scripts/bits_vs_parent.py OTHER/libcholmi.so

Runs the same calls in two fresh child processes, one per library (the other build through LIBCHOLMI_PATH, this tree's
as usual), and prints the SHA-256 of every output, identical / DIFFERENT per line, and a count; exit status 1 when a
line differs.  OTHER is typically a build of the parent commit (see scripts/compare_codeobj.py).  The calls: lansy
(max, one, Frobenius), pocon (rcond and the number of applications), trtrs and trmm for both transposes at nrhs 1, 3,
8, 9, porfs (X, ferr, berr) and posvx 'E' at nrhs 1 and 3, and in fp64 dsposv (X, iter) at nrhs 1 and 7 and sysv_rbt
(X, iter); and, for the host scaffolding these share with the other routines of spd.hip: potrs, trtri and potri, pstrf
(piv, rank and the factor), sygst, chud and chdd (r = 1 and 3), chex (both jobs), sytrf_nopiv and sytrs_nopiv,
sytrf_rbt, sytrs_rbt and rbt_apply, symm and logdet.  Lower and Upper, fp64 and fp32, on plgsy matrices factored by the
library itself.  The shapes (N, tile) are
the smallest that reach every mask of the block kernels: (512, 64) a stored edge of 64, one block per tile of which 64
rows are valid; (192, 192) one tile; (768, 192) a padded image, blocks of 128 + 64; (1000, 192) a ragged last tile;
(1024, 256) two full blocks per tile.  A call that raises in both builds alike is listed as refused and not counted: at
(192, 192) the library takes no n x nrhs image beside a one-tile A whose edge is no multiple of 128 (the image's
stored edge is padded, A's is not), so porfs, posvx, dsposv and sysv_rbt are not reached at that shape."""
import hashlib, os, subprocess, sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SHAPES = [(512, 64), (192, 192), (768, 192), (1000, 192), (1024, 256)]


def child():
    import numpy as np
    sys.path.insert(0, ROOT)
    from dense_linear_app_amd import chameleon as ch
    ch.CHAMELEON_Init(1, 1)

    def sha(*vals):
        h = hashlib.sha256()
        for v in vals:
            h.update(np.ascontiguousarray(np.asarray(v)).tobytes())
        return h.hexdigest()

    def emit(name, fn):
        try:
            out = fn()
        except Exception as e:  # (recorded: both builds must fail alike)
            out = "raised " + " ".join(str(e).split())[:160]
        print(f"@ {name} | {out}", flush=True)

    for N, T in SHAPES:
        for dt in ("d", "s"):
            npdt = np.float64 if dt == "d" else np.float32
            cdt = ch.ChamRealDouble if dt == "d" else ch.ChamRealFloat
            desc = lambda nc: ch.CHAMELEON_Desc_Create(None, cdt, T, T, T * T, N, nc, 0, 0, N, nc, 1, 1)

            def image(M):
                d = desc(M.shape[1])
                d.from_lapack(np.asfortranarray(M.astype(npdt)))
                return d

            gen = desc(N)
            ch.CHAMELEON_dplgsy_Tile(float(N), ch.ChamUpperLower, gen, 42)
            A0 = gen.to_lapack()
            rng = np.random.default_rng(5)
            rhs = {k: rng.standard_normal((N, k)) for k in (1, 3, 7, 8, 9)}
            for u, uc in (("L", ch.ChamLower), ("U", ch.ChamUpper)):
                tag = f"{N}/{T} {'fp64' if dt == 'd' else 'fp32'} {u}"
                dA, dAF = image(A0), image(A0)
                for nm, nc in (("max", ch.ChamMaxNorm), ("one", ch.ChamOneNorm), ("fro", ch.ChamFrobeniusNorm)):
                    emit(f"{tag} lansy {nm}", lambda: sha(ch.CHAMELEON_dlansy_Tile(nc, uc, dA)))
                anorm = ch.CHAMELEON_dlansy_Tile(ch.ChamOneNorm, uc, dA)
                assert ch.CHAMELEON_dpotrf_Tile(uc, dAF) == 0
                emit(f"{tag} potrf factor", lambda: sha(dAF.to_lapack()))

                def pocon():
                    rc = ch.CHAMELEON_dpocon_Tile(uc, dAF, anorm)
                    return f"{sha(rc)} applications {ch.last_pocon_stats()['applications']}"

                emit(f"{tag} pocon", pocon)
                factor = dAF.to_lapack()

                def on_copy(M, call, *more):
                    """the matrix the call leaves in a copy of M, with its info and what `more` returns"""
                    d = image(M)
                    info = call(d)
                    return f"{sha(d.to_lapack(), *[m(d) for m in more])} info {info}"

                def potrs():
                    dX = image(rhs[3])
                    info = ch.CHAMELEON_dpotrs_Tile(uc, dAF, dX)
                    return f"{sha(dX.to_lapack())} info {info}"

                def pstrf():
                    d = image(A0)
                    info, piv, rank = ch.CHAMELEON_dpstrf_Tile(uc, d)
                    return f"{sha(d.to_lapack(), piv, rank)} info {info}"

                def ldl():
                    d, dB = image(A0), image(rhs[3])
                    info = ch.CHAMELEON_dsytrf_nopiv_Tile(uc, d)
                    info2 = ch.CHAMELEON_dsytrs_nopiv_Tile(uc, d, dB)
                    return f"{sha(d.to_lapack(), dB.to_lapack())} info {info} {info2}"

                def rbt():
                    d, dW, dB, dT = image(A0), desc(2), image(rhs[3]), image(A0)
                    info = ch.CHAMELEON_dsytrf_rbt_Tile(uc, d, dW, 2, 1)
                    info2 = ch.CHAMELEON_dsytrs_rbt_Tile(uc, d, dW, 2, dB)
                    ch.CHAMELEON_drbt_apply_Tile(uc, dT, dW, 2)
                    return f"{sha(d.to_lapack(), dW.to_lapack(), dB.to_lapack(), dT.to_lapack())} info {info} {info2}"

                def symm():
                    dB, dC = image(rhs[3]), image(rhs[3][::-1])
                    ch.CHAMELEON_dsymm_Tile(ch.ChamLeft, uc, 1.25, dA, dB, 0.5, dC)
                    return sha(dC.to_lapack())

                def logdet():
                    info, v = ch.CHAMELEON_dlogdet_Tile(dAF)
                    return f"{sha(v)} info {info}"

                emit(f"{tag} potrs nrhs 3", potrs)
                emit(f"{tag} trtri", lambda: on_copy(factor, lambda d: ch.CHAMELEON_dtrtri_Tile(uc, ch.ChamNonUnit, d)))
                emit(f"{tag} potri", lambda: on_copy(factor, lambda d: ch.CHAMELEON_dpotri_Tile(uc, d)))
                emit(f"{tag} pstrf", pstrf)
                emit(f"{tag} sygst", lambda: on_copy(A0 + np.diag(np.arange(N) % 7.0),
                                                     lambda d: ch.CHAMELEON_dsygst_Tile(1, uc, d, dAF)))
                for r in (1, 3):
                    for nm, fn in (("chud", ch.CHAMELEON_dchud_Tile), ("chdd", ch.CHAMELEON_dchdd_Tile)):
                        emit(f"{tag} {nm} r {r}", lambda: on_copy(factor, lambda d: fn(uc, d, image(rhs[r] / 4))))
                for job in (1, 2):
                    emit(f"{tag} chex job {job}", lambda: on_copy(factor, lambda d: ch.CHAMELEON_dchex_Tile(uc, d, 3, N - 2, job)))
                emit(f"{tag} sytrf_nopiv sytrs_nopiv", ldl)
                emit(f"{tag} sytrf_rbt sytrs_rbt rbt_apply", rbt)
                emit(f"{tag} symm nrhs 3", symm)
                emit(f"{tag} logdet", logdet)
                for tn, tc in (("N", ch.ChamNoTrans), ("T", ch.ChamTrans)):
                    for k in (1, 3, 8, 9):
                        def trtrs():
                            dB = image(rhs[k])
                            info = ch.CHAMELEON_dtrtrs_Tile(uc, tc, ch.ChamNonUnit, dAF, dB)
                            return f"{sha(dB.to_lapack())} info {info}"

                        def trmm():
                            dB = image(rhs[k])
                            info = ch.CHAMELEON_dtrmm_Tile(ch.ChamLeft, uc, tc, ch.ChamNonUnit, 1.25, dAF, dB)
                            return f"{sha(dB.to_lapack())} info {info}"

                        emit(f"{tag} trtrs {tn} nrhs {k}", trtrs)
                        emit(f"{tag} trmm {tn} nrhs {k}", trmm)
                for k in (1, 3):
                    def porfs():
                        dB, dX = image(rhs[k]), image(rhs[k])
                        assert ch.CHAMELEON_dpotrs_Tile(uc, dAF, dX) == 0
                        info, ferr, berr = ch.CHAMELEON_dporfs_Tile(uc, dA, dAF, dB, dX)
                        return f"{sha(dX.to_lapack(), ferr, berr)} info {info}"

                    def posvx():
                        eA, eAF, dS = image(A0), desc(N), desc(1)
                        dB, dX = image(rhs[k]), image(np.zeros((N, k)))
                        info, eq, rcond, ferr, berr = ch.CHAMELEON_dposvx_Tile("E", uc, eA, eAF, "N", dS, dB, dX)
                        return f"{sha(dX.to_lapack(), ferr, berr, rcond, eAF.to_lapack())} info {info} equed {eq}"

                    emit(f"{tag} porfs nrhs {k}", porfs)
                    emit(f"{tag} posvx E nrhs {k}", posvx)
                if dt != "d":
                    continue
                for k in (1, 7):
                    def dsposv():
                        dB, dX = image(rhs[k]), image(np.zeros((N, k)))
                        info, it = ch.CHAMELEON_dsposv_Tile(uc, dA, dB, dX)
                        return f"{sha(dX.to_lapack())} info {info} iter {it}"

                    emit(f"{tag} dsposv nrhs {k}", dsposv)

                def sysv_rbt():
                    rAF, dW, dB, dX = desc(N), desc(2), image(rhs[3]), image(np.zeros((N, 3)))
                    info, it, berr = ch.CHAMELEON_dsysv_rbt_Tile(uc, dA, rAF, dW, 2, 1, dB, dX)
                    return f"{sha(dX.to_lapack(), berr)} info {info} iter {it}"

                emit(f"{tag} sysv_rbt nrhs 3", sysv_rbt)


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    if sys.argv[1] == "--child":
        return child()
    runs = []
    for lib in (os.path.abspath(sys.argv[1]), None):  # (a fresh process per library; this one never opens the GPU)
        env = dict(os.environ)
        env.pop("LIBCHOLMI_PATH", None)
        if lib:
            env["LIBCHOLMI_PATH"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"the run with {lib or 'this build'} ended with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        runs.append(dict(l[2:].split(" | ", 1) for l in r.stdout.splitlines() if l.startswith("@ ")))
    other, this = runs
    names = list(other) + [k for k in this if k not in other]
    same = refused = 0
    print("# scripts/bits_vs_parent.py: SHA-256 of every output, the other build against this one (N/tile dtype uplo call)")
    for k in names:
        a, b = other.get(k, "missing"), this.get(k, "missing")
        if a == b and a.startswith("raised "):  # (no output to compare: the library refuses the call in both builds)
            refused += 1
            print(f"{k:36s} refused    {b}")
            continue
        same += a == b
        print(f"{k:36s} {'identical' if a == b else 'DIFFERENT'}  {b if a == b else a + '  !=  ' + b}")
    print(f"{same} of {len(names) - refused} outputs identical; {refused} calls refused alike by both builds, nothing compared")
    sys.exit(0 if same == len(names) - refused else 1)


if __name__ == "__main__":
    main()
