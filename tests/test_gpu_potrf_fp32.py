"""The fp32 factorisation on matrices whose off-diagonal mass comes from the trailing update.

plgsy with bump = N is so diagonally dominant that a factor computed with a whole panel's update missing still
passes a check normalised by max|L| (a diagonal entry, about sqrt(N)).  Here the input is

  * gram:     M M^T / N + 0.05 I, M uniform in [-1, 1]  (kappa_2 about 30), or
  * kappa1e3: Q diag(logspace(0, -3)) Q^T               (kappa_2 = 1e3, as spd_spectral of test_gpu_conditioning.py),

rounded to fp32; the reference is the fp64 factor of that fp32 input.  Checked: the componentwise backward error
|L L^T - A| <= 8 B eps32 |L||L^T| (Higham Th. 10.3, the bound of test_gpu_conditioning.py with eps32), and the
forward error, both as max|L - Lref| / max|Lref| and over the strictly lower triangle, normalised by that
triangle's own maximum.

Forward-error bounds, per matrix kind, about 10x the largest error measured on the MI355X over the cases below
(full / strictly lower): gram 6e-6 / 1.2e-5 (measured 5.5e-7 / 1.1e-6), kappa1e3 3e-5 / 6e-5 (measured 2.6e-6 /
5.1e-6).  (LAPACK's spotrf on the CPU comes to about 5e-8 on all of them; the GPU factor solves with explicitly
inverted 128 x 128 diagonal blocks, whose error grows with their condition.  The backward error stays below 5e-3 of
its bound.)  A CPU model of the tiled algorithm on the same matrices and shapes, one fault per run, moves the factor
by at least 1.4e-2 (full) and 1.4e-1 (strictly lower) when the first 32 K-columns of every update are dropped, by at
least 1.6e-2 when one 128 x 128 block of the update of tile (2, 1) from panel 0 is dropped, and by at least 2.0e-2
when that tile's whole update is dropped, unless the matrix then fails to factor: at least 1000x the bound of its kind.
"""
import numpy as np
import pytest

from chol_testkit import spd_spectral

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
FWD = {"gram": (6e-6, 1.2e-5), "kappa1e3": (3e-5, 6e-5)}  # (full, strictly lower)


def spd_gram(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.uniform(-1, 1, (n, n))
    return M @ M.T / n + 0.05 * np.eye(n)


def spd_spectral_rowmajor(n, kappa, seed):
    """chol_testkit.spd_spectral in C order, as this file has always rounded it to fp32: the matrix is symmetric bit
    for bit, so its transposed view is that"""
    return spd_spectral(n, kappa, seed).T


def fp32_input(kind, N, B):
    A = spd_gram(N, 7 * N + B) if kind == "gram" else spd_spectral_rowmajor(N, 1e3, 11 * N + B)
    return np.asfortranarray(A.astype(np.float32).astype(np.float64))


def factor_on_gpu(ch, A, B, uplo):
    N = A.shape[0]
    d = ch.CHAMELEON_Desc_Create(None, ch.ChamRealFloat, B, B, B * B, N, N, 0, 0, N, N, 1, 1)
    try:
        d.from_lapack(A)
        info = ch.CHAMELEON_spotrf_Tile(uplo, d)
        R = d.to_lapack().astype(np.float64)
    finally:
        ch.CHAMELEON_Desc_Destroy(d)
    return info, R


def errors(L, A, B):
    """(backward error / its bound, max-rel forward error, strictly-lower self-normalised forward error)"""
    Lref = np.linalg.cholesky(A)
    E = np.abs(np.tril(L @ L.T - A))
    bound = 8 * B * EPS32 * np.tril(np.abs(L) @ np.abs(L).T)
    back = float((E / (bound + 1e-300)).max())
    full = np.abs(L - Lref).max() / np.abs(Lref).max()
    sl = np.abs(np.tril(L - Lref, -1)).max() / np.abs(np.tril(Lref, -1)).max()
    return back, full, sl


@pytest.mark.parametrize("kind", ["gram", "kappa1e3"])
@pytest.mark.parametrize("N,B", [(2048, 512), (3072, 256), (3072, 384), (4096, 1024), (1000, 192)])
def test_fp32_potrf_where_the_update_carries_the_factor(cham, kind, N, B):
    ch = cham
    A = fp32_input(kind, N, B)
    info, R = factor_on_gpu(ch, A, B, ch.ChamLower)
    assert info == 0
    back, full, sl = errors(np.tril(R), A, B)
    assert back <= 1.0 and full <= FWD[kind][0] and sl <= FWD[kind][1], (back, full, sl)


def test_fp32_potrf_upper_where_the_update_carries_the_factor(cham):
    """ChamUpper: U = L^T in the upper triangle, the strict lower triangle of the storage left as it was."""
    ch = cham
    N, B = 3072, 384
    A = fp32_input("gram", N, B)
    info, R = factor_on_gpu(ch, A, B, ch.ChamUpper)
    assert info == 0
    assert np.array_equal(np.tril(R, -1), np.tril(A, -1))
    back, full, sl = errors(np.triu(R).T, A, B)
    assert back <= 1.0 and full <= FWD["gram"][0] and sl <= FWD["gram"][1], (back, full, sl)
