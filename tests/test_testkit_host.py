"""chol_testkit's pure helpers against what they replaced.  The test files used to carry eight bodies of `stored`; they
were two operations, and on every input the tests pass they agree bit for bit with the two helpers that remain: here
each retired body is written out as the numpy one-liner it was and compared, on a non-symmetric 5 x 5 matrix and its
symmetrised form, both triangles, a NaN, a zero and an array as the fill.  Also: lower_of undoes stored_lower, other
is triu_indices / tril_indices, and bits tells apart what == cannot."""
import numpy as np
import pytest

from chol_testkit import bits, lower_of, other, other_triangle_kept, stored_lower, stored_sym

N = 5
M = np.random.default_rng(5).standard_normal((N, N))
SYM = M + M.T
FILLS = [np.nan, 0.0, np.arange(100.0, 100.0 + N * N).reshape(N, N)]


def filled(S, u, fill):
    """S in Fortran order with the strict triangle that `u` leaves alone overwritten, as every retired body did"""
    S = np.array(S, order="F")
    idx = np.triu_indices(N, 1) if u == "L" else np.tril_indices(N, -1)
    S[idx] = fill[idx] if isinstance(fill, np.ndarray) else fill
    return S


def identical(a, b):
    return (a.dtype == b.dtype and a.flags.f_contiguous and b.flags.f_contiguous
            and np.array_equal(bits(a), bits(b)))


@pytest.mark.parametrize("fill", FILLS, ids=["nan", "zero", "array"])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stored_lower_is_every_retired_body(u, fill, dtype):
    for A in (M.astype(dtype), SYM.astype(dtype)):
        got = stored_lower(A, u, fill)
        retired = [np.tril(A).T, np.triu(np.tril(A).T), np.triu(A.T), A.T]  # (A.T: the factor-only body of the inverse tests)
        for body in ([np.tril(A), A] if u == "L" else retired):
            assert identical(got, filled(body, u, fill))
        assert np.array_equal(lower_of(got, u), np.tril(A))


@pytest.mark.parametrize("fill", FILLS, ids=["nan", "zero", "array"])
@pytest.mark.parametrize("u", ["L", "U"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_stored_sym_is_the_retired_body(u, fill, dtype):
    A = SYM.astype(dtype)
    got = stored_sym(A, u, fill)
    assert identical(got, filled(A, u, fill))  # plain A, its `u` triangle as it is
    kept = np.tril_indices(N) if u == "L" else np.triu_indices(N)
    assert np.array_equal(bits(got[kept]), bits(A[kept]))
    # on a symmetric matrix the two helpers store the same thing; on M they do not
    assert identical(got, stored_lower(A, u, fill))
    assert not np.array_equal(stored_sym(M, "U", 0.0), stored_lower(M, "U", 0.0))


def test_other_and_other_triangle_kept():
    for k in (1, 2):
        assert all(np.array_equal(a, b) for a, b in zip(other(N, "L", k), np.triu_indices(N, k)))
        assert all(np.array_equal(a, b) for a, b in zip(other(N, "U", k), np.tril_indices(N, -k)))
    assert all(np.array_equal(a, b) for a, b in zip(other(N, "L"), np.triu_indices(N, 1)))
    for u in "LU":
        S = stored_lower(M, u)
        F = S.copy()
        F[np.tril_indices(N) if u == "L" else np.triu_indices(N)] = 7.0  # all of the `u` triangle
        assert other_triangle_kept(F, S, u)  # (NaN against NaN: compared as bits)
        F[other(N, u)[0][0], other(N, u)[1][0]] = 0.0
        assert not other_triangle_kept(F, S, u)


@pytest.mark.parametrize("dtype,word", [(np.float64, np.uint64), (np.float32, np.uint32)])
def test_bits(dtype, word):
    a = M.astype(dtype)
    b = bits(a)
    assert b.dtype == word and b.shape == a.shape and np.array_equal(b.view(dtype), a)
    assert np.array_equal(bits(np.asfortranarray(a)), b)  # (the entries, whatever the memory order)
    zeros = np.array([0.0, -0.0], dtype=dtype)
    assert zeros[0] == zeros[1] and bits(zeros)[0] != bits(zeros)[1]
    quiet = np.array([np.nan], dtype=dtype)
    other_payload = (bits(quiet) | word(1)).view(dtype)
    assert np.isnan(other_payload[0]) and bits(quiet)[0] != bits(other_payload)[0]
    assert np.array_equal(bits(quiet), bits(quiet.copy())) and not np.array_equal(quiet, quiet)
