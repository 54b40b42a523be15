"""What the tests of the routines share: the dtype and code maps, the bit view, the triangle helpers and the two ways of
storing a matrix in one triangle, the descriptor constructor, access to a descriptor's stored image on the device, and
the scaffolds of the tests that every routine repeats (a P x Q descriptor is refused, a sub-matrix view of a user
buffer, the padding of a ragged image, the checks without a GPU, a case list run in a fresh child process).  A plain module, imported like the *_model.py files:
no fixtures, no hooks.  It needs numpy alone to import; ctypes, torch and the library are touched inside the helpers
that use them, so the modules that import it still import on a machine without a GPU.

test_testkit_host.py holds the storing helpers to the numpy one-liners they replaced, bit for bit."""
import functools

import numpy as np

U = {"d": 2.0 ** -53, "s": 2.0 ** -24}  # the unit roundoff


# ---------------------------------------------------------------- dtypes and codes
def npdt(dt):
    return np.float64 if dt == "d" else np.float32


def chdt(ch, dt):
    return ch.ChamRealDouble if dt == "d" else ch.ChamRealFloat


def uplo_code(ch, u):
    return ch.ChamLower if u == "L" else ch.ChamUpper


def gamma(k, dt):
    """gamma_k = k u / (1 - k u)"""
    return k * U[dt] / (1 - k * U[dt])


def bits(a):
    """the entries as unsigned integers: equal bits, signed zeros and NaN payloads included"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---------------------------------------------------------------- triangles
def other(n, u, k=1):
    """indices of the strict triangle (from diagonal k on) that a `u` call must leave alone"""
    return np.triu_indices(n, k) if u == "L" else np.tril_indices(n, -k)


def lower_of(F, u):
    """what the `u` triangle of F stores, as Lower"""
    return np.tril(F) if u == "L" else np.triu(F).T


def other_triangle_kept(F, S, u):
    idx = other(S.shape[0], u)
    return np.array_equal(bits(F[idx]), bits(S[idx]))


def _fill_other(S, u, fill):
    idx = other(S.shape[0], u)
    S[idx] = fill[idx] if isinstance(fill, np.ndarray) else fill
    return S


def stored_lower(M, u, fill=np.nan):
    """the lower triangle of M (a Lower factor, or a symmetric matrix) put into the `u` triangle -- transposed for
    Upper -- and the other strict triangle = fill (a scalar, or an array read at those places); Fortran order"""
    return _fill_other(np.array(np.tril(M) if u == "L" else np.tril(M).T, order="F"), u, fill)


def stored_sym(A, u, fill=np.nan):
    """the `u` triangle of the symmetric A as it is, the other strict triangle = fill; Fortran order"""
    return _fill_other(np.array(A, order="F"), u, fill)


# ---------------------------------------------------------------- descriptors and their stored images
def desc(ch, n, tile, dt="d", cols=None, content=None):
    """an n x cols (default n) descriptor of the library's own storage on a 1 x 1 grid, filled with content if given"""
    cols = n if cols is None else cols
    d = ch.CHAMELEON_Desc_Create(None, chdt(ch, dt), tile, tile, tile * tile, n, cols, 0, 0, n, cols, 1, 1)
    if content is not None:
        d.from_lapack(np.asarray(content, dtype=npdt(dt)))
    return d


@functools.lru_cache(maxsize=None)
def _hip():
    """the HIP runtime this process has loaded"""
    import ctypes

    path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
    return ctypes.CDLL(path)


def raw_image(d):
    """the descriptor's stored tile image as bytes, padding included; .view() it to the dtype"""
    import ctypes

    ptr, nbytes = d.local_ptr()
    out = np.empty(nbytes, dtype=np.uint8)
    assert _hip().hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 2) == 0
    return out


def put_image(d, img):
    import ctypes

    ptr, nbytes = d.local_ptr()
    assert img.nbytes == nbytes
    assert _hip().hipMemcpy(ctypes.c_void_p(ptr), ctypes.c_void_p(img.ctypes.data), ctypes.c_size_t(nbytes), 1) == 0


def image_matrix(d, nt, B, dtype):
    """the stored image of nt x nt tiles of edge B as one (nt B) x (nt B) matrix"""
    return raw_image(d).view(dtype)[: nt * nt * B * B].reshape(nt, nt, B, B).transpose(1, 3, 0, 2).reshape(nt * B, nt * B)


def ragged_padding_mask(n, B, nt):
    """True at the padding of that matrix: the rows and columns from n on"""
    pad = np.zeros((nt * B, nt * B), dtype=bool)
    pad[n:, :] = pad[:, n:] = True
    return pad


# ---------------------------------------------------------------- scaffolds
def pxq_refused(ch, ndesc, *calls, tile=256, n=1024):
    """every call(*descriptors) on descriptors of a 1 x 2 grid raises CholmiError -104 (CHOL_ERR_NOT_SUPPORTED).
    ndesc: how many n x n descriptors, or their column counts"""
    import pytest

    from dense_linear_app_amd._lib import lib

    lib().chol_set_transport(None)
    ch.set_rank(0, 2)
    try:
        cols = (n,) * ndesc if isinstance(ndesc, int) else ndesc
        ds = [ch.CHAMELEON_Desc_Create(None, ch.ChamRealDouble, tile, tile, tile * tile, n, c, 0, 0, n, c, 1, 2)
              for c in cols]
        for call in calls:
            with pytest.raises(ch.CholmiError) as e:
                call(*ds)
            assert e.value.code == -104
        for d in ds:
            ch.CHAMELEON_Desc_Destroy(d)
    finally:
        ch.set_rank(0, 1)


class UserView:
    """a random fp64 user buffer of lt x lt tiles of edge mb on the device, and the tile-aligned view of vt x vt tiles
    at tile (oi, oj) of it; m is the view's order"""

    def __init__(self, ch, mb=256, lt=5, oi=1, oj=2, vt=3, seed=16):
        import torch

        self.ch, self.mb, self.lt, self.oi, self.oj, self.vt, self.m = ch, mb, lt, oi, oj, vt, vt * mb
        self.user = np.random.default_rng(seed).standard_normal(lt * lt * mb * mb)
        self.buf = torch.from_numpy(self.user.copy()).cuda()

    def view_desc(self):
        ch, mb, lm, m = self.ch, self.mb, self.lt * self.mb, self.m
        return ch.CHAMELEON_Desc_Create(self.buf, ch.ChamRealDouble, mb, mb, mb * mb, lm, lm, self.oi * mb,
                                        self.oj * mb, m, m, 1, 1)

    def outside_unchanged(self):
        """asserts that the user's tiles outside the view are what they were"""
        lt, oi, oj, vt = self.lt, self.oi, self.oj, self.vt
        now = self.buf.cpu().numpy().reshape(lt * lt, self.mb * self.mb)
        before = self.user.reshape(lt * lt, self.mb * self.mb)
        for J in range(lt):
            for I in range(lt):
                if not (oi <= I < oi + vt and oj <= J < oj + vt):
                    assert np.array_equal(now[I + J * lt], before[I + J * lt]), (I, J)


def assert_symbols_exported(symbols):
    """the header declares them and the library exports them"""
    from dense_linear_app_amd import _lib

    for s in symbols:
        assert s in _lib.abi_symbols()
        assert hasattr(_lib.lib(), s)


def assert_before_init_refused(sym, args):
    from dense_linear_app_amd import _lib

    L = _lib.lib()
    assert getattr(L, sym)(*args) == -101  # CHOL_ERR_NOT_INITIALIZED
    assert b"before chol_init" in L.chol_last_error()


# ---------------------------------------------------------------- child processes
def run_child(script, args, env, timeout, what):
    """`script args` in one fresh python process under the environment switches `env` (the library reads them once, at
    chol_init) with a time limit of its own -> the records of its "CASE <json>" lines.  A child that hangs or is killed by
    a signal (a GPU fault or abort, not a wrong number) ends the whole session: nothing more is started on that GPU"""
    import json
    import os
    import subprocess
    import sys

    import pytest

    try:
        r = subprocess.run([sys.executable, os.path.abspath(script), *args], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the child of {what} hung: nothing more is started on this GPU ({e.stdout})", returncode=3)
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"the child of {what} died ({r.returncode}): nothing more is started on this GPU\n"
                    f"{r.stdout}\n{r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    return [json.loads(ln[5:]) for ln in r.stdout.splitlines() if ln.startswith("CASE ")]


# ---------------------------------------------------------------- matrices
def spd_spectral(n, kappa, seed):
    """Q diag(logspace(0, -log10 kappa)) Q^T: kappa_2 = kappa exactly (up to rounding); Fortran order"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n)
    A = (Q * lam) @ Q.T
    return np.asfortranarray((A + A.T) * 0.5)
