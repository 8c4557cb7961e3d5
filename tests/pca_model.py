"""mg_pca_solve's reference, its checks, and a plain numpy restatement of its method.

The reference is numpy.linalg.eigh in float64.  The checks are functions of (G, result) and are the same for the restatement here and for
the device.  The restatement follows csrc/pca_kernels.h step for step -- the hashed start block, Cholesky QR twice with collapsed columns
replaced, a Rayleigh-Ritz step after every 4th product and after the last one allowed -- but sums in numpy's order and solves the small
eigenproblem with eigh, so it agrees with the device to rounding, not to the bit.

Notation of the bounds: L the largest |eigenvalue| of eigh (1 when that is 0), eps = 2^-52, allowance = tol L + 64 n eps L."""
import functools

import numpy as np

import pca_cases

EPS = 2.0 ** -52
CHECK_EVERY = 4
COLLAPSE, NOTHING = 1e-10, 1e-60
U64 = np.uint64


def reference(G):
    """-> (eigenvalues descending, eigenvectors as rows, L)"""
    w, V = np.linalg.eigh(np.asarray(G, dtype=np.float64))
    w, V = w[::-1].copy(), V[:, ::-1].T.copy()
    L = float(np.abs(w).max())
    return w, V, (L if L > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """the reference of a case of pca_cases, computed once"""
    return reference(pca_cases.matrix(pca_cases.BY_NAME[name]))


def allowance(n, L, tol):
    return tol * L + 64 * n * EPS * L


# ---- the checks ----------------------------------------------------------------------------------------------------------------------------

def check_result(G, ref, k, tol, values, vectors, resid, scale, info, cap, expect_converged=True):
    """every property the contract promises of a solve; prints each figure before it asserts"""
    w, Vref, L = ref
    n = G.shape[0]
    allow = allowance(n, L, tol)
    products, converged, m = info
    assert m == pca_cases.block(n, k)
    assert values.shape == (k,) and vectors.shape == (k, n) and resid.shape == (k,)
    assert products <= cap, "%d products, cap %d" % (products, cap)
    if m == n:
        assert products == 0
    if expect_converged:
        assert converged == k, "converged %d of %d after %d products; resid %s" % (converged, k, products, resid)
        assert (resid <= tol).all()
    assert converged == int((resid <= tol).sum())
    assert (np.diff(values) <= 0).all(), "values are not descending"
    # the recomputed residuals, and the returned ones against them
    R = vectors @ G - values[:, None] * vectors
    rnorm = np.sqrt((R * R).sum(axis=1))
    print("k=%d n=%d products=%d max|theta-lambda|=%.3e max resid=%.3e allowance=%.3e" % (k, n, products, np.abs(values - w[:k]).max(), rnorm.max(), allow))
    if expect_converged:
        assert (np.abs(values - w[:k]) <= allow).all(), "eigenvalues: %s against %s" % (values, w[:k])
        assert (rnorm <= allow).all(), "recomputed residuals %s above %.3e" % (rnorm, allow)
    for got, true in zip(resid * scale, rnorm):
        assert (got <= allow and true <= allow) or 0.5 * true <= got <= 2 * true, "resid_out %.3e against %.3e recomputed" % (got, true)
    # orthonormality, the sign rule
    ortho = np.abs(vectors @ vectors.T - np.eye(k)).max()
    print("orthonormality %.3e (bound %.3e)" % (ortho, 64 * n * EPS))
    assert ortho <= 64 * n * EPS
    for v in vectors:
        at = int(np.argmax(np.abs(v)))
        assert v[at] > 0, "sign rule: component %d is %g" % (at, v[at])
    if not expect_converged:
        return
    # isolated eigenvectors (Davis-Kahan)
    for i in range(k):
        gap = np.abs(np.delete(w, i) - w[i]).min() if n > 1 else np.inf
        if gap >= 0.05 * L:
            d = min(np.linalg.norm(vectors[i] - Vref[i]), np.linalg.norm(vectors[i] + Vref[i]))
            assert d <= 2 * allow / gap, "vector %d: %.3e from the reference, bound %.3e" % (i, d, 2 * allow / gap)


def check_projector(vectors, ref, first, gap, n, tol):
    """the projector onto the first `first` vectors against the reference's (a repeated eigenvalue)"""
    w, Vref, L = ref
    P, Pref = vectors[:first].T @ vectors[:first], Vref[:first].T @ Vref[:first]
    d = np.linalg.norm(P - Pref, 2)
    assert d <= 2 * allowance(n, L, tol) / gap, "projector %.3e from the reference's" % d


# ---- the method ------------------------------------------------------------------------------------------------------------------------------

def hash_block(n, m, salt, cols=None):
    """pca_hash_value of csrc/pca_plan.h over rows 0 .. n - 1 and columns 0 .. m - 1 (or `cols`)"""
    cols = np.arange(m, dtype=U64) if cols is None else np.asarray(cols, dtype=U64)
    with np.errstate(over="ignore"):
        x = (np.arange(n, dtype=U64)[:, None] * U64(0x9E3779B97F4A7C15) + cols[None, :] * U64(0xBF58476D1CE4E5B9)
             + U64(salt) * U64(0x94D049BB133111EB) + U64(0x2545F4914F6CDD1D))
        x ^= x >> U64(30)
        x *= U64(0xBF58476D1CE4E5B9)
        x ^= x >> U64(27)
        x *= U64(0x94D049BB133111EB)
        x ^= x >> U64(31)
    return (x >> U64(11)).astype(np.float64) * (1.0 / 4503599627370496.0) - 1.0


def _chol_inverse(W):
    """pca_chol_kernel: -> (R^-1 over the live columns, 0 in the row and column of a collapsed one; the collapsed columns)"""
    m = W.shape[0]
    S = np.triu(W).astype(np.float64)
    d0 = np.diag(W).copy()
    wmax = max(0.0, d0.max())
    dead = np.zeros(m, dtype=bool)
    for j in range(m):
        d = S[j, j]
        if not (d > COLLAPSE * d0[j] and d0[j] > NOTHING * wmax):
            dead[j] = True
            S[j, j:] = 0.0
            continue
        S[j, j:] /= np.sqrt(d)
        S[j + 1:, j + 1:] -= np.triu(np.outer(S[j, j + 1:], S[j, j + 1:]))
    live = ~dead
    Rinv = np.zeros((m, m))
    if live.any():
        Rinv[np.ix_(live, live)] = np.linalg.inv(S[np.ix_(live, live)])
    return Rinv, dead


def _orthonormalise(X, salt):
    n, m = X.shape
    Rinv, dead = _chol_inverse(X.T @ X)
    T = X @ Rinv
    if dead.any():
        T[:, dead] = hash_block(n, m, salt, np.nonzero(dead)[0])
    Rinv, _ = _chol_inverse(T.T @ T)
    return T @ Rinv


def _sign(v):
    return -v if v[int(np.argmax(np.abs(v)))] < 0 else v


def solve(G, k, tol, max_iters):
    """-> (values [k], vectors [k, n], resid [k], scale, (products, converged, m)), as mg_pca_solve returns them"""
    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    m = pca_cases.block(n, k)
    products = 0
    if m == n:
        theta, S = np.linalg.eigh(G)
        theta, Q = theta[::-1], S[:, ::-1]
        Y = G @ Q
    else:
        salt = 0
        Q = _orthonormalise(hash_block(n, m, salt), salt + 1)
        salt += 2
        while True:
            Y = G @ Q
            products += 1
            if products % CHECK_EVERY == 0 or products == max_iters:
                H = Q.T @ Y
                theta, S = np.linalg.eigh((H + H.T) / 2)
                theta, S = theta[::-1], S[:, ::-1]
                Q, Y = Q @ S, Y @ S
                scale = np.abs(theta).max() or 1.0
                norms = np.sqrt(((Y - Q * theta[None, :]) ** 2).sum(axis=0))
                if (norms[:k] / scale <= tol).all() or products == max_iters:
                    break
            Q = _orthonormalise(Y, salt)
            salt += 1
    scale = float(np.abs(theta).max()) or 1.0
    norms = np.sqrt(((Y - Q * theta[None, :]) ** 2).sum(axis=0))
    resid = norms[:k] / scale
    vectors = np.stack([_sign(Q[:, j]) for j in range(k)])
    return theta[:k].copy(), vectors, resid, scale, (products, int((resid <= tol).sum()), m)


# ---- the command line's files, as Python formats them ------------------------------------------------------------------------------------------

def format_files(names, G_trace, values, vectors, resid, scale, info, tol, ms):
    """-> (eigenval, eigenvec, pca.tsv without its trailer line) as `malva-geno pca` writes them"""
    k = len(values)
    eigenval = "".join("%.10g\n" % v for v in values)
    eigenvec = "".join("%s\t%s\t%s\n" % (nm, nm, "\t".join("%.10g" % vectors[j, i] for j in range(k))) for i, nm in enumerate(names))
    rows = ["PC\tEIGENVALUE\tSHARE\tRESIDUAL\tCONVERGED\n"]
    for j in range(k):
        share = "%.6f" % (values[j] / G_trace) if G_trace > 0 else "."
        rows.append("%d\t%.10g\t%s\t%.3e\t%d\n" % (j + 1, values[j], share, resid[j], int(resid[j] <= tol)))
    return eigenval, eigenvec, "".join(rows)
