"""The case table of mg_pca_solve: symmetric matrices with planted spectra at every seam of the solver's geometry -- n = 1, a block as
wide as the matrix (m == n), one MFMA tile and its neighbours, the smallest iterated matrix, ragged last tiles -- and at every seam of the
method: a dominant negative direction, rank 3, a double eigenvalue inside the K, the zero matrix, MG_PCA_MAX_K, and a three-population
genetic relationship matrix in float32 whose later components sit inside the bulk.  numpy only.

Planted matrices are G = U diag(lambda) U^T, symmetrised as (G + G^T) / 2, U the Q factor of a seeded normal matrix.
m = min(n, roundup16(max(2 K, K + 16)))."""
import functools

import numpy as np

TOP = [10.0, 8.0, 6.5, 5.0, 4.0]
CAP_PLANTED, CAP_GRM_LIKE = 40, 400       # products at most, at tol 1e-10
TOL = 1e-10


def block(n, k):
    return min(n, (max(2 * k, k + 16) + 15) // 16 * 16)


def _rest(n, lo, hi, seed):
    return np.random.default_rng(1000 + seed).uniform(lo, hi, size=n)


def _top_and_rest(n, seed, lo=-0.2, hi=1.0, extra=()):
    lam = np.concatenate([TOP, list(extra), _rest(n - len(TOP) - len(extra), lo, hi, seed)])
    return lam[:n]


def planted(lam, seed):
    n = len(lam)
    U = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))[0]
    G = (U * np.asarray(lam, dtype=np.float64)[None, :]) @ U.T
    return (G + G.T) / 2


@functools.lru_cache(maxsize=None)
def grm_like(n_pop=200, n_records=5000, F=0.05, seed=7):
    """three populations of n_pop samples: binomial genotypes at frequencies drifted by F from a common one (Balding-Nichols), standardised
    per record as the GRM does, G = Z Z^T / records, rounded to float32 -> (tri float32 [n (n + 1) / 2], G float64 of the rounded values)"""
    rng = np.random.default_rng(seed)
    p0 = rng.uniform(0.1, 0.9, size=n_records)
    a, b = p0 * (1 - F) / F, (1 - p0) * (1 - F) / F
    rows = []
    for _ in range(3):
        p = rng.beta(a, b)
        rows.append(rng.binomial(2, p[None, :], size=(n_pop, n_records)))
    X = np.concatenate(rows).astype(np.float64)
    ph = X.mean(axis=0) / 2
    keep = (ph > 0.01) & (ph < 0.99)
    X, ph = X[:, keep], ph[keep]
    Z = (X - 2 * ph[None, :]) / np.sqrt(2 * ph * (1 - ph))[None, :]
    G = (Z @ Z.T) / Z.shape[1]
    n = G.shape[0]
    i, j = np.tril_indices(n)
    tri = G[i, j].astype(np.float32)
    G32 = np.zeros((n, n), dtype=np.float64)
    G32[i, j] = tri
    G32[j, i] = tri
    return tri, G32


def _case(name, lam, k, seed, seam, cap=CAP_PLANTED):
    lam = np.asarray(lam, dtype=np.float64)
    return dict(name=name, n=len(lam), spectrum=lam, k=k, seed=seed, seam=seam, cap=cap, form="f64")


def _wide_spectrum():
    return np.concatenate([np.linspace(40.0, 9.0, 32), _rest(130 - 32, 0.0, 1.0, 12)])


CASES = [
    _case("one", [3.0], 1, 1, "n = 1"),
    _case("two", [2.0, -1.0], 2, 2, "m == n, a negative value returned"),
    _case("tile-1", _top_and_rest(15, 3), 5, 3, "one MFMA tile less one; m == n"),
    _case("tile", _top_and_rest(16, 4), 5, 4, "one MFMA tile; m == n"),
    _case("tile+1", _top_and_rest(17, 5), 5, 5, "one MFMA tile and one; m == n"),
    _case("first iterated", _top_and_rest(33, 6), 5, 6, "smallest n > m (m = 32)"),
    _case("64", _top_and_rest(64, 7), 5, 7, "a full tile row"),
    _case("65", _top_and_rest(65, 8), 5, 8, "a full tile row and one more"),
    _case("130", _top_and_rest(130, 9), 5, 9, "several tiles, a ragged last one"),
    _case("257", _top_and_rest(257, 10), 5, 10, "several tiles, a ragged last one; two reduction workgroups"),
    _case("negative", _top_and_rest(130, 11, extra=[-20.0]), 5, 11, "a dominant negative direction is not returned"),
    _case("rank3", [3.0, 2.0, 1.0] + [0.0] * 254, 5, 13, "the block cannot collapse; theta_3 = theta_4 = 0"),
    _case("repeated", np.concatenate([[5.0, 5.0, 3.0], _rest(254, 0.0, 1.0, 14)]), 3, 14, "a double eigenvalue inside the K"),
    _case("zero", [0.0] * 40, 3, 15, "s = 0, orthonormal vectors still"),
    _case("wide K", _wide_spectrum(), 32, 12, "MG_PCA_MAX_K, m = 64"),
]
GRM_LIKE = [dict(name="grm-like K=%d" % k, n=600, spectrum=None, k=k, seed=7, seam="float32 through the triangle form; slow bulk components",
                 cap=CAP_GRM_LIKE, form="tri") for k in (2, 10)]
ALL = CASES + GRM_LIKE
BY_NAME = {c["name"]: c for c in ALL}


@functools.lru_cache(maxsize=None)
def _matrix(name):
    c = BY_NAME[name]
    if c["form"] == "tri":
        return grm_like()[1]
    if not c["spectrum"].any():
        return np.zeros((c["n"], c["n"]))
    return planted(c["spectrum"], c["seed"])


def matrix(case):
    """the case's matrix, float64 [n, n]; shared between the tests and left unchanged"""
    G = _matrix(case["name"])
    G.setflags(write=False)
    return G


def triangle(case):
    """the float32 triangle of a grm-like case"""
    return grm_like()[0]
