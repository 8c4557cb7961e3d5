"""`malva-geno pca` and mg_pca_*: the leading eigenpairs of a symmetric matrix by blocked subspace iteration on the matrix cores.

The ABI is compared with numpy.linalg.eigh over the case table of tests/pca_cases.py by the checks of tests/pca_model.py (eigenvalues by
rank, recomputed residuals, orthonormality, Davis-Kahan for isolated vectors, the sign rule), through the host form and the device form,
at tol = 1e-10 with the table's caps as max_iters.  The command line's three files are compared byte for byte with what Python formats
from the ABI's result on the same input."""
import os
import subprocess

import numpy as np
import pytest
import torch

import pca_cases as Cs
import pca_model as M
from malva_amd import Context, MalvaError, capi
from test_gpu_ld import _dev

pytestmark = pytest.mark.gpu
MG_ERR_ARG, MG_ERR_STATE = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
PAD = 64        # poisoned bytes on both sides of every device output
POISON = 0x5A
IDS = [c["name"] for c in Cs.ALL]


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def test_the_constants_are_the_headers():
    assert (capi.PCA_MAX_N, capi.PCA_MAX_K) == (16384, 32)


def _load(ctx, case):
    if case["form"] == "tri":
        ctx.pca_load_tri(Cs.triangle(case), case["n"])
    else:
        ctx.pca_load(Cs.matrix(case))


def _device_solve(ctx, n, k, tol, max_iters):
    """the device form into poisoned buffers -> the host form's tuple; asserts that nothing beside the outputs was written"""
    sizes = [8 * k, 8 * k * n, 8 * k, 8, 12]
    bufs = [torch.full((s + 2 * PAD,), POISON, dtype=torch.uint8, device="cuda:0") for s in sizes]
    torch.cuda.synchronize()
    ctx.pca_solve_device(k, tol, max_iters, *[b.data_ptr() + PAD for b in bufs])
    ctx.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h, s in zip(host, sizes):
        assert (h[:PAD] == POISON).all() and (h[PAD + s:] == POISON).all(), "written outside an output of %d bytes" % s
    values, vectors, resid, scale = (h[PAD:PAD + s].copy().view(np.float64) for h, s in zip(host[:4], sizes[:4]))
    info = host[4][PAD:PAD + 12].copy().view(np.uint32)
    return values, vectors.reshape(k, n), resid, float(scale[0]), tuple(int(x) for x in info)


def _same_bytes(a, b):
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert x.tobytes() == y.tobytes()
        else:
            assert x == y or (x != x and y != y)


@pytest.mark.parametrize("case", Cs.ALL, ids=IDS)
def test_case_host_and_device_forms(ctx, case):
    G, ref = Cs.matrix(case), M.case_reference(case["name"])
    n, k = case["n"], case["k"]
    _load(ctx, case)
    host = ctx.pca_solve(n, k, Cs.TOL, case["cap"])
    M.check_result(G, ref, k, Cs.TOL, *host, cap=case["cap"])
    if case["name"] == "repeated":
        M.check_projector(host[1], ref, 2, 5.0 - 3.0, n, Cs.TOL)
    if case["name"] == "negative":
        assert host[0].min() > 0 and ref[0][-1] < -19
    if case["name"] == "zero":
        assert host[3] == 1.0 and not host[0].any()
    again = ctx.pca_solve(n, k, Cs.TOL, case["cap"])
    _same_bytes(host, again)                                    # two solves of one load
    _same_bytes(host, _device_solve(ctx, n, k, Cs.TOL, case["cap"]))   # the device form
    _load(ctx, case)
    _same_bytes(host, ctx.pca_solve(n, k, Cs.TOL, case["cap"]))   # a reload
    ms = ctx.pca_stats()
    assert len(ms) == 4 and ms[3] >= ms[0] >= 0 and ms[3] > 0
    ctx.pca_end()


def test_load_forms_agree(ctx):
    case = Cs.BY_NAME["grm-like K=2"]
    n, tri = case["n"], Cs.triangle(case)
    ctx.pca_load_tri(tri, n)
    a = ctx.pca_solve(n, 2, Cs.TOL, case["cap"])
    full = np.full((n, n), np.nan)                      # the upper triangle is poison and must not be read
    i, j = np.tril_indices(n)
    full[i, j] = tri.astype(np.float64)
    ctx.pca_load(full)
    _same_bytes(a, ctx.pca_solve(n, 2, Cs.TOL, case["cap"]))
    d_tri = _dev(tri)
    ctx.pca_load_tri_device(n, d_tri.data_ptr())
    _same_bytes(a, ctx.pca_solve(n, 2, Cs.TOL, case["cap"]))
    d_full = _dev(full)
    ctx.pca_load_device(n, d_full.data_ptr())
    _same_bytes(a, ctx.pca_solve(n, 2, Cs.TOL, case["cap"]))
    ctx.pca_end()


def test_asymmetric_input_gives_the_lower_triangle(ctx):
    case = Cs.BY_NAME["65"]
    G = Cs.matrix(case)
    ctx.pca_load(G)
    want = ctx.pca_solve(65, 5, Cs.TOL, case["cap"])
    A = np.tril(G) + np.triu(np.full((65, 65), 1e300), 1)
    ctx.pca_load(A)
    _same_bytes(want, ctx.pca_solve(65, 5, Cs.TOL, case["cap"]))
    ctx.pca_end()


def test_iteration_cap(ctx):
    case = Cs.BY_NAME["257"]
    G, ref = Cs.matrix(case), M.case_reference("257")
    ctx.pca_load(G)
    out = ctx.pca_solve(257, 5, Cs.TOL, 1)              # MG_OK: an unconverged result is a result
    assert out[4] == (1, out[4][1], 32) and out[4][1] < 5
    M.check_result(G, ref, 5, Cs.TOL, *out, cap=1, expect_converged=False)
    _same_bytes(out, _device_solve(ctx, 257, 5, Cs.TOL, 1))
    ctx.pca_end()


def _code(fn, *a):
    with pytest.raises(MalvaError) as e:
        fn(*a)
    return e.value.code


def test_errors(ctx):
    L, h = ctx._L, ctx.h
    ctx.pca_end()
    ctx.pca_end()                                        # legal without a load, and twice
    out = [np.zeros(8), np.zeros(128), np.zeros(8), np.zeros(1), np.zeros(3, dtype=np.uint32)]
    ptr = [capi._p(x) for x in out]
    assert L.mg_pca_solve(h, 1, 1e-10, 10, *ptr) == MG_ERR_STATE
    assert L.mg_pca_solve_device(h, 1, 1e-10, 10, *ptr) == MG_ERR_STATE
    fresh = Context(35, 43, 1 << 20)
    with fresh as c2:
        assert _code(c2.pca_stats) == MG_ERR_STATE       # before any solve
    one = np.ones(1, dtype=np.float32)
    for n in (0, capi.PCA_MAX_N + 1):
        assert L.mg_pca_load_tri_f32(h, n, capi._p(one)) == MG_ERR_ARG
        assert L.mg_pca_load_f64(h, n, capi._p(np.ones(1))) == MG_ERR_ARG
        assert L.mg_pca_load_tri_f32_device(h, n, capi._p(one)) == MG_ERR_ARG
        assert L.mg_pca_load_f64_device(h, n, capi._p(one)) == MG_ERR_ARG
    for f in (L.mg_pca_load_tri_f32, L.mg_pca_load_f64, L.mg_pca_load_tri_f32_device, L.mg_pca_load_f64_device):
        assert f(h, 4, None) == MG_ERR_ARG
    G = Cs.matrix(Cs.BY_NAME["tile"])                    # n = 16
    ctx.pca_load(G)
    for k in (0, 17, 33):
        assert L.mg_pca_solve(h, k, 1e-10, 10, *ptr) == MG_ERR_ARG
    ctx.pca_load(Cs.matrix(Cs.BY_NAME["65"]))
    assert L.mg_pca_solve(h, 33, 1e-10, 10, *ptr) == MG_ERR_ARG      # MG_PCA_MAX_K
    for tol in (0.0, -1e-3, float("nan"), float("inf")):
        assert L.mg_pca_solve(h, 1, tol, 10, *ptr) == MG_ERR_ARG
    assert L.mg_pca_solve(h, 1, 1e-10, 0, *ptr) == MG_ERR_ARG
    for i in range(5):
        p = list(ptr)
        p[i] = None
        assert L.mg_pca_solve(h, 1, 1e-10, 10, *p) == MG_ERR_ARG
        assert L.mg_pca_solve_device(h, 1, 1e-10, 10, *p) == MG_ERR_ARG
    assert L.mg_pca_stats(h, None) == MG_ERR_ARG
    ctx.pca_solve(65, 2, 1e-10, 40)
    assert len(ctx.pca_stats()) == 4                     # after a solve
    for bad in (np.nan, np.inf, -np.inf):
        tri = np.ones(10 * 11 // 2, dtype=np.float32)
        tri[17] = bad
        with pytest.raises(MalvaError, match="not finite") as e:
            ctx.pca_load_tri(tri, 10)
        assert e.value.code == MG_ERR_ARG
        assert L.mg_pca_solve(h, 1, 1e-10, 10, *ptr) == MG_ERR_STATE     # the refused load keeps no matrix
        full = np.eye(10)
        full[7, 3] = bad
        assert _code(ctx.pca_load, full) == MG_ERR_ARG
    d = _dev(np.array([1.0, np.nan, 1.0], dtype=np.float32))
    ctx.pca_load_tri_device(2, d.data_ptr())             # asynchronous: the first solve reports it
    assert L.mg_pca_solve(h, 1, 1e-10, 10, *ptr) == MG_ERR_ARG
    assert L.mg_pca_solve(h, 1, 1e-10, 10, *ptr) == MG_ERR_STATE
    ctx.pca_end()


# ---- the command line ------------------------------------------------------------------------------------------------------------------------

def _names(n):
    return ["s%04d" % i for i in range(n)]


def _write_gcta(prefix, tri, names):
    np.asarray(tri, dtype=np.float32).tofile(prefix + ".grm.bin")
    with open(prefix + ".grm.id", "w") as f:
        f.write("".join("%s\t%s\n" % (nm, nm) for nm in names))


def _tri_of(G):
    i, j = np.tril_indices(G.shape[0])
    return G[i, j].astype(np.float32)


def _full_of(tri, n):
    G = np.zeros((n, n))
    i, j = np.tril_indices(n)
    G[i, j] = tri
    G[j, i] = tri
    return G


def _trace(diag):
    t = 0.0
    for x in diag:
        t += float(x)
    return t


def _pca_cli(args):
    return subprocess.run([BIN, "pca"] + args, capture_output=True, text=True, timeout=300)


def _check_files(ctx, out, names, G, k, tol, max_iters, load):
    load()
    res = ctx.pca_solve(len(names), k, tol, max_iters)
    ctx.pca_end()
    eigenval, eigenvec, table = M.format_files(names, _trace(np.diag(G)), *res, tol, None)
    assert open(out + ".eigenval").read() == eigenval
    assert open(out + ".eigenvec").read() == eigenvec
    got = open(out + ".pca.tsv").read().split("\n")
    assert got[-1] == "" and got[-2].startswith("#") and "\n".join(got[:-2]) + "\n" == table
    trailer = got[-2]
    assert "n=%d" % len(names) in trailer and "m=%d" % res[4][2] in trailer and "products=%d" % res[4][0] in trailer and "tol=" in trailer and "ms=" in trailer
    return res


@pytest.mark.parametrize("name,k", [("130", 5), ("grm-like K=10", 10)])
def test_cli_gcta_input(ctx, tmp_path, name, k):
    case = Cs.BY_NAME[name]
    n, names = case["n"], _names(case["n"])
    tri = Cs.triangle(case) if case["form"] == "tri" else _tri_of(Cs.matrix(case))
    G = _full_of(tri.astype(np.float64), n)
    prefix, out = str(tmp_path / "in"), str(tmp_path / "out")
    _write_gcta(prefix, tri, names)
    r = _pca_cli(["--pcs", str(k), "-o", out, prefix])
    assert r.returncode == 0, r.stderr[-2000:]
    res = _check_files(ctx, out, names, G, k, 1e-10, 2000, lambda: ctx.pca_load_tri(tri, n))
    assert res[4][1] == k
    assert sorted(os.listdir(tmp_path)) == ["in.grm.bin", "in.grm.id", "out.eigenval", "out.eigenvec", "out.pca.tsv"]
    if name == "130":
        r = _pca_cli(["--pcs", str(k), "--max-iters", "1", "-o", out, prefix])
        assert r.returncode == 2 and "not converged" in r.stderr, r.stderr[-2000:]
        _check_files(ctx, out, names, G, k, 1e-10, 1, lambda: ctx.pca_load_tri(tri, n))
        rows = [l.split("\t") for l in open(out + ".pca.tsv").read().split("\n")[1:-2]]
        assert "0" in [row[4] for row in rows]


def _write_text_table(path, G, names, drop=None):
    n = len(names)
    with open(path, "w") as f:
        f.write("#A\tB\tN\tGRM\n")
        for a in range(n):
            for b in range(a, n):
                if (a, b) != drop:
                    f.write("%s\t%s\t%d\t%.6f\n" % (names[a], names[b], 100, G[a, b]))


def test_cli_text_table_input(ctx, tmp_path):
    case = Cs.BY_NAME["65"]
    G0, names = Cs.matrix(case), _names(65)
    table, out = str(tmp_path / "grm.tsv"), str(tmp_path / "out")
    _write_text_table(table, G0, names)
    G = np.array([[float("%.6f" % G0[max(a, b), min(a, b)]) for b in range(65)] for a in range(65)])     # the printed values
    r = _pca_cli(["--pcs", "5", "-o", out, table])
    assert r.returncode == 0, r.stderr[-2000:]
    res = _check_files(ctx, out, names, G, 5, 1e-10, 2000, lambda: ctx.pca_load(G))
    M.check_result(G, M.reference(G), 5, 1e-10, *res, cap=Cs.CAP_PLANTED)


def test_cli_refuses_broken_input(tmp_path):
    case = Cs.BY_NAME["65"]
    G, names = Cs.matrix(case), _names(65)
    prefix, out = str(tmp_path / "in"), str(tmp_path / "out")
    _write_gcta(prefix, _tri_of(G)[:-3], names)                       # a truncated .grm.bin
    r = _pca_cli(["-o", out, prefix])
    assert r.returncode == 1 and "malva : " in r.stderr and ".grm.bin" in r.stderr
    table = str(tmp_path / "grm.tsv")
    _write_text_table(table, G, names, drop=(3, 40))                  # a missing pair
    r = _pca_cli(["-o", out, table])
    assert r.returncode == 1 and "malva : " in r.stderr and "missing" in r.stderr
    assert sorted(os.listdir(tmp_path)) == ["grm.tsv", "in.grm.bin", "in.grm.id"]


from test_gpu_merged import COMMON, haploid_cohort  # noqa: E402,F401 (the fixture)


def test_cli_call_grm_then_pca(haploid_cohort, tmp_path):
    tmp, fa, vcf, fq, inputs = haploid_cohort
    X, Y = str(tmp_path / "X"), str(tmp_path / "Y")
    r = subprocess.run([BIN, "index"] + COMMON + [fa, vcf, fq], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([BIN, "call"] + COMMON + ["--cohort", "--merged", str(tmp_path / "m.vcf"), "--grm", X, "--grm-format", "gcta", "--grm-min-maf", "0.05", fa, vcf, str(tmp / "cohort.tsv")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = _pca_cli(["-o", Y, X])
    assert r.returncode in (0, 2), r.stderr[-2000:]
    names = list(inputs)
    n = len(names)
    lines = open(Y + ".eigenvec").read().split("\n")[:-1]
    assert [l.split("\t")[:2] for l in lines] == [[nm, nm] for nm in names]
    G = _full_of(np.fromfile(X + ".grm.bin", dtype=np.float32).astype(np.float64), n)
    w, _, L = M.reference(G)
    got = np.array([float(x) for x in open(Y + ".eigenval").read().split()])
    assert len(got) == n                                              # --pcs 20 lowered to n
    assert (np.abs(got - w[:n]) <= M.allowance(n, L, 1e-10) + 5e-10 * L).all()     # (%.10g keeps ten digits: half a unit of the tenth)
