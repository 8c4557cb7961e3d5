"""mg_pca_solve without a device: the case table of tests/pca_cases.py holds the spectra it says, the numpy restatement of the method
(tests/pca_model.py) converges on every case at tol = 1e-10 within the table's caps on products -- 40 for the planted matrices, 400 for the
three-population GRM at K = 10 -- and passes the checks the device must pass; the host half of `malva-geno pca` (readers, writers, parser,
block geometry, the small Jacobi solver) by tools/pca_host_check.cpp, built plain here (`make sanitize-host` builds it with -fsanitize);
the header's new symbols in the binding; and the sub-command's help and refused lines, which need no device.

Products the restatement took when the caps were chosen: m == n cases 0; 33: 8; 64 / 65: 12; 130 / 257: 16; negative: 16; rank3: 4;
repeated: 20; zero: 4; wide K: 12; grm-like: 12 at K = 2 and 260 at K = 10."""
import os
import re
import subprocess

import numpy as np
import pytest

import pca_cases as Cs
import pca_model as M
from malva_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "malva-geno")
needs_cli = pytest.mark.skipif(not os.path.exists(BIN), reason="bin/malva-geno not built")
IDS = [c["name"] for c in Cs.ALL]


def test_the_table_names_every_seam():
    assert (Cs.CAP_PLANTED, Cs.CAP_GRM_LIKE, Cs.TOL) == (40, 400, 1e-10)
    by = {c["name"]: (c["n"], c["k"], Cs.block(c["n"], c["k"])) for c in Cs.ALL}
    assert by == {"one": (1, 1, 1), "two": (2, 2, 2), "tile-1": (15, 5, 15), "tile": (16, 5, 16), "tile+1": (17, 5, 17), "first iterated": (33, 5, 32),
                  "64": (64, 5, 32), "65": (65, 5, 32), "130": (130, 5, 32), "257": (257, 5, 32), "negative": (130, 5, 32), "rank3": (257, 5, 32),
                  "repeated": (257, 3, 32), "zero": (40, 3, 32), "wide K": (130, 32, 64), "grm-like K=2": (600, 2, 32), "grm-like K=10": (600, 10, 32)}
    assert all(c["cap"] == (400 if c["name"].startswith("grm-like") else 40) for c in Cs.ALL)


@pytest.mark.parametrize("case", Cs.CASES, ids=[c["name"] for c in Cs.CASES])
def test_planted_spectrum(case):
    G = Cs.matrix(case)
    w, _, L = M.case_reference(case["name"])
    assert G.shape == (case["n"], case["n"]) and np.array_equal(G, G.T)
    assert np.abs(w - np.sort(case["spectrum"])[::-1]).max() <= 64 * case["n"] * M.EPS * L


def test_planted_spectra_are_the_tables():
    top = np.array(Cs.TOP)
    for name in ("tile-1", "tile", "tile+1", "first iterated", "64", "65", "130", "257"):
        lam = Cs.BY_NAME[name]["spectrum"]
        assert np.array_equal(lam[:5], top) and lam[5:].min() >= -0.2 and lam[5:].max() <= 1.0
    lam = Cs.BY_NAME["negative"]["spectrum"]
    assert np.array_equal(lam[:5], top) and lam[5] == -20.0 and lam[6:].min() >= -0.2 and lam[6:].max() <= 1.0
    assert np.array_equal(Cs.BY_NAME["rank3"]["spectrum"][:4], [3, 2, 1, 0]) and not Cs.BY_NAME["rank3"]["spectrum"][3:].any()
    lam = Cs.BY_NAME["repeated"]["spectrum"]
    assert np.array_equal(lam[:3], [5, 5, 3]) and lam[3:].min() >= 0 and lam[3:].max() <= 1
    lam = Cs.BY_NAME["wide K"]["spectrum"]
    assert lam[0] == 40 and lam[31] == 9 and (np.diff(lam[:32]) < -0.9).all() and lam[32:].max() <= 1 and lam[32:].min() >= 0
    assert list(Cs.BY_NAME["two"]["spectrum"]) == [2, -1] and list(Cs.BY_NAME["one"]["spectrum"]) == [3]


def test_grm_like_is_three_populations_in_float32():
    tri, G = Cs.grm_like()
    assert tri.dtype == np.float32 and tri.size == 600 * 601 // 2 and np.array_equal(G, G.T)
    i, j = np.tril_indices(600)
    assert np.array_equal(G[i, j].astype(np.float32), tri)                       # float32 values exactly
    w, V, L = M.case_reference("grm-like K=2")
    assert w[1] - w[2] >= 0.5 * L and w[0] - w[1] >= 0.02 * L                     # two structure components, far above the rest ...
    assert (np.diff(w[2:12]) > -0.01 * L).all()                                   # ... and a bulk whose neighbours are close: the slow ones
    assert abs(w[-1]) <= 1e-4 * L                                                 # the eigenvalue near 0 a GRM has by construction
    pops = np.repeat(np.arange(3), 200)
    means = np.array([[V[c][pops == p].mean() for p in range(3)] for c in range(2)])
    assert (np.abs(means).max(axis=1) > 0.02).all()                               # the two leading vectors separate the populations


@pytest.mark.parametrize("case", Cs.ALL, ids=IDS)
def test_the_method_converges_within_the_cap(case):
    G, ref = Cs.matrix(case), M.case_reference(case["name"])
    out = M.solve(G, case["k"], Cs.TOL, case["cap"])
    M.check_result(G, ref, case["k"], Cs.TOL, *out, cap=case["cap"])
    if case["name"] == "repeated":
        M.check_projector(out[1], ref, 2, 5.0 - 3.0, case["n"], Cs.TOL)


def test_the_method_under_an_iteration_cap():
    G, ref = Cs.matrix(Cs.BY_NAME["257"]), M.case_reference("257")
    out = M.solve(G, 5, Cs.TOL, 1)
    assert out[4][0] == 1 and out[4][1] < 5
    M.check_result(G, ref, 5, Cs.TOL, *out, cap=1, expect_converged=False)


def test_the_hash_is_the_plans():
    """three values of pca_hash_value, worked by hand from its definition in Python integers"""
    def one(row, col, salt):
        mask = (1 << 64) - 1
        x = (row * 0x9E3779B97F4A7C15 + col * 0xBF58476D1CE4E5B9 + salt * 0x94D049BB133111EB + 0x2545F4914F6CDD1D) & mask
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & mask
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & mask
        x ^= x >> 31
        return (x >> 11) / 4503599627370496.0 - 1.0
    H = M.hash_block(300, 64, 5)
    for row, col in ((0, 0), (299, 63), (17, 31)):
        assert H[row, col] == one(row, col, 5)
    assert np.array_equal(M.hash_block(300, 64, 5, [31])[:, 0], H[:, 31])


def test_pca_host_check(tmp_path):
    exe = tmp_path / "pca_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "malva_amd", "host"), "-o", str(exe),
                    os.path.join(ROOT, "tools", "pca_host_check.cpp"), "-lz"], check=True, timeout=300)
    scratch = tmp_path / "scratch"
    scratch.mkdir()
    r = subprocess.run([str(exe), str(scratch)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert r.stdout == "pca_host_check: ok\n"
    assert not os.listdir(scratch)                                                # every file it made is gone again


def test_the_binding_has_the_headers_symbols():
    text = open(os.path.join(ROOT, "include", "malva_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mg_pca_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(["mg_pca_load_tri_f32", "mg_pca_load_f64", "mg_pca_load_tri_f32_device", "mg_pca_load_f64_device", "mg_pca_solve", "mg_pca_solve_device",
                               "mg_pca_end", "mg_pca_stats"])
    assert set(declared) <= set(capi.EXPORTED)
    L = capi.lib()
    assert all(hasattr(L, n) for n in declared)
    assert re.search(r"#define MG_PCA_MAX_N (\d+)", text).group(1) == str(capi.PCA_MAX_N)
    assert re.search(r"#define MG_PCA_MAX_K (\d+)", text).group(1) == str(capi.PCA_MAX_K)
    for method in ("pca_load_tri", "pca_load", "pca_solve", "pca_solve_device", "pca_end", "pca_stats"):
        assert callable(getattr(capi.Context, method))


@needs_cli
def test_cli_help_and_refused_lines(tmp_path):
    for flag in ("-h", "--help"):
        r = subprocess.run([BIN, "pca", flag], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.startswith("Usage: malva-geno pca [--pcs K] [--tol T] [--max-iters N] [-d DEVICE] -o OUT <GRM>\n")
    usage = r.stdout
    assert "design choice, not a measurement" in usage
    out = str(tmp_path / "out")
    for args, faults in ((["-o", out], 1), ([str(tmp_path / "g")], 1), (["-o", out, "g", "--pcs", "33"], 1), (["-o", out, "g", "--tol", "1"], 1),
                         (["-o", out, "g", "--max-iters", "0"], 1), (["-o", out, "g", "--ld"], 1), (["--pcs", "0", "--tol", "0"], 4)):
        r = subprocess.run([BIN, "pca"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "", args
        assert r.stderr.count("malva : ") == faults and r.stderr.endswith(usage), args
    r = subprocess.run([BIN, "pca", "-o", out, str(tmp_path / "no_such")], capture_output=True, text=True, timeout=60)     # (read before any device is asked for)
    assert r.returncode == 1 and r.stderr.startswith("malva : cannot read ") and r.stdout == ""
    assert not os.listdir(tmp_path)
    r = subprocess.run([BIN, "pcas"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Accepted commands are index and call." in r.stderr
