"""mg_genotype_cohort on the device against its definition in numpy (tests/cohort_prior_model.py), bit for bit: the re-estimated
frequencies, the planes that count, every cell's GT / GQ / status and its likelihood list.  max_cov is 200 and the coverages stay
at or below 220, so every total is far below the ln table's end and nothing may differ in the last bit.

The shapes are the smallest at which the kernel takes another path: every segment width (1, 2, 4, 8, 16, 32, 64 lanes) with one
plane below and one above each, record counts around a wave's and a workgroup's share and a last partial workgroup, records of 1,
2, 3, 4, 8 and 9 alleles next to each other in one wave."""
import numpy as np
import pytest

from malva_amd import capi
from malva_amd.capi import Context, MalvaError

import cohort_prior_model as M

pytestmark = pytest.mark.gpu

E, MAX_COV = 0.001, 200
PLANES = (1, 2, 3, 5, 16, 17, 32, 33, 64)
N_VARS = (0, 1, 3, 4, 5, 63, 64, 65, 257)
ITER_WEIGHT = ((0, 1.0), (1, 0.0), (1, 1.0), (5, 1.0), (5, 2.5), (64, 1.0))
NAMES = ("freq_out", "n_informative", "gt1", "gt2", "gq", "status", "probs")


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


_MODEL = {}


def model(seed, planes, n_vars, haploid, iters, weight):
    """inputs and the model's outputs, made once per case and shared (never written to)"""
    key = (seed, planes, n_vars, haploid, iters, weight)
    if key not in _MODEL:
        cov, freq, vo = M.synth_batch(seed, planes, n_vars, haploid, MAX_COV)
        out = M.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, iters, weight)
        for x in (cov, freq, vo) + out:
            x.setflags(write=False)
        _MODEL[key] = (cov, freq, vo, out)
    return _MODEL[key]


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def assert_same(got, want, status, goff, what=""):
    """freq_out, n_informative, gt1, gt2, gq, status bit for bit; probs where the cell's status is NORMAL (elsewhere they are not written)"""
    for name, g, w in zip(NAMES[:6], got[:6], want[:6]):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        bad = np.argwhere(bits(g) != bits(w))
        assert not len(bad), "%s %s differs at %s: %r != %r" % (what, name, bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
    gp, wp = got[6], want[6]
    assert gp.shape == wp.shape
    for p, v in np.argwhere(status == 0):
        a, b = int(goff[v]), int(goff[v + 1])
        same = (bits(gp[p, a:b]) == bits(wp[p, a:b])) | (np.isnan(gp[p, a:b]) & np.isnan(wp[p, a:b]))   # (0/0: the host's NaN has its sign set, the device's not)
        assert same.all(), (what, "probs", p, v, gp[p, a:b], wp[p, a:b])


def run_device_form(ctx, cov, freq, vo, haploid, iters, weight):
    import torch
    dev = torch.device("cuda:0")
    planes, n = cov.shape[0], len(vo) - 1
    goff = M.gt_offsets(vo, haploid)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_cov, d_freq, d_vo, d_go = up(cov), up(freq), up(vo), up(goff)
    z = lambda nbytes: torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=dev)
    d_fo, d_ni = z(4 * len(freq)), z(4 * n)
    d_g1, d_g2, d_gq, d_st, d_pr = z(4 * planes * n), z(4 * planes * n), z(4 * planes * n), z(planes * n), z(8 * planes * int(goff[-1]))
    torch.cuda.synchronize()
    ctx.genotype_cohort_device(n, planes, d_cov.data_ptr(), d_freq.data_ptr(), d_vo.data_ptr(), E, MAX_COV, haploid, iters, weight, d_fo.data_ptr(),
                               d_ni.data_ptr(), d_g1.data_ptr(), d_g2.data_ptr(), d_gq.data_ptr(), d_st.data_ptr(), d_pr.data_ptr(), d_go.data_ptr())
    ctx.synchronize()
    down = lambda t, dt, shape, count: np.frombuffer(t.cpu().numpy().tobytes()[:count * np.dtype(dt).itemsize], dtype=dt).reshape(shape)
    return (down(d_fo, np.float32, (len(freq),), len(freq)), down(d_ni, np.uint32, (n,), n), down(d_g1, np.int32, (planes, n), planes * n),
            down(d_g2, np.int32, (planes, n), planes * n), down(d_gq, np.int32, (planes, n), planes * n), down(d_st, np.uint8, (planes, n), planes * n),
            down(d_pr, np.float64, (planes, int(goff[-1])), planes * int(goff[-1])), goff)


def check_case(ctx, seed, planes, n_vars, haploid, iters, weight, device_form=True):
    cov, freq, vo, want = model(seed, planes, n_vars, haploid, iters, weight)
    what = "P=%d n=%d hap=%d T=%d w=%g" % (planes, n_vars, haploid, iters, weight)
    got = ctx.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, iters, weight, want_probs=True)
    assert_same(got, want, want[5], want[7], what + " host form")
    assert np.array_equal(got[7], want[7])
    ms = ctx.cohort_prior_stats()
    assert np.isfinite(ms) and ms >= 0
    if device_form:
        assert_same(run_device_form(ctx, cov, freq, vo, haploid, iters, weight), want, want[5], want[7], what + " device form")
    # without the likelihood lists: the same calls
    plain = ctx.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, iters, weight)
    assert plain[6] is None
    for name, g, w in zip(NAMES[:6], plain[:6], want[:6]):
        assert np.array_equal(bits(g), bits(w)), (what, name, "without probs")
    return cov, freq, vo, got


def test_stats_before_the_first_call_and_argument_errors():
    """a context of its own: MG_ERR_STATE before the first call; every argument error is MG_ERR_ARG and writes nothing"""
    with Context(35, 43, 1 << 20) as c:
        with pytest.raises(MalvaError) as e:
            c.cohort_prior_stats()
        assert e.value.code == -3
        cov, freq, vo = M.synth_batch(3, 3, 4, False, MAX_COV)
        for kw in (dict(iters=65), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=-0.5, iters=0)):
            with pytest.raises(MalvaError) as e:
                c.genotype_cohort(cov, freq, vo, E, MAX_COV, False, **kw)
            assert e.value.code == -1, kw
        with pytest.raises(MalvaError) as e:
            c.cohort_prior_stats()                                                 # still no call that ran
        assert e.value.code == -3
        # raw calls: sentinels stay in every output
        L, n, P = capi.lib(), 4, 3
        import ctypes as C
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        goff = M.gt_offsets(vo, False)

        def outs():
            return [np.full(len(freq), 7.5, np.float32), np.full(n, 77, np.uint32), np.full((P, n), 77, np.int32), np.full((P, n), 77, np.int32),
                    np.full((P, n), 77, np.int32), np.full((P, n), 77, np.uint8), np.full((P, int(goff[-1])), 7.5, np.float64)]

        def call(planes=P, cov_=cov, freq_=freq, vo_=vo, iters=5, weight=1.0, drop=None, goff_=goff, with_probs=True):
            o = outs()
            args = [p(x) for x in o]
            if drop is not None:
                args[drop] = None
            if not with_probs:
                args[6] = None
            rc = L.mg_genotype_cohort(c.h, n, planes, p(cov_), p(freq_), p(vo_), C.c_float(E), MAX_COV, 0, iters, weight, *args, p(goff_))
            fresh = outs()
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(o, fresh)), "an output was written"
            return rc

        assert call(planes=0) == -1 and call(planes=65) == -1
        assert call(iters=65) == -1 and call(weight=-1e-300) == -1 and call(weight=float("-inf")) == -1
        assert call(cov_=None) == -1 and call(freq_=None) == -1 and call(vo_=None) == -1
        for k in range(6):
            assert call(drop=k) == -1, k
        assert call(goff_=None) == -1                                              # probs without var_gt_off
        assert L.mg_genotype_cohort(c.h, 0, 3, None, None, None, C.c_float(E), MAX_COV, 0, 5, 1.0, None, None, None, None, None, None, None, None) == 0
        assert np.isfinite(c.cohort_prior_stats()) and c.cohort_prior_stats() >= 0  # n_vars == 0 is a call


def test_the_inputs_move_the_priors_and_some_calls():
    """asserted from the model alone: in the T = 5 cases at least half of the records with 2 <= A <= 8 end with other frequencies than
    the panel's, and at least one cell's GT is not the GT under the panel's prior"""
    for haploid in (False, True):
        for weight in (1.0, 2.5):
            cov, freq, vo, want = model(11, 5, 65, haploid, 5, weight)
            base = model(11, 5, 65, haploid, 0, 1.0)[3]
            A = np.diff(vo.astype(np.int64))
            moved = np.array([(bits(want[0][vo[v]:vo[v + 1]]) != bits(freq[vo[v]:vo[v + 1]])).any() for v in range(len(A))])
            el = (A >= 2) & (A <= 8)
            assert moved[el].sum() * 2 >= el.sum() and not moved[~el].any() and not want[1][~el].any()
            assert ((want[2] != base[2]) | (want[3] != base[3])).any()
            assert np.array_equal(bits(base[0]), bits(freq)) and not base[1].any()


@pytest.mark.parametrize("haploid", (False, True), ids=("diploid", "haploid"))
@pytest.mark.parametrize("planes", PLANES)
def test_every_segment_width(ctx, planes, haploid):
    check_case(ctx, 20 + planes, planes, 5, haploid, 5, 1.0)
    if planes in (17, 64):                                                          # more than one workgroup of 16 records
        check_case(ctx, 40 + planes, planes, 33, haploid, 1, 1.0, device_form=False)


@pytest.mark.parametrize("haploid", (False, True), ids=("diploid", "haploid"))
@pytest.mark.parametrize("n_vars", N_VARS)
def test_record_counts_around_a_wave_and_a_workgroup(ctx, n_vars, haploid):
    check_case(ctx, 60 + n_vars, 3, n_vars, haploid, 5, 2.5)                        # 4 lanes a record: 16 a wave, 64 a workgroup
    if n_vars <= 65:
        check_case(ctx, 90 + n_vars, 1, n_vars, haploid, 1, 1.0, device_form=False)  # 1 lane a record: 64 a wave


@pytest.mark.parametrize("haploid", (False, True), ids=("diploid", "haploid"))
@pytest.mark.parametrize("iters,weight", ITER_WEIGHT)
def test_iterations_and_weights(ctx, iters, weight, haploid):
    cov, freq, vo, got = check_case(ctx, 11, 5, 65, haploid, iters, weight)
    # self-consistency through the existing entry: every plane under freq_out
    for p in range(cov.shape[0]):
        g1, g2, gq, st, probs, goff = ctx.genotype(cov[p], got[0], vo, E, MAX_COV, haploid, want_probs=True)
        assert np.array_equal(g1, got[2][p]) and np.array_equal(g2, got[3][p]) and np.array_equal(gq, got[4][p]) and np.array_equal(st, got[5][p])
        for v in np.flatnonzero(st == 0):
            a, b = int(goff[v]), int(goff[v + 1])
            assert ((bits(probs[a:b]) == bits(got[6][p, a:b])) | (np.isnan(probs[a:b]) & np.isnan(got[6][p, a:b]))).all(), (p, v)


def directed(ctx, cov, freq, vo, haploid, iters, weight):
    cov, freq, vo = np.asarray(cov, dtype=np.uint32), np.asarray(freq, dtype=np.float32), np.asarray(vo, dtype=np.uint32)
    want = M.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, iters, weight)
    got = ctx.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, iters, weight, want_probs=True)
    assert_same(got, want, want[5], want[7], "directed host form")
    assert_same(run_device_form(ctx, cov, freq, vo, haploid, iters, weight), want, want[5], want[7], "directed device form")
    return got


def test_directed_records(ctx):
    vo = [0, 2]
    f = [0.9, 0.1]
    # every plane over-covered: nothing counts, the frequencies stay, n = 0
    got = directed(ctx, [[201, 3], [5, 220], [201, 201]], f, vo, False, 5, 1.0)
    assert got[0].tolist() == np.float32(f).tolist() and got[1].tolist() == [0] and (got[5] == M.OVERCOV).all()
    # every total 0
    got = directed(ctx, [[0, 0]] * 5, f, vo, False, 5, 1.0)
    assert got[0].tolist() == np.float32(f).tolist() and got[1].tolist() == [0] and (got[5] == M.NOCOV).all()
    # exactly one plane that counts (the others: over-covered, empty), diploid and haploid, at an odd plane
    for haploid in (False, True):
        got = directed(ctx, [[0, 0], [300, 1], [0, 0], [4, 9], [0, 0]], f, vo, haploid, 3, 1.0)
        assert got[1].tolist() == [1] and got[0][1] != np.float32(0.1)
    # a panel frequency of 0 on a covered ALT allele: its genotypes have a log prior of -inf, and 200 reads against REF alone underflow
    # exp() -- every value is 0, the sum is 0, the plane does not count (its cell: 0/0 = NaN, which never wins)
    for haploid in (False, True):
        got = directed(ctx, [[0, 200], [0, 180]], [1.0, 0.0], vo, haploid, 4, 1.0)
        assert got[1].tolist() == [0] and got[0].tolist() == [1.0, 0.0] and (got[5] == M.NORMAL).all() and np.isnan(got[6]).all()
        # the same beside a plane that does count: n = 1
        got = directed(ctx, [[0, 200], [9, 0], [0, 180]], [1.0, 0.0], vo, haploid, 4, 1.0)
        assert got[1].tolist() == [1]
    # f0 that makes the REF value negative before the clamp: ALT frequencies that sum above 1 (three alleles, weight large enough to keep them)
    got = directed(ctx, [[0, 10, 10], [0, 12, 9], [1, 8, 14]], [0.0, 0.7, 0.6], [0, 3], False, 2, 50.0)
    assert got[0][0] == 0.0 and got[0][1] + got[0][2] > 1
    # w = 0 with every posterior on REF: the ALT frequency becomes exactly 0 and stays
    got = directed(ctx, [[150, 0], [170, 0], [190, 0]], [0.5, 0.5], vo, False, 6, 0.0)
    assert got[0].tolist() == [1.0, 0.0] and got[1].tolist() == [3]
    # frequencies that repeat after two iterations: T = 2, T = 3 and T = 64 give the same bits (and the model without its early stop agrees)
    cov = [[150, 0], [170, 0], [190, 0]]
    a, b, c = (directed(ctx, cov, [0.5, 0.5], vo, False, T, 0.0) for T in (2, 3, 64))
    for x, y in ((a, b), (b, c)):
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(x[:7], y[:7]))
    slow = M.genotype_cohort(np.uint32(cov), np.float32([0.5, 0.5]), vo, E, MAX_COV, False, 64, 0.0, early_stop=False)
    assert np.array_equal(bits(slow[0]), bits(c[0])) and np.array_equal(slow[1], c[1])
    # a record too wide for the coverages' LDS share (300 alleles) between two that are re-estimated: the run reads global memory
    rng = np.random.default_rng(5)
    vo3 = [0, 2, 302, 305]
    cov3 = rng.integers(0, 40, (9, 305))
    f3 = np.full(305, 1.0 / 305, dtype=np.float32)
    f3[:2] = (0.8, 0.2)
    f3[302:] = (0.5, 0.25, 0.25)
    directed(ctx, cov3, f3, vo3, False, 5, 1.0)
