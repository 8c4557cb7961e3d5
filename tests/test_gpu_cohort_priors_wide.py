"""mg_estimate_priors on the device, bit for bit: up to 64 planes against mg_genotype_cohort on the same arrays (and the two-step
form -- the estimate, then mg_genotype_cohort(iters = 0, freq = f_T) -- against the one-step form, cell for cell), beyond 64 planes
against the wide definition in numpy (tests/cohort_prior_wide_model.py).  max_cov is 200 and the coverages stay at or below 220,
so every total is far below the ln table's end and nothing may differ in the last bit.

The shapes are the smallest at which the kernel takes another path: one plane past a chunk (65), two (66), one short of two chunks,
two exactly, one past (127, 128, 129), a short fourth chunk (200); record counts around the workgroup's run of 16 and a last
partial one; runs whose coverages do not fit the LDS share.  The model walks every plane of every record in Python, so the large
record counts go with the small plane counts."""
import ctypes as C

import numpy as np
import pytest

from malva_amd import capi
from malva_amd.capi import Context, MalvaError

import cohort_prior_model as M
import cohort_prior_wide_model as WM

pytestmark = pytest.mark.gpu

E, MAX_COV = 0.001, 200
NARROW = (1, 2, 3, 16, 63, 64)
# (planes, n_vars, haploid, iters, weight): every P of 65, 66, 127, 128, 129, 200, every n_vars of 0, 1, 15, 16, 17, 65, 257, both
# ploidies, T of 0, 1, 5 and w of 0, 1, 2.5 at least once
WIDE = ((65, 257, False, 1, 1.0), (66, 65, True, 5, 2.5), (127, 17, False, 5, 0.0), (128, 16, True, 5, 1.0), (129, 15, False, 5, 1.0),
        (200, 1, True, 1, 2.5), (200, 0, False, 0, 1.0), (129, 65, False, 0, 0.0), (200, 17, False, 5, 1.0), (66, 16, True, 1, 0.0))


@pytest.fixture(scope="module")
def ctx():
    with Context(35, 43, 1 << 20) as c:
        yield c


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]) if x.dtype.kind == "f" else x


def same(got, want, what):
    for name, g, w in zip(("freq_out", "n_informative"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert not len(bad), "%s %s differs at %d (%d places): %r != %r" % (what, name, bad[0], len(bad), g[bad[0]], w[bad[0]])


def run_device_form(ctx, cov, freq, vo, haploid, iters, weight, guard=64):
    """-> (freq_out, n_informative) through mg_estimate_priors_device, with `guard` bytes of 0xA5 in front of and behind both outputs,
    which must come back untouched"""
    import torch
    dev = torch.device("cuda:0")
    planes, n = cov.shape[0], len(vo) - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_cov, d_freq, d_vo = up(cov), up(freq), up(vo)
    d_fo = torch.full((guard + 4 * len(freq) + guard,), 0xA5, dtype=torch.uint8, device=dev)
    d_ni = torch.full((guard + 4 * n + guard,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.estimate_priors_device(n, planes, d_cov.data_ptr(), d_freq.data_ptr(), d_vo.data_ptr(), E, MAX_COV, haploid, iters, weight,
                               d_fo.data_ptr() + guard, d_ni.data_ptr() + guard)
    ctx.synchronize()
    fo, ni = d_fo.cpu().numpy(), d_ni.cpu().numpy()
    for name, x, body in (("freq_out", fo, 4 * len(freq)), ("n_informative", ni, 4 * n)):
        assert (x[:guard] == 0xA5).all() and (x[guard + body:] == 0xA5).all(), "a guard word around %s was written" % name
    return (np.frombuffer(fo[guard:guard + 4 * len(freq)].tobytes(), dtype=np.float32), np.frombuffer(ni[guard:guard + 4 * n].tobytes(), dtype=np.uint32))


def both_forms(ctx, cov, freq, vo, haploid, iters, weight, what):
    cov, freq, vo = np.ascontiguousarray(cov, dtype=np.uint32), np.ascontiguousarray(freq, dtype=np.float32), np.ascontiguousarray(vo, dtype=np.uint32)
    got = ctx.estimate_priors(cov, freq, vo, E, MAX_COV, haploid, iters, weight)
    ms = ctx.estimate_priors_stats()
    assert np.isfinite(ms) and ms >= 0
    same(run_device_form(ctx, cov, freq, vo, haploid, iters, weight), got, what + " device form against host form")
    return got


@pytest.mark.parametrize("haploid", (False, True), ids=("diploid", "haploid"))
@pytest.mark.parametrize("planes", NARROW)
def test_up_to_64_planes_it_is_the_cohort_entry(ctx, planes, haploid):
    """the existing segment widths; 300 records: more than one workgroup at every width (a run is 256 records at one plane)"""
    cov, freq, vo = M.synth_batch(100 + planes, planes, 300, haploid, MAX_COV)
    for iters, weight in ((5, 1.0), (1, 0.0), (0, 1.0)):
        what = "P=%d hap=%d T=%d w=%g" % (planes, haploid, iters, weight)
        one = ctx.genotype_cohort(cov, freq, vo, E, MAX_COV, haploid, iters, weight, want_probs=True)
        got = both_forms(ctx, cov, freq, vo, haploid, iters, weight, what)
        same(got, one[:2], what)
        # the estimate, then the cells under it: the one-step form's calls, cell for cell
        two = ctx.genotype_cohort(cov, got[0], vo, E, MAX_COV, haploid, 0, weight, want_probs=True)
        assert np.array_equal(bits(two[0]), bits(got[0])) and not two[1].any()
        for name, g, w in zip(("gt1", "gt2", "gq", "status"), two[2:6], one[2:6]):
            assert np.array_equal(g, w), (what, name)
        goff = one[7]
        for p, v in np.argwhere(one[5] == 0):                                        # (probs of a cell that is not NORMAL are not written)
            a, b = int(goff[v]), int(goff[v + 1])
            assert np.array_equal(bits(two[6][p, a:b]), bits(one[6][p, a:b])), (what, "probs", p, v)
        if iters == 0:
            assert np.array_equal(bits(got[0]), bits(freq)) and not got[1].any()


_MODEL = {}


def model(seed, planes, n_vars, haploid, iters, weight):
    """inputs and the wide model's outputs, made once per case and shared (never written to)"""
    key = (seed, planes, n_vars, haploid, iters, weight)
    if key not in _MODEL:
        cov, freq, vo = M.synth_batch(seed, planes, n_vars, haploid, MAX_COV)
        out = WM.estimate_priors(cov, freq, vo, E, MAX_COV, haploid, iters, weight)
        for x in (cov, freq, vo) + out:
            x.setflags(write=False)
        _MODEL[key] = (cov, freq, vo, out)
    return _MODEL[key]


@pytest.mark.parametrize("planes,n_vars,haploid,iters,weight", WIDE)
def test_beyond_64_planes_against_the_wide_model(ctx, planes, n_vars, haploid, iters, weight):
    cov, freq, vo, want = model(200 + planes + n_vars, planes, n_vars, haploid, iters, weight)
    what = "P=%d n=%d hap=%d T=%d w=%g" % (planes, n_vars, haploid, iters, weight)
    got = both_forms(ctx, cov, freq, vo, haploid, iters, weight, what)
    same(got, want, what)
    if iters and n_vars >= 15:
        assert want[1].max() > 32 and not np.array_equal(bits(want[0]), bits(freq))  # the inputs move the priors, from many planes


def directed(ctx, cov, freq, vo, haploid, iters, weight, what):
    cov, freq, vo = np.asarray(cov, dtype=np.uint32), np.asarray(freq, dtype=np.float32), np.asarray(vo, dtype=np.uint32)
    want = WM.estimate_priors(cov, freq, vo, E, MAX_COV, haploid, iters, weight)
    got = both_forms(ctx, cov, freq, vo, haploid, iters, weight, what)
    same(got, want, what)
    return got


def test_a_record_of_300_alleles_inside_a_run(ctx):
    """the run's coverages exceed the LDS share: every chunk reads global memory; the records around it are re-estimated"""
    rng = np.random.default_rng(5)
    vo = [0, 2, 5, 305, 308, 310]
    cov = rng.integers(0, 40, (70, 310))
    f = np.full(310, 1.0 / 310, dtype=np.float32)
    f[0:2], f[2:5], f[305:308], f[308:310] = (0.8, 0.2), (0.5, 0.25, 0.25), (0.6, 0.3, 0.1), (0.9, 0.1)
    got = directed(ctx, cov, f, vo, False, 5, 1.0, "A=300 in a run")
    assert got[1].tolist()[2] == 0 and got[1][0] > 60 and np.array_equal(bits(got[0][5:305]), bits(f[5:305]))


def test_a_run_of_records_with_eight_alleles(ctx):
    """seventeen records of eight alleles (a run and one record of the next), 65 planes: every lane's copies go through LDS"""
    rng = np.random.default_rng(6)
    n, P = 17, 65
    vo = np.arange(n + 1) * 8
    cov = rng.integers(0, 12, (P, 8 * n)) * (rng.random((P, 8 * n)) < 0.4)
    f = np.tile(np.float32([0.65, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05]), n)
    for haploid in (False, True):
        got = directed(ctx, cov, f, vo, haploid, 3, 1.0, "A=8 run hap=%d" % haploid)
        assert got[1].min() > 32


def test_chunks_that_do_not_count(ctx):
    cov, freq, vo = M.synth_batch(31, 130, 20, False, MAX_COV)
    cov = cov.copy()
    # chunk 1 entirely over-covered: c and n are those of chunks 0 and 2
    cov[64:128] = MAX_COV + 1
    got = directed(ctx, cov, freq, vo, False, 5, 1.0, "chunk 1 over-covered")
    rest = WM.estimate_priors(np.concatenate([cov[:64], cov[128:]]), freq, vo, E, MAX_COV, False, 5, 1.0)
    same(got, rest, "chunk 1 over-covered against the cohort without it")
    assert got[1].max() > 32
    # only plane 64 counts
    cov66 = np.zeros((66, cov.shape[1]), dtype=np.uint32)
    cov66[:32] = MAX_COV + 1
    cov66[64] = cov[3]
    for haploid in (False, True):
        got = directed(ctx, cov66, freq, vo, haploid, 5, 1.0, "only plane 64 hap=%d" % haploid)
        alone = ctx.genotype_cohort(cov66[64:65], freq, vo, E, MAX_COV, haploid, 5, 1.0)
        same(got, alone[:2], "only plane 64 against that plane alone")
        assert got[1].max() == 1
    # no plane has coverage: the frequencies stay, n = 0
    got = directed(ctx, np.zeros((130, cov.shape[1]), dtype=np.uint32), freq, vo, False, 5, 1.0, "no coverage")
    assert np.array_equal(bits(got[0]), bits(freq)) and not got[1].any()


@pytest.mark.parametrize("k", (16, 17))
def test_record_ranges_called_separately_equal_the_whole(ctx, k):
    cov, freq, vo, want = model(233, 70, 33, False, 5, 1.0)
    whole = ctx.estimate_priors(cov, freq, vo, E, MAX_COV, False, 5, 1.0)
    same(whole, want, "whole")
    parts = [ctx.estimate_priors(*WM.record_range(cov, freq, vo, lo, hi), E, MAX_COV, False, 5, 1.0) for lo, hi in ((0, k), (k, 33))]
    same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), whole, "ranges cut at %d" % k)


def test_stats_before_the_first_call_and_argument_errors():
    """a context of its own: MG_ERR_STATE before the first call; every argument error is MG_ERR_ARG and writes nothing"""
    with Context(35, 43, 1 << 20) as c:
        with pytest.raises(MalvaError) as e:
            c.estimate_priors_stats()
        assert e.value.code == -3
        cov, freq, vo = M.synth_batch(3, 3, 4, False, MAX_COV)
        for kw in (dict(iters=65), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(weight=-0.5, iters=0)):
            with pytest.raises(MalvaError) as e:
                c.estimate_priors(cov, freq, vo, E, MAX_COV, False, **kw)
            assert e.value.code == -1, kw
        with pytest.raises(MalvaError) as e:
            c.estimate_priors_stats()                                              # still no call that ran
        assert e.value.code == -3
        L, n, P = capi.lib(), 4, 3
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

        def outs():
            return [np.full(len(freq), 7.5, np.float32), np.full(n, 77, np.uint32)]

        def call(planes=P, cov_=cov, freq_=freq, vo_=vo, iters=5, weight=1.0, drop=None):
            o = outs()
            args = [p(x) for x in o]
            if drop is not None:
                args[drop] = None
            rc = L.mg_estimate_priors(c.h, n, planes, p(cov_), p(freq_), p(vo_), C.c_float(E), MAX_COV, 0, iters, weight, *args)
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(o, outs())), "an output was written"
            return rc

        assert call(planes=0) == -1 and call(planes=16385) == -1
        assert call(iters=65) == -1 and call(weight=-1e-300) == -1 and call(weight=float("-inf")) == -1
        assert call(cov_=None) == -1 and call(freq_=None) == -1 and call(vo_=None) == -1
        assert call(drop=0) == -1 and call(drop=1) == -1
        with pytest.raises(MalvaError) as e:
            c.estimate_priors_stats()
        assert e.value.code == -3
        assert L.mg_estimate_priors(c.h, 0, 16384, None, None, None, C.c_float(E), MAX_COV, 0, 5, 1.0, None, None) == 0
        assert np.isfinite(c.estimate_priors_stats()) and c.estimate_priors_stats() >= 0  # n_vars == 0 is a call
        # mg_genotype_cohort keeps its own range
        with pytest.raises(MalvaError) as e:
            c.genotype_cohort(np.zeros((65, len(freq)), dtype=np.uint32), freq, vo, E, MAX_COV, False)
        assert e.value.code == -1
