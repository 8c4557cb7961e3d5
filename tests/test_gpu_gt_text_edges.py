"""mg_decode_gt_text / mg_decode_gt_entries (csrc/gt_text_kernels.h) against oracle/model.py on the directed cases of
tests/gt_text_cases.py: tabs on every seam of the scan (16-byte piece, 1,024-byte wave, 4,096-byte tile), spans of every length
around them, widths and keep masks around the 256-sample tiles, more records than either persistent grid, every GT form in every
place, allele numbers past the words, the default word at its tie, spans anywhere in the text, and what the call refuses.
Everything is exact.  tests/test_gt_text_cases_cpu.py asserts, without a GPU, that each case's bytes hold what its name says."""
import numpy as np
import pytest

import gt_text_cases as gtc
from malva_amd import Context, MalvaError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(35, 43, 1 << 16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the model's reading of a case, made once per (case, mode) and left unchanged"""
    memo = {}

    def get(name, haploid):
        if (name, haploid) not in memo:
            memo[name, haploid] = gtc.build(gtc.get(name), str(tmp_path_factory.mktemp("gt")), haploid)
        return memo[name, haploid]
    return get


def _check(ctx, case, b, haploid):
    dflt, sp_off, ss, sg, mask, mx = ctx.decode_gt_text(b.raw, b.off, b.ln, b.gi, b.n_columns, b.keep, haploid)
    n = len(b.want)
    assert len(sp_off) == n + 1 and sp_off[0] == 0 and len(mask) == len(mx) == n
    beyond = gtc.claim(case, "max_only")
    beyond = set(beyond[0]) if beyond else set()
    sel_beyond = {i for i, r in enumerate(b.select) if r in beyond}
    got = gtc._dense(b.n_keep, dflt, sp_off, ss, sg)                     # (asserts ascending samples and no default word among the entries)
    assert len(ss) == len(sg) == int(sp_off[-1])
    if not sel_beyond:                                                   # the default word: the model's words, counted as the host counts the device's
        assert dflt == gtc.default_word(b.want, haploid)
        claimed = gtc.claim(case, "default")
        if claimed is not None:
            assert dflt == (gtc.PHASED0 if haploid else claimed[0])
    assert dflt in (0, gtc.PHASED0) and (not haploid or dflt == gtc.PHASED0)
    for i in range(n):
        if i in sel_beyond:
            assert int(mx[i]) == 32767, (i, int(mx[i]))
            continue
        g, w = got[i], b.want[i]
        assert np.array_equal(g, w), (i, np.flatnonzero(g != w)[:5], g[g != w][:5], w[g != w][:5])
        assert int(sp_off[i + 1]) - int(sp_off[i]) == int((w != dflt).sum()), i
        assert int(mask[i]) == b.masks[i], (i, hex(int(mask[i])), hex(b.masks[i]))
        assert int(mx[i]) == b.maxes[i], (i, int(mx[i]), b.maxes[i])
    return dflt, sp_off


@pytest.mark.parametrize("name,haploid", gtc.runs(), ids=["%s-%s" % (n, "haploid" if h else "diploid") for n, h in gtc.runs()])
def test_case(ctx, built, name, haploid):
    case = gtc.get(name)
    dflt, sp_off = _check(ctx, case, built(name, haploid), haploid)
    if name == "F-only-unphased" and not haploid:
        assert dflt == 0 and int(sp_off[-1]) == 0                        # nothing to copy, and mg_decode_gt_entries said so without complaint
    if name == "G-zero-records":
        assert len(sp_off) == 1
    if name == "E-largest-allele":
        b = built(name, haploid)
        assert 128 in b.maxes and 32767 in b.maxes                       # (the two the model is asked about are among the records compared)


@pytest.mark.parametrize("haploid", [False, True])
def test_a_smaller_batch_after_a_larger_one(ctx, built, haploid):
    """3,100 records, then 1,025 on the same context: the scratch the larger batch left (tokens, words, offsets) must not show"""
    for name in gtc.LOOP_TWICE:
        _check(ctx, gtc.get(name), built(name, haploid), haploid)
    _check(ctx, gtc.get("B-width-513"), built("B-width-513", haploid), haploid)     # and a wider one after the many narrow ones
    _check(ctx, gtc.get("C-records-1"), built("C-records-1", haploid), haploid)


@pytest.mark.parametrize("refusal", list(gtc.REFUSALS))
def test_refused_and_the_next_batch_is_still_right(ctx, built, refusal):
    case = gtc.get(gtc.REFUSALS_OVER)
    b = built(gtc.REFUSALS_OVER, False)
    a = dict(raw=b.raw, off=b.off, ln=b.ln, gi=b.gi, n_columns=b.n_columns, keep=b.keep)
    gtc.REFUSALS[refusal](a)
    with pytest.raises(MalvaError):
        ctx.decode_gt_text(a["raw"], a["off"], a["ln"], a["gi"], a["n_columns"], a["keep"], False)
    _check(ctx, case, b, False)
