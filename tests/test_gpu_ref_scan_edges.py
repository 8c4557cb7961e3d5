"""The index-time reference scan on the device against the oracle on the directed cases of tests/ref_scan_cases.py.  For every case:
`bf` is filled through bf_insert with the restated centre strings of the claimed windows and must equal the oracle's words; then
the contig is scanned three ways -- mg_ref_scan (packed on the fly), mg_ref_scan_resident inside the buffer the case uploads, and
the byte-wise kernel for every window (use_packed_ref_scan 0) -- and after bf_finalize the set positions of context_bf must be
the oracle's, one per claimed window.  Everything is exact.  tests/test_ref_scan_cases_cpu.py proves, without a GPU, that each
case holds what its name says and that its expected filter has one bit per claimed window."""
import numpy as np
import pytest
import torch

import ref_scan_cases as rc
from malva_amd import BF_ALT, BF_CTX, Context
from malva_amd.capi import MG_ERR_ARG, MalvaError, rows_of

pytestmark = pytest.mark.gpu

MG_ERR_STATE = -3
NONE = np.zeros(0, dtype=np.uint64)


@pytest.fixture(scope="module")
def context_of():
    """one context per setup, shared by its consecutive cases: both filters are emptied (an import of no positions) between them"""
    held = {}

    def get(S):
        if S.name not in held:
            for ctx in held.values():
                ctx.close()
            held.clear()
            held[S.name] = Context(S.k, S.ref_k, S.bits)
        return held[S.name]
    yield get
    for ctx in held.values():
        ctx.close()


def _empty(ctx, which, S):
    ctx.bf_import_sparse(which, 0, S.bits, NONE, np.zeros(0, dtype=np.uint16))


def _fill_bf(ctx, S, keys, obf):
    _empty(ctx, BF_ALT, S)
    if keys:
        ctx.bf_insert(BF_ALT, rows_of(keys, stride=(max(S.k, max(len(x) for x in keys)) + 8) // 8 * 8))
    ctx.bf_finalize(BF_ALT)
    got = ctx.bf_export(BF_ALT)[2]
    assert np.array_equal(got, obf.words())


def _run(ctx, c, route):
    if route == "resident":
        ctx.reference_upload(c.buffer)
        ctx.ref_scan_resident(c.offset, c.length)
    elif route == "resident-device":
        d = torch.from_numpy(np.frombuffer(c.buffer + b"\0", dtype=np.uint8).copy()).to("cuda:0")
        torch.cuda.synchronize()
        ctx.reference_upload_device(d.data_ptr(), len(c.buffer))
        del d                                                    # (the context keeps a copy: the caller's buffer may go)
        ctx.ref_scan_resident(c.offset, c.length)
    else:
        ctx.ref_scan(c.contig)


def _scan_and_compare(ctx, S, c, route, want):
    _empty(ctx, BF_CTX, S)
    ctx.set_option("use_packed_ref_scan", 0 if route == "bytewise" else 1)
    try:
        if c.err:
            with pytest.raises(MalvaError) as e:
                _run(ctx, c, route)
            assert e.value.code == MG_ERR_ARG, route
        else:
            _run(ctx, c, route)
    finally:
        ctx.set_option("use_packed_ref_scan", 1)
    ctx.bf_finalize(BF_CTX)
    got = ctx.bf_export_sparse(BF_CTX)[2]
    assert len(got) == len(want), (c.name, route, len(got), len(want))
    assert np.array_equal(got, want), (c.name, route)


ROUTES = ("host", "resident", "bytewise")


@pytest.mark.parametrize("name", rc.case_ids())
def test_ref_scan_case(context_of, name):
    c = rc.case(name)
    S = rc.setup(c.setup)
    ctx = context_of(S)
    obf, octx = rc.expected(c)
    want = octx.set_positions()
    assert len(want) == len(c.hits)
    _fill_bf(ctx, S, rc.bf_keys(c), obf)
    for route in ROUTES:
        _scan_and_compare(ctx, S, c, route, want)


SAMPLE = [n for n in rc.case_ids(("full",)) if n.split("/")[1] in ("P0", "P31", "P12345", "ends-buffer", "N64-P1", "N71-P31", "nb-B1", "quirk-all", "len-r+2048", "len-off")
          or "short" in rc.case(n).seams]


@pytest.mark.parametrize("name", SAMPLE)
def test_resident_scan_of_a_reference_uploaded_from_the_device(context_of, name):
    c = rc.case(name)
    S = rc.setup(c.setup)
    ctx = context_of(S)
    obf, octx = rc.expected(c)
    _fill_bf(ctx, S, rc.bf_keys(c), obf)
    _scan_and_compare(ctx, S, c, "resident-device", octx.set_positions())


@pytest.mark.parametrize("setup", [S.name for S in rc.SETUPS.values() if S.table == "full"])
@pytest.mark.parametrize("P", [0, 1, 31])
def test_two_contigs_scanned_by_two_calls_accumulate(context_of, setup, P):
    A, B = rc.case("%s/nb-A%d" % (setup, P)), rc.case("%s/nb-B%d" % (setup, P))
    S = rc.setup(setup)
    ctx = context_of(S)
    keys = rc.bf_keys(A) + rc.bf_keys(B)
    obf = rc.oracle_bf(S, keys)
    from oracle import capi as ocapi
    octx = ocapi.BF(S.bits)
    ocapi.ref_scan(obf, octx, A.contig, S.k, S.ref_k)
    ocapi.ref_scan(obf, octx, B.contig, S.k, S.ref_k)
    want = octx.set_positions()
    assert len(want) == len(A.hits) + len(B.hits)               # no window of one contig shares a bit with one of the other
    _fill_bf(ctx, S, keys, obf)
    for resident in (False, True):
        _empty(ctx, BF_CTX, S)
        if resident:
            ctx.reference_upload(A.buffer)
            ctx.ref_scan_resident(B.offset, B.length)           # (B first: the order of the calls is nothing to the filter)
            ctx.ref_scan_resident(A.offset, A.length)
        else:
            ctx.ref_scan(A.contig)
            ctx.ref_scan(B.contig)
        ctx.bf_finalize(BF_CTX)
        assert np.array_equal(ctx.bf_export_sparse(BF_CTX)[2], want), resident


def test_a_second_shorter_upload_replaces_a_longer_one(context_of):
    long_, short = rc.case("35-44/P12345"), rc.case("35-44/ends-buffer")
    assert len(short.buffer) < len(long_.buffer) - 10000
    S = rc.setup("35-44")
    ctx = context_of(S)
    obf, octx = rc.expected(short)
    _fill_bf(ctx, S, rc.bf_keys(short), obf)
    _empty(ctx, BF_CTX, S)
    ctx.reference_upload(long_.buffer)
    ctx.reference_upload(short.buffer)
    with pytest.raises(MalvaError) as e:                        # where the longer one had bases, the shorter has none
        ctx.ref_scan_resident(long_.offset, long_.length)
    assert e.value.code == MG_ERR_ARG
    with pytest.raises(MalvaError) as e:
        ctx.ref_scan_resident(short.offset + 1, short.length)   # one base beyond the upload's end
    assert e.value.code == MG_ERR_ARG
    assert not ctx.bf_export(BF_CTX)[2].any()
    ctx.ref_scan_resident(short.offset, short.length)
    ctx.bf_finalize(BF_CTX)
    assert np.array_equal(ctx.bf_export_sparse(BF_CTX)[2], octx.set_positions()) and octx.popcount() == len(short.hits)


def test_calls_out_of_order_answer_their_code_and_leave_the_context_filter_alone():
    c = rc.case("35-43/P7")
    S = rc.setup(c.setup)
    keys = rc.bf_keys(c)

    def refused(ctx, code, call, *args):
        before = ctx.bf_export(BF_CTX)[2].copy()
        with pytest.raises(MalvaError) as e:
            call(*args)
        assert e.value.code == code, (call.__name__, e.value.code)
        assert np.array_equal(ctx.bf_export(BF_CTX)[2], before)

    with Context(S.k, S.ref_k, 1 << 20) as ctx:
        ctx.bf_insert(BF_ALT, rows_of(keys))
        ctx.bf_insert(BF_CTX, rows_of([c.contig[:S.ref_k]]))      # a bit that must stay, and stay alone
        refused(ctx, MG_ERR_STATE, ctx.ref_scan_resident, 0, 10)                        # nothing uploaded
        ctx.reference_upload(c.buffer)
        refused(ctx, MG_ERR_STATE, ctx.ref_scan, c.contig)                              # `bf` not finalised
        refused(ctx, MG_ERR_STATE, ctx.ref_scan_resident, c.offset, c.length)
        ctx.bf_finalize(BF_ALT)
        refused(ctx, MG_ERR_ARG, ctx.ref_scan_resident, c.offset, len(c.buffer) - c.offset + 1)   # offset + len beyond the upload
        refused(ctx, MG_ERR_ARG, ctx.ref_scan_resident, len(c.buffer) + 1, 0)
        ctx.bf_finalize(BF_CTX)
        assert ctx.bf_info(BF_CTX)[1] == 1
        refused(ctx, MG_ERR_STATE, ctx.ref_scan, c.contig)                              # context_bf finalised
        refused(ctx, MG_ERR_STATE, ctx.ref_scan_resident, c.offset, c.length)
        ctx.cohort_begin(2)
        refused(ctx, MG_ERR_STATE, ctx.ref_scan, c.contig)                              # cohort mode
        refused(ctx, MG_ERR_STATE, ctx.ref_scan_resident, c.offset, c.length)
        ctx.cohort_end()
        assert ctx.bf_info(BF_CTX)[1] == 1
