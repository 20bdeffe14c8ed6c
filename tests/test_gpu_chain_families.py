"""The quality chain stage of the encoder (fqcomp28_amd/csrc/enc_chains_generic.h) class by class and at its item edges:
every case of tests/chain_ref.py's families is coded through the C ABI with the case's segment length and compared in full
-- the streams with the oracle's byte for byte, every segment's class, anchor and context (DBlock.qual_segments) with the
restatement, the class counts with the sums of the same list -- and decoded back from the device's own streams.  The
families whose function slots are sparse run once more on a handle whose scratch was all ones and then all zeros.
tests/test_chain_families_host.py holds the same cases and the restatement to the oracle and to second statements."""
import numpy as np
import pytest

import chain_ref as C
from test_gpu_parity import assert_same_encoding

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module")
def handles(F):
    """one handle per table set, made when first asked for"""
    made = {}

    def get(key):
        if key not in made:
            made[key] = F.Context(*C.tables(key))
        return made[key]

    yield get
    for c in made.values():
        c.close()


def check_case(ctx, case, what=""):
    """one encode of the case on ctx, compared in full"""
    name = (what, C.case_id(case))
    ctx.set_chain_params(case.extra["S"], seq_generic=case.extra.get("seq_generic", False))
    b = ctx.dblock(case.raw, case.recs)
    try:
        b.encode()
        g = b.fetch()
        assert_same_encoding(dict(g, rc=b.status()[0]), C.coded(case))
        if case.family in C.QUAL_FAMILIES:
            got = b.qual_segments()
            ctx_want, outcomes, _ = C.segments(case)
            assert np.array_equal(got["ctx"], ctx_want), name
            same = [np.array_equal(got["cls"], cls) and np.array_equal(got["anchor"], anchor) for cls, anchor in outcomes]
            if not any(same):
                cls, anchor = outcomes[0]
                bad = np.flatnonzero((got["cls"] != cls) | (got["anchor"] != anchor))
                raise AssertionError((name, "first segments that differ from the first allowed outcome",
                                      [(int(i), int(ctx_want[i]), (int(got["cls"][i]), int(got["anchor"][i])), (int(cls[i]), int(anchor[i]))) for i in bad[:5]]))
            cls = got["cls"]
            assert b.qual_segment_classes() == dict(transparent=int((cls == 1).sum()), anchored=int(((cls >= 2) & (cls <= C.MAX_CAND)).sum()),
                                                    uniform=int((cls == C.UNIFORM).sum()), opaque=int((cls == C.OPAQUE).sum())), name
        b.wipe()
        ctx.decode_dblocks([b])
        assert b.status()[0] == 0 and np.array_equal(b.fetch_raw(), case.raw), name
    finally:
        b.close()


def by_tables(cases):
    out = {}
    for c in cases:
        out.setdefault(c.tables, []).append(c)
    return out


FAMILIES = C.QUAL_FAMILIES + ("seq-generic",)
SPARSE = ("pairs", "heads", "items", "uniform")  # their function slots are sparse: run again over a filled scratch


@pytest.mark.parametrize("family", FAMILIES)
def test_family(F, handles, family):
    cases = C.of_family(family)
    assert cases
    for key, group in by_tables(cases).items():
        ctx = handles(key)
        for case in group:
            check_case(ctx, case)
            if family == "seq-generic":  # ... and the default path on the same tables
                check_case(ctx, case._replace(extra=dict(case.extra, seq_generic=False)), "default sequence path")


@pytest.mark.parametrize("family", SPARSE)
def test_family_over_a_scratch_of_all_ones_and_then_all_zeros(F, family):
    """the unwritten entries of the sparse function slots are first all ones and then all zeros when k_seg_compose pulls
    them into range; zero is also a reset symbol of the crafted rows, in the padding behind a short last segment"""
    for key, group in by_tables(C.of_family(family)).items():
        ctx = F.Context(*C.tables(key))
        try:
            # (a handle that has done nothing owns no scratch to fill: the largest case sizes it)
            check_case(ctx, max(group, key=lambda c: c.raw.size), "sizes the scratch")
            for byte in (0xFF, 0x00):
                for case in group:
                    buffers, n_bytes = ctx.fill_scratch(byte)
                    assert buffers > 0 and n_bytes > 0
                    check_case(ctx, case, "scratch of 0x%02X" % byte)
        finally:
            ctx.close()


def test_the_segment_list_answers_and_refuses_as_the_class_counts_do(F):
    """fqgpu_dblock_qual_segments shares its guards with fqgpu_dblock_qual_segment_classes: FQGPU_E_ARG before the block's
    first encode, once another block has gone through the lane and after a fill of the scratch; a capacity that is too small
    is FQGPU_E_OVERFLOW with the number of segments, nothing written"""
    import ctypes as C_

    case, other = C.of_family("walk-ends")[0], C.of_family("pairs")[0]
    ctx = F.Context(*C.tables("main"))
    ctx.set_lanes(1)
    ctx.set_chain_params(1024)
    a, b = ctx.dblock(case.raw, case.recs), ctx.dblock(other.raw, other.recs)

    def rc_of(blk, cap, arrays=True):
        n = C_.c_size_t(77)
        cls, anchor, cx = np.full(max(cap, 1), 0xEE, dtype=np.uint8), np.zeros(max(cap, 1), dtype=np.uint32), np.zeros(max(cap, 1), dtype=np.uint32)
        p = (lambda x: x.ctypes.data_as(C_.c_void_p)) if arrays else (lambda x: None)
        rc = F.lib().fqgpu_dblock_qual_segments(ctx.h, blk.h, p(cls), p(anchor), p(cx), cap, C_.byref(n))
        return rc, n.value, cls
    try:
        assert rc_of(a, 4096)[:2] == (-4, 0)          # no encode yet
        a.encode()
        n = len(C.segments(case)[0])
        rc, got, cls = rc_of(a, n - 1)
        assert (rc, got) == (-1, n) and (cls == 0xEE).all()
        assert rc_of(a, 0, arrays=False)[:2] == (-1, n)
        assert rc_of(a, 5, arrays=False)[0] == -4     # a capacity without arrays
        assert rc_of(a, n)[:2] == (0, n) and len(a.qual_segments()["cls"]) == n
        b.encode()
        assert rc_of(a, 4096)[:2] == (-4, 0)          # the lane's segments are b's now
        with pytest.raises(F.FqgpuError):
            a.qual_segments()
        assert len(b.qual_segments()["cls"]) == len(C.segments(other)[0])
        ctx.fill_scratch(0xA5)
        assert rc_of(b, 4096)[:2] == (-4, 0)
    finally:
        a.close(); b.close(); ctx.close()
