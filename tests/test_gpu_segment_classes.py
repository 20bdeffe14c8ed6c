"""fqgpu_dblock_qual_segment_classes reads the scratch of the encode lane that coded the block.  It answers only while that
lane still holds THIS block's encode -- the lane keeps the stamp of its last encode, the block the stamp of its own -- and
refuses (FQGPU_E_ARG) whatever would mean reading another block's classes or memory that is gone."""
import ctypes as C

import pytest

import oracle_lib as O
from test_gpu_parity import _synth

pytestmark = pytest.mark.gpu

E_ARG = -4


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def classes_rc(F, ctx, block):
    c = (C.c_size_t * 4)()
    return F.lib().fqgpu_dblock_qual_segment_classes(ctx.h, block.h, c)


def test_a_stale_diagnostic_is_refused_and_a_fresh_one_is_not(F):
    """One lane.  Block A (3 MiB of synth mode 6: two quality levels, every segment opaque, as in
    test_two_quality_levels_every_segment_needs_its_full_function) answers after its encode; once block B (6 MiB, mode 2) has
    gone through the lane, A is refused; re-encoded, A answers again with the same classes.  A block that was never
    encoded, a block of another handle, and a block that was not encoded since fqgpu_ctx_reserve grew the lane's buffers,
    since a fill_scratch or since set_lanes are refused too."""
    raw_a, recs_a = _synth(F, 6, 3 << 20)
    raw_b, recs_b = _synth(F, 2, 6 << 20)
    _, _, sft, qft = O.freq_tables(raw_a, recs_a)
    ctx, other = F.Context(sft, qft), F.Context(sft, qft)
    ctx.set_lanes(1)
    a, b, foreign = ctx.dblock(raw_a, recs_a), ctx.dblock(raw_b, recs_b), other.dblock(raw_a, recs_a)
    try:
        assert classes_rc(F, ctx, a) == E_ARG   # no encode yet
        a.encode()
        cls = a.qual_segment_classes()
        assert cls["opaque"] > 0.9 * sum(cls.values()) and cls["transparent"] == 0, cls
        assert classes_rc(F, ctx, b) == E_ARG   # (a block the lane has not seen)
        b.encode()
        assert sum(b.qual_segment_classes().values()) > 0
        assert classes_rc(F, ctx, a) == E_ARG   # the lane's classes are B's now
        with pytest.raises(F.FqgpuError) as err:
            a.qual_segment_classes()
        assert err.value.code == E_ARG
        a.encode()
        assert a.qual_segment_classes() == cls
        assert classes_rc(F, ctx, b) == E_ARG
        # reserving ahead for a block four times B's size moves the lane's buffers without being an encode
        n_bases_b = int(recs_b["len"].sum())
        assert F.lib().fqgpu_ctx_reserve(ctx.h, 4 * raw_b.size, 4 * len(recs_b), 4 * n_bases_b) == 0
        assert classes_rc(F, ctx, a) == E_ARG
        a.encode()
        assert a.qual_segment_classes() == cls
        # a fill overwrites the classes and their number
        ctx.fill_scratch(0xA5)
        assert classes_rc(F, ctx, a) == E_ARG
        a.encode()
        assert a.qual_segment_classes() == cls
        foreign.encode()
        assert foreign.qual_segment_classes() == cls   # asked through its own handle
        assert classes_rc(F, ctx, foreign) == E_ARG    # ... and through another one
        assert a.qual_segment_classes() == cls          # (which has not been disturbed)
        ctx.set_lanes(2)
        assert classes_rc(F, ctx, a) == E_ARG   # the lanes were dealt anew
        a.encode()
        assert a.qual_segment_classes() == cls
    finally:
        for blk in (a, b, foreign):
            blk.close()
        ctx.close()
        other.close()
