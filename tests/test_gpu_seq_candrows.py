"""k_seq_candwalk's rows (enc_chains_seq.h): a handed-over group is walked by rows of 16 lanes, every row loads the 256 symbols
of its group's segment itself and its lanes get their table rows by DPP broadcast from the row's own lanes.  However many
rows a group has (one, two, four), however many groups share a wave and whichever of them were handed over: the five
streams are the CPU oracle's, byte for byte."""
import pytest

from seq_blocks import block as _block
from test_gpu_seq_handover import _assert_oracle, _encode

BASES = ["uniform", "skewed", "markov", "mixed", "two_letters"]
GROUPS = [(16, 4), (8, 1), (3, 1)]
HANDOVER = [(64, 1), (32, 1), (16, 4)]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.mark.gpu
def test_smallest_case(F):
    """6 MiB, chains of some 11 segments of 1024: 10 functions in a group of 8 and a short one of 2 behind it, two groups to
    an item, four rows to a group"""
    blk = _block("uniform")
    got, (handed, kept) = _encode(F, blk, 1024, (8, 1), (64, 1))
    _assert_oracle(got, blk)
    assert handed > 0, (handed, kept)


@pytest.mark.gpu
@pytest.mark.parametrize("handover", HANDOVER, ids=lambda h: "cap%d_p%d" % h)
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "q%d_g%d" % g)
@pytest.mark.parametrize("bases", BASES)
def test_rows_give_the_oracles_streams(F, bases, group, handover):
    """6 MiB: chains of some 11 segments ("two_letters": 170, "mixed": both), so items with fewer than 16 groups, last groups
    shorter than the others of their wave, waves in which only some groups were handed over"""
    blk = _block(bases)
    got, (handed, kept) = _encode(F, blk, 1024, group, handover)
    _assert_oracle(got, blk)
    assert handed + kept > 0


@pytest.mark.gpu
@pytest.mark.parametrize("handover", [(64, 1), (32, 1), (16, 1)], ids=lambda h: "cap%d_p%d" % h)
def test_long_chains_take_several_rounds_per_item(F, handover):
    """bases from {A, C}: 16 chains of ~170 segments in groups of 2 -- 32 groups to an item, which is two rounds of a
    workgroup's waves at 32 slots per group and four at 64 -- and the chain's last group shorter than the rest of its wave"""
    blk = _block("two_letters")
    got, (handed, kept) = _encode(F, blk, 1024, (2, 1), handover)
    _assert_oracle(got, blk)
    assert handed + kept > 16 * 64
    if handover[0] >= 32:  # (at most 64 states behind 1024 symbols: test_gpu_seq_handover.py's model)
        assert handed > 0, (handed, kept)


@pytest.mark.gpu
def test_long_groups_of_a_uniform_block(F):
    """24 MiB: chains of ~45 segments of 1024 in groups of 11, handed over with up to 64 states"""
    blk = _block("uniform", 24 << 20)
    got, (handed, kept) = _encode(F, blk, 1024, (16, 4), (64, 1))
    _assert_oracle(got, blk)
    assert handed > 0, (handed, kept)


@pytest.mark.gpu
def test_shipped_segment_and_group_sizes(F):
    """segments of 4096 in groups of 8 with the shipped hand-over (32 slots: two rows to a group), on a 24 MiB block"""
    blk = _block("uniform", 24 << 20)
    got, (handed, kept) = _encode(F, blk, 4096, (8, 16), (32, 1))
    _assert_oracle(got, blk)
    assert handed > 0, (handed, kept)
