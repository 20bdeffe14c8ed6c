"""Hand-over of collapsed segment groups (k_seq_setfunc -> k_seq_candwalk -> k_seq_resolve, enc_chains_seq.h): a wave of
the set walk that is down to <= cap states behind a prefix of a group leaves the rest of the group to a kernel that walks
one lane per remaining state, and the resolve step finds a group entry's lane through the function behind the prefix.
Whatever (cap, prefix), group size and table shape: the five streams are the CPU oracle's, byte for byte."""
import numpy as np
import pytest

from seq_blocks import block as _block

BASES = ["uniform", "skewed", "markov", "all_A", "mostly_A"]
GROUPS = [(2, 1), (3, 1), (8, 1), (16, 4)]
HANDOVER = [(64, 1), (32, 2), (16, 4), (1, 1), (0, 1)]
STREAMS = ("seq", "qual", "readlens", "n_count", "n_pos")


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def _encode(F, blk, segment, group, handover):
    """-> (streams, (groups handed over, groups kept)) of one device-resident encode"""
    raw, recs, sft, qft, _ = blk
    ctx = F.Context(sft, qft)
    ctx.set_chain_params(0, seq_segment=segment, seq_group=group)
    ctx.set_seq_handover(*handover)
    b = ctx.dblock(raw, recs)
    b.encode()
    ctx.sync()
    rc, _ = b.status()
    assert rc == 0
    got, counts = b.fetch(), b.seq_handover()
    b.close()
    ctx.close()
    return got, counts


def _assert_oracle(got, blk):
    for k in STREAMS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(blk[4][k])), k


# ---------------------------------------------------------------- the expectation, on the CPU
def _fse_next(norm, log):
    """zstd's FSE_buildCTable for normalised counts (all >= 1 here: no low-probability cells) -> next[s][x - size],
    the state after coding s in state x (FSE_encodeSymbol)"""
    size = 1 << log
    step = (size >> 1) + (size >> 3) + 3
    cell_sym = np.zeros(size, dtype=np.int64)
    pos = 0
    for s, cnt in enumerate(norm):
        for _ in range(cnt):
            cell_sym[pos] = s
            pos = (pos + step) & (size - 1)
    assert pos == 0
    cumul = np.concatenate([[0], np.cumsum(norm)])
    state_table = np.zeros(size, dtype=np.int64)
    fill = cumul[:-1].copy()
    for u in range(size):
        s = cell_sym[u]
        state_table[fill[s]] = size + u
        fill[s] += 1
    nxt = np.zeros((len(norm), size), dtype=np.int64)
    x = np.arange(size, 2 * size)
    for s, cnt in enumerate(norm):
        if cnt == 1:
            dnb, dfs = (log << 16) - (1 << log), cumul[s] - 1
        else:
            max_bits = log - (int(cnt - 1).bit_length() - 1)
            dnb, dfs = (max_bits << 16) - (cnt << max_bits), cumul[s] - cnt
        nb = (x + dnb) >> 16
        nxt[s] = state_table[(x >> nb) + dfs] - size
    return nxt


def _distinct_after(norm, symbols, log=11):
    nxt = _fse_next(norm, log)
    x = np.arange(1 << log)
    for s in symbols:
        x = np.unique(nxt[s][x])
    return len(x)


def test_model_uniform_contexts_collapse_and_single_symbol_ones_do_not():
    """What the mixed-block case below relies on: behind one 1024-symbol segment a near-uniform context of log 11 carries
    at most 64 distinct states (cap 64 hands it over); a context fed its one frequent symbol is nearly a permutation of
    its states and stays far above 64, the most a group may be handed over with."""
    rng = np.random.default_rng(11)
    for norm in ([512, 510, 510, 516], [511, 513, 511, 513], [520, 505, 515, 508]):
        n = _distinct_after(norm, rng.integers(0, 4, size=1024))
        assert 16 < n <= 64, (norm, n)
    assert _distinct_after([2045, 1, 1, 1], np.zeros(1024, dtype=np.int64)) > 64
    # the long-chain case: contexts that only ever see A and C
    n = _distinct_after([1228, 818, 1, 1], rng.choice(2, size=1024, p=[0.6, 0.4]))
    assert n <= 64, n


# ---------------------------------------------------------------- bits
@pytest.mark.gpu
@pytest.mark.parametrize("handover", HANDOVER, ids=lambda h: "cap%d_p%d" % h)
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "q%d_g%d" % g)
@pytest.mark.parametrize("bases", BASES)
def test_handover_gives_the_oracles_streams(F, bases, group, handover):
    blk = _block(bases)
    got, (handed, kept) = _encode(F, blk, 1024, group, handover)
    _assert_oracle(got, blk)
    if handover[0] == 0:
        assert (handed, kept) == (0, 0)
    else:
        assert handed + kept > 0


@pytest.mark.gpu
def test_mixed_block_hands_some_groups_over_and_keeps_others(F):
    """half the reads all A (their context never merges: kept), half uniform (33-59 states behind 1024 symbols: handed over)"""
    blk = _block("mixed")
    got, (handed, kept) = _encode(F, blk, 1024, (8, 1), (64, 1))
    _assert_oracle(got, blk)
    assert handed > 0 and kept > 0, (handed, kept)


@pytest.mark.gpu
@pytest.mark.parametrize("handover", [(64, 1), (32, 1)], ids=lambda h: "cap%d_p%d" % h)
def test_long_chain_resolves_through_handed_over_groups(F, handover):
    """bases from {A, C}: 16 contexts of ~170 segments, in groups of 2 more than 64 groups per chain -- compose, resolve and
    expand of k_seq_resolve all meet handed-over groups"""
    blk = _block("two_letters")
    got, (handed, kept) = _encode(F, blk, 1024, (2, 1), handover)
    _assert_oracle(got, blk)
    assert handed > 0, (handed, kept)
    assert handed + kept > 16 * 64


@pytest.mark.gpu
def test_chains_shorter_than_the_prefix_keep_their_groups(F):
    """1 MiB: some 480 k bases over 256 contexts, no chain comes near the 5 segments of 4096 that a hand-over behind a
    prefix of 4 needs"""
    blk = _block("uniform", 1 << 20)
    got, (handed, kept) = _encode(F, blk, 4096, (8, 1), (32, 4))
    _assert_oracle(got, blk)
    assert handed == 0 and kept > 0, (handed, kept)


@pytest.mark.gpu
def test_shipped_segment_and_group_sizes(F):
    """segments of 4096 in groups of 8, the handle's own hand-over setting, on a 24 MiB block"""
    raw, recs, sft, qft, _ = blk = _block("uniform", 24 << 20)
    ctx = F.Context(sft, qft)
    ctx.set_chain_params(0, seq_segment=4096, seq_group=(8, 16))
    b = ctx.dblock(raw, recs)
    b.encode()
    ctx.sync()
    assert b.status()[0] == 0
    _assert_oracle(b.fetch(), blk)
    b.close()
    ctx.close()
