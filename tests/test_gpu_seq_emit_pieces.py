"""k_seq_emit (enc_chains_seq.h, step C of the sequence chains) walks a segment in rounds of 64 symbols -- the next round's
symbols asked for ahead, a cache line of out16 stored per round -- and the end of a chain's last segment in groups of 16.
A round too many or too few, a state that moves behind the chain's end, a pad written into the next context's run: each
changes the bytes of the sequence stream, so every case compares the five streams with the CPU oracle's encoding.

The chain lengths are chosen by their remainders mod PIECE = 512 and mod the segment length (the places where a variant
that splits a segment into pieces of 512 symbols can go wrong as well); mod 64, the round, the
remainders 0, 1, 15, 16, 17 and 511 are 0, 1, 15, 16, 17 and 63."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from seq_blocks import block as _block

STREAMS = ("seq", "qual", "readlens", "n_count", "n_pos")
PIECE = 512   # the remainders are chosen mod 512 ...
ROUND = 64    # ... and are what the kernel sees mod its round of 64 symbols and mod its group of 16
SEGMENTS = [1024, 2048, 4096]
SIZE = 3 << 20   # of the pattern blocks: some 1.4 M bases, 5 600 per context when they are uniform


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def _encode(F, blk, segment=None, group=None, handover=None):
    """-> (streams, (groups handed over, groups kept)) of one device-resident encode on a fresh handle"""
    raw, recs, sft, qft, _ = blk
    ctx = F.Context(sft, qft)
    try:
        if segment is not None:
            ctx.set_chain_params(0, seq_segment=segment, seq_group=group)
        if handover is not None:
            ctx.set_seq_handover(*handover)
        b = ctx.dblock(raw, recs)
        try:
            b.encode()
            ctx.sync()
            assert b.status()[0] == 0
            return b.fetch(), b.seq_handover()
        finally:
            b.close()
    finally:
        ctx.close()


def _same(got, want, what=""):
    for k in STREAMS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def _with_oracle(raw, recs):
    """(raw, recs, sft, qft, the oracle's encoding), the tuple seq_blocks.block returns"""
    _, _, sft, qft = O.freq_tables(raw, recs)
    o = O.OracleCtx(sft, qft)
    want = o.encode(raw, recs)
    o.close()
    assert want["rc"] == 0
    return raw, recs, sft, qft, want


def _reads(lengths, seed, base=None):
    """a FASTQ block of reads of the given lengths: random bases (or one base everywhere), Phred ~ N(30, 6) in 2 .. 41"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts = []
    for i, n in enumerate(lengths):
        seq = letters[rng.integers(0, 4, size=n)] if base is None else np.full(n, ord(base), dtype=np.uint8)
        qual = (np.clip(np.rint(rng.normal(30, 6, size=n)), 2, 41) + 33).astype(np.uint8)
        parts.append(b"@r%d\n" % i + bytes(seq) + b"\n+\n" + bytes(qual) + b"\n")
    raw = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    recs = O.parse_fastq(raw)
    assert int(recs["len"].sum()) == int(np.sum(lengths))
    return raw, recs


# ---------------------------------------------------------------- chain lengths, on the CPU
VIRTUAL = [3, 1, 1, 3]   # the bases in front of a read, positions -4 .. -1: T, C, C, T (FSE_Sequence::INITIAL_CONTEXT)
CODE = np.full(256, 255, dtype=np.uint8)
CODE[[ord(c) for c in "ACGTN"]] = [0, 1, 2, 3, 0]   # an N is coded as A


def chain_lengths(raw, recs):
    """symbols per sequence context: the context of a base is the four bases in front of it, the nearest in bits 7:6"""
    n = np.zeros(256, dtype=np.int64)
    for off, ln in zip(recs["seq_off"].astype(np.int64), recs["len"].astype(np.int64)):
        e = np.concatenate([VIRTUAL, CODE[raw[off: off + ln]]]).astype(np.int64)
        assert e.max() <= 3
        ctx = (e[3: 3 + ln] << 6) | (e[2: 2 + ln] << 4) | (e[1: 1 + ln] << 2) | e[0: ln]
        n += np.bincount(ctx, minlength=256)
    return n


def test_chain_lengths_follow_the_models_context():
    """an all-A read of L bases: one symbol each in the contexts of its first four bases, L - 4 in context 0"""
    raw, recs = _reads([10, 4, 3], seed=1, base="A")
    n = chain_lengths(raw, recs)
    assert n.sum() == 17 and n[0] == 6
    assert [int(n[c]) for c in (0xD7, 0x35, 0x0D, 0x03)] == [3, 3, 3, 2]


# ---------------------------------------------------------------- segment lengths
@pytest.mark.gpu
@pytest.mark.parametrize("segment", SEGMENTS, ids=lambda s: "S%d" % s)
@pytest.mark.parametrize("bases", ["uniform", "markov", "all_A", "mostly_A"])
def test_every_segment_length_gives_the_oracles_streams(F, bases, segment):
    """uniform: a handful of segments per context, most lanes of an item are behind the chain's end; all_A: one chain of
    hundreds to thousands of segments (many items, full waves) and 251 contexts with no symbol at all"""
    blk = _block(bases, SIZE)
    got, _ = _encode(F, blk, segment)
    _same(got, blk[4], (bases, segment))


def test_the_shapes_the_sweep_relies_on():
    for bases in ("uniform", "all_A"):
        raw, recs = _block(bases, SIZE)[:2]
        n = chain_lengths(raw, recs)
        assert n.sum() == int(recs["len"].sum())
        if bases == "uniform":   # every context: some segments, never a full item of 64
            assert n.min() > 1024 and n.max() < 64 * 1024, (n.min(), n.max())
        else:                    # one long chain, five contexts in use
            assert n[0] > 64 * 4096 * 4 and np.count_nonzero(n) == 5, (n[0], np.count_nonzero(n))


# ---------------------------------------------------------------- piece edges of the last segment
def _poly_a(n0):
    """all-A reads whose context 0 (AAAA in front) gets exactly n0 symbols: reads of 104 give it 100 each, the last one the rest"""
    k = (n0 - 1) // 100
    lengths = [104] * k + [n0 - 100 * k + 4]
    return _reads(lengths, seed=n0 % 1000, base="A")


# (segment, chain length of context 0, what it is about)
EDGES = [(S, full * S + pieces * PIECE + r, "r%d" % r)
         for S, full, pieces in ((1024, 3, 1), (4096, 2, 3), (4096, 1, 7), (2048, 0, 2))
         for r in (0, 1, 15, 16, 17, PIECE - 1)]
EDGES += [(1024, 4 * 1024, "whole"), (2048, 3 * 2048, "whole"), (4096, 2 * 4096, "whole"),
          (1024, 300, "short"), (4096, 300, "short"), (1024, 7, "tiny"), (4096, 15, "tiny"), (2048, 16, "tiny"),
          (1024, 64 * 1024 + 17, "item2"), (1024, 129 * 1024 + 512 + 16, "item3"), (4096, 64 * 4096 + PIECE - 1, "item2")]


@functools.lru_cache(maxsize=None)
def _edge_block(n0):
    return _with_oracle(*_poly_a(n0))


@pytest.mark.gpu
@pytest.mark.parametrize("segment,n0,kind", EDGES, ids=lambda v: str(v))
def test_last_segment_ends_at_a_chosen_place_of_a_piece(F, segment, n0, kind):
    blk = _edge_block(n0)
    raw, recs = blk[:2]
    n = chain_lengths(raw, recs)
    assert n.sum() == int(recs["len"].sum())
    assert n[0] == n0 and np.count_nonzero(n) == 5
    if kind.startswith("r"):
        r = int(kind[1:])
        assert n0 % PIECE == r and n0 % segment != 0 and n0 > PIECE
        assert (n0 % segment) % ROUND == r % ROUND and (n0 % segment) % 16 == r % 16   # where the last segment ends in its round, its group
    elif kind == "whole":
        assert n0 % segment == 0
    elif kind == "short":
        assert 16 < n0 < PIECE
    elif kind == "tiny":
        assert n0 <= 16
    else:   # the chain's last segment is the first lane of a later item
        assert (n0 // segment) % 64 in (0, 1) and n0 // segment >= 64
    got, _ = _encode(F, blk, segment)
    _same(got, blk[4], (segment, n0))


def test_the_listed_remainders_occur():
    for S in SEGMENTS:
        rem = {n0 % PIECE for s, n0, kind in EDGES if s == S and kind.startswith("r")}
        assert rem >= {0, 1, 15, 16, 17, PIECE - 1}, (S, rem)
        assert {r % ROUND for r in rem} >= {0, 1, 15, 16, 17, ROUND - 1}, (S, rem)
    assert {kind for _, _, kind in EDGES} >= {"whole", "short", "tiny", "item2"}


# ---------------------------------------------------------------- hand-over upstream
@pytest.mark.gpu
@pytest.mark.parametrize("handover", [(0, 1), None, (64, 1)], ids=["off", "default", "cap64_p1"])
@pytest.mark.parametrize("bases", ["uniform", "mostly_A"])
def test_handover_on_and_off(F, bases, handover):
    """segments of 1024 in groups of 8: behind one segment a uniform context is down to fewer than 64 states and is handed
    over at cap 64, the context that sees A after A never is (tests/test_gpu_seq_handover.py) -- step C gets its entry
    states through both kinds of group"""
    blk = _block(bases, SIZE)
    got, (handed, kept) = _encode(F, blk, 1024, (8, 1), handover)
    _same(got, blk[4], (bases, handover))
    print("handed over, kept:", handed, kept)
    if handover == (0, 1):
        assert (handed, kept) == (0, 0)
    else:
        assert handed + kept > 0
    if handover == (64, 1):
        assert (handed if bases == "uniform" else kept) > 0, (handed, kept)


# ---------------------------------------------------------------- N, short reads, run padding
@functools.lru_cache(maxsize=None)
def _mode4():
    import fqcomp28_amd as F
    raw, n = F.synth_fastq(200 << 10, 4, seed=28)   # lengths 50 .. 300, N with probability 0.01
    recs = F.parse_fastq(raw)
    assert len(recs) == n
    return _with_oracle(raw, recs)


@functools.lru_cache(maxsize=None)
def _short_reads():
    rng = np.random.default_rng(3)
    raw, recs = _reads([int(x) for x in rng.integers(3, 16, size=4000)], seed=4)
    raw = raw.copy()
    for off, ln in zip(recs["seq_off"].astype(np.int64)[::7], recs["len"].astype(np.int64)[::7]):
        raw[off + int(rng.integers(0, ln))] = ord("N")
    return _with_oracle(raw, O.parse_fastq(raw))


@pytest.mark.gpu
@pytest.mark.parametrize("segment", [None] + SEGMENTS, ids=lambda s: "S%s" % s)
@pytest.mark.parametrize("which", ["mode4", "short_reads"])
def test_reads_with_n_and_reads_shorter_than_a_group(F, which, segment):
    """few symbols per context: every run ends inside its first segment, most inside the first piece, and is padded to 16"""
    blk = _mode4() if which == "mode4" else _short_reads()
    got, _ = _encode(F, blk, segment)
    _same(got, blk[4], (which, segment))


def test_the_small_blocks_have_n_short_reads_and_padded_runs():
    for which, blk in (("mode4", _mode4()), ("short_reads", _short_reads())):
        raw, recs = blk[:2]
        n = chain_lengths(raw, recs)
        assert n.sum() == int(recs["len"].sum())
        assert int(np.asarray(blk[4]["n_count"]).sum()) > 0, which
        if which == "short_reads":
            assert recs["len"].max() < 16
        assert np.count_nonzero(n % 16) > 100 and np.count_nonzero((n > 0) & (n < PIECE)) > 50, which


# ---------------------------------------------------------------- the handle's scratch
@pytest.mark.gpu
def test_second_encode_on_one_handle_equals_the_first(F):
    """all_A, the uniform block, all_A again through ONE lane's scratch, segments of 4096 then 1024 then 4096: out16, the
    entry states and the plan of the block in between are what the third encode finds"""
    a, u = _block("all_A", SIZE), _block("uniform", SIZE)
    sft, qft = u[2:4]   # the uniform block's tables: both blocks stay inside their capacity rule under them
    want = {}
    for name, blk in (("a", a), ("u", u)):
        o = O.OracleCtx(sft, qft)
        want[name] = o.encode(*blk[:2])
        o.close()
        assert want[name]["rc"] == 0
    ctx = F.Context(sft, qft)
    ctx.set_lanes(1)
    got = []
    try:
        for name, blk, segment in (("a", a, 4096), ("u", u, 1024), ("a", a, 4096)):
            ctx.set_chain_params(0, seq_segment=segment)
            b = ctx.dblock(*blk[:2])
            try:
                b.encode()
                ctx.sync()
                assert b.status()[0] == 0
                got.append(b.fetch())
            finally:
                b.close()
            _same(got[-1], want[name], (name, segment))
    finally:
        ctx.close()
    _same(got[2], got[0], "second against first")
