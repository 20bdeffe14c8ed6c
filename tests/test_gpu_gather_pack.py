"""K6 (k_tile_gather_pack: gather of the sorted tile's codes, bit offsets, bit packing) at the smallest shapes at which it
can go wrong: every stream byte for byte against the CPU oracle, then back to the raw block.  A tile is 32 768 symbols
= 256 reads of 128; a packing round is 4 096 symbols, eight per thread."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

READ = 128
TILE = 32768
NW = 1540  # words of K6's packing buffer: up to NW - 1 runs of a tile keep their offsets in LDS, more are read from the run list


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def _fastq(seqs, quals):
    """one record per (bases, qualities) pair: uint8 arrays of letters / of Phred values"""
    parts = []
    for i, (s, q) in enumerate(zip(seqs, quals)):
        parts.append(b"@r%d\n" % i + bytes(s) + b"\n+\n" + bytes((np.asarray(q) + 33).astype(np.uint8)) + b"\n")
    raw = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    return raw, O.parse_fastq(raw)


def _block(lengths, seed, qual="normal", base=None):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs, quals = [], []
    for n in lengths:
        seqs.append(letters[rng.integers(0, 4, size=n)] if base is None else np.full(n, ord(base), dtype=np.uint8))
        if qual == "normal":
            quals.append(np.clip(np.rint(rng.normal(30, 6, size=n)), 2, 41).astype(np.uint8))
        elif qual == "uniform":
            quals.append(rng.integers(2, 42, size=n).astype(np.uint8))
        else:
            quals.append(np.full(n, qual, dtype=np.uint8))
    return _fastq(seqs, quals)


def _same_streams_and_back(F, ctx, octx, raw, recs, **caps):
    e = octx.encode(raw, recs, **caps)
    g = ctx.encode_block(raw, recs, **caps)
    assert e["rc"] == 0 and g["rc"] == 0, (e["rc"], g["rc"])
    for k in ("seq", "qual", "readlens", "n_count", "n_pos"):
        assert np.array_equal(np.asarray(g[k]), np.asarray(e[k])), k
    rc, out = ctx.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs))
    assert rc == 0 and np.array_equal(out, raw)
    return e


def _check(F, raw, recs):
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx, octx = F.Context(sft, qft), O.OracleCtx(sft, qft)
    try:
        return _same_streams_and_back(F, ctx, octx, raw, recs)
    finally:
        ctx.close()
        octx.close()


@pytest.mark.parametrize("lengths", [
    [READ] * 5,              # one partial tile
    [READ] * 256,            # exactly one full tile and nothing else
    [READ] * 256 + [3],      # a full tile and three symbols
    [READ] * 513,            # two full tiles and a partial one: edge words between tiles beside the full-tile path
    [3],                     # less than one thread's share of a round
], ids=["5_reads", "one_full_tile", "full_tile_plus_3", "two_full_tiles_and_a_part", "one_read_of_3"])
def test_tile_edges(F, lengths):
    raw, recs = _block(lengths, seed=len(lengths))
    assert int(recs["len"].sum()) == sum(lengths)
    _check(F, raw, recs)


def test_both_run_list_paths(F):
    """Qualities uniform in [2, 41]: the symbols of a tile spread over far more contexts than the run offsets K6 keeps in
    LDS, so the quality tiles look their runs up in the run list; the sequence tiles of the same block have at most 256
    runs and stay in LDS."""
    raw, recs = _block([READ] * 513, seed=7, qual="uniform")
    ctxs = []
    for r in recs[:256]:  # contexts of the first tile (numpy restatement of FSE_Quality::calcContext)
        q = raw[r["qual_off"]: r["qual_off"] + r["len"]].astype(np.int64) - 33
        a = np.concatenate(([0], q[:-1])); b = np.concatenate(([0, 0], q[:-2])); c = np.concatenate(([0, 0, 0], q[:-3]))
        ctxs.append(((np.maximum(b, c) << 6) + a) & 0xFFF | ((b == c).astype(np.int64) << 12))
    assert np.unique(np.concatenate(ctxs)).size > NW
    _check(F, raw, recs)


def test_one_context_per_tile_codes_in_zero_bits(F):
    """Every base A, every quality one value, tables from the block itself: 0 bits per symbol -- every thread's string is
    empty, no OR is issued, a tile's total is 0 and all tiles share one stream word."""
    raw, recs = _block([READ] * 513, seed=1, qual=40, base="A")
    e = _check(F, raw, recs)
    n = int(recs["len"].sum())
    assert 8 * e["seq"].size < 256 * 12 + 64 + n // 64 and 8 * e["qual"].size < 8192 * 12 + 64 + n // 64


# ---------------------------------------------------------------- the packer's widest case
RARE_BASE, RARE_QUAL = 3, 20  # T, Phred 20


@pytest.fixture(scope="module")
def wide_tables():
    """Tables of log 12 in which every symbol has count 1 except symbol 0, which takes the rest of 2^12: a rare symbol
    costs 12 bits, 96 per thread and packing round."""
    raw, recs = _block([READ] * 8, seed=3)
    _, _, sft, qft = O.freq_tables(raw, recs)
    sft, qft = sft.copy(), qft.copy()
    for ft, alpha in ((sft, 4), (qft, 64)):
        ft["norm"][0][:, :] = 1
        ft["norm"][0][:, 0] = 4096 - (alpha - 1)
        ft["logs"][0][:] = 12
        ft["max_log"][0] = 12
    return sft, qft


def _wide_block(random_half):
    n_reads = 260
    rng = np.random.default_rng(12)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = np.full((n_reads, READ), letters[RARE_BASE], dtype=np.uint8)
    quals = np.full((n_reads, READ), RARE_QUAL, dtype=np.uint8)
    if random_half:
        pick = rng.random((n_reads, READ)) < 0.5
        seqs[pick] = letters[rng.integers(0, 4, size=int(pick.sum()))]
        pick = rng.random((n_reads, READ)) < 0.5
        quals[pick] = rng.integers(2, 42, size=int(pick.sum())).astype(np.uint8)
    return _fastq(list(seqs), list(quals))


@pytest.fixture(scope="module")
def wide(F, wide_tables):
    sft, qft = wide_tables
    ctx, octx = F.Context(sft, qft), O.OracleCtx(sft, qft)
    yield ctx, octx
    ctx.close()
    octx.close()


@pytest.mark.parametrize("random_half", [False, True], ids=["all_rare", "half_random"])
def test_twelve_bits_per_symbol(F, wide, random_half):
    """12 bits per symbol overflow the plain capacity rule (both coders say so); with room the streams are the oracle's.
    Oracle figures: 12.09 bits per base and 14.95 per quality (8 192 x 12 bits of state flush included) with every symbol
    rare, 10.61 / 14.95 with half of them drawn at random."""
    ctx, octx = wide
    raw, recs = _wide_block(random_half)
    n = int(recs["len"].sum())
    assert n == 260 * READ
    assert octx.encode(raw, recs)["rc"] == -1
    assert ctx.encode_block(raw, recs)["rc"] == -1
    cap = 2 * n + 4096
    e = _same_streams_and_back(F, ctx, octx, raw, recs, seq_cap=cap, qual_cap=cap)
    bits_seq, bits_qual = 8 * e["seq"].size / n, 8 * e["qual"].size / n
    print("bits per base %.2f, per quality %.2f" % (bits_seq, bits_qual))
    assert abs(bits_seq - (10.61 if random_half else 12.09)) < 0.05 and abs(bits_qual - 14.95) < 0.05


def test_overflow_inside_a_tile(F, wide):
    """The quality stream of the all-rare block with a capacity one byte below its length: the words stop fitting in the
    middle of a tile's rounds, nothing is stored behind the buffer, both coders refuse."""
    ctx, octx = wide
    raw, recs = _wide_block(False)
    cap = 2 * int(recs["len"].sum()) + 4096
    qlen = octx.encode(raw, recs, seq_cap=cap, qual_cap=cap)["qual"].size
    assert octx.encode(raw, recs, seq_cap=cap, qual_cap=qlen - 1)["rc"] == -1
    assert ctx.encode_block(raw, recs, seq_cap=cap, qual_cap=qlen - 1)["rc"] == -1
    # and the handle is as good as before
    _same_streams_and_back(F, ctx, octx, raw, recs, seq_cap=cap, qual_cap=cap)
