"""K3 (k_tile_partition: stable sort of a tile by context inside LDS, the patch of the records' first symbols, the run list)
at the smallest shapes at which it can go wrong: every stream byte for byte against the CPU oracle, then back to the raw
block.  A tile is 32 768 symbols, a batch 4 096, a key piece 8; the kernel has 512 threads and prefetches one record start
per thread from the record K1 names for the tile (the one that holds the tile's first symbol)."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

TILE = 32768
BATCH = 4096
THREADS = 512


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
        else:
            quals.append(np.full(n, qual, dtype=np.uint8))
    raw, recs = _fastq(seqs, quals)
    assert int(recs["len"].sum()) == int(np.sum(lengths))
    return raw, recs


def _check(F, raw, recs):
    """tables from the block itself; five streams equal to the oracle's; decoded back to the raw block"""
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx, octx = F.Context(sft, qft), O.OracleCtx(sft, qft)
    try:
        e = octx.encode(raw, recs)
        g = ctx.encode_block(raw, recs)
        assert e["rc"] == 0 and g["rc"] == 0, (e["rc"], g["rc"])
        for k in ("seq", "qual", "readlens", "n_count", "n_pos"):
            assert np.array_equal(np.asarray(g[k]), np.asarray(e[k])), k
        rc, out = ctx.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs))
        assert rc == 0 and np.array_equal(out, raw)
    finally:
        ctx.close()
        octx.close()


def _starts_per_tile(lengths):
    starts = np.concatenate(([0], np.cumsum(lengths)[:-1]))
    return np.bincount(starts // TILE, minlength=(int(np.sum(lengths)) + TILE - 1) // TILE)


# ---------------------------------------------------------------- where the tile's first record is
@pytest.mark.parametrize("read", [128, 100], ids=["boundary_at_a_record_start", "boundary_inside_a_record"])
def test_tile_boundary_and_record_start(F, read):
    """Reads of 128: 256 per tile, every tile starts with a record -- the record that HOLDS the tile's first symbol is the
    one that STARTS there and must be patched.  Reads of 100: the tile's first symbol lies inside a record that started in
    the tile in front, which must not be patched a second time."""
    lengths = [read] * (2 * TILE // read + 40)
    starts = np.cumsum(lengths) - read
    assert bool(np.any(starts == TILE)) == (read == 128)
    _check(F, *_block(lengths, seed=read))


@pytest.mark.parametrize("read,qual,base", [(128, 40, None), (100, 40, None), (128, "normal", "A"), (100, "normal", "A"), (100, 40, "A")],
                         ids=["const_qual_128", "const_qual_100", "poly_a_128", "poly_a_100", "both_100"])
def test_combining_ranker_in_the_same_shapes(F, read, qual, base):
    """One quality everywhere / one base everywhere: one context holds the whole tile, so the stream's tiles take the
    combining ranker, which stores the positions and places the symbols itself."""
    _check(F, *_block([read] * (2 * TILE // read + 40), seed=read + 1, qual=qual, base=base))


# ---------------------------------------------------------------- no record start in a tile
def test_a_tile_without_any_record_start(F):
    """A read of 40 000 bases between short ones: it starts at symbol 30 000 and ends at 70 000, so NO record starts in
    tile 1 (symbols 32 768 .. 65 535)."""
    lengths = [100] * 300 + [40000] + [100] * 30
    assert list(_starts_per_tile(lengths)) == [301, 0, 30]
    _check(F, *_block(lengths, seed=40))


def test_a_block_that_is_one_read(F):
    lengths = [40000]
    assert list(_starts_per_tile(lengths)) == [1, 0]
    _check(F, *_block(lengths, seed=41))


# ---------------------------------------------------------------- more record starts in a tile than K3 has threads
@pytest.mark.parametrize("kind", ["3_to_40", "all_4", "all_3"])
def test_more_record_starts_than_threads(F, kind):
    """Reads of 3 .. 40 bases (about 1 500 starts per tile), of 4 (8 192 per tile, one of them on every tile boundary) and
    of 3 (10 923, the boundary inside a read): the starts behind the first 512 come from the remainder loop."""
    rng = np.random.default_rng(5)
    if kind == "3_to_40":
        lengths = list(rng.integers(3, 41, size=3 * TILE // 21))
    else:
        n = int(kind[-1])
        lengths = [n] * (2 * TILE // n + 700)
    per_tile = _starts_per_tile(lengths)
    assert per_tile[0] > 2 * THREADS and 1000 <= per_tile[:2].min() and per_tile.max() <= 11000
    _check(F, *_block(lengths, seed=6))


# ---------------------------------------------------------------- small tiles
@pytest.mark.parametrize("tail", [1, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH])
def test_small_last_tile(F, tail):
    """A full tile and a last tile of `tail` symbols: one batch or two, with the edges of a key piece (8 symbols) and of a
    batch.  The single symbol of the 1-symbol tile belongs to a read that starts in the tile in front."""
    if tail == 1:
        lengths = [128] * 255 + [129]
    else:
        lengths = [128] * (256 + tail // 128)
        lengths[-1] += tail % 128
    assert sum(lengths) == TILE + tail
    _check(F, *_block(lengths, seed=tail))


def test_a_block_smaller_than_one_batch(F):
    _check(F, *_block([100] * 7, seed=9))


# ---------------------------------------------------------------- K3's second caller
def test_quality_table_sampling_counts(F):
    """From 2^20 symbols up the quality counts of the dataset analysis come from K1 + K3 + a histogram of the sorted runs
    (fq_qual_counts_sorted): equal to the host's histogram, count for count."""
    rng = np.random.default_rng(20)
    lengths = list(rng.integers(3, 151, size=15000))
    assert sum(lengths) >= 1 << 20
    raw, recs = _block(lengths, seed=21)
    sc, qc, sft, qft = O.freq_tables(raw, recs)
    gs, gq, gsc, gqc = F.freq_tables(raw, recs, want_counts=True)
    assert np.array_equal(gqc, qc) and np.array_equal(gsc, sc)
    assert gs.tobytes() == sft.tobytes() and gq.tobytes() == qft.tobytes()
