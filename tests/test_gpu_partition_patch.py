"""K3 (k_tile_partition): the patch of the records' first symbols at the positions where it can go wrong, and the output loop,
where pieces of the sorted tile with a run boundary inside are stored by the whole wave: every stream byte for byte against the
CPU oracle, then back to the raw block.  A tile is 32 768 symbols, a batch 4 096, a key piece 8, an output piece 16; the
kernel has 512 threads and prefetches one record start per thread; a tile with more starts than that patches the rest in a
loop.  Blocks are one to three tiles.
(The format has no reads shorter than three bases -- the oracle refuses them --, so "several starts in one piece" is reads of
3 .. 7 bases, and the record starts one symbol apart around a batch's edge come from three blocks, not one.)"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

TILE = 32768
BATCH = 4096
THREADS = 512
GD_CAP = 4608  # runs whose offsets K3 keeps in LDS; later runs are read back from the run list
RUNS_PAIRS = 7790  # contexts in the "every pair" block below


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


def _block(lengths, seed, phred=None):
    """random bases; qualities normal around 30, or uniform over phred = (lo, hi)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs, quals = [], []
    for n in lengths:
        seqs.append(letters[rng.integers(0, 4, size=n)])
        if phred is None:
            quals.append(np.clip(np.rint(rng.normal(30, 6, size=n)), 2, 41).astype(np.uint8))
        else:
            quals.append(rng.integers(phred[0], phred[1] + 1, size=n).astype(np.uint8))
    raw, recs = _fastq(seqs, quals)
    assert int(recs["len"].sum()) == int(np.sum(lengths))
    return raw, recs, quals


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


def _starts(lengths):
    return np.concatenate(([0], np.cumsum(lengths)[:-1]))


def _starts_per_tile(lengths):
    return np.bincount(_starts(lengths) // TILE, minlength=(int(np.sum(lengths)) + TILE - 1) // TILE)


def _lengths_with_starts_at(wanted, total):
    """reads of about 100 bases, cut so that a record starts at every index in `wanted`"""
    marks = sorted(set([0] + list(wanted) + [total]))
    starts = []
    for a, b in zip(marks, marks[1:]):
        starts.append(a)
        while b - starts[-1] > 160:
            starts.append(starts[-1] + 100)
    lengths = list(np.diff(starts + [total]))
    assert min(lengths) >= 3 and set(wanted) <= set(_starts(lengths))
    return lengths


# ---------------------------------------------------------------- where in a piece and a batch the corrected byte lies
def test_record_starts_on_every_position_of_a_key_piece(F):
    """Reads of 100 .. 107 bases in turn: the starts walk through all eight positions of a key piece, in every batch of two
    tiles, and every tile has fewer starts than threads."""
    lengths = [100 + (i % 8) for i in range(420)]
    st = _starts(lengths)
    for b in range(int(np.sum(lengths)) // BATCH):
        assert set(st[st // BATCH == b] % 8) == set(range(8)), b
    assert len(_starts_per_tile(lengths)) == 2 and _starts_per_tile(lengths).max() < THREADS - 1
    _check(F, *_block(lengths, seed=1)[:2])


@pytest.mark.parametrize("wanted", [(BATCH - 1, TILE - 1), (BATCH, TILE), (BATCH + 1,)],
                         ids=["last_of_batch_and_tile", "first_of_batch_and_next_tile", "second_of_batch"])
def test_record_starts_at_batch_and_tile_edges(F, wanted):
    """A record starts at local index 0 and at 4 095 and 32 767 / at 4 096 and index 0 of the next tile / at 4 097."""
    lengths = _lengths_with_starts_at(wanted, TILE + 3000)
    assert _starts_per_tile(lengths).max() < THREADS - 1
    _check(F, *_block(lengths, seed=2 + len(wanted) + wanted[0])[:2])


@pytest.mark.parametrize("n_short", [300, 600], ids=["fewer_than_threads", "more_than_threads_in_tile_0"])
def test_several_record_starts_in_one_piece(F, n_short):
    """Reads of 3 .. 7 bases: up to three starts in one key piece.  300 of them and long reads behind: every start of the
    tile is one thread's.  600 of them: tile 0 has more starts than threads (the remainder loop), tile 1 (long reads only)
    has not."""
    rng = np.random.default_rng(30 + n_short)
    lengths = list(rng.integers(3, 8, size=n_short)) + [2000] * 20
    per_tile = _starts_per_tile(lengths)
    st = _starts(lengths)
    assert np.bincount(st[:n_short] // 8).max() >= 2 and len(per_tile) == 2
    assert (per_tile[0] > THREADS) == (n_short == 600) and per_tile[1] < 20
    _check(F, *_block(lengths, seed=31)[:2])


# ---------------------------------------------------------------- the combining ranker: a missed patch must show
@pytest.mark.parametrize("read", [100, 128])
def test_combining_ranker_patches_each_first_symbol_once(F, read):
    """Reads that are C + A x (n - 1) with qualities 12 + 40 x (n - 1): one context holds nearly the whole tile, so both
    streams' tiles take the combining ranker -- and the first symbol of every record differs from what its neighbour's
    context says, so a missed or a doubled patch changes both streams (all-A reads cannot show it)."""
    n_reads = 2 * TILE // read + 40
    seqs = [np.frombuffer(b"C" + b"A" * (read - 1), dtype=np.uint8)] * n_reads
    quals = [np.array([12] + [40] * (read - 1), dtype=np.uint8)] * n_reads
    _check(F, *_fastq(seqs, quals))


# ---------------------------------------------------------------- the output: run boundaries inside a 16-byte piece
@pytest.fixture(scope="module")
def one_tile_reads():
    rng = np.random.default_rng(50)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = [letters[rng.integers(0, 4, size=100)] for _ in range(200)]
    quals = [np.clip(np.rint(rng.normal(30, 6, size=100)), 2, 41).astype(np.uint8) for _ in range(200)]
    return seqs, quals


@pytest.mark.parametrize("shift", range(16))
def test_sequence_run_boundaries_on_every_offset_of_a_piece(F, one_tile_reads, shift):
    """One tile of 20 000 symbols whose sequence runs (about 78 symbols per context) all move by `shift` positions: a read of
    `shift` + 3 bases in front whose symbols all fall into the first contexts (AAAA and the record's first three).  Over the
    sixteen variants every boundary of the tile falls on every offset of a 16-byte piece, and the last piece is short."""
    seqs, quals = one_tile_reads
    n = shift + 3
    seqs = [np.full(n, ord("A"), dtype=np.uint8)] + list(seqs)
    quals = [np.full(n, 30, dtype=np.uint8)] + list(quals)
    _check(F, *_fastq(seqs, quals))


def _qual_contexts(quals):
    """context of every quality symbol of the block (the codec's calcContext: the three qualities in front, 0 before the read)"""
    out = []
    for q in quals:
        q = np.asarray(q, dtype=np.int64)
        p1, p2, p3 = (np.concatenate((np.zeros(k, dtype=np.int64), q[:-k])) for k in (1, 2, 3))
        out.append((((np.maximum(p2, p3) << 6) + p1) & 0xFFF) + ((p2 == p3).astype(np.int64) << 12))
    return np.concatenate(out)


@pytest.mark.parametrize("tail,phred,runs", [(1, (2, 41), 2210), (15, (2, 41), 2203), (7, "pairs", RUNS_PAIRS)],
                         ids=["phred_2_41_tail_1", "phred_2_41_tail_15", "every_pair_beyond_lds"])
def test_many_short_quality_runs_and_a_short_last_piece(F, tail, phred, runs):
    """ONE tile of 16 k + tail symbols.  Uniform random Phred 2 .. 41 (seeds 61 and 75): 2 210 / 2 203 contexts occur in the
    tile (counted here with the codec's context function: the tile's run count), fifteen symbols per run, so most 16-byte
    pieces hold boundaries, several of them, and with tail = 15 so does the short last piece (nine runs in it).  No tile of
    such data reaches what K3 keeps in LDS (4 608 runs; uniform Phred 0 .. 63 gives 4 352), so a third block is made to:
    the triple a, a, b for every pair of qualities 0 .. 63 -- every "equal neighbours" context once -- and uniform 0 .. 63
    behind; the runs beyond the 4 608th take their offsets from the run list in global memory."""
    n_sym = TILE - 16 + tail
    lengths = [128] * (n_sym // 128) + [n_sym % 128]
    raw, recs, quals = _block(lengths, seed=60 + tail, phred=(0, 63) if phred == "pairs" else phred)
    if phred == "pairs":
        rng = np.random.default_rng(7)
        flat = np.concatenate(quals)
        ab = rng.permutation(64 * 64)
        flat[:3 * ab.size] = np.stack((ab >> 6, ab >> 6, ab & 63), axis=1).reshape(-1)
        quals = np.split(flat, np.cumsum(lengths)[:-1])
        seqs = [raw[r["seq_off"]:r["seq_off"] + r["len"]] for r in recs]
        raw, recs = _fastq(seqs, quals)
    ctx = np.sort(_qual_contexts(quals))
    assert ctx.size == n_sym and n_sym % 16 == tail
    _, qc, _, _ = O.freq_tables(raw, recs)  # the oracle's histogram (every count starts at 1): the contexts that occur
    assert int((qc.sum(axis=1) > qc.shape[1]).sum()) == runs
    assert np.array_equal(np.unique(ctx), np.flatnonzero(qc.sum(axis=1) > qc.shape[1]))  # and the context function below is the codec's
    assert (runs > GD_CAP) == (phred == "pairs")
    assert tail == 1 or np.unique(ctx[n_sym - tail:]).size >= 2  # boundaries inside the short last piece
    _check(F, raw, recs)
