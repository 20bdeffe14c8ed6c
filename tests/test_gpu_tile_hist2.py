"""K1 (k_tile_hist2: keys, tile histograms, records' first symbols and N counts of both streams, four consecutive encode
indices of one read per lane) at the smallest shapes at which it can go wrong: every stream byte for byte against the CPU
oracle, then back to the raw block.  A tile is 32 768 symbols, a wave's range 8 192, a chunk 64 quads, a record window 64
records; a read's last quad is short unless its length is a multiple of four, and a quad at the edge of a wave's range
belongs to two waves."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

TILE = 32768
WAVE = 8192
E_ARG = -4
LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def _fastq(seqs, quals):
    """one record per (letters, Phred values) pair of uint8 arrays"""
    parts = []
    for i, (s, q) in enumerate(zip(seqs, quals)):
        parts.append(b"@r%d\n" % i + bytes(s) + b"\n+\n" + bytes((np.asarray(q) + 33).astype(np.uint8)) + b"\n")
    raw = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    recs = O.parse_fastq(raw)
    assert [int(n) for n in recs["len"]] == [len(s) for s in seqs]
    return raw, recs


def _reads(lengths, seed, qual="normal", base=None):
    rng = np.random.default_rng(seed)
    seqs, quals = [], []
    for n in lengths:
        seqs.append(LETTERS[rng.integers(0, 4, size=n)] if base is None else np.full(n, ord(base), dtype=np.uint8))
        if qual == "normal":
            quals.append(np.clip(np.rint(rng.normal(30, 6, size=n)), 2, 41).astype(np.uint8))
        else:
            quals.append(np.full(n, qual, dtype=np.uint8))
    return seqs, quals


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
    return e


def _fill(lengths, total):
    """`lengths` cycled until the block holds `total` symbols or a little more"""
    out, s, i = [], 0, 0
    while s < total:
        out.append(lengths[i % len(lengths)])
        s += out[-1]
        i += 1
    return out


# ---------------------------------------------------------------- read lengths
def test_every_length_from_3_to_40(F):
    """Every residue mod 4 (and mod 8), reads shorter than a window's context bytes, about 380 records per wave range."""
    lengths = _fill(list(range(3, 41)), 2 * TILE + 5000)
    assert WAVE // 40 > 64 and 2 * TILE < sum(lengths) < 3 * TILE
    _check(F, *_fastq(*_reads(lengths, seed=1)))


@pytest.mark.parametrize("n", [3, 7, 8, 9, 15, 16, 17, 150, 151])
def test_uniform_length(F, n):
    lengths = _fill([n], 2 * TILE + 3001)
    assert sum(lengths) % TILE != 0
    _check(F, *_fastq(*_reads(lengths, seed=10 + n)))


@pytest.mark.parametrize("k", range(8))
def test_boundaries_on_every_offset_of_a_group(F, k):
    """Reads of 150 behind one of 150 + k: the wave ranges and tiles cut the quads at every offset; the last tile is partial."""
    lengths = [150 + k] + [150] * ((2 * TILE + 9000) // 150)
    assert 2 * TILE < sum(lengths) < 3 * TILE and sum(lengths) % TILE != 0
    _check(F, *_fastq(*_reads(lengths, seed=30 + k)))


@pytest.mark.parametrize("long", [WAVE + 1001, TILE + 2003, 65535], ids=["over_a_wave_range", "over_a_tile", "longest"])
def test_long_reads(F, long):
    """One record fills whole windows of 64 records and whole chunks: short reads in front of it and behind it."""
    lengths = [100] * 37 + [long] + _fill([101, 7, 150], 2 * TILE + 500 - long if long < 2 * TILE else 3000)
    assert 2 * TILE < sum(lengths) < 3 * TILE + 4000
    _check(F, *_fastq(*_reads(lengths, seed=long)))


# ---------------------------------------------------------------- Ns
def test_ns(F):
    """An N at each of the eight offsets of a group from the read's end (encode order runs backwards) and from its start,
    as first and as last base, a run across group boundaries, an all-N read; reads of several lengths in between, so that
    the Ns meet full quads, short quads and quads cut by a wave's range.  n_count and n_pos are compared."""
    lengths = _fill([150, 151, 37, 150, 12, 150, 150, 9], 2 * TILE + 4000)
    seqs, quals = _reads(lengths, seed=50)
    want = 0
    for r, s in enumerate(seqs):
        n = len(s)
        kind = r % 23
        if kind < 8:
            pos = [n - 1 - kind]          # offset `kind` of the read's first group in encode order
        elif kind < 16:
            pos = [kind - 8]              # ... of its last one
        elif kind == 16:
            pos = [0, n - 1]
        elif kind == 17:
            pos = list(range(max(0, n - 13), n - 2))   # a run across a group boundary (two for quads)
        elif kind == 18:
            pos = list(range(n))          # all N
        elif kind == 19:
            pos = list(range(1, min(n, 10)))
        else:
            pos = []
        pos = sorted({p for p in pos if 0 <= p < n})
        if pos:
            s[pos] = ord("N")
        want += len(pos)
    raw, recs = _fastq(seqs, quals)
    e = _check(F, raw, recs)
    assert int(e["n_count"].sum()) == want and want > 1000


def test_ns_one_per_cent(F):
    lengths = _fill([150], 2 * TILE + 700)
    seqs, quals = _reads(lengths, seed=51)
    rng = np.random.default_rng(52)
    for s in seqs:
        s[rng.random(len(s)) < 0.01] = ord("N")
    _check(F, *_fastq(seqs, quals))


# ---------------------------------------------------------------- one bin takes a whole tile
@pytest.mark.parametrize("qual,base", [(40, None), ("normal", "A"), (0, "A")], ids=["constant_quality", "poly_a", "both"])
def test_one_bin_takes_a_tile(F, qual, base):
    """32 768 counts in one 16-bit entry of the packed rows (the quality stream's) / in one word of the sequence stream's."""
    lengths = _fill([150], 2 * TILE + 1500)
    _check(F, *_fastq(*_reads(lengths, seed=60, qual=qual, base=base)))


# ---------------------------------------------------------------- refusals
@pytest.fixture(scope="module")
def clean(F):
    """one clean block, its tables, one handle of each coder and the oracle's streams: shared by the refusals"""
    lengths = _fill([150, 149, 38], 2 * TILE + 2000)
    raw, recs = _fastq(*_reads(lengths, seed=70))
    assert [int(recs["len"][r]) for r in (300, 301, 302)] == [150, 149, 38]
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx, octx = F.Context(sft, qft), O.OracleCtx(sft, qft)
    want = octx.encode(raw, recs)
    assert want["rc"] == 0
    yield raw, recs, ctx, octx, want
    ctx.close()
    octx.close()


def _refused(clean, off, rec, pos, byte):
    raw, recs, ctx, octx, want = clean
    bad = raw.copy()
    bad[recs[off][rec] + pos] = byte
    e, g = octx.encode(bad, recs), ctx.encode_block(bad, recs)
    assert e["rc"] == E_ARG and g["rc"] == e["rc"], (e["rc"], g["rc"])
    g = ctx.encode_block(raw, recs)   # the handle is as good as new
    assert g["rc"] == 0, g["rc"]
    for k in ("seq", "qual", "readlens", "n_count", "n_pos"):
        assert np.array_equal(np.asarray(g[k]), np.asarray(want[k])), k


# The spoilt byte: read 300 has 150 bases (positions 149 .. 2 lie in full quads of the encode order, 1 and 0 in the short
# last one), read 301 has 149 (a tail of one), read 302 has 38; read 0 opens the block.
@pytest.mark.parametrize("rec,pos", [(300, 149), (300, 77), (300, 1), (300, 0), (301, 0), (302, 3), (0, 0)])
def test_a_byte_that_is_no_base(clean, rec, pos):
    _refused(clean, "seq_off", rec, pos, ord("X"))


@pytest.mark.parametrize("rec,pos", [(300, 149), (300, 1), (301, 0), (302, 3)])
@pytest.mark.parametrize("byte", [33 + 64, 255, 32, 0], ids=lambda b: "byte_%d" % b)
def test_a_quality_outside_the_alphabet(clean, rec, pos, byte):
    """At or above QualModel::A (64), and below 33, where the byte-parallel subtraction of 33 borrows from the byte above."""
    _refused(clean, "qual_off", rec, pos, byte)


def test_quality_63_is_the_last_one_coded(F):
    """Phred 63 right beside the limit must NOT be refused (the range test is exact)."""
    lengths = _fill([150, 149, 38], 2 * TILE + 2000)
    seqs, quals = _reads(lengths, seed=71)
    for r in (0, 300, 301, 302):
        quals[r][[0, 1, len(quals[r]) - 1]] = 63
    _check(F, *_fastq(seqs, quals))
