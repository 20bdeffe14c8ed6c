"""No result may depend on what a handle's scratch held before the call.  A handle's device scratch (the grow-only DevBufs
of its lanes, its decode, parser, header, chunk, checksum, summary and selection scratch, the staging block of the
host-pointer calls) is never cleared between calls: a worker that keeps one handle for hours pushes unlike chunks through
the same buffers, large then small, one kind then another.  Two ways to meet what a fresh handle per test never meets:

  history  unlike blocks one after another through ONE lane's scratch, settings changing in between
  fill     Context.fill_scratch(byte) sets every scratch byte that is not state on purpose before the call under test, so
           that "right by luck of what the buffer held" becomes wrong for sure

Every comparison is byte equality with a reference the suite already trusts: the CPU oracle for the five streams, the
block's own bytes for decodes, headers_oracle, zlib.crc32 and the Python references of the chunk services.  The history
tests come first in the file, then every fill test with 0x00, then with the other bytes (the `byte` fixture is module-scoped).
"""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import pytest

import adapter_ref as AR
import filter_ref as FR
import oracle_lib as O
import probe_ref as PR
import stats_ref as SR
import tail_ref as TR
import test_gpu_build_index as TB
import test_gpu_decode_chunk as TD
import test_gpu_headers as TH
import test_gpu_partition_edges as PE
import test_gpu_probe as TP
import test_gpu_stats as TS
import test_gpu_tail as TG
import trim_ref as R
from seq_blocks import block

pytestmark = pytest.mark.gpu

STREAMS = ("seq", "qual", "readlens", "n_count", "n_pos")
SEGMENT = 1024   # seq_segment throughout: chains of many segments at small sizes
STRIDE = 65536   # decode index: a snapshot per partition tile pair, so that blocks of 2 MiB have a dozen
E_ARG = -4

# the bytes of the fill tests, and the sentinel each one turns against the code
FILL = [
    pytest.param(0x00, id="00"),  # a cand0 head nobody wrote reads "handed over, candidate 0"; look-back flags read "not ready";
                                  # first_error / bad read "record 0"; stream words that are OR-ed into start clean (the lucky case)
    pytest.param(0xFF, id="FF"),  # a cand0 head nobody wrote reads SEQ_CAND_KEPT; first_error = ~0 reads "no error"; look-back
                                  # words read "inclusive total, ready"; stream words that are OR-ed into are all ones
    pytest.param(0xA5, id="A5"),  # neither sentinel: a "handed over" head whose candidates are no states, look-back flag 2
                                  # ("inclusive") with a wrong total, counters and OR-ed words that start from rubbish
]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module", params=FILL)
def byte(request):
    return request.param


# ---------------------------------------------------------------- blocks, and the oracle's encoding of each, computed once
@functools.lru_cache(maxsize=None)
def blk(name):
    """-> (raw, recs) of a named block; the kinds of seq_blocks as "kind:bytes", the K3 edge shapes by name"""
    if name == "one_read":
        b = PE._block([40000], seed=41)
    elif name == "sub_batch":                      # smaller than one batch of K3
        b = PE._block([100] * 7, seed=9)
        assert int(b[1]["len"].sum()) < PE.BATCH
    elif name == "tile_plus_1":                    # one partition tile plus one symbol
        b = PE._block([128] * 255 + [129], seed=1)
        assert int(b[1]["len"].sum()) == PE.TILE + 1
    else:
        kind, size = name.split(":")
        b = block(kind, int(size))[:2]
    for a in b:
        a.setflags(write=False)
    return b


L = "mixed:%d" % (6 << 20)   # the large block: half the reads all A, half uniform


@functools.lru_cache(maxsize=None)
def tables(name):
    _, _, sft, qft = O.freq_tables(*blk(name))
    return sft, qft


@functools.lru_cache(maxsize=None)
def oracle(name, tables_of):
    """the oracle's encoding of block `name` under the tables of block `tables_of`"""
    o = O.OracleCtx(*tables(tables_of))
    want = o.encode(*blk(name))
    o.close()
    assert want["rc"] == 0, (name, tables_of, want["rc"])
    return want


def context(F, tables_of, lanes=1):
    ctx = F.Context(*tables(tables_of))
    ctx.set_chain_params(0, seq_segment=SEGMENT)
    ctx.set_index_stride(STRIDE)
    ctx.set_lanes(lanes)
    return ctx


def same_streams(got, want, what):
    for k in STREAMS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k)


def encode(F, ctx, name, flags=0):
    """one device-resident encode of a block on this handle -> (streams, (handed, kept), (seq index, qual index))"""
    b = ctx.dblock(*blk(name))
    try:
        b.encode(flags)
        ctx.sync()
        assert b.status()[0] == 0, name
        return b.fetch(), b.seq_handover(), (b.fetch_index(0), b.fetch_index(1))
    finally:
        b.close()


def filled(ctx, byte, n_sym):
    """fills the handle's scratch; n_sym: the symbols of the largest block it has coded.  Per symbol and stream encode_stream
    reserves (encode.hip) slot_of 2 (the tile path's u16 positions; 4 on the slot path), keys 3, sorted_sym 1, out16 2."""
    buffers, n_bytes = ctx.fill_scratch(byte)
    assert buffers > 0
    assert n_bytes >= 2 * (2 + 3 + 1 + 2) * n_sym, (buffers, n_bytes, n_sym)
    return buffers, n_bytes


def n_sym(name):
    return int(blk(name)[1]["len"].sum())


# ================================================================ history
SMALL = ["markov:%d" % (300 << 10), "one_read", "sub_batch", "tile_plus_1"]


def test_large_then_small_then_large(F):
    """L, a small block, L again, the next small block ...: every encode in the scratch the one before left"""
    ctx = context(F, L)
    try:
        for small in SMALL:
            for name in (L, small):
                same_streams(encode(F, ctx, name)[0], oracle(name, L), name)
        same_streams(encode(F, ctx, L)[0], oracle(L, L), "L at the end")
    finally:
        ctx.close()


TWO = "two_letters:%d" % (6 << 20)
# (block, hand-over (cap, prefix), group (segments, min groups)): the layout of seq_cand (cand0 | cand at seq_max_segs * W,
# W = 16 / 32 / 64 by cap) changes with every step.  A prefix of 4 in groups of 2 can hand nothing over: every group is kept.
# The two blocks of 2 MiB move the other term of that offset, the segment count.
TWO_S, MIXED_S = "two_letters:%d" % (2 << 20), "mixed:%d" % (2 << 20)
LAYOUTS = [(L, (64, 1), (8, 1)), (TWO, (16, 4), (2, 1)), (L, (32, 2), (16, 4)), (TWO_S, (32, 2), (8, 1)), (MIXED_S, (64, 1), (2, 1)),
           (TWO, (0, 1), (8, 1)), (L, (32, 1), (2, 1)), (TWO, (64, 1), (2, 1)), (L, (16, 4), (16, 4)), (TWO, (32, 1), (2, 1)),
           (L, (64, 1), (8, 1))]


def test_handover_layouts_changing_on_one_handle(F):
    """the tables are the two-letter block's: both blocks stay inside their capacity rule under them"""
    ctx = context(F, TWO)
    counts = []
    try:
        for name, handover, group in LAYOUTS:
            what = (name, handover, group)
            ctx.set_chain_params(0, seq_segment=SEGMENT, seq_group=group)
            ctx.set_seq_handover(*handover)
            got, hk, _ = encode(F, ctx, name)
            same_streams(got, oracle(name, TWO), what)
            fresh = context(F, TWO)
            fresh.set_chain_params(0, seq_segment=SEGMENT, seq_group=group)
            fresh.set_seq_handover(*handover)
            fgot, fhk, _ = encode(F, fresh, name)
            fresh.close()
            same_streams(fgot, oracle(name, TWO), ("fresh",) + what)
            assert hk == fhk, (what, hk, fhk)
            if handover[0] == 0:
                assert hk == (0, 0), what
            counts.append(hk)
    finally:
        ctx.close()
    print("handed over, kept:", counts)
    assert any(h > 0 for h, _ in counts) and any(k > 0 for _, k in counts), counts


# (block, seq_generic, segment of the generic chain kernels, decode index): seq_fbuf and seg_arrays change hands
SHARED = [(L, True, 1024, True), ("all_A:%d" % (2 << 20), False, 2048, False), ("markov:%d" % (300 << 10), True, 4096, True),
          ("mostly_A:%d" % (2 << 20), False, 1024, True), ("mixed:%d" % (2 << 20), True, 2048, False), ("one_read", False, 4096, True),
          (L, False, 2048, True)]


def test_buffers_shared_by_the_serial_and_the_generic_chains(F):
    ctx = context(F, L)
    try:
        for name, generic, segment, index in SHARED:
            what = (name, generic, segment, index)
            flags = F.F_DECODE_INDEX if index else 0
            ctx.set_chain_params(segment, seq_generic=generic, seq_segment=SEGMENT)
            raw, recs = blk(name)
            b = ctx.dblock(raw, recs)
            b.encode(flags)
            ctx.sync()
            assert b.status()[0] == 0, what
            same_streams(b.fetch(), oracle(name, L), what)
            got_index = (b.fetch_index(0), b.fetch_index(1))
            fresh = context(F, L)
            fresh.set_chain_params(segment, seq_generic=generic, seq_segment=SEGMENT)
            _, _, want_index = encode(F, fresh, name, flags)
            fresh.close()
            assert [len(x) > 0 for x in want_index] == [index, index], what
            TB.same_index(got_index, want_index, str(what))
            b.wipe()
            ctx.decode_dblocks([b])   # through the index where the encode left one
            assert b.status()[0] == 0, what
            assert np.array_equal(b.fetch_raw(), raw), what
            b.close()
    finally:
        ctx.close()


LANES = [L, "mostly_A:%d" % (2 << 20), "markov:%d" % (300 << 10), "sub_batch", "one_read", "all_A:%d" % (2 << 20), L]


def test_three_lanes_seven_blocks_no_sync_in_between(F):
    """sizes going down, then up: blocks 0, 3, 6 / 1, 4 / 2, 5 share a lane each"""
    ctx = context(F, L, lanes=3)
    blocks = [ctx.dblock(*blk(name)) for name in LANES]
    try:
        for b in blocks:
            b.encode()
        ctx.sync()
        got = []
        for b, name in zip(blocks, LANES):
            assert b.status()[0] == 0, name
            got.append(b.fetch())
        for b in blocks:
            b.wipe()
        ctx.decode_dblocks(blocks)
        for b, name, g in zip(blocks, LANES, got):
            same_streams(g, oracle(name, L), name)
            assert b.status()[0] == 0, name
            assert np.array_equal(b.fetch_raw(), blk(name)[0]), name
    finally:
        for b in blocks:
            b.close()
        ctx.close()


# ================================================================ fill
def test_fill_is_refused_while_a_block_is_pending_and_drops_the_staged_chunk(F, byte):
    """the hook's own rules: FQGPU_E_ARG between fqgpu_encode_begin and _end; afterwards the staging block holds no chunk"""
    ctx = context(F, L)
    raw, recs = blk("one_read")
    try:
        assert ctx.fill_scratch(byte) == (0, 0)   # a handle that has done nothing owns no scratch
        raw = np.array(raw)
        n, nb, used = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        lib = F.lib()
        assert lib.fqgpu_encode_begin(ctx.h, raw.ctypes.data, raw.size, None, 0, 0, C.byref(n), C.byref(nb), C.byref(used)) == 0
        assert lib.fqgpu_ctx_fill_scratch(ctx.h, byte, None, None) == E_ARG
        assert lib.fqgpu_encode_cancel(ctx.h) == 0
        g = ctx.encode_raw(raw)
        assert g["rc"] == 0 and ctx.chunk_crc32()[0] == 0
        filled(ctx, byte, n_sym("one_read"))
        assert ctx.chunk_crc32()[0] == E_ARG and ctx.chunk_stats(64)[0] == E_ARG
        same_streams(ctx.encode_raw(raw), oracle("one_read", L), "behind the fill")
    finally:
        ctx.close()


@pytest.mark.parametrize("handover", [None, (64, 1)], ids=["default", "cap64_p1"])
@pytest.mark.parametrize("kind", ["uniform", "mixed", "all_A", "two_letters"])
def test_resident_encode_in_filled_scratch(F, byte, kind, handover):
    """a 6 MiB block sizes and uses the lane; then the 2 MiB block of the same kind is coded once, the scratch is filled, the
    block's own stream buffers are loaded with 0xFF of the lengths they held, and the block is coded again"""
    big, name = "%s:%d" % (kind, 6 << 20), "%s:%d" % (kind, 2 << 20)
    ctx = context(F, big)
    if handover:
        ctx.set_seq_handover(*handover)
    b = ctx.dblock(*blk(name))
    try:
        same_streams(encode(F, ctx, big)[0], oracle(big, big), big)
        b.encode()
        ctx.sync()
        first = b.fetch()
        same_streams(first, oracle(name, big), "before the fill")
        filled(ctx, byte, n_sym(big))
        b.load_streams(np.full(first["seq"].size, 0xFF, np.uint8), np.full(first["qual"].size, 0xFF, np.uint8),
                       np.full(first["n_count"].size, 0xFFFF, np.uint16), np.full(first["n_pos"].size, 0xFFFF, np.uint16))
        b.encode(F.F_DECODE_INDEX)
        ctx.sync()
        assert b.status()[0] == 0
        same_streams(b.fetch(), oracle(name, big), "behind the fill")
        fresh = context(F, big)
        if handover:
            fresh.set_seq_handover(*handover)
        _, hk, want_index = encode(F, fresh, name, F.F_DECODE_INDEX)
        fresh.close()
        assert b.seq_handover() == hk
        assert all(len(x) > TB.IX_HEAD for x in want_index)
        TB.same_index((b.fetch_index(0), b.fetch_index(1)), want_index, "behind the fill")
    finally:
        b.close()
        ctx.close()


DECODED = ["mostly_A:%d" % (2 << 20), "markov:%d" % (300 << 10), "tile_plus_1"]


@functools.lru_cache(maxsize=None)
def encoder_index(name, tables_of):
    """the decode indexes a fresh handle's encode leaves for the block"""
    import fqcomp28_amd as F
    ctx = context(F, tables_of)
    try:
        return encode(F, ctx, name, F.F_DECODE_INDEX)[2]
    finally:
        ctx.close()


def loaded(ctx, name, tables_of, index):
    """a block that holds the skeleton and the oracle's streams, with the encoder's indexes or without"""
    raw, recs = blk(name)
    want = oracle(name, tables_of)
    b = ctx.dblock(O.blank_skeleton(raw, recs), recs)
    b.load_streams(want["seq"], want["qual"], want["n_count"], want["n_pos"])
    if index:
        for s, ix in enumerate(encoder_index(name, tables_of)):
            assert b.load_index(s, ix) == 0
    return b


@pytest.mark.parametrize("how", ["plain", "indexed", "indexing"])
def test_decode_in_filled_scratch(F, byte, how):
    """L is coded once (a handle that has only decoded owns no encode lane, and the fill's bound is the encoder's) and decoded
    (the same way); then three smaller blocks of different sizes in one call, behind the fill"""
    ctx = context(F, L)
    decode = ctx.decode_dblocks_indexing if how == "indexing" else ctx.decode_dblocks
    blocks = []
    try:
        same_streams(encode(F, ctx, L)[0], oracle(L, L), L)
        big = loaded(ctx, L, L, how == "indexed")
        blocks.append(big)
        decode([big])
        assert big.status()[0] == 0 and np.array_equal(big.fetch_raw(), blk(L)[0])
        filled(ctx, byte, n_sym(L))
        small = [loaded(ctx, name, L, how == "indexed") for name in DECODED]
        blocks += small
        decode(small)
        for b, name in zip(small, DECODED):
            assert b.status()[0] == 0, name
            assert np.array_equal(b.fetch_raw(), blk(name)[0]), name
            if how == "indexing":
                TB.same_index((b.fetch_index(0), b.fetch_index(1)), encoder_index(name, L), name)
    finally:
        for b in blocks:
            b.close()
        ctx.close()


def test_host_pointer_encode_and_decode_in_filled_scratch(F, byte):
    ctx = context(F, L)
    raw_l, recs_l = blk(L)
    try:
        same_streams(ctx.encode_block(raw_l, recs_l), oracle(L, L), "L")
        g = ctx.encode_raw(raw_l)
        assert g["rc"] == 0
        for name in ("markov:%d" % (300 << 10), "tile_plus_1", "sub_batch"):
            raw, recs = blk(name)
            want = oracle(name, L)
            filled(ctx, byte, n_sym(L))
            g = ctx.encode_block(raw, recs)
            assert g["rc"] == 0, name
            same_streams(g, want, (name, "encode_block"))
            filled(ctx, byte, n_sym(L))
            g = ctx.encode_raw(raw, flags=F.F_DECODE_INDEX)   # the device parser builds the record table
            assert g["rc"] == 0, name
            same_streams(g, want, (name, "encode_raw"))
            assert np.array_equal(g["recs"], O.parse_fastq(raw)), name
            assert g["used_len"] == raw.size
            TB.same_index(tuple(g["index"]), encoder_index(name, L), name)
            for index in (None, g["index"]):
                filled(ctx, byte, n_sym(L))
                rc, out = ctx.decode_block(want["seq"], want["qual"], want["n_count"], want["n_pos"], recs, O.blank_skeleton(raw, recs),
                                           index=index)
                assert rc == 0 and np.array_equal(out, raw), (name, index is not None)
    finally:
        ctx.close()


def test_header_fields_and_chunk_decode_in_filled_scratch(F, byte, golden_dir):
    """3 000 synthetic headers over the fixture's reads first, coded and decoded; then the golden fixture, fields against
    headers_oracle and the chunk through decode_chunk, each step behind a fill"""
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    ctx = F.Context(sft, qft)
    ctx.set_index_stride(STRIDE)
    try:
        big_hdrs = [b"@run%d.%d lane:%d:%d:%d length=100" % (i // 1000, i + 1, i % 8, 7 * i % 2000, 100000 - 3 * i) for i in range(3000)]
        big = TH.fastq_of(big_hdrs)
        assert big.size > 2 * raw.size
        big_sym = int(O.parse_fastq(big)["len"].sum())   # the encode lane is sized by this chunk
        g = TD.round_trip(F, ctx, big, big_hdrs[0], index=True)
        TH.assert_fields_equal(g, big_hdrs, big_hdrs[0])
        hdrs = TH.headers_of(raw, recs)
        for index in (False, True):
            filled(ctx, byte, big_sym)
            g = TD.encode(F, ctx, raw, hdrs[0], index)
            TH.assert_fields_equal(g, hdrs, hdrs[0])
            filled(ctx, byte, big_sym)
            d = TD.decode(ctx, g, hdrs[0])
            assert d["rc"] == 0 and d["bad_record"] is None, (d["rc"], d["bad_record"])
            assert d["laid_out_len"] == raw.size and np.array_equal(d["raw"], raw)
            assert np.array_equal(d["recs"], F.parse_fastq(raw))
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def service_chunks():
    """a chunk of 3 000 planted reads (poly-G tails, adapters, quality drops, N) and a small one of 257"""
    big, small = TG.planted(3000, 77), TG.planted(257, 78)
    return big, small


def test_chunk_services_small_chunk_after_large_chunk(F, byte):
    (big, big_recs), (raw, recs) = service_chunks()
    table = recs.astype(R.REC_DTYPE)
    ctx = TS.context_for(F, big, big_recs)   # (the tables of the large chunk: the small one stays inside its capacity rule)
    P = 128
    big_sym = int(big_recs["len"].sum())   # the encode lane is sized by the large chunk
    probes = PR.prb(TP.builtin_set() + [AR.adp(TG.ADAPTER, 5, 10)])
    a, x, t, f = AR.adp(TG.ADAPTER, 5, 10), TG.BOTH, R.trm(**TG.TT.Q20), FR.flt(max_n=0, min_len=20)
    try:
        # the large chunk through every service: the scratch of each is sized and used
        g = ctx.encode_raw(big, want_crc=True, want_stats=P, want_probes=(probes, P))
        assert g["rc"] == 0 and g["crc32"] == zlib.crc32(big.tobytes())
        TG.holds(ctx.chunk_tailtrim(len(big_recs), a, x, t, f), TR.tail_records(big, big_recs.astype(R.REC_DTYPE), a, x, t, f), "large")
        filled(ctx, byte, big_sym)
        g = ctx.encode_raw(raw, want_crc=True, want_stats=P, want_probes=(probes, P))
        assert g["rc"] == 0
        assert (g["crc32"], g["crc_len"]) == (zlib.crc32(raw.tobytes()), raw.size)
        TS.same(g["stats"], SR.stats_of(raw, table, P), "stats")
        TP.holds(dict(rc=0, out=g["probe"], places=g["probe_places"]), PR.probe_of(raw, table, probes, P), "probe")
        # each service alone behind a fill of its own (the chunk has to be staged again: the fill drops it)
        for service in ("crc", "stats", "select", "probe"):
            assert ctx.encode_raw(big)["rc"] == 0
            filled(ctx, byte, big_sym)
            assert ctx.encode_raw(raw)["rc"] == 0
            if service == "crc":
                assert ctx.chunk_crc32() == (0, zlib.crc32(raw.tobytes()), raw.size)
            elif service == "stats":
                rc, words = ctx.chunk_stats(P)
                assert rc == 0
                TS.same(words, SR.stats_of(raw, table, P), "stats alone")
            elif service == "select":   # adapter clip, poly-G, window, quality trim, filter
                want = TR.tail_records(raw, table, a, x, t, f)
                assert 0 < int(want[1][R.N_KEPT]) < len(recs)
                assert min(int(want[1][k]) for k in (AR.READS_WITH_ADAPTER, TR.READS_WITH_POLY, TR.READS_WINDOW_CUT)) > 10
                TG.holds(ctx.chunk_tailtrim(len(recs), a, x, t, f), want, "select")
            else:
                TP.holds(ctx.chunk_probe(probes, P, len(recs)), PR.probe_of(raw, table, probes, P), "probe alone")
    finally:
        ctx.close()


# ================================================================ the staging block's sizes
# (buffers, bytes) that fill_scratch(0xA5) returns after each step of test_staging_block_sizes_over_a_host_pointer_history,
# measured with FQGPU_LIB pointing at the library of the parent commit (fbea9db, before the block's buffers became typed
# arrays): the staging block allocates what it allocated, and the fill covers what it covered.
PARENT_PAIRS = [(56, 125979823), (58, 128121608), (74, 128131764), (75, 128137420), (75, 128137420)]


@functools.lru_cache(maxsize=None)
def hp_chunks():
    """-> (tables, small, large): the fixture's tables; a chunk of 4 of its reads; one of 400 records of 200 bases (two reads
    each: 80 000 symbols, a snapshot in either index at the smallest stride)"""
    raw, recs = O.load_fastq(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "SRR065390_sub_1.fastq"))
    _, _, sft, qft = O.freq_tables(raw, recs)
    b = raw.tobytes()
    line = lambda r, off: b[int(r[off]): int(r[off]) + int(r["len"])]
    small = TH.fastq_of([b"@run1.%d lane:%d length=100" % (i + 1, i % 8) for i in range(4)])
    large = b"".join(b"@run2.%d lane:%d length=200\n" % (i + 1, i % 8) + line(recs[2 * i], "seq_off") + line(recs[2 * i + 1], "seq_off") +
                     b"\n+\n" + line(recs[2 * i], "qual_off") + line(recs[2 * i + 1], "qual_off") + b"\n" for i in range(400))
    small.setflags(write=False)
    return (sft, qft), small, np.frombuffer(large, dtype=np.uint8)


def test_staging_block_sizes_over_a_host_pointer_history(F):
    """small encode, large encode with decode indexes, indexing decode of the small chunk, indexed decode of the large one, the
    small encode again, all through ONE staging block, a fill behind each: every output is the oracle's (the restored chunks
    their inputs, the built index a fresh handle's encoder's), and every fill visits the buffers and bytes the parent's visits"""
    tables, small, large = hp_chunks()
    first_small, first_large = b"@run1.1 lane:0 length=100", b"@run2.1 lane:0 length=200"
    octx = O.OracleCtx(*tables)
    want_small, want_large = (octx.encode(c, O.parse_fastq(c)) for c in (small, large))
    octx.close()
    fresh = F.Context(*tables)
    fresh.set_index_stride(STRIDE)
    small_index = TD.encode(F, fresh, small, first_small, True)["index"]
    fresh.close()
    ctx = F.Context(*tables)
    ctx.set_index_stride(STRIDE)
    pairs = []

    def encoded(chunk, first, want, index):
        g = TD.encode(F, ctx, chunk, first, index)
        assert want["rc"] == 0
        same_streams(g, want, ("encode", chunk.size))
        assert np.array_equal(g["recs"], O.parse_fastq(chunk)) and g["used_len"] == chunk.size
        pairs.append(ctx.fill_scratch(0xA5))
        return g

    try:
        g_small = encoded(small, first_small, want_small, False)
        g_large = encoded(large, first_large, want_large, True)
        assert all(TB.index_fields(ix, s)[1] == 1 for s, ix in enumerate(g_large["index"]))
        d = ctx.decode_chunk(TD.fmt_of(first_small), g_small["header_fields"], g_small["readlens"], g_small["seq"], g_small["qual"],
                             g_small["n_count"], g_small["n_pos"], small.size, build_index=True)
        assert d["rc"] == 0 and d["bad_record"] is None and np.array_equal(d["raw"], small)
        TB.same_index(d["index"], small_index, "built by the decode")
        pairs.append(ctx.fill_scratch(0xA5))
        recs = O.parse_fastq(large)
        w = want_large
        rc, out = ctx.decode_block(w["seq"], w["qual"], w["n_count"], w["n_pos"], recs, O.blank_skeleton(large, recs), index=g_large["index"])
        assert rc == 0 and np.array_equal(out, large)
        pairs.append(ctx.fill_scratch(0xA5))
        encoded(small, first_small, want_small, False)
    finally:
        ctx.close()
    print("fill_scratch pairs:", pairs)
    assert pairs == PARENT_PAIRS, pairs
