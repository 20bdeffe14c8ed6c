"""Dataset analysis and table construction on the device (fqcomp28_amd/csrc/tables.hip) against the plain reference of
tables_ref.py, which tests/test_tables_host.py holds against oracle/fse_oracle.c, libzstd and the reference's compiled
calculateFreqTable first.  Every comparison is an equality: of structs, of table words, of error codes, of streams.

  k_normalize<4>, <64>, normalize_m2   every count-vector family, each vector in a context of its own (T.packed_counts):
      ones, skew, zeros, wrap, log_edges, low_edge, rtb, tie, m2_edge, m2, m2_second_lowone, m2_total0; the refusals
      (RLE, empty, total above 2^32 - 1) in the first, a middle and the last context of either stream
  k_log_prefix, k_build_tables         CTable and DTable words of all 256 sequence contexts and of every quality context
      that holds a family vector: absent symbols, -1 symbols, log 5 (32 cells: half a step), both fast flags; tables
      whose logs alternate between 5 and 12
  fqgpu_ctx_create                     a table is accepted exactly when every log is in 5..12, every entry is -1 or more
      and the entries sum to 2^log with -1 counted as 1
  k_build_seq_next, _next2, _pow, k_reset_masks   through the streams: three sets of family tables code a two-letter
      block and a fixture, segments of 1024 and the default, hand-over on and off
  k_hist_seq, k_hist_qual, the switch to the encoder's sort   every read family of T.read_cases()"""
import os

import numpy as np
import pytest

import oracle_lib as O
import seq_blocks
import tables_ref as T

pytestmark = pytest.mark.gpu

E_ARG = -4
STREAMS = ("seq", "qual", "readlens", "n_count", "n_pos")
FT_DTYPE = {4: O.SEQ_FT_DTYPE, 64: O.QUAL_FT_DTYPE}


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


def oracle_ft(counts):
    """the oracle's FreqTable struct of a (models, alpha) count array"""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    alpha = counts.shape[1]
    ft = np.zeros(1, dtype=FT_DTYPE[alpha])
    make = O.lib().fqo_seq_ft_from_counts if alpha == 4 else O.lib().fqo_qual_ft_from_counts
    assert make(O.ptr(counts), O.ptr(ft)) == 0
    return ft


def oracle_tables(norm_row, log):
    """fo_build_ctable / fo_build_dtable of one context"""
    L = O.lib()
    norm_row = np.ascontiguousarray(norm_row, dtype=np.int16)
    ct = np.zeros(L.fo_ctable_words(log, len(norm_row) - 1), dtype=np.uint32)
    dt = np.zeros(L.fo_dtable_words(log), dtype=np.uint32)
    assert L.fo_build_ctable(O.ptr(ct), O.ptr(norm_row), len(norm_row) - 1, log) == 0
    assert L.fo_build_dtable(O.ptr(dt), O.ptr(norm_row), len(norm_row) - 1, log) == 0
    return ct, dt


def assert_tables(ctx, stream, ft, contexts):
    for m in contexts:
        ct, dt = ctx.dump_tables(stream, m)
        oc, od = oracle_tables(ft["norm"][0][m], int(ft["logs"][0][m]))
        assert np.array_equal(ct, oc), (stream, m, "CTable")
        assert np.array_equal(dt, od), (stream, m, "DTable")


@pytest.fixture(scope="module")
def packed(F):
    """the family counts of both streams, the oracle's structs of them and the device's"""
    sc, swhere = T.packed_counts(4)
    qc, qwhere = T.packed_counts(64)
    want = oracle_ft(sc), oracle_ft(qc)
    got = F.tables_from_counts(sc, qc)
    return dict(sc=sc, qc=qc, swhere=swhere, qwhere=qwhere, want=want, got=got)


# ------------------------------------------------------------------------------------------------------- normalisation
def test_tables_from_counts_on_every_family_vector(packed):
    """k_normalize<4> / <64> with normalize_m2 on every accepted family vector, the edge vectors in contexts 0, 1, 63, 64,
    255 and 8191 among others, classified random draws in the rest: both structs are the oracle's byte for byte"""
    assert set(T.EDGE_CONTEXTS) <= set(packed["qwhere"]) and {0, 1, 63, 64, 255} <= set(packed["swhere"])
    for stream, alpha in enumerate((4, 64)):
        got, want = packed["got"][stream], packed["want"][stream]
        where = packed["swhere" if alpha == 4 else "qwhere"]
        for m, name in where.items():   # (a family vector that differs is named before the whole struct is compared)
            assert got["logs"][0][m] == want["logs"][0][m], (name, m)
            assert np.array_equal(got["norm"][0][m], want["norm"][0][m]), (name, m, got["norm"][0][m], want["norm"][0][m])
        assert got.tobytes() == want.tobytes()
        assert int(got["max_log"][0]) == int(want["logs"][0].max())
    assert int(packed["got"][0]["max_log"][0]) == 11 and int(packed["got"][1]["max_log"][0]) == 11


@pytest.mark.parametrize("alpha", [4, 64])
@pytest.mark.parametrize("refusal", ["rle-first", "rle-last", "rle-2^32-1", "empty", "too-large-by-one", "too-large-by-one-in-three",
                                     "too-large-all"])
def test_one_refused_context_refuses_the_call(F, packed, alpha, refusal):
    """the RLE refusal (err 4), the empty context and the total above 2^32 - 1 (err 2), as the only bad context of an
    otherwise good call: FQGPU_E_ARG; the good call behind it gives the right bytes"""
    verdict, vec = T.REFUSED[alpha][refusal]
    assert T.normalize(vec) == verdict
    models = T.MODELS[alpha]
    for m in (0, models // 2 + 1, models - 1):
        counts = [packed["sc"].copy(), packed["qc"].copy()]
        counts[alpha == 64][m] = vec
        with pytest.raises(F.FqgpuError) as ei:
            F.tables_from_counts(*counts)
        assert ei.value.code == E_ARG, (refusal, m)
    got = F.tables_from_counts(packed["sc"], packed["qc"])
    assert got[0].tobytes() == packed["want"][0].tobytes() and got[1].tobytes() == packed["want"][1].tobytes()


# --------------------------------------------------------------------------------------------------------- table build
def test_table_words_of_every_family_context(F, packed):
    """k_log_prefix and k_build_tables: all 256 sequence contexts and every quality context that holds a family vector
    (no stride), word for word against fo_build_ctable / fo_build_dtable"""
    sft, qft = packed["got"]
    # the contexts named for what they cover
    cover = {}
    for stream, (ft, where) in enumerate(((sft, packed["swhere"]), (qft, packed["qwhere"]))):
        for m in where:
            norm, log = ft["norm"][0][m], int(ft["logs"][0][m])
            present = norm[norm != 0]
            if (norm == 0).any():
                cover.setdefault((stream, "a symbol with count 0"), m)
            if (norm == -1).any():
                cover.setdefault((stream, "symbols with -1"), m)
            if log == 5:
                cover.setdefault((stream, "log 5: 32 cells, half a step"), m)
            cover.setdefault((stream, "fast flag %d" % (not (present >= (1 << log) // 2).any())), m)
    for stream in (0, 1):
        for what in ("a symbol with count 0", "symbols with -1", "log 5: 32 cells, half a step", "fast flag 0", "fast flag 1"):
            assert (stream, what) in cover, (stream, what)
    ctx = F.Context(sft, qft)
    try:
        assert_tables(ctx, 0, sft, range(256))
        assert len(packed["qwhere"]) > 200
        assert_tables(ctx, 1, qft, sorted(packed["qwhere"]))
        for (stream, what), m in cover.items():   # the fast flag of the named contexts is what the name says
            if what.startswith("fast flag"):
                assert int(ctx.dump_tables(stream, m)[1][0]) >> 16 == int(what[-1]), (stream, what, m)
    finally:
        ctx.close()


def mixed_log_tables():
    """FreqTable structs a foreign writer could have made: the contexts alternate between log 5 and log 12 (sequence:
    every symbol present, so any read can be coded; quality: log 5 holds 20 symbols at the most)"""
    rng = np.random.default_rng(12)
    out = []
    for alpha in (4, 64):
        ft = np.zeros(1, dtype=FT_DTYPE[alpha])
        for m in range(T.MODELS[alpha]):
            log = 5 if m % 2 == 0 else 12
            k = alpha if alpha == 4 or log == 12 else int(rng.integers(2, 21))
            row = np.zeros(alpha, dtype=np.int64)
            at = rng.permutation(alpha)[:k]
            row[at] = 1
            extra = rng.multinomial((1 << log) - k, rng.dirichlet(np.full(k, 0.5)))
            row[at] += extra
            low = at[(row[at] == 1) & (rng.random(k) < 0.5)]
            assert int(row.sum()) == 1 << log
            row[low] = -1
            ft["norm"][0][m] = row
            ft["logs"][0][m] = log
        ft["max_log"][0] = 12
        out.append(ft)
    return out


def test_tables_whose_logs_alternate_between_5_and_12(F, golden_dir):
    """uneven offsets in k_log_prefix, the one-symbol transition table at the stride of log 12 (no two-symbol table): the
    table words of every sequence context and of quality contexts at both ends and in between; a fixture coded with the
    sequence tables gives the oracle's streams"""
    sft, qft = mixed_log_tables()
    ctx = F.Context(sft, qft)
    try:
        assert_tables(ctx, 0, sft, range(256))
        assert_tables(ctx, 1, qft, [0, 1, 2, 3, 62, 63, 64, 65, 4095, 4096, 8190, 8191] + list(range(5, 8192, 97)))
    finally:
        ctx.close()
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    _, _, _, own_qft = O.freq_tables(raw, recs)
    same_streams_and_back(F, sft, own_qft, raw, recs, [dict()])


# ------------------------------------------------------------------------------------------------------ foreign tables
def good_tables(golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    return (raw, recs) + tuple(O.freq_tables(raw, recs)[2:])


def spoil(ft, m, how):
    """one context of a good struct turned into what fqgpu_ctx_create must refuse"""
    ft = ft.copy()
    norm, logs = ft["norm"][0], ft["logs"][0]
    log = int(logs[m])
    big = int(np.argmax(norm[m]))
    assert norm[m][big] >= 2
    if how == "sum 2^log - 1":
        norm[m][big] -= 1
    elif how == "sum 2^log + 1":
        norm[m][big] += 1
    elif how == "log 4":
        logs[m] = 4
    elif how == "log 13":
        logs[m] = 13
    elif how == "an entry of -2, the sum still right":
        # [-2, 2^log, 0, 0 ...]: k_build_tables' prefix sums count the -2 as 0
        norm[m] = 0
        norm[m][0], norm[m][1] = -2, 1 << log
    elif how == "an entry of -2 beside the others":
        other = int(np.argmin(norm[m])) if int(np.argmin(norm[m])) != big else (big + 1) % norm.shape[1]
        norm[m][big] += max(int(norm[m][other]), 0) if norm[m][other] != -1 else 1
        norm[m][other] = -2
        assert int(np.where(norm[m] == -1, 1, np.maximum(norm[m], 0)).sum()) == 1 << log   # (as k_build_tables sums)
    else:
        raise AssertionError(how)
    return ft


@pytest.mark.parametrize("how", ["sum 2^log - 1", "sum 2^log + 1", "log 4", "log 13", "an entry of -2, the sum still right",
                                 "an entry of -2 beside the others"])
def test_foreign_tables_that_are_refused(F, golden_dir, how):
    """in the first, a middle and the last context of either stream: FQGPU_E_ARG and no handle; a good handle works
    afterwards"""
    raw, recs, sft, qft = good_tables(golden_dir)
    for stream, ft in ((0, sft), (1, qft)):
        models = ft["norm"][0].shape[0]
        for m in (0, models // 2 + 1, models - 1):
            bad = spoil(ft, m, how)
            with pytest.raises(F.FqgpuError) as ei:
                F.Context(bad if stream == 0 else sft, bad if stream == 1 else qft)
            assert ei.value.code == E_ARG, (how, stream, m)
    same_streams_and_back(F, sft, qft, raw, recs, [dict()])


def test_foreign_tables_at_the_edge_of_the_rule_are_accepted(F, golden_dir):
    """what the rule still lets in: a context of one symbol at 2^log - 1 and one -1; 2^log / 2 twice; log 5 and log 12
    beside each other; every entry -1 but one.  The table words are libzstd's (the oracle's builders)"""
    _, _, sft, qft = good_tables(golden_dir)
    sft, qft = sft.copy(), qft.copy()
    rows = {0: (5, [31, -1, 0, 0]), 1: (12, [2048, 2048, 0, 0]), 128: (5, [-1, -1, -1, 29]), 255: (12, [0, -1, 4095, 0])}
    for m, (log, row) in rows.items():
        sft["norm"][0][m], sft["logs"][0][m] = row, log
    qrows = {0: (5, [-1] * 31 + [1] + [0] * 32), 4097: (6, [-1] * 63 + [1]), 8191: (12, [0] * 62 + [4095, -1])}
    for m, (log, row) in qrows.items():
        qft["norm"][0][m], qft["logs"][0][m] = row, log
    sft["max_log"][0] = qft["max_log"][0] = 12
    ctx = F.Context(sft, qft)
    try:
        assert_tables(ctx, 0, sft, sorted(rows) + [2, 127, 129, 254])
        assert_tables(ctx, 1, qft, sorted(qrows) + [1, 4096, 4098, 8190])
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------- transition tables
def same_streams_and_back(F, sft, qft, raw, recs, settings):
    """the block coded under these tables on the device, once a setting, against the oracle's coding; where both say the
    capacity rule is broken, again with generous capacities; the device restores the block from its streams"""
    octx = O.OracleCtx(sft, qft)
    e = octx.encode(raw, recs)
    caps = {}
    if e["rc"] == -1:
        n = int(recs["len"].sum())
        caps = dict(seq_cap=2 * n + 4096, qual_cap=2 * n + (8 << 20))
        e2 = octx.encode(raw, recs, **caps)
        assert e2["rc"] == 0
    octx.close()
    ctx = F.Context(sft, qft)
    try:
        for s in settings:
            if "segment" in s:
                ctx.set_chain_params(s["segment"], seq_segment=s["segment"])
            if "handover" in s:
                ctx.set_seq_handover(*s["handover"])
            g = ctx.encode_block(raw, recs)
            assert g["rc"] == e["rc"], (s, g["rc"], e["rc"])
            want = e
            if e["rc"] == -1:
                g = ctx.encode_block(raw, recs, **caps)
                want = e2
            assert g["rc"] == 0, (s, g["rc"])
            for k in STREAMS:
                assert np.array_equal(np.asarray(g[k]), np.asarray(want[k])), (s, k)
            rc, out = ctx.decode_block(g["seq"], g["qual"], g["n_count"], g["n_pos"], recs, O.blank_skeleton(raw, recs))
            assert rc == 0 and np.array_equal(out, raw), s
    finally:
        ctx.close()


def table_set(name):
    """sequence and quality tables from family counts, every count 1 or more: any data can be coded"""
    rng = np.random.default_rng(21)
    qc = T.packed_counts(64, True)[0]
    if name == "the random mix":
        sc = T.packed_counts(4, True)[0]
    elif name == "many -1 symbols":
        sc = np.ones((256, 4), dtype=np.uint32)
        for m in range(256):   # one to three symbols stay at 1 beside counts of thousands: low-probability symbols
            big = rng.permutation(4)[: int(rng.integers(1, 4))]
            sc[m, big] = rng.integers(5000, 60000, len(big))
    else:
        assert name == "many log-5 and log-6 contexts"
        sc = np.ones((256, 4), dtype=np.uint32)
        for m in range(256):   # totals of 5..256 give log 5, of 257..512 log 6
            total = int(rng.integers(6, 257)) if m % 2 else int(rng.integers(257, 513))
            sc[m] += rng.multinomial(total - 4, rng.dirichlet(np.ones(4))).astype(np.uint32)
    return oracle_ft(sc), oracle_ft(qc)


SETTINGS = [dict(), dict(handover=(0, 1)), dict(segment=1024), dict(segment=1024, handover=(64, 1))]


@pytest.mark.parametrize("tables", ["the random mix", "many -1 symbols", "many log-5 and log-6 contexts"])
@pytest.mark.parametrize("block", ["two_letters", "SRR065390_sub_1"])
def test_transition_tables_through_the_streams(F, golden_dir, tables, block):
    """next1, next2, the power tables and the reset masks have no dump: a two-letter block (sixteen contexts, each tens
    of segments long) and a fixture coded under family tables give the oracle's streams, with the default segment and
    segments of 1024, hand-over off and on"""
    sft, qft = table_set(tables)
    logs, norm = sft["logs"][0], sft["norm"][0]
    if tables == "many -1 symbols":
        assert int((norm == -1).sum()) > 256
    if tables == "many log-5 and log-6 contexts":
        assert int((logs == 5).sum()) >= 100 and int((logs == 6).sum()) >= 100 and int(logs.max()) == 6
    if block == "two_letters":
        raw, recs = seq_blocks.block("two_letters", 1 << 20)[:2]
        per_context = O.freq_tables(raw, recs)[0].astype(np.int64).sum(axis=1) - 4
        assert int(recs["len"].sum()) == int(per_context.sum())
        assert int(per_context.max()) >= 3 * 1024   # a context of three segments and more: the power tables are used
    else:
        raw, recs = O.load_fastq(os.path.join(golden_dir, block + ".fastq"))
    same_streams_and_back(F, sft, qft, raw, recs, SETTINGS)


# ---------------------------------------------------------------------------------------------------------- histograms
@pytest.mark.parametrize("family", T.READ_FAMILIES)
def test_histograms_on_every_read_family(F, family):
    """k_hist_seq and k_hist_qual (the encoder's sort from 2^20 symbols on): raw counts and both structs; a byte that is no
    base and a quality outside 0..63 are refused, the same bytes behind a read are not; the good call behind a refusal
    gives the right counts"""
    names = T.read_names(family)
    assert names
    good = ("records:one", np.frombuffer(T.shared_read_cases()["records:one"][0], dtype=np.uint8),
            T.shared_read_cases()["records:one"][1]) + T.read_reference("records:one")[1:]
    for name in names:
        raw, recs, verdict = T.shared_read_cases()[name]
        raw = np.frombuffer(raw, dtype=np.uint8)
        if verdict == "bad":
            with pytest.raises(F.FqgpuError) as ei:
                F.freq_tables(raw, recs, want_counts=True)
            assert ei.value.code == E_ARG, name
            check_counts(F, *good)
            continue
        if family == "switch":   # (the oracle counts a million symbols where the byte loops take seconds)
            sc, qc = O.freq_tables(raw, recs)[:2]
        else:
            _, sc, qc = T.read_reference(name)
        good = (name, raw, recs, sc, qc)
        check_counts(F, *good)


def check_counts(F, name, raw, recs, sc, qc):
    gs, gq, gsc, gqc = F.freq_tables(raw, recs, want_counts=True)
    if not np.array_equal(gsc, sc):
        at = np.argwhere(gsc != sc)[:4].tolist()
        raise AssertionError((name, "sequence counts", at, [(int(gsc[a, b]), int(sc[a, b])) for a, b in at]))
    if not np.array_equal(gqc, qc):
        at = np.argwhere(gqc != qc)[:4].tolist()
        raise AssertionError((name, "quality counts", at, [(int(gqc[a, b]), int(qc[a, b])) for a, b in at]))
    assert gs.tobytes() == oracle_ft(sc).tobytes() and gq.tobytes() == oracle_ft(qc).tobytes(), name
