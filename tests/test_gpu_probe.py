"""Adapter content on the device (k_adapter_find's probe form in fqcomp28_amd/csrc/select.hip, behind fqgpu_chunk_probe /
fqgpu_dblock_probe) against the numpy restatement in probe_ref.py: the result words and the places, word for word.  Integer
arithmetic: every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import adapter_ref as AR
import oracle_lib as O
import probe_ref as PR
import stats_ref as SR
import test_adapter_host as AH
import test_gpu_adapter as TA
import test_gpu_stats as TS
import test_gpu_trim as TT
import trim_ref as R

pytestmark = pytest.mark.gpu

E_OVERFLOW, E_SHORT_READ, E_CORRUPT, E_ARG = -1, -2, -3, -4
TRUSEQ = AH.TRUSEQ
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
LENGTHS = [3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, 511, 513, 700]
PROBE_LENGTHS = [1, 12, 13, 31, 32, 33, 63, 64]
W = PR.WINDOW_ROWS


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def ctx(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    c = TS.context_for(F, raw, recs)
    yield c
    c.close()


def device(ctx, raw, recs, p, P, **kw):
    b = ctx.dblock(raw, recs)
    try:
        return b.probe(p, P, **kw)
    finally:
        b.close()


def holds(g, want, what=""):
    """a device result against (words, places) of the reference"""
    assert g["rc"] == 0, (what, g["rc"])
    TS.same(g["out"], want[0], what)
    if g["places"] is not None and not np.array_equal(g["places"], want[1]):
        r, k = (int(x[0]) for x in np.nonzero(g["places"] != want[1]))
        raise AssertionError("%s: the places differ, first at record %d, probe %d: %d, expected %d" % (what, r, k, g["places"][r, k], want[1][r, k]))


def same(ctx, raw, recs, p, P, what="", **kw):
    want = PR.probe_of(raw, recs, p, P)
    g = device(ctx, raw, recs, p, P, **kw)
    holds(g, want, what)
    return g, want


def probe_set(n, seed, first=None):
    """n probes of the lengths PROBE_LENGTHS in turn, drawn; `first`: adapters that stand in front.  A probe of one base hits
    nearly every read at a small place; the long ones need planting"""
    rng = np.random.default_rng(seed)
    out = list(first or [])
    for k in range(len(out), n):
        m = PROBE_LENGTHS[(k + seed) % len(PROBE_LENGTHS)]
        out.append(AR.adp(BASES[rng.integers(0, 4, m)].tobytes(), min(m, [5, 1, 12][k % 3]), [10, 0, 20][k % 3]))
    return out[:n]


def reads_with(lens, adapters, seed, places=None):
    """reads of these lengths at every alignment of the sequence line in turn; read r holds adapter r mod n -- as much of it
    as fits -- at places[r] (None: nothing), by default in turn at 0, at L - min_overlap, somewhere, nowhere -> (raw, recs)"""
    rng = np.random.default_rng(seed)
    seqs, hls, at = [], [], 0
    for r, L in enumerate(lens):
        L = int(L)
        s = BASES[rng.integers(0, 4, L)].copy()
        seq64, m, mo, _, _ = AR.fields(adapters[r % len(adapters)])
        p = [0, max(L - mo, 0), int(rng.integers(0, L)), None][r // len(adapters) % 4] if places is None else places[r]
        if p is not None and p < L:
            k = min(m, L - p)
            s[p:p + k] = seq64[:k]
        if r % 5 == 4:
            s[int(rng.integers(0, L))] = ord("N")
        seqs.append(s.tobytes())
        hls.append(TT.aligned_header(at, L, (r + seed) % 16))
        at += hls[-1] + 2 * L + 5
    raw, recs = TA.chunk_with(hls, seqs)
    assert [int(x) & 15 for x in recs["seq_off"]] == [(r + seed) % 16 for r in range(len(lens))]
    return raw, recs


# ---------------------------------------------------------------- 1. reads worked out by hand
def test_reads_built_by_hand(F, ctx):
    """Every row of test_adapter_host.HAND, its adapter one probe among others.  A read of fewer than three bases never
    reaches the device (every way to a block refuses it, FQGPU_E_SHORT_READ): those two rows are checked to be refused there,
    as test_gpu_adapter.py does, and rows of three bases stand beside them."""
    others = [AR.adp(b"A" * 20, 20, 0), AR.adp(b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"), AR.adp(b"ACGT" * 16, 40, 10)]
    for seq, A, mo, pct, clip in AH.HAND:
        for hl in (2, 9):
            raw, recs = TA.chunk_with([hl], [seq])
            if len(seq) < 3:
                with pytest.raises(F.binding.FqgpuError) as refused:
                    ctx.dblock(raw, recs)
                assert refused.value.code == E_SHORT_READ
                continue
            for at in (0, 1, 3):
                set_ = others[:at] + [AR.adp(A, mo, pct)] + others[at:]
                g, want = same(ctx, raw, recs, PR.prb(set_), 16, what="%s %s %d %d" % (seq, A, mo, pct))
                assert g["places"][0, at] == clip
                v = PR.view(g["out"])
                assert int(v["tables"][at, 0]) == (clip < len(seq)) and int(v["tables"][at, 1]) == len(seq) - clip
                assert int(v["tables"][at, 3]) == (clip == 0) and int(v["rows"][at].sum()) == (clip < len(seq))
    rows = [row for row in AH.HAND if len(row[0]) >= 3]
    raw, recs = TA.chunk_with(2 + np.arange(len(rows)) * 5 % 16, [row[0] for row in rows])
    adapters = sorted({row[1:4] for row in rows})
    g, want = same(ctx, raw, recs, PR.prb([AR.adp(*a) for a in adapters]), 8, what="all rows, all their adapters")
    assert [int(g["places"][r, adapters.index(row[1:4])]) for r, row in enumerate(rows)] == [row[4] for row in rows]


def test_one_probe_is_the_clip(F, ctx):
    """n = 1: the places are the windows fqgpu_dblock_clip gives for the same adapter (no trim: a window is (0, clip place))"""
    raw, recs, a = TA.planted(1000, 1100)
    b = ctx.dblock(raw, recs)
    clip = b.clip(a)
    g = b.probe(PR.prb([a]), 64)
    b.close()
    want = PR.probe_of(raw, recs, PR.prb([a]), 64)
    holds(g, want, "one probe")
    assert clip["rc"] == 0 and (clip["win"] >> 16).tolist() == g["places"][:, 0].tolist() and not (clip["win"] & 0xFFFF).any()
    v = PR.view(g["out"])
    assert int(v["tables"][0, 0]) == int(clip["report"][AR.READS_WITH_ADAPTER]) > 200
    assert int(v["tables"][0, 1]) == int(clip["report"][AR.BASES_CUT_ADAPTER])
    assert v["tables"][0, [0, 1, 3]].tolist() == v["tables"][1, [0, 1, 3]].tolist() and v["rows"][0].tolist() == v["rows"][1].tolist(), "any is the one"


# ---------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("n_recs,n,P", [(1, 1, 37), (7, 2, 1), (8, 3, 512), (9, 15, 37), (63, 16, W - 1), (64, 1, W), (65, 2, W + 1),
                                        (255, 3, 512), (256, 15, 65535), (257, 16, 37), (1000, 16, 512), (1000, 3, W + 1)])
def test_record_counts_lengths_alignments_and_probe_sets(F, ctx, n_recs, n, P):
    adapters = probe_set(n, n_recs + n)
    lens = [LENGTHS[(r + n_recs) % len(LENGTHS)] for r in range(n_recs)]
    raw, recs = reads_with(lens, adapters, n_recs)
    g, want = same(ctx, raw, recs, PR.prb(adapters), P, what="%d records, %d probes, P %d" % (n_recs, n, P))
    v = PR.view(want[0])
    assert v["n_records"] == n_recs and v["n_bases"] == sum(lens)
    if n_recs >= 255:
        ms = [AR.fields(a)[1] for a in adapters]
        assert n < 8 or set(ms) == set(PROBE_LENGTHS), "probes of every length in one set"
        hit = want[1] < np.asarray(lens)[:, None]
        assert hit.any(axis=0).all() and not hit.all(axis=0)[[m > 1 for m in ms]].any(), "every probe hits somewhere, none of the long ones everywhere"
        assert (want[1] == 0).any(), "a hit at place 0"
        assert (hit & (want[1] >= min(P, 300))).any(), "a hit at or beyond P, or deep in a long read"


def long_chunk():
    """300 reads of 300, 511, 513 and 700 bases, probes of 13, 33 and 64 bases -- probe 0 and probe 3 equal --, planted
    at the places 255, 256, 257 (across a long read's request boundary, whatever the line's alignment), at W - 1, W, W + 1 and
    deep in the read (beyond the window of rows summed on chip), at 0 and at L - min_overlap"""
    rng = np.random.default_rng(5)
    adapters = [AR.adp(TRUSEQ), AR.adp(BASES[rng.integers(0, 4, 33)].tobytes(), 12, 10), AR.adp(BASES[rng.integers(0, 4, 64)].tobytes(), 20, 20),
                AR.adp(TRUSEQ)]
    lens = [[300, 511, 513, 700][r % 4] for r in range(300)]
    spots = [255, 256, 257, W - 1, W, W + 1, 330, 400, 505, 512, 650, 695, 0, None, "end"]
    places = []
    for r, L in enumerate(lens):
        p = spots[r // 4 % len(spots)]
        p = L - AR.fields(adapters[r % 4])[2] if p == "end" else p
        places.append(None if p is not None and p >= L else p)     # (a place the read does not have: nothing is planted)
    raw, recs = reads_with(lens, adapters, 77, places)
    p = PR.prb(adapters)
    return raw, recs, p, PR.places_of(raw, recs, p), places


@pytest.fixture(scope="module")
def long_reads():
    return long_chunk()


@pytest.mark.parametrize("P", [1, 37, W - 1, W, W + 1, 512, 65535])
def test_positions_around_the_window(F, ctx, long_reads, P):
    raw, recs, p, places, planted = long_reads
    want = PR.tables_of(places, recs["len"], p, P), places
    g = device(ctx, raw, recs, p, P)
    holds(g, want, "P %d" % P)
    v = PR.view(g["out"])
    assert v["tables"][0].tolist() == v["tables"][3].tolist() and v["rows"][0].tolist() == v["rows"][3].tolist(), "equal probes, equal tables"
    # the planted occurrence is the one found wherever no chance hit stands in front of it
    found = [(want, int(places[r, r % 4])) for r, want in enumerate(planted) if want is not None]
    assert np.mean([a == b for a, b in found]) > 0.8
    met = {a for a, b in found if a == b}
    assert {255, 256, 257, W - 1, W, W + 1, 0, 650} <= met
    rows = v["rows"][4]
    assert rows.sum() == v["tables"][4, 0] > 150
    if P >= 512:
        assert rows[W:P].sum() > 20, "hits between the window and P: the cells that go to global memory one by one"
    else:
        assert rows[P] > 20, "hits at and beyond P share the last row"
    assert device(ctx, raw, recs, p, P, want_places=False)["out"].tolist() == g["out"].tolist(), "the places are stored only when asked for"


def test_the_longest_read(F, ctx):
    L = 65535
    rng = np.random.default_rng(4)
    seqs = []
    for p in (65500, 0, 65530, None, 65279, 256 * 100 - 7):
        s = BASES[rng.integers(0, 4, L)].copy()
        if p is not None:
            k = min(len(TRUSEQ), L - p)
            s[p:p + k] = np.frombuffer(TRUSEQ[:k], dtype=np.uint8)
        seqs.append(s.tobytes())
    seqs.insert(2, BASES[rng.integers(0, 4, 100)].tobytes())     # short reads among them, in the same rounds
    raw, recs = TA.chunk_with([5, 2, 9, 16, 3, 11, 7], seqs)
    adapters = [AR.adp(TRUSEQ), AR.adp(b"ACGT" * 16, 64, 0), AR.adp(TRUSEQ + b"ACACGTCTGAACTCCAGTCA")]
    g, want = same(ctx, raw, recs, PR.prb(adapters), 65535, what="65535")
    assert want[1][:, 0].tolist() == [65500, 0, 100, 65530, 65535, 65279, 25593]


# ---------------------------------------------------------------- 3. the fixture, all built-ins
def builtin_set(mo=5, pct=10):
    return [AR.adp(seq, min(mo, len(seq)), pct) for _, seq in PR.BUILTIN]


def test_the_fixture_with_an_adapter_in_every_third_read(F, ctx, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    raw = raw.copy()
    rng = np.random.default_rng(3)
    for r in range(0, len(recs), 3):
        A = np.frombuffer(PR.BUILTIN[r // 3 % len(PR.BUILTIN)][1], dtype=np.uint8)
        L, so = int(recs["len"][r]), int(recs["seq_off"][r])
        p = int(rng.integers(0, L))
        raw[so + p:so + p + min(A.size, L - p)] = A[:min(A.size, L - p)]
    p = PR.prb(builtin_set())
    g, want = same(ctx, raw, recs.astype(R.REC_DTYPE), p, 128, what="the fixture")
    v = PR.view(g["out"])
    print("SRR065390_sub_1, planted: reads_with %s, whole %s" % (v["tables"][:, 0].tolist(), v["tables"][:, 2].tolist()))
    assert (v["tables"][:9, 0] >= len(recs) // 30).all() and int(v["tables"][9, 0]) >= len(recs) // 3
    # the three TruSeq probes share 13 bases: reads_whole tells them apart
    assert int(v["tables"][0, 2]) > int(v["tables"][1, 2]) > 0 and int(v["tables"][0, 2]) > int(v["tables"][2, 2]) > 0


# ---------------------------------------------------------------- 4. the lines that are read
def test_quality_lines_are_not_read(F, ctx, long_reads):
    raw, recs, p, places, _ = long_reads
    spoilt = raw.copy()
    for r in range(len(recs)):
        qo, L = int(recs["qual_off"][r]), int(recs["len"][r])
        spoilt[qo:qo + L] = [0, 200, ord(" "), ord("a"), 127][r % 5]
    want = PR.tables_of(places, recs["len"], p, 64), places
    holds(device(ctx, spoilt, recs, p, 64), want, "qualities no quality judge takes")
    b = ctx.dblock(spoilt, recs)
    rc, _ = F.binding._stats_call(F.binding.lib().fqgpu_dblock_stats, 64, ctx.h, b.h)
    b.close()
    assert rc == E_ARG, "the summary, which reads them, refuses the chunk"


def raw_call(F, ctx, b, p, P, out, cap, places=None):
    ptr = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    return F.binding.lib().fqgpu_dblock_probe(ctx.h, b.h if b is not None else None, ptr(p), P, ptr(out), cap, ptr(places))


@pytest.mark.parametrize("byte", [ord("a"), ord("X"), 0xC1, 0])
def test_a_byte_that_is_no_base_refuses_the_chunk(F, ctx, long_reads, byte):
    raw, recs, p, places, _ = long_reads
    raw = raw.copy()
    r = 123
    raw[int(recs["seq_off"][r]) + int(recs["len"][r]) - 1] = byte
    b = ctx.dblock(raw, recs)
    out = np.full(PR.words(4, 64), 7, dtype=np.uint64)
    pl = np.full((len(recs), 4), 7, dtype=np.uint16)
    assert raw_call(F, ctx, b, p, 64, out, out.size, pl) == E_ARG and not out.any() and not pl.any()
    out[:] = 7
    assert raw_call(F, ctx, b, p, 64, out, out.size, None) == E_ARG and not out.any()
    b.close()
    with pytest.raises(PR.Refused):
        PR.probe_of(raw, recs, p, 64)


def test_arguments(F, ctx, long_reads):
    raw, recs, p, places, _ = long_reads
    P = 64
    want = PR.tables_of(places, recs["len"], p, P)
    b = ctx.dblock(raw, recs)
    before = b.crc32()
    out = np.full(want.size + 8, 7, dtype=np.uint64)
    pl = np.full((len(recs), 4), 7, dtype=np.uint16)
    assert raw_call(F, ctx, b, p, P, out, want.size - 1, pl) == E_OVERFLOW and (out == 7).all() and (pl == 7).all(), "nothing is written"
    assert raw_call(F, ctx, b, p, P, out, want.size, pl) == 0 and out[:want.size].tolist() == want.tolist() and (out[want.size:] == 7).all()
    assert pl.tolist() == places.tolist()
    for P_bad in (0, 65536):
        out[:] = 7
        assert raw_call(F, ctx, b, p, P_bad, out, out.size, pl) == E_ARG
    import test_probe_host as PH
    for kw in PH.BAD:
        assert raw_call(F, ctx, b, PR.prb(**kw), P, out, out.size, pl) == E_ARG, kw
    assert raw_call(F, ctx, b, None, P, out, out.size, pl) == E_ARG and raw_call(F, ctx, b, p, P, None, out.size, pl) == E_ARG
    assert raw_call(F, ctx, None, p, P, out, out.size, pl) == E_ARG
    assert b.crc32() == before and np.array_equal(b.fetch_raw(), raw), "the chunk is left as it is"
    g = b.probe(p, P)
    holds(g, (want, places), "behind the refused calls")
    b.close()


# ---------------------------------------------------------------- 5. the chunk on the handle's staging block
def test_the_chunk_on_the_staging_block(F, golden_dir):
    raw, recs = O.load_fastq(os.path.join(golden_dir, "SRR065390_sub_1.fastq"))
    table = recs.astype(R.REC_DTYPE)
    p, P = PR.prb(builtin_set(4, 20)), 96
    want = PR.probe_of(raw, table, p, P)
    assert int(PR.view(want[0])["tables"][9, 0]) > 10
    c = TS.context_for(F, raw, recs)
    b = c.dblock(raw, recs)
    holds(b.probe(p, P), want, "the dblock")
    b.close()
    fmt = TS.fmt_of(TS.first_header_of(raw))
    g = c.encode_raw(raw, flags=F.F_DECODE_INDEX, header_format=fmt, want_crc=True, want_stats=P, want_probes=(p, P))
    assert g["rc"] == 0 and g["headers_rc"] == 0
    holds(dict(rc=0, out=g["probe"], places=g["probe_places"]), want, "in flight")
    stats = SR.stats_of(raw, recs, P)
    TS.same(g["stats"], stats, "the summary beside it")
    holds(c.chunk_probe(p, P, len(recs)), want, "behind fqgpu_encode_end")
    args = (fmt, g["header_fields"], g["readlens"], g["seq"], g["qual"], g["n_count"], g["n_pos"], g["used_len"])
    d = c.decode_chunk(*args, index=g["index"], want_probes=(p, P))
    assert d["rc"] == 0 and d["probe_rc"] == 0 and np.array_equal(d["raw"], raw)
    holds(dict(rc=0, out=d["probe"], places=d["probe_places"]), want, "decoded")
    # digest, summary and a selection before it and after it
    crc, (rc, before) = c.chunk_crc32(), c.chunk_stats(P)
    clip = c.chunk_clip(AR.adp(TRUSEQ), len(recs), R.trm(q_tail=20))
    assert crc == (0, g["crc32"], g["crc_len"]) and rc == 0 and clip["rc"] == 0
    holds(c.chunk_probe(p, P, len(recs), want_places=False), want, "decoded, no places")
    again = c.chunk_clip(AR.adp(TRUSEQ), len(recs), R.trm(q_tail=20))
    assert c.chunk_crc32() == crc and c.chunk_stats(P)[1].tolist() == before.tolist() == stats.tolist()
    assert again["out"].tobytes() == clip["out"].tobytes() and again["report"].tolist() == clip["report"].tolist()
    c.set_check_only(True)
    d = c.decode_chunk(*args, want_raw=False, index=g["index"], want_probes=(p, P))
    assert d["rc"] == 0 and d["raw"] is None and d["probe_rc"] == 0
    holds(dict(rc=0, out=d["probe"], places=d["probe_places"]), want, "check-only")
    c.set_check_only(False)
    # where the summary is refused, so is this: a range, a refused decode
    assert c.decode_chunk_range(*args, 3, 40, index=g["index"])["rc"] == 0
    r = c.chunk_probe(p, P, len(recs))
    assert r["rc"] == E_ARG and not r["out"].any() and c.chunk_stats(P)[0] == E_ARG
    assert c.decode_chunk(*args)["rc"] == 0 and c.chunk_probe(p, P, len(recs))["rc"] == 0
    for at in range(g["qual"].size // 2, g["qual"].size // 2 + 64):
        q = g["qual"].copy()
        q[at] ^= 0x10
        d = c.decode_chunk(fmt, g["header_fields"], g["readlens"], g["seq"], q, g["n_count"], g["n_pos"], g["used_len"])
        if d["rc"] != 0:
            break
    assert d["rc"] == E_CORRUPT
    r = c.chunk_probe(p, P, len(recs))
    assert r["rc"] == E_ARG and not r["out"].any(), "after a refused decode"
    c.enable_timing(True)
    b = c.dblock(raw, recs)
    assert b.probe(p, P)["rc"] == 0
    _, groups = c.last_timing()
    assert [(name, calls) for name, _, calls in groups if name in ("probe", "clip", "stats")] == [("probe", 1)], groups
    b.close()
    c.close()


def test_two_halves_merged_are_the_whole(F, ctx):
    raw, recs, a = TA.planted(1000, 1100)
    p, P = PR.prb([a, AR.adp(TRUSEQ), AR.adp(b"G", 1, 0)]), 200
    whole = device(ctx, raw, recs, p, P)
    holds(whole, PR.probe_of(raw, recs, p, P), "the whole")
    cut = int(recs["seq_off"][500]) - 1
    while raw[cut - 1] != 10:
        cut -= 1     # the start of record 500's header line
    first, second = raw[:cut], raw[cut:]
    ra, rb = recs[:500].copy(), recs[500:].copy()
    rb["seq_off"] -= cut
    rb["qual_off"] -= cut
    ga, gb = device(ctx, first, ra, p, P), device(ctx, second, rb, p, P)
    assert ga["rc"] == 0 == gb["rc"]
    dst = ga["out"].copy()
    assert F.binding.probe_merge(dst, gb["out"]) == 0 and dst.tolist() == whole["out"].tolist()
    assert np.vstack([ga["places"], gb["places"]]).tolist() == whole["places"].tolist()
    dst = np.zeros_like(dst)
    assert F.binding.probe_merge(dst, gb["out"]) == 0 and F.binding.probe_merge(dst, ga["out"]) == 0 and dst.tolist() == whole["out"].tolist()
