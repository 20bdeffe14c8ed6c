"""The reference of the table tests (tables_ref.py) and its inputs, judged before they judge a kernel: the Python
normaliser agrees with oracle/fse_oracle.c and with libzstd 1.4.8 on every family vector -- the log, the counts, the
refusal -- and both table builders agree with libzstd's word for word on what it accepts; the byte-loop histograms
agree with the oracle's and, where it is built, with the reference's compiled calculateFreqTable (oracle/_ref/ref_tool_asan
analyze).  Generating the families runs the generator's own assertions that each vector takes the branch it is named for.
No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_pin as R
import tables_ref as T

TOOL = R.REF_TOOL_ASAN
ALPHAS = (4, 64)


def _zstd():
    for cand in ("/usr/lib/x86_64-linux-gnu/libzstd.so.1", "/opt/conda/lib/libzstd.so.1"):
        if os.path.exists(cand):
            Z = C.CDLL(cand)
            if hasattr(Z, "FSE_normalizeCount") and hasattr(Z, "FSE_buildCTable_wksp"):
                vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
                Z.FSE_optimalTableLog.restype = u
                Z.FSE_optimalTableLog.argtypes = [u, sz, u]
                Z.FSE_normalizeCount.restype = sz
                Z.FSE_normalizeCount.argtypes = [vp, u, vp, sz, u, u]
                Z.FSE_buildCTable_wksp.restype = sz
                Z.FSE_buildCTable_wksp.argtypes = [vp, vp, u, u, vp, sz]
                Z.FSE_buildDTable_wksp.restype = sz
                Z.FSE_buildDTable_wksp.argtypes = [vp, vp, u, u, vp, sz]
                Z.FSE_isError.restype = u
                Z.FSE_isError.argtypes = [sz]
                return Z
    return None


Z = _zstd()   # (absent: the legs against libzstd are left out, the ones against the oracle stay)


# ------------------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("alpha", ALPHAS)
def test_families_are_deterministic_and_each_asserts_its_tag(alpha):
    a, b = T.families(alpha), T.shared_families(alpha)   # (making them runs the assertions)
    assert a == b and list(a) == list(T.FAMILIES)
    names = [n for n, _ in T.family_vectors(alpha)]
    assert len(set(names)) == len(names)
    for fam in T.FAMILIES:
        if fam.startswith("m2") and fam != "m2_edge" and alpha == 4:
            assert not a[fam]   # UNREACHED
        else:
            assert a[fam], fam
    if alpha == 64:
        assert len(a["m2"]) >= 64 and all("m2" in T.tags_of(c) for _, c in a["m2"])
    for fam, tag in (("zeros", "zero"), ("tie", "tie"), ("skew", "low"), ("low_edge", "low")):
        assert all(tag in T.tags_of(c) for _, c in a[fam]), fam
    for name, (verdict, c) in T.REFUSED[alpha].items():
        assert T.normalize(c) == verdict and len(c) == alpha, name


@pytest.mark.parametrize("alpha", ALPHAS)
def test_every_branch_is_reached_or_listed_with_the_search_that_missed_it(alpha):
    met = set()
    for _, c in T.family_vectors(alpha):
        met |= T.tags_of(c)
    unreached = set(T.UNREACHED[alpha])
    assert unreached <= set(T.M2_INNER) | ({"m2"} if alpha == 4 else set())
    assert set(T.REQUIRED) - unreached <= met, sorted(set(T.REQUIRED) - unreached - met)
    # what is listed as unreached is met by no family and by no vector of the bounded search
    searched, n = T.search_unreached(alpha)
    assert n >= len(T.SEARCH_SEEDS) * T.SEARCH_DRAWS + T.SEARCH_DIRECTED - 100
    assert not unreached & (met | searched), sorted(unreached & (met | searched))
    assert all(isinstance(why, str) and why for why in T.UNREACHED[alpha].values())


@pytest.mark.parametrize("alpha", ALPHAS)
def test_rounding_thresholds_are_met_on_equality_and_one_count_above(alpha):
    best = T.rtb_search(alpha)
    assert set(best) == {(p, side) for p in range(1, 8) for side in "+-"}
    for (p, side), (diff, c) in best.items():
        assert diff == T.RTB_DISTANCE[side], (p, side, diff)
        total = sum(c)
        assert T.normalize(c)[0] == 11 and total & (total - 1) == 0
        if side == "-":   # count / total = (P + rtb[P] / 2^20) / 2^11 exactly: the remainder equals the rest to beat
            assert c[0] << 31 == ((p << 20) + T.RTB[p]) * total and T.normalize(c)[1][0] == p
        else:
            assert T.normalize(c)[1][0] == p + 1


def test_normaliser_on_vectors_worked_out_by_hand():
    assert T.normalize((1, 1, 1, 1))[:2] == (11, [512] * 4)
    assert T.normalize((1,) * 64)[:2] == (7, [2] * 64)
    assert T.normalize((3, 1, 0, 0))[:2] == (11, [1536, 512, 0, 0])          # total 4: the wrap
    assert T.normalize((4, 1, 0, 0))[:2] == (5, [26, 6, 0, 0])               # total 5: no wrap
    assert T.normalize((1, 1, 1, 900000))[:2] == (11, [-1, -1, -1, 2045])
    assert T.normalize((0, 7, 0, 0)) == "rle" and T.normalize((0,) * 4) == "empty"
    assert T.normalize((1 << 31, 1 << 31, 0, 0)) == "too_large"
    assert T.optimal_table_log(4, 3) == (11, True) and T.optimal_table_log(5, 3) == (5, False)


# --------------------------------------------------------------------------------------- the normaliser and the builders
def _vectors(alpha, family):
    if family == "refused":
        return [(n, c) for n, (_, c) in T.REFUSED[alpha].items()]
    if family == "draws":
        return [("draw-%d" % i, c) for i, c in enumerate(T.random_draws(alpha, 300, 50 + alpha))]
    return T.shared_families(alpha)[family]


@pytest.mark.parametrize("family", T.FAMILIES + ("refused", "draws"))
@pytest.mark.parametrize("alpha", ALPHAS)
def test_normaliser_and_builders_against_the_oracle_and_libzstd(alpha, family):
    """the log, the counts and the refusal; on every accepted vector the CTable and the DTable of the oracle against
    libzstd's, absent symbols and log 5 under 64 symbols included"""
    L = O.lib()
    wksp = np.zeros(1 << 16, dtype=np.uint8)
    for name, counts in _vectors(alpha, family):
        r = T.normalize(counts)
        if r in ("empty", "too_large"):
            continue   # (a total of 0 or above 2^32 - 1 is the library's own refusal: zstd's functions take a u32 above 0)
        c = np.array(counts, dtype=np.uint32)
        total = int(c.sum())
        t_o = L.fo_optimal_table_log(0, total, alpha - 1)
        n_o = np.zeros(alpha, dtype=np.int16)
        r_o = L.fo_normalize_count(O.ptr(n_o), t_o, O.ptr(c), total, alpha - 1, 1)
        if Z is not None:
            t_z = Z.FSE_optimalTableLog(0, total, alpha - 1)
            n_z = np.zeros(alpha, dtype=np.int16)
            r_z = Z.FSE_normalizeCount(O.ptr(n_z), t_z, O.ptr(c), total, alpha - 1, 1)
            assert not Z.FSE_isError(r_z), name
        if r == "rle":
            assert r_o == 0 and (Z is None or r_z == 0), name
            continue
        t, norm, tags = r
        assert t_o == t and r_o == t and n_o.tolist() == norm, (name, t, t_o, norm, n_o)
        cw, dw = L.fo_ctable_words(t, alpha - 1), L.fo_dtable_words(t)
        ct_o, dt_o = np.zeros(cw, dtype=np.uint32), np.zeros(dw, dtype=np.uint32)
        assert L.fo_build_ctable(O.ptr(ct_o), O.ptr(n_o), alpha - 1, t) == 0
        assert L.fo_build_dtable(O.ptr(dt_o), O.ptr(n_o), alpha - 1, t) == 0
        assert (int(dt_o[0]) >> 16 == 0) == ("notfast" in tags), name
        if Z is not None:
            assert t_z == t and r_z == t and n_z.tolist() == norm, (name, t, t_z, norm, n_z)
            ct_z, dt_z = np.zeros(cw, dtype=np.uint32), np.zeros(dw, dtype=np.uint32)
            assert Z.FSE_buildCTable_wksp(O.ptr(ct_z), O.ptr(n_z), alpha - 1, t, O.ptr(wksp), wksp.size) == 0
            assert Z.FSE_buildDTable_wksp(O.ptr(dt_z), O.ptr(n_z), alpha - 1, t, O.ptr(wksp), wksp.size) == 0
            assert np.array_equal(ct_o, ct_z) and np.array_equal(dt_o, dt_z), name


@pytest.mark.parametrize("alpha", ALPHAS)
def test_packed_counts_hold_every_family_vector_and_the_structs_are_the_oracles(alpha):
    """the count arrays the device tests normalise: every family vector in a context of its own, the edge contexts
    taken; the FreqTable struct the Python normaliser makes of them is the oracle's byte for byte"""
    L = O.lib()
    for positive in (False, True):
        counts, where = T.packed_counts(alpha, positive)
        vecs = dict(T.family_vectors(alpha))
        assert set(m for m in T.EDGE_CONTEXTS if m < T.MODELS[alpha]) <= set(where)
        for m, name in where.items():
            assert tuple(counts[m].tolist()) == vecs[name]
        assert len(where) == len([1 for c in vecs.values() if not positive or min(c) >= 1])
        assert not positive or counts.min() >= 1
        ft = T.freq_table(counts)
        want = np.zeros(1, dtype=O.SEQ_FT_DTYPE if alpha == 4 else O.QUAL_FT_DTYPE)
        make = L.fqo_seq_ft_from_counts if alpha == 4 else L.fqo_qual_ft_from_counts
        assert make(O.ptr(np.ascontiguousarray(counts)), O.ptr(want)) == 0
        assert ft.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------ histograms
def test_read_cases_are_deterministic():
    a, b = T.read_cases(), T.shared_read_cases()
    assert list(a) == list(b)
    for k in a:
        assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and a[k][2] == b[k][2]
    assert {k.split(":")[0] for k in a} == set(T.READ_FAMILIES)
    assert {T.read_reference(k)[0] for k in a} == {"ok", "bad"}


def test_histograms_on_reads_worked_out_by_hand():
    raw, recs = T.block_of([(b"ACNG", b"II5!")])
    sc, qc = T.seq_counts(raw, recs), T.qual_counts(raw, recs)
    want = np.ones((256, 4), dtype=np.uint32)
    want[0xD7, 0] += 1                           # A behind T, C, C, T
    want[0xD7 >> 2, 1] += 1                      # C behind A, T, C, C
    want[(0xD7 >> 4) + (1 << 6), 2] += 1         # G behind C, A, T, C: the N moved nothing
    assert np.array_equal(sc, want)
    q = [40, 40, 20, 0]
    wq = np.ones((8192, 64), dtype=np.uint32)
    wq[T.qual_context(0, 0, 0), q[0]] += 1
    wq[T.qual_context(q[0], 0, 0), q[1]] += 1
    wq[T.qual_context(q[1], q[0], 0), q[2]] += 1
    wq[T.qual_context(q[2], q[1], q[0]), q[3]] += 1
    assert np.array_equal(qc, wq)
    assert T.qual_context(0, 0, 0) == 4096 and T.qual_context(40, 0, 0) == 4096 + 40 and T.qual_context(20, 40, 40) == 4096 + 40 * 64 + 20
    assert T.qual_context(5, 7, 9) == 9 * 64 + 5 and T.qual_context(63, 63, 62) == 63 * 64 + 63
    assert T.fold_profile(b"I" * 70) == [(1, 1, 62), (6, 0, 0)]   # the first three symbols of a read have contexts of their own


@pytest.mark.parametrize("family", T.READ_FAMILIES)
def test_histograms_against_the_oracle(family):
    L = O.lib()
    for name in T.read_names(family):
        raw, recs, _ = T.shared_read_cases()[name]
        verdict, sc, qc = T.read_reference(name)
        raw = np.frombuffer(raw, dtype=np.uint8)
        osc = np.zeros((256, 4), dtype=np.uint32)
        oqc = np.zeros((8192, 64), dtype=np.uint32)
        rs = L.fqo_seq_counts(O.ptr(raw), O.ptr(recs), len(recs), O.ptr(osc))
        rq = L.fqo_qual_counts(O.ptr(raw), O.ptr(recs), len(recs), O.ptr(oqc))
        if verdict == "bad":
            assert (rs != 0) != (rq != 0), name   # each refusal case spoils one of the two lines
            assert (rs != 0) == isinstance(T.seq_counts(raw, recs), str), name
            continue
        assert rs == 0 and rq == 0, name
        assert np.array_equal(sc, osc) and np.array_equal(qc, oqc), name


def whole_lines(name):
    """a case the reference's parser makes the same record table of: nothing behind a read's length"""
    raw, recs, verdict = T.shared_read_cases()[name]
    return verdict == "ok" and all(raw[so + n] == 10 and raw[qo + n] == 10 for so, qo, n in recs.tolist())


needs_ref_tool = pytest.mark.skipif(not os.path.exists(TOOL) and not R.reference_tree_present(),
                                    reason="neither oracle/_ref/ref_tool_asan nor the reference tree it is built from is here")


@needs_ref_tool
@pytest.mark.parametrize("family", T.READ_FAMILIES)
def test_histograms_against_the_compiled_reference(family, tmp_path):
    """both calculateFreqTable functions themselves (`analyze`) on every case whose lines are its reads: the two structs
    equal the ones the Python normaliser makes of the Python counts"""
    assert os.path.exists(TOOL), "oracle/_ref/ref_tool_asan is missing: run build() (make -C oracle) where the reference tree is"
    seen = 0
    for name in T.read_names(family):
        if not whole_lines(name):
            continue
        seen += 1
        raw, _, _ = T.shared_read_cases()[name]
        _, sc, qc = T.read_reference(name)
        a = R.analyze(TOOL, np.frombuffer(raw, dtype=np.uint8), tmp_path, "analyze%d" % seen)
        assert a["seq_ft"].tobytes() == T.freq_table(sc).tobytes(), name
        assert a["qual_ft"].tobytes() == T.freq_table(qc).tobytes(), name
    assert seen or family == "refusals"
