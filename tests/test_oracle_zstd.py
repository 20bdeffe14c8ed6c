"""Pins oracle/fse_oracle.c byte-for-byte against the system libzstd.so.1 (1.4.8),
the only piece of the reference's arithmetic that exists in this image
(SURVEY.md 8(c)): table log, normalised counts, CTable bytes, DTable bytes, and
-- through FSE_compress_usingCTable / FSE_decompress_usingDTable -- the inline
bit-writer / encodeSymbol / decodeSymbol primitives."""
import ctypes as C
import ctypes.util
import os

import numpy as np
import pytest

import oracle_lib as O


def _zstd():
    for cand in ("/usr/lib/x86_64-linux-gnu/libzstd.so.1", "/opt/conda/lib/libzstd.so.1",
                 ctypes.util.find_library("zstd")):
        if cand and os.path.exists(cand):
            Z = C.CDLL(cand)
            if hasattr(Z, "FSE_normalizeCount") and hasattr(Z, "FSE_buildCTable_wksp"):
                return Z
    return None


Z = _zstd()
pytestmark = pytest.mark.skipif(Z is None, reason="libzstd.so.1 with FSE exports not found")

if Z is not None:
    vp, sz, u = C.c_void_p, C.c_size_t, C.c_uint
    Z.FSE_optimalTableLog.restype = u
    Z.FSE_optimalTableLog.argtypes = [u, sz, u]
    Z.FSE_normalizeCount.restype = sz
    Z.FSE_normalizeCount.argtypes = [vp, u, vp, sz, u, u]
    Z.FSE_buildCTable_wksp.restype = sz
    Z.FSE_buildCTable_wksp.argtypes = [vp, vp, u, u, vp, sz]
    Z.FSE_buildDTable_wksp.restype = sz
    Z.FSE_buildDTable_wksp.argtypes = [vp, vp, u, u, vp, sz]
    Z.FSE_compress_usingCTable.restype = sz
    Z.FSE_compress_usingCTable.argtypes = [vp, sz, vp, sz, vp]
    Z.FSE_decompress_usingDTable.restype = sz
    Z.FSE_decompress_usingDTable.argtypes = [vp, sz, vp, sz, vp]
    Z.FSE_isError.restype = u
    Z.FSE_isError.argtypes = [sz]


def _count_vectors(rng, alpha, n):
    """Count vectors in the shapes the reference produces (all >= 1, src/fse_sequence.cpp:148-149)
    plus sparse ones with zeros, heavy skew and near-uniform cases."""
    out = []
    for k in range(n):
        kind = k % 6
        if kind == 0:
            c = np.ones(alpha, dtype=np.uint32)
        elif kind == 1:
            c = 1 + rng.integers(0, 50, alpha).astype(np.uint32)
        elif kind == 2:
            c = 1 + (rng.pareto(0.7, alpha) * 20).astype(np.uint32)
        elif kind == 3:
            c = np.ones(alpha, dtype=np.uint32)
            c[rng.integers(0, alpha)] += np.uint32(rng.integers(1, 1 << 22))
        elif kind == 4:
            c = (rng.integers(0, 3, alpha) * rng.integers(0, 4000, alpha)).astype(np.uint32)
            if np.count_nonzero(c) < 2:
                c[:2] = [3, 5]
        else:
            c = 1 + rng.integers(0, 1 << 18, alpha).astype(np.uint32)
        out.append(np.ascontiguousarray(c, dtype=np.uint32))
    return out


@pytest.mark.parametrize("alpha", [4, 64])
def test_tables_match_libzstd(alpha):
    L = O.lib()
    rng = np.random.default_rng(28 + alpha)
    wksp = np.zeros(1 << 16, dtype=np.uint8)
    n_m2 = n_low = 0
    for c in _count_vectors(rng, alpha, 1500):
        total = int(c.sum())
        if int(c.max()) == total:
            continue
        t_ref = Z.FSE_optimalTableLog(0, total, alpha - 1)
        t = L.fo_optimal_table_log(0, total, alpha - 1)
        assert t == t_ref, (c, t, t_ref)
        n_ref = np.zeros(alpha, dtype=np.int16)
        n_our = np.zeros(alpha, dtype=np.int16)
        r_ref = Z.FSE_normalizeCount(O.ptr(n_ref), t, O.ptr(c), total, alpha - 1, 1)
        assert not Z.FSE_isError(r_ref)
        r_our = L.fo_normalize_count(O.ptr(n_our), t, O.ptr(c), total, alpha - 1, 1)
        assert r_our == r_ref == t
        assert np.array_equal(n_ref, n_our), (c, n_ref, n_our)
        assert int(np.where(n_our == -1, 1, n_our).sum()) == 1 << t
        n_low += int((n_our == -1).any())

        cw = L.fo_ctable_words(t, alpha - 1)
        ct_ref = np.zeros(cw, dtype=np.uint32)
        ct_our = np.zeros(cw, dtype=np.uint32)
        assert Z.FSE_buildCTable_wksp(O.ptr(ct_ref), O.ptr(n_ref), alpha - 1, t, O.ptr(wksp), wksp.size) == 0
        assert L.fo_build_ctable(O.ptr(ct_our), O.ptr(n_our), alpha - 1, t) == 0
        assert np.array_equal(ct_ref, ct_our)

        dw = L.fo_dtable_words(t)
        dt_ref = np.zeros(dw, dtype=np.uint32)
        dt_our = np.zeros(dw, dtype=np.uint32)
        assert Z.FSE_buildDTable_wksp(O.ptr(dt_ref), O.ptr(n_ref), alpha - 1, t, O.ptr(wksp), wksp.size) == 0
        assert L.fo_build_dtable(O.ptr(dt_our), O.ptr(n_our), alpha - 1, t) == 0
        assert np.array_equal(dt_ref, dt_our)

        # bit writer + encodeSymbol + flush/close through the 2-state driver
        p = c.astype(np.float64) / total
        for n in (3, 4, 5, 6, 7, 257, 1000):
            src = rng.choice(alpha, size=n, p=p).astype(np.uint8)
            cap = n * 2 + 64
            o_ref = np.zeros(cap, dtype=np.uint8)
            o_our = np.zeros(cap, dtype=np.uint8)
            s_ref = Z.FSE_compress_usingCTable(O.ptr(o_ref), cap, O.ptr(src), n, O.ptr(ct_ref))
            s_our = L.fo_compress_using_ctable(O.ptr(o_our), cap, O.ptr(src), n, O.ptr(ct_our))
            assert s_ref == s_our and s_ref > 0
            assert np.array_equal(o_ref[:s_ref], o_our[:s_our])
            # decoder primitives: libzstd decodes ours, we decode libzstd's
            back = np.zeros(n, dtype=np.uint8)
            assert Z.FSE_decompress_usingDTable(O.ptr(back), n, O.ptr(o_our), s_our, O.ptr(dt_ref)) == n
            assert np.array_equal(back, src)
            back2 = np.zeros(n, dtype=np.uint8)
            assert L.fo_decompress_using_dtable(O.ptr(back2), n, O.ptr(o_ref), s_ref, O.ptr(dt_our)) == n
            assert np.array_equal(back2, src)
    assert n_low > 50  # the -1 (low-probability) path was exercised


def test_normalize_m2_path_matches_libzstd():
    """Count vectors that enter FSE_normalizeM2, by the classifier of tables_ref.py (which test_tables_host.py holds against
    libzstd): the `m2` families and seeded directed draws.  (Of the 4000 vectors this test drew before it counted its M2
    entries, 14 entered M2.)"""
    import tables_ref as T
    L = O.lib()
    alpha = 64
    vectors = [c for fam in ("m2", "m2_edge", "m2_second_lowone", "m2_total0") for _, c in T.shared_families(alpha)[fam]]
    vectors += T.m2_draws(1000, 7)
    hits, inner = 0, set()
    for counts in vectors:
        c = np.array(counts, dtype=np.uint32)
        total = int(c.sum())
        t = Z.FSE_optimalTableLog(0, total, alpha - 1)
        a = np.zeros(alpha, dtype=np.int16)
        b = np.zeros(alpha, dtype=np.int16)
        ra = Z.FSE_normalizeCount(O.ptr(a), t, O.ptr(c), total, alpha - 1, 1)
        rb = L.fo_normalize_count(O.ptr(b), t, O.ptr(c), total, alpha - 1, 1)
        assert not Z.FSE_isError(ra) and rb == ra == t
        assert np.array_equal(a, b), (c, a, b)
        tags = T.tags_of(counts)
        hits += "m2" in tags
        inner |= tags & set(T.M2_INNER)
    assert hits >= 1000 + 96
    assert inner == {"m2_spread", "m2_second_lowone", "m2_total0"}


def test_empty_context_quirks():
    """an empty sequence context (1,1,1,1) gets log 11 / 512 each; an
    empty quality context (64 ones) gets log 7 / 2 each."""
    L = O.lib()
    assert L.fo_optimal_table_log(0, 4, 3) == Z.FSE_optimalTableLog(0, 4, 3) == 11
    assert L.fo_optimal_table_log(0, 64, 63) == Z.FSE_optimalTableLog(0, 64, 63) == 7
    n = np.zeros(4, dtype=np.int16)
    c = np.ones(4, dtype=np.uint32)
    assert L.fo_normalize_count(O.ptr(n), 11, O.ptr(c), 4, 3, 1) == 11
    assert n.tolist() == [512] * 4
    n = np.zeros(64, dtype=np.int16)
    c = np.ones(64, dtype=np.uint32)
    assert L.fo_normalize_count(O.ptr(n), 7, O.ptr(c), 64, 63, 1) == 7
    assert n.tolist() == [2] * 64
