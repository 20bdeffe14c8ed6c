"""The block-decoder families of tests/decode_ref.py on the CPU: the generator's own property asserts run (a family that
has drifted off its edge fails here, without a GPU), every case is coded by the oracle and decoded back to the input, and
where oracle/_ref/ref_tool is built the reference's compiled decoder (DecompressionWorkspace::decodeChunk) restores the
same streams to the same bytes and judges the damaged ones as the oracle does.
tests/test_gpu_decode_families.py holds the device decoder to the same cases."""
import os

import numpy as np
import pytest

import decode_ref as D
import oracle_lib as O
import ref_pin as R

CASES = D.families()
GOOD = [c for c in CASES if c.kind == "ok"]
DAMAGED = [c for c in CASES if c.kind == "damage"]

needs_ref_tool = pytest.mark.skipif(not os.path.exists(R.REF_TOOL) or not os.path.exists(R.REF_TOOL_ASAN),
                                    reason="oracle/_ref/ref_tool is not built (no reference tree where build() ran)")


def ids(cases):
    return [D.case_id(c) for c in cases]


def verdict(case):
    """the oracle's: ("refused", None) or ("same" | "other", the restored bytes)"""
    rc, out = D.oracle_decode(case)
    if rc != 0:
        return "refused", None
    return ("same" if np.array_equal(out, case.raw) else "other"), out


def test_every_family_is_there_and_names_its_cases_once():
    assert [f.__name__ for f in D.FAMILIES] == ["_lengths", "_runs", "_window", "_n", "_strides"]
    assert {c.family for c in CASES} == {"lengths", "runs", "window", "n", "strides", "damage"}
    assert len(set(ids(CASES))) == len(CASES)
    # (the property asserts of every family ran when D.families() was made, at import)
    small = [c for c in GOOD if c.family not in ("strides",) and str(D.LONGEST) not in c.name]
    # (the largest of the rest: six lengths of 1 Ki at four alignments each, and the 2 x FQ_BITBUF_DW dwords of sequence stream)
    assert max(c.raw.size for c in small) <= 50 << 10, "only strides and the 65535-base reads exceed a few tens of KiB"


def test_the_model_restated_is_the_oracles():
    """contexts(): the contexts the oracle's count pass files a block's symbols under are the restated ones"""
    case = next(c for c in GOOD if c.name == "inserted-1-to-12-at-0-to-3-own-tables")
    sc, qc, _, _ = O.freq_tables(case.raw, case.recs)
    want_s, want_q = np.ones_like(sc), np.ones_like(qc)  # (the reference starts every count at one)
    b = case.raw.tobytes()
    assert b"N" not in b  # (the count pass does not advance the context over an N; the coder codes an A)
    for r in case.recs:
        s, q, n = int(r["seq_off"]), int(r["qual_off"]), int(r["len"])
        syms = D.symbols_of(b[s: s + n], b[q: q + n])
        for c, x in zip(D.contexts(syms[0], 0), syms[0]):
            want_s[c][x] += 1
        for c, x in zip(D.contexts(syms[1], 1), syms[1]):
            want_q[c][x] += 1
    assert np.array_equal(sc, want_s) and np.array_equal(qc, want_q)


@pytest.mark.parametrize("case", GOOD, ids=ids(GOOD))
def test_the_oracle_codes_and_restores_every_case(case):
    e = D.coded(case)
    assert e["rc"] == 0
    assert e["readlens"].tolist() == case.recs["len"].tolist()
    rc, out = D.oracle_decode(case)
    assert rc == 0 and out.tobytes() == case.raw.tobytes()


def test_damage_gives_refusals_and_streams_accepted_with_other_bytes():
    got = {}
    for c in DAMAGED:
        got.setdefault(verdict(c)[0], []).append(D.case_id(c))
    assert got.get("refused") and got.get("other"), {k: len(v) for k, v in got.items()}
    assert len(DAMAGED) == 2 * len(D.DAMAGE) * len(D.DAMAGE_BASES), "every damage on either stream of every base"
    assert {c.extra["base"].family for c in DAMAGED} == {"lengths", "runs", "window", "n", "strides"}
    # the three ways a stream is refused before its walk starts or while it runs: no end mark, an end mark below the
    # state flush (open_at_end), bits left over or invented (the rest)
    how = set()
    for c in DAMAGED:
        stream = c.extra["damage"][0]
        b = D.coded(c)[("seq", "qual")[stream]].tobytes()
        if not b or not b[-1]:
            how.add("no-end-mark")
        elif D.payload_bits(b, D.case_tables(c)[stream]) < 0:
            how.add("mark-below-the-state-flush")
        elif verdict(c)[0] == "refused":
            how.add("bits-left-or-invented")
    assert how == {"no-end-mark", "mark-below-the-state-flush", "bits-left-or-invented"}, how
    for c in DAMAGED:  # the damage is there: the stream differs from the base's, the other stream does not
        stream = c.extra["damage"][0]
        e, base = D.coded(c), D.coded(c.extra["base"])
        k, other = ("seq", "qual")[stream], ("qual", "seq")[stream]
        assert e[k].tobytes() != base[k].tobytes() and e[other].tobytes() == base[other].tobytes(), D.case_id(c)


def _ref_dir(case, tmp_path):
    hdrs = R.headers_of(case.raw, case.recs)
    _, _, fields = R.oracle_fields(hdrs)
    sft, qft = D.case_tables(case)
    return R.write_encoded(R.fresh_dir(tmp_path, "from_oracle"), hdrs[0], sft, qft, D.coded(case), fields, case.raw.size, len(case.recs))


@needs_ref_tool
@pytest.mark.parametrize("case", GOOD, ids=ids(GOOD))
def test_the_references_decoder_restores_the_oracles_streams(case, tmp_path):
    assert R.decode(R.REF_TOOL, _ref_dir(case, tmp_path)).tobytes() == case.raw.tobytes()


@needs_ref_tool
@pytest.mark.parametrize("case", DAMAGED, ids=ids(DAMAGED))
def test_the_references_decoder_judges_damage_as_the_oracle_does(case, tmp_path):
    """Comparable are: a refusal of the reference (its one assert on the way, the size BIT_initDStream returns: a last byte
    without an end mark) -- the oracle refuses too --, and a stream both restore -- to the same bytes.  Not comparable is a
    stream the oracle refuses for bits left over or invented: DecompressionWorkspace::decodeChunk never calls the decoders'
    endChunk (the assert on BIT_endOfDStream), so the reference restores whatever the walk gives.  Under AddressSanitizer,
    so that a verdict reached by reading outside a buffer is a failure and not a verdict."""
    what, want = verdict(case)
    try:
        got = R.decode(R.REF_TOOL_ASAN, _ref_dir(case, tmp_path))
    except R.Refused:
        got = None
    if case.extra["damage"][1] == "last-byte-zero":
        assert got is None and what == "refused", "no end mark: both refuse"
    if got is None:
        assert what == "refused", "the reference refuses, the oracle restores"
    elif what != "refused":
        assert got.tobytes() == want.tobytes()
