"""The reference of the device parser's tests (parse_ref.py) and its inputs, judged before they judge a kernel: on every
generated case the line-by-line restatement agrees with the host parser (fqgpu_parse_fastq) and, where it is built, with
the reference's compiled FastqReader::parseRecords (oracle/_ref/ref_tool_asan).  Generating the cases runs the
generator's own assertions that each case has the property it is named for.  No GPU."""
import os

import numpy as np
import pytest

import parse_ref as P
import ref_pin as R

TOOL = R.REF_TOOL_ASAN


all_cases, reference, names_of = P.shared_cases, P.reference, P.names_of
FAMILIES = list(P.FAMILIES)


def test_cases_are_deterministic_and_their_names_unique():
    a, b = P.cases(), all_cases()
    assert list(a) == list(b) and all(a[k] == b[k] for k in a)
    assert len(set(a)) == len(a) and {P.family(k) for k in a} == set(FAMILIES)
    assert P.MANY in a and set(P.PARSE_ONLY) <= set(a)
    # every family the tests name is there, in the numbers the generator is written for
    count = {f: len(names_of(f)) for f in FAMILIES}
    assert count["boundary"] == 64 and count["ends"] == len(P.END_SIZES) and count["defect"] == 37, count
    for k, raw in a.items():
        assert k == P.MANY or P.family(k) == "sparse" or len(raw) <= 80000, (k, len(raw))


def test_every_verdict_is_met():
    verdicts = {reference(k)[0] for k in all_cases()} | {P.parse(b"@r\nACGT\n+\n")[0], P.parse(b"")[0]}
    assert verdicts == {"ok", "format", "short", "empty"}


def test_reference_on_inputs_worked_out_by_hand():
    assert P.parse(b"@r\nACGT\n+\nIIII\n")[1:] == (np.array([(3, 10, 4)], dtype=P.REC_DTYPE), 15, 4, 0)
    v, recs, used, n_bases, n_n = P.parse(b"@N\nNACN\n+N\nNIII\n@r\nAC")
    assert (v, recs.tolist(), used, n_bases, n_n) == ("ok", [(3, 11, 4)], 16, 4, 2)   # N's of the sequence line only
    for raw, verdict in ((b"@r\nACGT\n-\nIIII\n", "format"), (b"@r\nACGT\n+\nIII\n", "format"), (b"r\nACGT\n+\nIIII\n", "format"),
                         (b"@r\nAC\n+\nII\n", "short"), (b"@r\nAC\n+\nI\n", "format"), (b"no newline", "empty"),
                         (b"\n\n\n\n", "format"), (b"@\n\n+\n\n", "short"), (b"@r\nACGT\n+\nIIII", "empty")):
        assert P.parse(raw)[0] == verdict, raw


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_against_the_host_parser(family):
    import fqcomp28_amd as F
    for name in names_of(family):
        raw = np.frombuffer(all_cases()[name], dtype=np.uint8)
        verdict, recs, used, n_bases, _ = reference(name)
        if verdict == "format":
            with pytest.raises(F.FqgpuError) as ei:
                F.parse_fastq(raw)
            assert ei.value.code == -4, name
            continue
        got = F.parse_fastq(raw)
        assert got.dtype == recs.dtype and np.array_equal(got, recs), name
        if verdict == "empty":
            assert len(got) == 0 and used == 0, name
        else:
            assert used == int(got[-1]["qual_off"]) + int(got[-1]["len"]) + 1 and n_bases == int(got["len"].sum()), name


needs_ref_tool = pytest.mark.skipif(not os.path.exists(TOOL) and not R.reference_tree_present(),
                                    reason="neither oracle/_ref/ref_tool_asan nor the reference tree it is built from is here")


@needs_ref_tool
@pytest.mark.parametrize("family", FAMILIES)
def test_reference_against_the_compiled_reference(family, tmp_path):
    """FastqReader::parseRecords itself on every case it takes: the table, the header lines and where the cut-off record
    starts"""
    assert os.path.exists(TOOL), "oracle/_ref/ref_tool_asan is missing: run build() (make -C oracle) where the reference tree is"
    seen = 0
    for name in names_of(family):
        verdict, recs, used, _, _ = reference(name)
        if verdict not in ("ok", "short"):   # (a short read is the library's refusal, not the reference parser's)
            continue
        seen += 1
        table, ref_used = R.parse(TOOL, np.frombuffer(all_cases()[name], dtype=np.uint8), tmp_path)
        assert len(table) == len(recs) and ref_used == used, name
        for k in ("seq_off", "qual_off", "len"):
            assert np.array_equal(table[k], recs[k]), (name, k)
        ends = recs["qual_off"].astype(np.int64) + recs["len"] + 1
        hdr_off = np.concatenate(([0], ends[:-1]))
        assert np.array_equal(table["hdr_off"], hdr_off) and np.array_equal(table["hdr_len"], recs["seq_off"] - 1 - hdr_off), name
    assert seen
