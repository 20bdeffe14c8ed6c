"""`fqc_tool s --adapters` and `fqc_tool c --stats --adapters`: the adapter content of a whole file through the farm
(process.hpp), against the rendered numpy restatement (probe_ref.py) of the file behind the summary's (stats_ref.py), byte
for byte."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import adapter_ref as AR
import probe_ref as PR
import stats_ref as SR
import test_gpu_stats_farm as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import fqc_archive as A  # noqa: E402

pytestmark = pytest.mark.gpu

run_tool, run_any = SF.run_tool, SF.run_any
NAMES = [name for name, _ in PR.BUILTIN]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    if F.device_count() < 1:
        pytest.fail("no GPU visible: the product path has no CPU fallback")
    return F


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe_farm_tool") / "fqc_tool")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "fqc_tool.cpp"),
                    "-L" + os.path.join(ROOT, "fqcomp28_amd"), "-lfqgpu", "-Wl,-rpath," + os.path.join(ROOT, "fqcomp28_amd"),
                    "-lpthread"], check=True)
    return exe


def all_probes(mo=5, pct=10):
    return PR.prb([AR.adp(seq, min(mo, len(seq)), pct) for _, seq in PR.BUILTIN])


@pytest.fixture(scope="module")
def farm(F, tool, tmp_path_factory):
    """about 6 MiB of mode 4 with a built-in adapter planted in every fourth read, compressed with -R 1 -t 3: plain, with
    --stats, and with --stats --adapters all"""
    d = tmp_path_factory.mktemp("probe_farm")
    raw, _ = F.synth_fastq(6 << 20, 4, seed=41)
    raw = raw.copy()
    recs = F.parse_fastq(raw)
    rng = np.random.default_rng(41)
    for r in range(0, len(recs), 4):
        adapter = np.frombuffer(PR.BUILTIN[r // 4 % len(PR.BUILTIN)][1], dtype=np.uint8)
        L, so = int(recs["len"][r]), int(recs["seq_off"][r])
        p = int(rng.integers(0, L))
        raw[so + p:so + p + min(adapter.size, L - p)] = adapter[:min(adapter.size, L - p)]
    src = d / "in.fastq"
    raw.tofile(src)
    common = ["-t", 3, "-R", 1, "-S", 1, "--index", "--checksum"]
    plain = run_tool(tool, "c", src, d / "plain.fqc", *common)
    stats = run_tool(tool, "c", src, d / "stats.fqc", *common, "--stats", d / "stats.tsv")
    rep = run_tool(tool, "c", src, d / "probe.fqc", *common, "--stats", d / "c.tsv", "--adapters", "all")
    p = all_probes()
    words, _ = PR.probe_of(raw, recs, p, 512)
    return dict(dir=d, raw=raw, recs=recs, plain=plain, stats=stats, rep=rep, p=p, words=words,
                want=SR.render(SR.stats_of(raw, recs, 512)) + PR.render(words, p, NAMES))


def test_c_stats_adapters_reports_the_input_and_leaves_the_archive_alone(farm):
    d, rep = farm["dir"], farm["rep"]
    assert rep["blocks"] >= 5
    assert (d / "c.tsv").read_bytes() == farm["want"]
    assert not os.path.exists(str(d / "c.tsv") + ".part")
    v = PR.view(farm["words"])
    assert (v["tables"][:9, 0] > len(farm["recs"]) // 50).all(), "every built-in is found"
    assert rep["adapters"] == 9 and rep["reads_with_any"] == int(v["tables"][9, 0]) >= len(farm["recs"]) // 4
    # the archive equals the one written without the option (blocks lie in completion order: compared block by block)
    x, y = A.read_archive(str(d / "plain.fqc")), A.read_archive(str(d / "probe.fqc"))
    key = lambda p: (p.idx, p.total, p.n_records, p.seq, p.qual, p.readlens, p.n_count, p.n_pos, p.fields)  # noqa: E731
    assert x[:3] == y[:3] and [key(p) for p in x[3]] == [key(p) for p in y[3]]
    assert os.path.getsize(d / "plain.fqc") == os.path.getsize(d / "probe.fqc")
    # without --adapters the report, and the JSON line's keys, are what they were
    assert (d / "stats.tsv").read_bytes() == SR.render(SR.stats_of(farm["raw"], farm["recs"], 512))
    assert "adapters" not in farm["stats"] and "reads_with_any" not in farm["stats"] and "adapters" not in farm["plain"]
    assert set(rep) - set(farm["stats"]) == {"adapters", "reads_with_any"}


def test_s_adapters_gives_the_same_bytes_whatever_the_workers_and_the_index(tool, farm, tmp_path):
    d = farm["dir"]
    arc = tmp_path / "a.fqc"
    for ext in ("", ".fqx", ".fqs"):
        shutil.copy(str(d / "probe.fqc") + ext, str(arc) + ext)
    for with_index in (True, False):
        if not with_index:
            os.remove(str(arc) + ".fqx")
        for t in (1, 3):
            out = tmp_path / "s.tsv"
            before = sorted(os.listdir(tmp_path))
            rep = run_tool(tool, "s", arc, out, "-t", t, "--adapters", "all")
            assert out.read_bytes() == farm["want"], (with_index, t)
            assert sorted(os.listdir(tmp_path)) == sorted(before + ["s.tsv"]), "the report and nothing else"
            assert rep["index"] == ("used" if with_index else "none") and rep["sums"] == "used" and rep["verified"] == farm["rep"]["blocks"]
            assert rep["adapters"] == 9 and rep["reads_with_any"] == farm["rep"]["reads_with_any"]
            os.remove(out)
    out = tmp_path / "plain.tsv"
    rep = run_tool(tool, "s", arc, out, "-t", 3)
    assert out.read_bytes() == SR.render(SR.stats_of(farm["raw"], farm["recs"], 512)) and "adapters" not in rep


def test_names_sequences_and_the_options_for_every_probe(tool, farm, tmp_path):
    """a list of a built-in name, NAME=SEQ and a bare sequence, with --adapter-overlap, --adapter-err and --positions"""
    d = farm["dir"]
    out = tmp_path / "s.tsv"
    rep = run_tool(tool, "s", d / "probe.fqc", out, "-t", 2, "--adapters", "nextera,mine=AGATCGGAAGAGCACAC,GGGGGGGG,truseq", "--adapter-overlap", 8,
                   "--adapter-err", 20, "--positions", 40)
    seqs = [b"CTGTCTCTTATACACATCT", b"AGATCGGAAGAGCACAC", b"GGGGGGGG", b"AGATCGGAAGAGC"]
    p = PR.prb([AR.adp(s, 8, 20) for s in seqs])
    words, _ = PR.probe_of(farm["raw"], farm["recs"], p, 40)
    assert out.read_bytes() == SR.render(SR.stats_of(farm["raw"], farm["recs"], 40)) + PR.render(words, p, ["nextera", "mine", "GGGGGGGG", "truseq"])
    assert rep["adapters"] == 4 and rep["reads_with_any"] == int(PR.view(words)["tables"][4, 0])
