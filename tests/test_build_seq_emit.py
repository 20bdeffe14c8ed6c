"""What k_seq_emit (enc_chains_seq.h) may cost, checked on the compiler's output (CPU only: hipcc cross-compiles for gfx950
without a GPU).  A lane walks one segment; a lone wave issues one instruction per four cycles, so what the loop holds is
what the kernel takes.  A round of the main loop is 64 symbols: one ds_read_u16 of next1[s][x] per symbol and no branch;
the symbols of the next round are asked for in front of the walk and waited for behind it; the round's 128 bytes of out16
leave with eight stores in a row that the main loop never waits for (its only waits for memory stand behind the stores
and leave them in flight).  Nothing is spilled, and the kernel has no LDS beside the dynamic
block of its launch, the context's one-symbol table: 16 KB at log 11, below the 20 KB stated here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fqcomp28_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LDS_BOUND = 20 * 1024   # per workgroup at log 11, the largest table of the two-symbol path
PER_SYMBOL = 22         # instructions of a round per symbol (parent: some 30 and a branch)
STORES = ("global_store", "flat_store", "buffer_store", "scratch_store", "global_atomic", "flat_atomic")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def emit(tmp_path_factory):
    """(instructions and labels of k_seq_emit, its kernel descriptor)"""
    out = tmp_path_factory.mktemp("isa") / "encode.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "encode.hip")],
                   check=True, capture_output=True, timeout=900)
    lines = out.read_text().splitlines()
    start = [i for i, ln in enumerate(lines) if re.match(r"_ZN\S*10k_seq_emitE\S*:", ln)]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    body = [ln.strip() for ln in lines[start[0]:end]]
    code = [ln for ln in body if ln and not ln.startswith(";") and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln))]
    return code, "\n".join(body)


def _loops(code):
    """innermost loops: from a label to the first branch back to it, no other label in between"""
    at = {ln.split(":")[0]: i for i, ln in enumerate(code) if ln.startswith(".LBB")}
    loops = []
    for i, ln in enumerate(code):
        m = re.match(r"s_cbranch_\w+ (\.LBB\d+_\d+)$", ln)
        if m and m.group(1) in at and at[m.group(1)] < i:
            inner = code[at[m.group(1)] + 1: i]
            if not any(x.startswith(".LBB") for x in inner):
                loops.append(inner)
    return loops


def test_emit_spills_nothing_and_has_no_static_lds(emit):
    code, meta = emit
    assert any(ln.startswith("s_endpgm") for ln in code)
    assert not [ln for ln in code if ln.startswith("scratch_")]
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0
    assert not [ln for ln in code if ln.startswith("s_barrier")]   # one wave: nothing to wait for


def test_emit_launch_asks_for_the_table_alone():
    """the dynamic LDS of the launch, evaluated: the one-symbol table next1[4][2^log] of u16, for the log of the two-symbol
    path (11) and for the largest a sequence table can have (12)"""
    src = open(os.path.join(CSRC, "encode.hip")).read()
    m = re.search(r"hipLaunchKernelGGL\(\s*k_seq_emit\s*,\s*dim3\(([^)]*)\)\s*,\s*dim3\(([^)]*)\)\s*,\s*([^,]+?)\s*,\s*st\s*,", src)
    assert m, "k_seq_emit's launch not found"
    assert m.group(2).strip() == "64"
    assert re.search(r"const unsigned log_size = 1u << tab\.max_log;", src)
    lds = lambda log: eval(m.group(3), {"__builtins__": {}}, {"log_size": 1 << log})
    assert lds(11) == 4 * 2048 * 2 and lds(11) < LDS_BOUND
    assert lds(12) == 4 * 4096 * 2 and lds(12) < 2 * LDS_BOUND


def _store_loops(code):
    return [lp for lp in _loops(code) if any(ln.startswith("global_store_dwordx4") for ln in lp)]


def test_a_round_is_64_symbols_one_lds_read_each_and_no_branch(emit):
    code, _ = emit
    loops = _store_loops(code)
    assert len(loops) == 2, [len(lp) for lp in loops]   # whole rounds; the groups of 16 at the end of a chain's last segment
    main, tail = max(loops, key=len), min(loops, key=len)
    for lp, symbols in ((main, 64), (tail, 16)):
        assert sum(ln.startswith("ds_read_u16") for ln in lp) == symbols               # exactly one LDS read per symbol
        assert not [ln for ln in lp if ln.startswith("ds_") and not ln.startswith("ds_read_u16")]
        assert sum(ln.startswith("global_load_dwordx4") for ln in lp) * 16 == symbols
        assert sum(ln.startswith("global_store_dwordx4") for ln in lp) * 8 == symbols
        assert not [ln for ln in lp if ln.startswith(("s_cbranch", "s_branch"))]       # the symbol's deltaNbBits: selects
    assert len(main) <= 64 * PER_SYMBOL, len(main)


def test_a_round_stores_a_whole_line_and_never_waits_for_it(emit):
    """the loop asks for the next 64 symbols first and stores behind the walk, eight stores in a row.  Loads and stores
    share one counter on gfx9, so the stores stay in flight only if NO wait for memory stands between the loads and the
    first store (with eight stores and four loads outstanding any wait below vmcnt(12) there would drain the stores), and
    the waits for the next symbols behind the stores leave eight operations in flight.  That needs the loop to be entered
    with nothing pending: the kernel uses its first symbols and its entry state in front of the loop."""
    code, _ = emit
    lp = max(_store_loops(code), key=len)
    stores = [i for i, ln in enumerate(lp) if ln.startswith("global_store_dwordx4")]
    loads = [i for i, ln in enumerate(lp) if ln.startswith("global_load_dwordx4")]
    first_read = next(i for i, ln in enumerate(lp) if ln.startswith("ds_read_u16"))
    assert len(stores) == 8 and stores[-1] - stores[0] == 7, stores
    assert max(loads) < first_read, (loads, first_read)
    assert not [ln for ln in lp[:stores[0]] if "vmcnt" in ln], "a wait for memory in front of the stores drains the round before's"
    count = lambda ln: int(re.search(r"vmcnt\((\d+)\)", ln).group(1))
    behind = [count(ln) for ln in lp[stores[-1]:] if "vmcnt" in ln]
    assert behind and min(behind) == 8, behind
