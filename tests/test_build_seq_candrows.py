"""The walk loop of k_seq_candwalk (enc_chains_seq.h) on the compiler's output (CPU only: hipcc cross-compiles for gfx950
without a GPU).  A row of 16 lanes gets its table row by DPP broadcast, as a modifier of the add in front of every gather:
row_newbcast is there, nothing picks a slot's symbols with v_readlane between the gathers, and what the kernel may take of
a CU stays what tests/test_build_seq_candwalk.py allows -- 64 VGPRs, no scratch, no static LDS (the launch's dynamic block is
the table alone: that file reads it)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "fqcomp28_amd", "csrc")


@pytest.fixture(scope="module")
def encode_isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "encode.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(out), os.path.join(CSRC, "encode.hip")],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().splitlines()


def _kernel(lines, slots):
    start = [i for i, ln in enumerate(lines) if ln.startswith("_ZN12_GLOBAL__N_114k_seq_candwalkILj%dEEE" % slots)]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    body = lines[start[0]:end]
    code = [ln.strip() for ln in body if ln.strip() and not ln.strip().startswith(";") and not ln.strip().startswith(".")]
    return code, "\n".join(body)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("slots", [16, 32, 64])
def test_walk_loop_is_fed_by_row_broadcast(encode_isa, slots):
    code, meta = _kernel(encode_isa, slots)
    # the gathers of the walk: a ds_read_u16 whose address the instruction before it (waits and nops aside) made by a DPP add
    ops = [ln for ln in code if not ln.startswith(("s_waitcnt", "s_nop"))]
    walk = [i for i, ln in enumerate(ops) if ln.startswith("ds_read_u16") and "row_newbcast" in ops[i - 1]]
    assert len(walk) == 128, len(walk)  # 16 lanes of a row x 8 symbol pairs each, unrolled
    for n in range(16):  # every lane of the row is broadcast, eight times
        assert sum(("row_newbcast:%d " % n) in ops[i - 1] for i in walk) == 8, n
    loop = ops[walk[0] - 1: walk[-1] + 1]
    assert not [ln for ln in loop if ln.startswith("v_readlane_b32")]
    assert not [ln for ln in loop if ln.startswith(("v_cndmask", "s_barrier"))]
    # one VALU instruction per gather and the lane's eight table rows unpacked beside them: the design's 1.4 per gather
    valu = [ln for ln in loop if ln.startswith("v_")]
    assert len(valu) <= int(128 * 1.4), len(valu)
    assert not [ln for ln in code if ln.startswith("scratch_")]
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 64
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0

