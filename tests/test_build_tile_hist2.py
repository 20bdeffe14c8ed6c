"""What K1 (k_tile_hist2, enc_records_hist.h) relies on for its place on a CU, checked on the compiler's output (CPU only:
hipcc cross-compiles for gfx950 without a GPU): five waves per SIMD or more (96 VGPRs at most), nothing in scratch, a
workgroup's LDS small enough to sit beside k_seq_setfunc's 118 KB, and no scalar register spilled to the lanes of a
vector register.  Nothing else about the instruction mix: the counters decide that."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def k1_isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "encode.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(out), os.path.join(ROOT, "fqcomp28_amd", "csrc", "encode.hip")],
                   check=True, capture_output=True, timeout=900)
    lines = out.read_text().splitlines()
    start = [i for i, ln in enumerate(lines) if ln.startswith("_ZN12_GLOBAL__N_112k_tile_hist2")]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    return lines[start[0]:end]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_tile_hist2_registers_lds_and_no_spills(k1_isa):
    code = [ln.strip() for ln in k1_isa if ln.strip() and not ln.strip().startswith(";") and not ln.strip().startswith(".")]
    assert any(ln.startswith("s_endpgm") for ln in code)
    meta = "\n".join(k1_isa)
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 96
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) <= 40960
    assert not [ln for ln in code if ln.startswith("scratch_")]
    assert not [ln for ln in code if ln.startswith("v_writelane_b32")]
