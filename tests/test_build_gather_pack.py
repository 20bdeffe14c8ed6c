"""What K6 (k_tile_gather_pack, enc_tile_sort.h) relies on for its speed, checked on the compiler's output (CPU only: hipcc
cross-compiles for gfx950 without a GPU): its scans are DPP adds with no LDS round trip, and two workgroups of eight waves
fit a CU (128 VGPRs, 80 KB of LDS, nothing spilled)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def encode_isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "encode.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(out), os.path.join(ROOT, "fqcomp28_amd", "csrc", "encode.hip")],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().splitlines()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("model", ["9QualModel", "8SeqModel"])
def test_gather_pack_scans_by_dpp_and_fits_two_workgroups_per_cu(encode_isa, model):
    lines = encode_isa
    start = [i for i, ln in enumerate(lines) if ln.startswith("_ZN12_GLOBAL__N_118k_tile_gather_packI" + model)]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    body = lines[start[0]:end]
    code = [ln.strip() for ln in body if ln.strip() and not ln.strip().startswith(";") and not ln.strip().startswith(".")]
    assert any(ln.startswith("s_endpgm") for ln in code)
    n_dpp = sum(ln.startswith("v_add_u32_dpp") or ln.startswith("v_mov_b32_dpp") for ln in code)
    assert n_dpp >= 6, n_dpp
    assert not [ln for ln in code if ln.startswith("ds_bpermute_b32")]
    assert not [ln for ln in code if ln.startswith("scratch_")]
    meta = "\n".join(body)
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 128
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) <= 81920
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
