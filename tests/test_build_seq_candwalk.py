"""What k_seq_candwalk (enc_chains_seq.h) is allowed to take of a CU, checked on the compiler's output (CPU only: hipcc
cross-compiles for gfx950 without a GPU).  It runs while the other lanes' K3 and K6 workgroups want room: at most 64 VGPRs,
nothing spilled, and no LDS of its own beside the dynamic block that encode.hip gives it -- the context's two-symbol table,
64 KB at log 11, at LDS address 0 (its gathers add nothing for a base) -- which stays below 163 840 - 77 888 (K6) bytes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
LDS_BUDGET = 163840 - 77888  # a CU's LDS less one K6 workgroup


@pytest.fixture(scope="module")
def encode_isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "encode.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-I" + os.path.join(ROOT, "include"), "-o", str(out), os.path.join(ROOT, "fqcomp28_amd", "csrc", "encode.hip")],
                   check=True, capture_output=True, timeout=900)
    return out.read_text().splitlines()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("slots", [16, 32, 64])
def test_candwalk_fits_beside_a_tile_workgroup(encode_isa, slots):
    lines = encode_isa
    start = [i for i, ln in enumerate(lines) if ln.startswith("_ZN12_GLOBAL__N_114k_seq_candwalkILj%dEEE" % slots)]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    body = lines[start[0]:end]
    code = [ln.strip() for ln in body if ln.strip() and not ln.strip().startswith(";") and not ln.strip().startswith(".")]
    assert any(ln.startswith("s_endpgm") for ln in code)
    assert sum(ln.startswith("ds_read_u16") for ln in code) >= 8       # the walk gathers from LDS ...
    assert not [ln for ln in code if ln.startswith("scratch_")]        # ... and nothing goes to scratch
    meta = "\n".join(body)
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 64
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    # no static LDS: the dynamic block starts at address 0 and is the table alone
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) == 0


def test_candwalk_launch_asks_for_the_table_alone():
    """the dynamic LDS of the launch: 16 rows of 2^log u16 entries, log <= 11 on this path"""
    src = open(os.path.join(ROOT, "fqcomp28_amd", "csrc", "encode.hip")).read()
    m = re.search(r"const unsigned clds = (\d+)u << tab\.max_log;", src)
    assert m, "k_seq_candwalk's launch not found"
    assert (int(m.group(1)) << 11) <= LDS_BUDGET
