"""K3 (k_tile_partition, enc_tile_sort.h) fills a CU by its LDS: two workgroups of eight waves, nothing beside them, so every
wait in it is exposed -- and a third of its speed goes if only one workgroup fits.  Checked on the compiler's output (CPU
only: hipcc cross-compiles for gfx950 without a GPU): the instantiations on the fused K1's keys fit twice (128 VGPRs, 80 KB of
LDS, nothing spilled), and their entry asks for everything the tile number alone addresses before it waits for any of it."""
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


def _kernel(lines, model):
    start = [i for i, ln in enumerate(lines) if ln.startswith("_ZN12_GLOBAL__N_116k_tile_partitionI" + model + "Lb1E")]
    assert len(start) == 1, start
    end = next(i for i in range(start[0], len(lines)) if ".end_amdhsa_kernel" in lines[i])
    return lines[start[0]:end]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("model", ["9QualModel", "8SeqModel"])
def test_partition_on_derived_keys_fits_two_workgroups_per_cu(encode_isa, model):
    body = _kernel(encode_isa, model)
    code = [ln.strip() for ln in body if ln.strip() and not ln.strip().startswith(";") and not ln.strip().startswith(".")]
    assert any(ln.startswith("s_endpgm") for ln in code)
    assert not [ln for ln in code if ln.startswith("scratch_")]
    meta = "\n".join(body)
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", meta).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", meta).group(1)) <= 81920
    assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 128


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("model,n_loads", [("9QualModel", 9), ("8SeqModel", 8)])
def test_partition_entry_requests_everything_before_it_waits(encode_isa, model, n_loads):
    """The tile's first record, the histogram row, batch 0 and batch 1 are in flight together: no wait for global memory
    in front of the last of these loads (a branch around one of them makes hipcc wait on the spot)."""
    code = [ln.strip() for ln in _kernel(encode_isa, model) if ln.strip() and not ln.strip().startswith(";")]
    loads = [i for i, ln in enumerate(code) if ln.startswith("global_load_")]
    assert len(loads) > n_loads
    head = code[:loads[n_loads - 1]]
    assert not [ln for ln in head if "vmcnt" in ln], [ln for ln in head if "vmcnt" in ln]
    assert not [ln for ln in head if ln.startswith("s_barrier")]
