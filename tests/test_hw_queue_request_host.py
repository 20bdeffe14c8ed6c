"""The library's load-time constructor (api.hip, fq_ask_for_hw_queues) and GPU_MAX_HW_QUEUES: a count below 16 is raised
to 16, a count of 16 or more and a value that is no number stay, nothing above 16 is ever written, and
FQGPU_KEEP_HW_QUEUES=1 leaves the environment alone.  Each case loads libfqgpu.so with ctypes in a FRESH process and reads
the variable back through libc's getenv: os.environ does not see a setenv from C.  No GPU: loading the library does not
initialise HIP."""
import os
import subprocess
import sys

import pytest

import fqcomp28_amd as F

CHILD = r"""
import ctypes, sys
libc = ctypes.CDLL(None)
libc.getenv.restype = ctypes.c_char_p
before = libc.getenv(b"GPU_MAX_HW_QUEUES")
ctypes.CDLL(sys.argv[1])
after = libc.getenv(b"GPU_MAX_HW_QUEUES")
print("BEFORE %r AFTER %r" % (before, after))
"""

# (GPU_MAX_HW_QUEUES before the load or None, FQGPU_KEEP_HW_QUEUES or None, expected after)
CASES = [
    pytest.param(None, None, "16", id="unset"),
    pytest.param("1", None, "16", id="1"),
    pytest.param("4", None, "16", id="4"),
    pytest.param("15", None, "16", id="15"),
    pytest.param("16", None, "16", id="16"),
    pytest.param("24", None, "24", id="24"),
    pytest.param("32", None, "32", id="32"),
    pytest.param("abc", None, "abc", id="abc"),
    pytest.param("4", "1", "4", id="4_keep"),
]


@pytest.mark.parametrize("before, keep, after", CASES)
def test_queue_count_after_loading_the_library(before, keep, after):
    assert os.path.exists(F.lib_path()), "libfqgpu.so has not been built"
    env = {k: v for k, v in os.environ.items() if k not in ("GPU_MAX_HW_QUEUES", "FQGPU_KEEP_HW_QUEUES")}
    if before is not None:
        env["GPU_MAX_HW_QUEUES"] = before
    if keep is not None:
        env["FQGPU_KEEP_HW_QUEUES"] = keep
    out = subprocess.run([sys.executable, "-c", CHILD, F.lib_path()], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    want_before = "None" if before is None else repr(before.encode())
    assert out.stdout.strip() == "BEFORE %s AFTER %r" % (want_before, after.encode()), out.stdout
