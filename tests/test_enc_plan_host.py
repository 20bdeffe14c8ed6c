"""The encoder's scratch plan (fqcomp28_amd/csrc/enc_plan.h) on the host: sizes, offsets, alignment.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_sizes_and_offsets_are_the_recorded_ones(tmp_path):
    """tests/cpp/enc_plan_check.cpp builds an EncPlan and an EncLanePlan for every row of tests/cpp/enc_plan_table.inc and
    asserts that every derived size, every buffer's byte size and every sub-array offset equals the row, that the sub-arrays
    the recorded code kept 16-byte aligned (the kernels load them as 16-byte vectors) are so aligned, and that the sub-arrays of one
    buffer do not overlap and end inside the reserved size.  Built with -fsanitize=address,undefined: nothing may be
    computed in 32 bits that overflows there (the largest n_sym is 0xFFEFFFFF, the largest block the API takes).

    Where the table comes from: it was printed once by a throwaway program holding the expressions of encode_stream and
    fq_encode_launch as they stood in the commit before the plan existed (one 350-line function that sized, carved and
    launched), so the plan is pinned to what that code allocated, byte for byte, `+ 64` paddings included.  Rows: n_sym in
    {1, 32767, 32768, 32769, 4 Mi - 1, 4 Mi, 24 Mi, 48 Mi, 0xFFEFFFFF} on each of the five paths (sequence: tile + chains,
    batch-sorted + chains, slots + generic; quality: tile, slots), with R in {1, 1000}, seg_len in {0, 2, 100000},
    seq_segment in {0, 1024}, the hand-over cap in {0, 16, 32, 64} and max_log in {11, 12} rotating through them; the program
    itself checks that every value, and every hand-over width, is met."""
    exe = str(tmp_path / "enc_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(ROOT, "tests", "cpp", "enc_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.splitlines()[-1] == "45 rows, 0 failures", r.stdout[-2000:]
