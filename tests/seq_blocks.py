"""Synthetic blocks whose bases follow a chosen pattern, each with its own tables and the CPU oracle's encoding of it:
shared by the tests of the sequence chains (tests/test_gpu_seq_handover.py, tests/test_gpu_scratch_history.py)."""
import functools

import numpy as np

import oracle_lib as O


def _rewrite_bases(raw, recs, make):
    """the block with its bases replaced by make(n) -> codes 0..3 (A, C, G, T)"""
    raw = raw.copy()
    lens = recs["len"].astype(np.int64)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[make(int(lens.sum()))]
    at = 0
    for off, ln in zip(recs["seq_off"].astype(np.int64), lens):
        raw[off: off + ln] = letters[at: at + ln]
        at += ln
    return raw


def _markov(rng, n):  # 70 %: repeat the previous base, else a fresh uniform one
    fresh = rng.integers(0, 4, size=n)
    keep = rng.random(n) < 0.7
    keep[0] = False
    return fresh[np.maximum.accumulate(np.where(keep, 0, np.arange(n)))]


def _half_all_a(rng, recs, n):  # first half of the reads all A, the rest uniform
    out = rng.integers(0, 4, size=n)
    out[: int(recs["len"][: len(recs) // 2].sum())] = 0
    return out


MAKERS = {
    "skewed": lambda rng, recs, n: rng.choice(4, size=n, p=[0.55, 0.05, 0.1, 0.3]),
    "markov": lambda rng, recs, n: _markov(rng, n),
    "all_A": lambda rng, recs, n: np.zeros(n, dtype=np.int64),
    "mostly_A": lambda rng, recs, n: rng.choice(4, size=n, p=[0.997, 0.001, 0.001, 0.001]),
    "mixed": _half_all_a,
    "two_letters": lambda rng, recs, n: rng.choice(4, size=n, p=[0.6, 0.4, 0.0, 0.0]),
}


@functools.lru_cache(maxsize=None)
def block(bases, size=6 << 20):
    """(raw, recs, sft, qft, the oracle's encoding): computed once per shape of the bases, shared by every case"""
    import fqcomp28_amd as F
    raw, n = F.synth_fastq(size, 2, seed=28)
    recs = F.parse_fastq(raw)
    assert len(recs) == n
    if bases != "uniform":
        rng = np.random.default_rng(5)
        raw = _rewrite_bases(raw, recs, lambda m: MAKERS[bases](rng, recs, m))
    _, _, sft, qft = O.freq_tables(raw, recs)
    want = O.OracleCtx(sft, qft).encode(raw, recs)
    assert want["rc"] == 0
    for a in (raw, recs):
        a.setflags(write=False)
    return raw, recs, sft, qft, want
