"""The cases of tests/chain_ref.py on the CPU: every family's own assert (made while the cases are generated), the oracle
codes and restores every block, and the restatement is held against second statements of the same rules -- `classify`
against a loop over single symbols, `set_sizes` and the chain's final state against single states stepped on Python ints
and against the state flush of the oracle's C coder, the premise of anchored segments against every crafted table.  One
test looks over all cases for the (predecessor class, class) pairs and the routes they reach.  Where oracle/_ref/ref_tool
is built the reference's compiled encoder gives the oracle's bytes on every case.
tests/test_gpu_chain_families.py holds the device's chain kernels to the same cases."""
import os

import numpy as np
import pytest

import chain_ref as C
import ref_pin as R

CASES = C.families()
QUAL = [c for c in CASES if c.family in C.QUAL_FAMILIES]
needs_ref_tool = pytest.mark.skipif(not os.path.exists(R.REF_TOOL), reason="oracle/_ref/ref_tool is not built (no reference tree where build() ran)")
WALK_LIMIT = 1 << 18   # contexts up to this many symbols are walked state by state on Python ints: all there are


def ids(cases):
    return [C.case_id(c) for c in cases]


def test_the_families_are_there():
    assert {c.family for c in CASES} == set(C.QUAL_FAMILIES) | {"seq-generic"}
    assert all(c.raw.size <= C.MAX_FASTQ for c in CASES)
    assert C._opaque.found == ["above-512-through-3-stops", "level1-at-stop-0", "never-512", "walk-1", "walk-2", "walk-8"], C._opaque.found
    assert C._opaque.tried <= C.OPAQUE_SEARCH


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_the_oracle_codes_and_restores(case):
    e = C.coded(case)
    assert e["rc"] == 0
    rc, out = C.oracle_decode(case)
    assert rc == 0 and out.tobytes() == case.raw.tobytes()


def classify_by_symbol(run, norm_row, S):
    """k_seg_scan's rules, one symbol at a time -> per segment (1, offset), (cells, offset), ("asks", symbol) or (0, none)"""
    out = []
    run = [int(v) for v in run]
    for begin in range(0, len(run), S):
        seg = run[begin: begin + S]
        verdict, fewest, same = None, None, True
        for off, s in enumerate(seg):
            n = int(norm_row[s])
            if n == 1 or n == -1:
                verdict = (1, off)
                break
            if 2 <= n <= 64 and (fewest is None or n < fewest[0]):
                fewest = (n, off)
            same = same and s == seg[0]
        if verdict is None:
            if fewest is not None:
                verdict = fewest
            elif same and len(seg) == S:
                verdict = ("asks", seg[0])
            else:
                verdict = (C.OPAQUE, C.SEG_NONE)
        out.append(verdict)
    return out


@pytest.mark.parametrize("case", QUAL, ids=ids(QUAL))
def test_classify_agrees_with_a_loop_over_single_symbols(case):
    qft, S = C.tables(case.tables)[1], case.extra["S"]
    targets = {C.target(a) for a in case.extra["chains"]}
    for c, run in C.runs(case.raw, case.recs).items():
        if c not in targets:
            run = run[: 2 * S + 7]   # (the side contexts: n times one reset symbol)
        loop = classify_by_symbol(run, qft["norm"][0][c], S)
        alts = C.classify(run, C.cells(qft, c), S)
        askers = sorted({v[1] for v in loop if v[0] == "asks"})
        assert len(alts) == max(len(askers), 1), (c, askers)
        for winner, alt in zip(askers or [None], alts):
            want = [((C.UNIFORM, v[1]) if v[1] == winner else (C.OPAQUE, C.SEG_NONE)) if v[0] == "asks" else v for v in loop]
            assert alt == want, (c, winner)


def crafted_contexts():
    return [(a, C.target(a)) for a in sorted(C.ROWS)]


def test_behind_an_anchor_symbol_of_n_cells_the_state_is_one_of_exactly_n():
    """the premise of anchored segments, on every table the families craft: from all 2^log states"""
    for key in ("main",):
        qft = C.tables(key)[1]
        checked = 0
        for c in [t for _, t in crafted_contexts()] + [0, 4096, 8191]:
            ct = C.ctable(qft, c)
            size = 1 << ct[0]
            cell = C.cells(qft, c)
            for s in np.flatnonzero(cell <= C.MAX_CAND):
                after = C.step_all(ct, np.arange(size, 2 * size, dtype=np.int64), int(s))
                assert len(np.unique(after)) == int(cell[s]), (c, int(s))
                checked += 1
        assert checked > 400


def test_set_sizes_agrees_with_single_states_stepped_on_python_ints():
    """the numpy step over all states against FSE_encodeSymbol's state change on one Python int at a time: the states single
    entry states reach lie in the set at every stop, and all entry states together (small tables) ARE the set"""
    qft = C.tables("main")[1]
    rng = np.random.default_rng(5)
    for a, c in crafted_contexts():
        ct = C.ctable(qft, c)
        size = 1 << ct[0]
        big = [int(s) for s in np.flatnonzero(qft["norm"][0][c] != 0)]
        run = np.array(big, dtype=np.uint8)[rng.integers(0, len(big), size=600)]
        sizes = C.set_sizes(ct, run)
        assert len(sizes) == 5
        entries = range(size, 2 * size) if size <= 128 else [size, 2 * size - 1] + [int(v) for v in rng.integers(size, 2 * size, size=6)]
        for i, stop in enumerate(C.STOPS[:5]):
            x = np.arange(size, 2 * size, dtype=np.int64)
            for s in run[:stop]:
                x = C.step_all(ct, x, int(s))
            whole = set(int(v) for v in x)
            assert len(whole) == sizes[i]
            reached = {C.walk_ints(ct, run[:stop], e) for e in entries}
            assert reached <= whole and (size > 128 or reached == whole), (a, stop)


@pytest.mark.parametrize("case", QUAL, ids=ids(QUAL))
def test_final_states_walked_on_python_ints_are_the_oracles_state_flush(case):
    """the oracle's C steps fo_encode_symbol through every context's run and flushes the states at the end of the stream: the
    restated runs, walked from the initial state one Python int at a time, end in the flushed states (walk-ends: whichever
    pass writes final_state, these are the bytes it must give).  Contexts of more than WALK_LIMIT symbols are left out."""
    qft = C.tables(case.tables)[1]
    got = C.runs(case.raw, case.recs)
    walked = {c: C.walk_ints(C.ctable(qft, c), run) for c, run in got.items() if len(run) <= WALK_LIMIT}
    assert walked and set(C.target(a) for a, r in case.extra["chains"].items() if len(r) <= WALK_LIMIT) <= set(walked)
    empty = [c for c in (1, 4097, 8191) if c not in got]
    flushed = C.flushed_states(C.coded(case)["qual"], qft, list(walked) + empty)
    for c, x in walked.items():
        assert flushed[c] == x, c
    for c in empty:
        assert flushed[c] == 1 << int(qft["logs"][0][c])


def test_every_pair_of_classes_and_every_route_is_reached():
    """over all cases, the way tables_ref.UNREACHED does it: what is listed as unreached must stay unreached, everything
    else must be reached"""
    pairs, routes, items = C.reached(QUAL)
    kinds = "TAUO"
    assert pairs == {(p, k) for p in (None,) + tuple(kinds) for k in kinds}
    want = set()
    for pred in (None,) + tuple(kinds):
        want |= {("none", "T", pred), ("pow", "U", pred), ("setfunc", "O", pred), ("setfunc" if pred in ("O", "U") else "cand", "A", pred)}
    assert {r[:3] for r in routes if not r[3]} == want
    assert {r[:2] for r in routes if r[3]} == {("none", k) for k in kinds}, "every class stands last in a chain"
    assert items == {(False, False), (False, True), (True, False), (True, True)}


def test_the_cand_waves_of_mixed_contexts_exist_in_the_segment_numbering():
    """(asserted by the generator; here: the numbering it relies on is the device's -- contexts ascending, ceil(n / S) each)"""
    case = [c for c in QUAL if c.name == "cand-mixed-contexts"][0]
    ctx, _, where = C.segments(case)
    assert list(ctx) == sorted(ctx)
    for c, (first, run) in where.items():
        assert int((ctx == c).sum()) == -(-len(run) // case.extra["S"]) and ctx[first] == c and (first == 0 or ctx[first - 1] < c)


@needs_ref_tool
@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_the_references_encoder_gives_the_oracles_bytes(case, tmp_path):
    e = C.coded(case)
    r = R.encode(R.REF_TOOL, case.raw, tmp_path, tables=C.tables(case.tables))
    for k in R.STREAMS:
        assert np.array_equal(np.asarray(r[k]), np.asarray(e[k])), k
