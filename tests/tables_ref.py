"""A plain restatement, in Python integers, of what the dataset analysis computes -- the two calculateFreqTable loops
(reference src/fse_sequence.cpp:145-169, src/fse_quality.cpp:69-97) and makeNormalizedFreqTable (src/fse_common.hpp:179-200)
= zstd's FSE_optimalTableLog(0, total, maxSV) + FSE_normalizeCount(useLowProbCount = 1) with FSE_normalizeM2 -- and the
inputs that pin fqcomp28_amd/csrc/tables.hip to it.  Test code: it imports nothing from the library, and the product never
imports it.  The normaliser is written from zstd's published behaviour (lib/compress/fse_compress.c of 1.4.8), as
oracle/fse_oracle.c is; tests/test_tables_host.py holds it against that file and against libzstd before it judges a kernel.

`classify` says which branches a count vector takes; every family of `families(alpha)` asserts, through it, the branch it
is named for.  `read_cases()` are the inputs of the two histogram kernels, by family, each with its record table.
"""
import functools

import numpy as np

REC_DTYPE = np.dtype([("seq_off", "<u4"), ("qual_off", "<u4"), ("len", "<u4")])
SEQ_MODELS, SEQ_ALPHA, QUAL_MODELS, QUAL_ALPHA = 256, 4, 8192, 64
MODELS = {SEQ_ALPHA: SEQ_MODELS, QUAL_ALPHA: QUAL_MODELS}
U32 = 0xFFFFFFFF
MIN_LOG, MAX_LOG, DEFAULT_LOG = 5, 12, 11
RTB = (0, 473195, 504333, 520860, 550000, 700000, 750000, 830000)
REFUSALS = ("rle", "empty", "too_large", "m2_fail")
M2_INNER = ("m2_todist0", "m2_second_lowone", "m2_all_dist", "m2_total0", "m2_spread", "m2_fail")


def hb32(v):
    assert 0 < v <= U32
    return v.bit_length() - 1


def optimal_table_log(total, max_sv):
    """FSE_optimalTableLog(0, total, max_sv) -> (log, wrapped).  highbit32(total - 1) - 2 is a u32: below 0 for a total of
    4 or less, where it wraps to a huge value and stops bounding the log"""
    max_bits_src = (hb32(total - 1) - 2) & U32
    min_bits = min(hb32(total) + 1, hb32(max_sv) + 2)
    t = DEFAULT_LOG
    if max_bits_src < t:
        t = max_bits_src
    if min_bits > t:
        t = min_bits
    return min(max(t, MIN_LOG), MAX_LOG), max_bits_src > 31


def _normalize_m2(norm, t, count, total, tags):
    """FSE_normalizeM2 -> False where it gives up"""
    unset = None
    distributed = 0
    low_thr = total >> t
    low_one = ((total * 3) >> (t + 1)) & U32
    for s, c in enumerate(count):
        if c == 0:
            norm[s] = 0
        elif c <= low_thr:
            norm[s] = -1
            distributed += 1
            total -= c
        elif c <= low_one:
            norm[s] = 1
            distributed += 1
            total -= c
        else:
            norm[s] = unset
    to_dist = ((1 << t) - distributed) & U32
    if to_dist == 0:
        tags.add("m2_todist0")
        return True
    if total // to_dist > low_one:
        tags.add("m2_second_lowone")
        low_one = ((total * 3) // ((to_dist * 2) & U32)) & U32
        for s, c in enumerate(count):
            if norm[s] is unset and c <= low_one:
                norm[s] = 1
                distributed += 1
                total -= c
        to_dist = ((1 << t) - distributed) & U32
    if distributed == len(count):
        tags.add("m2_all_dist")
        norm[count.index(max(count))] += to_dist   # the first of the largest counts
        return True
    if total == 0:
        tags.add("m2_total0")
        s = 0
        while to_dist > 0:
            if norm[s] > 0:
                to_dist -= 1
                norm[s] += 1
            s = (s + 1) % len(count)
        return True
    vsl = 62 - t
    mid = (1 << (vsl - 1)) - 1
    rstep = (((1 << vsl) * to_dist) + mid) // total
    run = mid
    for s, c in enumerate(count):
        if norm[s] is unset:
            end = run + c * rstep
            w = ((end >> vsl) - (run >> vsl)) & U32
            if w < 1:
                tags.add("m2_fail")
                return False
            norm[s] = w
            run = end
    tags.add("m2_spread")
    return True


def classify(counts):
    """-> (verdict, log, norm, tags, info).  verdict: "ok" or one of REFUSALS (log, norm are then None).  info: "rtb" =
    {(P, side): remainder - rest_to_beat nearest to 0}, "m2_gap" = (norm[largest] >> 1) + still (M2 is entered at 0 and
    below), "low_thr", "total"."""
    count = [int(c) for c in counts]
    assert all(0 <= c <= U32 for c in count)
    total = sum(count)
    if total == 0:
        return "empty", None, None, {"empty"}, {}
    if total > U32:
        return "too_large", None, None, {"too_large"}, {}
    if max(count) == total:
        return "rle", None, None, {"rle"}, {}
    t, wrapped = optimal_table_log(total, len(count) - 1)
    tags = {"log%d" % t}
    if wrapped:
        tags.add("wrap")
    scale = 62 - t
    step = (1 << 62) // total
    vstep = 1 << (scale - 20)
    still = 1 << t
    low_thr = total >> t
    largest, largest_p = 0, 0
    norm = [0] * len(count)
    rtb = {}
    for s, c in enumerate(count):
        if c == 0:
            tags.add("zero")
        elif c <= low_thr:
            tags.add("low")
            norm[s] = -1
            still -= 1
        else:
            p = (c * step) >> scale
            if p < 8:
                diff = c * step - (p << scale) - vstep * RTB[p]
                side = "+" if diff > 0 else "-"
                tags.add("rtb%d%s" % (p, side))
                if (p, side) not in rtb or abs(diff) < abs(rtb[p, side]):
                    rtb[p, side] = diff
                p += diff > 0
            if p > largest_p:
                largest_p, largest = p, s
            elif p == largest_p:
                tags.add("tie")
            norm[s] = p
            still -= p
    info = dict(rtb=rtb, m2_gap=(norm[largest] >> 1) + still, low_thr=low_thr, total=total, largest=largest, still=still)
    if -still >= (norm[largest] >> 1):
        tags.add("m2")
        if not _normalize_m2(norm, t, count, total, tags):
            return "m2_fail", None, None, tags, info
    else:
        tags.add("simple")
        if still == 0:
            tags.add("still0")
        elif still < 0:
            tags.add("still_neg")
        norm[largest] += still
    if any(n >= (1 << t) // 2 for n in norm):
        tags.add("notfast")
    assert sum(1 if n == -1 else n for n in norm) == 1 << t and all(n >= -1 for n in norm)
    return "ok", t, norm, tags, info


def normalize(counts):
    """-> (log, norm, tags), or the refusal as a string"""
    verdict, t, norm, tags, _ = classify(counts)
    return (t, norm, tags) if verdict == "ok" else verdict


def tags_of(counts):
    return classify(counts)[3]


# ------------------------------------------------------------------------------------------------- count-vector families
# The tags every alphabet has to reach (test_tables_host.py); what a bounded search does not reach is in UNREACHED.
REQUIRED = (["log%d" % t for t in range(5, 12)] + ["wrap", "zero", "low", "tie", "simple", "still0", "still_neg", "notfast"]
            + ["rtb%d%s" % (p, side) for p in range(1, 8) for side in "+-"] + ["m2"] + list(M2_INNER))

# Branches no count vector of the alphabet reaches, each with why; search_unreached() is the bounded search that backs it.
UNREACHED = {
    4: {
        "m2": "the first pass hands out fewer than 2^log + 4 cells, so it over-allocates by 3 at the most, and the largest "
              "of four probabilities is 2^log / 4 >= 8 or more: -still >= norm[largest] >> 1 >= 4 never holds",
        **{k: "inside FSE_normalizeM2, which four symbols never enter" for k in M2_INNER},
    },
    64: {
        "m2_todist0": "needs 2^log symbols at the low-one mark or below; 64 present symbols force log 7 or more, and log 6 "
                      "(5) needs a total below 64 (32), which 64 (32) present symbols exceed",
        "m2_all_dist": "needs all 64 symbols present and each at 1.5 times the mean count of a remaining cell or below: "
                       "64 * 1.5 = 96 cells' worth, less than the 2^7 cells 64 present symbols force",
        "m2_fail": "a symbol left for the proportional spread holds more than 1.5 times the mean count of a remaining "
                   "cell, so its weight is 1 or more",
    },
}


def _vec(alpha, head, fill=0):
    """head (a list) padded to the alphabet with `fill`"""
    assert len(head) <= alpha
    return tuple(int(c) for c in head) + (fill,) * (alpha - len(head))


def _has(counts, *tags):
    got = tags_of(counts)
    assert set(tags) <= got, (tags, sorted(got), counts)
    return tuple(int(c) for c in counts)


def _random_draw(rng, alpha, kind):
    """the shapes a sample produces (every count 1 or more) and sparse ones"""
    if kind == 0:
        c = 1 + rng.integers(0, 50, alpha)
    elif kind == 1:
        c = 1 + (rng.pareto(0.7, alpha) * 20).astype(np.int64)
    elif kind == 2:
        c = np.ones(alpha, dtype=np.int64)
        c[rng.integers(0, alpha)] += rng.integers(1, 1 << 22)
    elif kind == 3:
        c = rng.integers(0, 3, alpha) * rng.integers(0, 4000, alpha)
        if np.count_nonzero(c) < 2:
            c[:2] = [3, 5]
    elif kind == 4:
        c = 1 + rng.integers(0, 1 << 18, alpha)
    else:
        k = int(rng.integers(min(20, alpha - 1), alpha + 1))
        c = np.zeros(alpha, dtype=np.int64)
        c[:k] = rng.integers(1, 40, k)
        c[rng.integers(0, k)] += rng.integers(0, 2000)
        rng.shuffle(c)
    return tuple(int(v) for v in c)


def random_draws(alpha, n, seed, positive=False):
    """n classified draws that normalise"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = _random_draw(rng, alpha, len(out) % 6)
        if positive:
            c = tuple(max(v, 1) for v in c)
        if classify(c)[0] == "ok":
            out.append(c)
    return out


def _fam_ones(alpha):
    """the empty-context quirk: a context nothing was counted in gets log 11 (4 symbols: the wrap) or 7"""
    c = _has((1,) * alpha, "wrap", "log11") if alpha == 4 else _has((1,) * alpha, "log7")
    t, norm, _ = normalize(c)
    assert norm == [(1 << t) // alpha] * alpha
    return [("all-ones", c)]


def _fam_skew(alpha):
    out = []
    for big in (900000, (1 << 31) - 3, (1 << 32) - alpha):
        c = _has((1,) * (alpha - 1) + (big,), "low", "notfast")
        out.append(("ones-and-%d" % big, c))
    assert sum(out[-1][1]) == U32
    # ([2^31, 2^31 - 1, 0, 1] itself sums to 2^32: it is among the refusals)
    c = _has(_vec(alpha, [1 << 31, (1 << 31) - 2, 0, 1]), "zero", "low", "notfast")
    assert sum(c) == U32
    out.append(("two-halves-of-2^32-1", c))
    c = _has(((1 << 31),) + (0,) * (alpha - 3) + (1, (1 << 31) - 2), "zero", "low", "notfast")
    assert sum(c) == U32
    out.append(("two-halves-at-both-ends", c))
    return out


def _fam_zeros(alpha):
    out = []
    rng = np.random.default_rng(100 + alpha)
    for k in sorted({2, 3, alpha // 2, alpha - 2, alpha - 1} - {0, 1, alpha}):
        for rep in range(3):
            c = np.zeros(alpha, dtype=np.int64)
            c[rng.permutation(alpha)[:k]] = 1 + rng.integers(0, (5, 300, 100000)[rep], k)
            if c.max() == c.sum():
                continue
            c = _has(c, "zero")
            assert sum(v > 0 for v in c) == k
            out.append(("%d-present-%d" % (k, rep), c))
    return out


def _fam_wrap(alpha):
    out = []
    shapes = {2: [[1, 1]], 3: [[1, 1, 1], [2, 1], [1, 0, 2]], 4: [[1, 1, 1, 1], [2, 2], [3, 1], [1, 2, 0, 1]],
              5: [[2, 1, 1, 1], [4, 1], [3, 0, 2]]}
    for total, heads in shapes.items():
        for head in heads:
            for at_end in (False, True):
                c = _vec(alpha, head)
                if at_end:
                    c = c[::-1]
                got = tags_of(c)
                assert ("wrap" in got) == (total <= 4), (c, got)
                assert ("log11" in got) == (total <= 4) and ("log5" in got) == (total == 5), (c, got)
                out.append(("total-%d-%s%s" % (total, "-".join(map(str, head)), "-reversed" if at_end else ""), c))
    return out


def _fam_log_edges(alpha):
    """totals 2^k - 1, 2^k, 2^k + 1: where highbit32(total - 1) and highbit32(total) step"""
    out, logs = [], set()
    rng = np.random.default_rng(200 + alpha)
    for k in range(5, 14):
        for total in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            for present in sorted({2, 3, alpha}):
                if present > total:
                    continue
                cuts = np.sort(rng.choice(np.arange(1, total), present - 1, replace=False))
                head = np.diff(np.concatenate(([0], cuts, [total])))
                c = _vec(alpha, list(head))
                verdict, t, _, tags, _ = classify(c)
                assert verdict == "ok" and sum(c) == total
                want = min(max(min(hb32(total - 1) - 2, 11), min(hb32(total) + 1, hb32(alpha - 1) + 2), 5), 12)
                assert t == want, (c, t, want)
                logs.add(t)
                out.append(("total-%d-%d-present" % (total, present), c))
    assert logs == set(range(5, 12)), logs
    return out


def _fam_low_edge(alpha):
    """one count at total >> log exactly (the last low-probability count), another one above it"""
    out = []
    for thr, t in ((1, 5), (1, 9), (3, 11), (40, 11), (1 << 20, 11)):
        rest_n = alpha - 2
        total_min = thr << t
        for slack in (0, (1 << t) - 1):
            total = total_min + slack
            rest = total - (2 * thr + 1)
            if rest < rest_n:
                continue
            head = [thr, thr + 1] + [rest // rest_n] * (rest_n - 1) + [rest - (rest // rest_n) * (rest_n - 1)]
            c = tuple(head)
            verdict, log, norm, tags, info = classify(c)
            if verdict != "ok" or info["low_thr"] != thr:
                continue
            assert "low" in tags and norm[0] == -1 and norm[1] != -1, (c, norm)
            out.append(("threshold-%d-log-%d-total-%d" % (thr, log, total), c))
    assert len(out) >= 3, out
    return out


RTB_DISTANCE = {"-": 0, "+": 1 << 31}   # what the search reaches: equality, and one count (one step of 2^62 / 2^31) above


def rtb_search(alpha):
    """The bounded search of the `rtb` family: for every P and both sides the vector whose remainder lies nearest its
    rest-to-beat.  Candidates: totals 2^k, k = 21..31 (the step is exact), and for each the two counts around
    (P + rtb[P] / 2^20) * total / 2^log; 11 totals x 7 P x 2 counts = 154 vectors an alphabet.  Equality is met at total
    2^31 (log 11): count = P * 2^20 + rtb[P] exactly.  -> {(P, side): (distance, vector)}"""
    best = {}
    for k in range(21, 32):
        total = 1 << k
        t = optimal_table_log(total, alpha - 1)[0]
        for p in range(1, 8):
            at = ((p << 20) + RTB[p]) * total // (1 << (t + 20))
            for cnt in (at, at + 1):
                rest = total - cnt
                # the other symbols: one large one (it is the largest, so the probe is not adjusted) and ones
                head = [cnt, rest - (alpha - 2)] + [1] * (alpha - 2)
                c = tuple(head)
                verdict, _, _, tags, info = classify(c)
                assert verdict == "ok" and info["largest"] == 1
                for (pp, side), diff in info["rtb"].items():
                    if pp == p and ((pp, side) not in best or abs(diff) < abs(best[pp, side][0])):
                        best[pp, side] = (diff, c)
    return best


def _fam_rtb(alpha):
    out = []
    best = rtb_search(alpha)
    for p in range(1, 8):
        for side in "+-":
            diff, c = best[p, side]
            _has(c, "rtb%d%s" % (p, side))
            # equality falls on the '-' side (the comparison is a strict >); the '+' side is 2^31 above at every total 2^k
            assert diff == RTB_DISTANCE[side], (p, side, diff)
            out.append(("rtb%d%s-distance-%d" % (p, side, diff), c))
    return out




def _fam_tie(alpha):
    """two symbols share the largest probability and something is left to hand out: the first of them takes it"""
    out = []
    mid = (alpha // 2 - 1, alpha // 2)
    for name, pair in (("first-and-last", (0, alpha - 1)), ("two-middle", mid)):
        kept = 0
        for big, small in ((1000, 10), (7, 1), (300000, 299), (41, 3), (5000, 77), (90, 7)):
            c = [small] * alpha
            c[pair[0]] = c[pair[1]] = big
            verdict, t, norm, tags, info = classify(c)
            if not {"tie", "simple"} <= tags or info["still"] == 0:
                continue
            assert info["largest"] == pair[0] and norm[pair[0]] == norm[pair[1]] + info["still"], (c, norm)
            assert max(norm) in (norm[pair[0]], norm[pair[1]])
            out.append(("%s-%d-%d-still-%d" % (name, big, small, info["still"]), _has(c, "tie")))
            kept += 1
        assert kept >= 2, (alpha, name)
    return out


def m2_edge_search(alpha, seed=7, draws=6000):
    """bounded search for vectors at m2_gap 0 (FSE_normalizeM2 entered on equality) and 1 (the simple path by one):
    `draws` seeded draws of many mid-weight symbols -> {gap: [vectors]}"""
    rng = np.random.default_rng(seed)
    found = {0: [], 1: []}
    for i in range(draws):
        c = _random_draw(rng, alpha, 5)
        verdict, _, _, _, info = classify(c)
        if verdict == "ok" and info["m2_gap"] in found and len(found[info["m2_gap"]]) < 4:
            found[info["m2_gap"]].append(c)
    return found


def _fam_m2_edge(alpha):
    found = m2_edge_search(alpha)
    out = []
    for i, c in enumerate(found[1]):
        out.append(("simple-by-one-%d" % i, _has(c, "simple", "still_neg")))
    if alpha == 4:
        # four symbols never come nearer than this (UNREACHED): the nearest a search finds stands in
        assert not found[0]
        c = min(random_draws(4, 600, 9), key=lambda c: classify(c)[4]["m2_gap"])
        return out + [("nearest-a-search-finds-gap-%d" % classify(c)[4]["m2_gap"], _has(c, "simple"))]
    for i, c in enumerate(found[0]):
        out.append(("m2-on-equality-%d" % i, _has(c, "m2")))
    assert found[0] and found[1]
    return out


def _fam_m2(alpha):
    if alpha == 4:
        return []
    rng = np.random.default_rng(300)
    out = []
    while len(out) < 96:
        c = _random_draw(rng, alpha, 5)
        if "m2" in tags_of(c):
            out.append(("draw-%d" % len(out), _has(c, "m2", "m2_spread")))
    return out


def m2_draws(n, seed):
    """n seeded vectors of 64 symbols that enter FSE_normalizeM2, by the classifier: 20 to 59 symbols of count 1 or 2, the
    others near one larger value (the tiny ones each take a cell they do not earn: the first pass over-allocates)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k, big = int(rng.integers(20, 60)), int(rng.integers(4, 120))
        c = [int(v) for v in rng.integers(1, 3, k)] + [big + int(v) for v in rng.integers(0, 1 + big // 3, 64 - k)]
        c = tuple(int(v) for v in rng.permutation(c))
        if "m2" in tags_of(c):
            out.append(c)
    return out


def _fam_m2_second_lowone(alpha):
    """many tiny symbols take their cell each, so the mean of what is left rises above the low-one mark"""
    if alpha == 4:
        return []
    out = []
    c = _has([1] * 54 + [97] * 10, "m2", "m2_second_lowone", "m2_spread")           # the second pass moves nothing
    out.append(("54-ones-10-large", c))
    c = _has([1] * 54 + [15] * 3 + [132, 133, 132] + [97] * 4, "m2", "m2_second_lowone")
    t, norm, _ = normalize(c)
    assert norm[54:57] == [1, 1, 1]                                                 # ... and here it settles three symbols
    out.append(("54-ones-3-settled-in-the-second-pass", c))
    out.append(("the-same-reversed", _has(c[::-1], "m2", "m2_second_lowone")))
    return out


def _fam_m2_total0(alpha):
    """22 to 31 symbols of count 1 among zeros, log 5: every symbol is at the low-one mark, nothing is left to spread"""
    if alpha == 4:
        return []
    out = []
    c = _has([1] * 22 + [0] * 42, "m2", "m2_total0", "log5", "zero")
    t, norm, _ = normalize(c)
    assert norm[:22] == [2] * 10 + [1] * 12
    out.append(("22-ones-in-front", c))
    out.append(("22-ones-behind", _has([0] * 42 + [1] * 22, "m2", "m2_total0")))
    out.append(("22-ones-every-other-place", _has(([1, 0] * 32)[:44] + [0] * 20, "m2", "m2_total0")))
    return out


FAMILY_MAKERS = dict(ones=_fam_ones, skew=_fam_skew, zeros=_fam_zeros, wrap=_fam_wrap, log_edges=_fam_log_edges,
                     low_edge=_fam_low_edge, rtb=_fam_rtb, tie=_fam_tie, m2_edge=_fam_m2_edge, m2=_fam_m2,
                     m2_second_lowone=_fam_m2_second_lowone, m2_total0=_fam_m2_total0)
FAMILIES = tuple(FAMILY_MAKERS)
REFUSED = {   # the refusal vectors, an alphabet each
    alpha: {"rle-first": ("rle", _vec(alpha, [7])), "rle-last": ("rle", _vec(alpha, [7])[::-1]),
            "rle-2^32-1": ("rle", _vec(alpha, [0, U32])), "empty": ("empty", (0,) * alpha),
            "too-large-by-one": ("too_large", _vec(alpha, [1 << 31, 1 << 31])),
            "too-large-by-one-in-three": ("too_large", _vec(alpha, [1 << 31, (1 << 31) - 1, 0, 1])),
            "too-large-all": ("too_large", (U32,) * alpha)}
    for alpha in (4, 64)}


def families(alpha):
    """-> {family: [(name, counts)]}; every vector normalises; making them runs the assertions they are named for"""
    out = {}
    for fam, make in FAMILY_MAKERS.items():
        out[fam] = [("%s:%s" % (fam, name), tuple(c)) for name, c in make(alpha)]
        for name, c in out[fam]:
            assert len(c) == alpha and classify(c)[0] == "ok", name
    return out


@functools.lru_cache(maxsize=None)
def shared_families(alpha):
    return families(alpha)


def family_vectors(alpha):
    """every (name, counts) of every family, in order"""
    return [nc for fam in shared_families(alpha).values() for nc in fam]


SEARCH_SEEDS, SEARCH_DRAWS, SEARCH_DIRECTED = (11, 12, 13), 2000, 3000


def search_unreached(alpha):
    """The bounded search behind UNREACHED: SEARCH_DRAWS random draws for each seed of SEARCH_SEEDS, and SEARCH_DIRECTED
    directed ones (k tiny symbols, the rest near-equal: the shapes that reach m2_second_lowone and m2_total0), classified.
    -> (the tags met, the number of vectors tried)"""
    met, n = set(), 0
    for seed in SEARCH_SEEDS:
        rng = np.random.default_rng(seed)
        for i in range(SEARCH_DRAWS):
            met |= tags_of(_random_draw(rng, alpha, i % 6))
            n += 1
    rng = np.random.default_rng(SEARCH_SEEDS[0] + 100)
    for i in range(SEARCH_DIRECTED):
        k = int(rng.integers(0, alpha))
        tiny = int(rng.integers(0, 3))
        big = int(rng.integers(1, 200))
        c = [tiny] * k + [big + int(v) for v in rng.integers(0, 1 + big // 4, alpha - k)]
        if i % 3 == 0:
            c = [int(v) for v in rng.permutation(c)]
        if sum(c):
            met |= tags_of(c)
            n += 1
    return met, n


# ------------------------------------------------------------------------------------------------------ the FreqTable PODs
def ft_dtype(alpha):
    m = MODELS[alpha]
    return np.dtype([("norm", "<i2", (m, alpha)), ("logs", "<u4", (m,)), ("max_log", "<u4")])


def freq_table(counts):
    """makeNormalizedFreqTable over a (models, alpha) count array -> the FreqTable struct; None where a context is refused"""
    counts = np.asarray(counts)
    ft = np.zeros(1, dtype=ft_dtype(counts.shape[1]))
    memo = {}   # (most contexts of a small input hold the same counts)
    for m, row in enumerate(counts.tolist()):
        row = tuple(row)
        r = memo[row] if row in memo else memo.setdefault(row, normalize(row))
        if isinstance(r, str):
            return None
        ft["logs"][0][m] = r[0]
        ft["norm"][0][m] = r[1]
    ft["max_log"][0] = ft["logs"][0].max()
    return ft


EDGE_CONTEXTS = (0, 1, 63, 64, 255, 8191)


@functools.lru_cache(maxsize=None)
def packed_counts(alpha, positive=False, seed=1):
    """-> (counts (models, alpha) uint32, {context: name}): every family vector in a context of its own -- the first ones
    in contexts 0, 1, 63, 64, 255 (and 8191) -- the rest of the contexts classified random draws.  positive: only vectors
    with every count 1 or more (tables any data can be coded with)"""
    models = MODELS[alpha]
    vecs = [(n, c) for n, c in family_vectors(alpha) if not positive or min(c) >= 1]
    places = [m for m in EDGE_CONTEXTS if m < models]
    # spread what is left evenly over the contexts
    free = [m for m in range(models) if m not in places]
    assert len(vecs) <= models, (len(vecs), models)
    stride = max(1, len(free) // max(1, len(vecs) - len(places)))
    places += free[::stride]
    # the vectors that matter most at an edge context first: one of each family
    firsts, seen = [], set()
    for nc in vecs:
        fam = nc[0].split(":")[0]
        (firsts if fam not in seen else []).append(nc)
        seen.add(fam)
    rest = [nc for nc in vecs if nc not in firsts]
    counts = np.array(random_draws(alpha, models, seed + alpha, positive), dtype=np.uint32)
    where = {}
    for m, (name, c) in zip(places, firsts + rest):
        counts[m] = c
        where[m] = name
    assert len(where) == len(vecs)
    counts.setflags(write=False)
    return counts, where


# ------------------------------------------------------------------------------------------------------------ histograms
SEQ_INITIAL_CONTEXT = 0xD7   # FSE_Sequence::INITIAL_CONTEXT (src/fse_sequence.h:42-63): T, C, C, T in front of a read
BASE_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def seq_counts(raw, recs):
    """FSE_Sequence::calculateFreqTable's counting, one record and one byte at a time -> (256, 4) counts, or "bad" """
    b = bytes(raw)
    counts = [[1] * SEQ_ALPHA for _ in range(SEQ_MODELS)]
    for off, _, n in recs.tolist():
        ctx = SEQ_INITIAL_CONTEXT
        for ch in b[off: off + n]:
            if ch == 0x4E:   # N: skipped, the context stays
                continue
            sym = BASE_CODE.get(ch)
            if sym is None:
                return "bad"
            counts[ctx][sym] += 1
            ctx = (ctx >> 2) + (sym << 6)
    return np.array(counts, dtype=np.uint32)


def qual_context(q, q1, q2):
    """FSE_Quality::calcContext (src/fse_quality.h:40-44)"""
    return (((max(q1, q2) << 6) + q) & 0xFFF) + ((q1 == q2) << 12)


def qual_counts(raw, recs):
    """FSE_Quality::calculateFreqTable's counting -> (8192, 64) counts, or "bad" """
    b = bytes(raw)
    counts = np.ones((QUAL_MODELS, QUAL_ALPHA), dtype=np.uint32)
    flat = {}
    for _, off, n in recs.tolist():
        ctx, q1, q2 = qual_context(0, 0, 0), 0, 0
        for ch in b[off: off + n]:
            q = ch - 33
            if not 0 <= q < QUAL_ALPHA:
                return "bad"
            key = ctx * QUAL_ALPHA + q
            flat[key] = flat.get(key, 0) + 1
            ctx = qual_context(q, q1, q2)
            q2, q1 = q1, q
    for key, v in flat.items():
        counts[key >> 6, key & 63] += v
    return counts


def fold_profile(qual):
    """what k_hist_qual does with one read, 64 symbols a step: [(lanes folded in round 1, in round 2, left to atomics)]"""
    cells = []
    ctx, q1, q2 = qual_context(0, 0, 0), 0, 0
    for ch in qual:
        q = ch - 33
        cells.append(ctx * QUAL_ALPHA + q)
        ctx = qual_context(q, q1, q2)
        q2, q1 = q1, q
    out = []
    for at in range(0, len(cells), 64):
        left = cells[at: at + 64]
        folded = []
        for _ in range(2):
            n = left.count(left[0]) if left else 0
            folded.append(n)
            left = [c for c in left if c != left[0]] if left else left
        out.append((folded[0], folded[1], len(left)))
    return out


def block_of(reads):
    """reads: [(sequence line, quality line)] or [(sequence line, quality line, len)] -> (raw, recs).  `len` below the
    lines' length leaves bytes behind the read that belong to no read"""
    parts, recs, at = [], [], 0
    for r in reads:
        seq, qual = bytes(r[0]), bytes(r[1])
        assert len(seq) == len(qual)
        n = r[2] if len(r) > 2 else len(seq)
        rec = b"@r\n" + seq + b"\n+\n" + qual + b"\n"
        recs.append((at + 3, at + 3 + len(seq) + 3, n))
        parts.append(rec)
        at += len(rec)
    raw = b"".join(parts)
    recs = np.array(recs, dtype=REC_DTYPE)
    for so, qo, n in recs.tolist():
        assert raw[so - 1] == 10 and raw[qo - 3: qo] == b"\n+\n"
    return raw, recs


LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 192, 300)
QUALS = b"#+05:<@ABDGI"


class _Reads:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def seq(self, n, p_n=0.0):
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[self.rng.integers(0, 4, size=n)].copy()
        s[self.rng.random(n) < p_n] = ord("N")
        return s.tobytes()

    def qual(self, n):
        return np.frombuffer(QUALS, dtype=np.uint8)[self.rng.integers(0, len(QUALS), size=n)].tobytes()

    def read(self, n, p_n=0.0):
        return self.seq(n, p_n), self.qual(n)


def _with_n(seq, places):
    s = bytearray(seq)
    for p in places:
        s[p] = 0x4E
    return bytes(s)


def _many_reads(g, n_reads, n, last=None, p_n=0.01):
    """n_reads reads of n symbols from two large draws (the last one `last` long)"""
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[g.rng.integers(0, 4, size=n_reads * n)].copy()
    s[g.rng.random(s.size) < p_n] = ord("N")
    q = np.frombuffer(QUALS, dtype=np.uint8)[g.rng.integers(0, len(QUALS), size=n_reads * n)]
    s, q = s.tobytes(), q.tobytes()
    reads = [(s[i * n: (i + 1) * n], q[i * n: (i + 1) * n]) for i in range(n_reads)]
    if last is not None:
        reads[-1] = (reads[-1][0][:last], reads[-1][1][:last])
    return reads


SWITCH_BASES = 1 << 20   # fq_build_freq_tables: the encoder's sort counts the qualities from here on, if no read is short


def read_cases():
    """-> {"family:name": (raw, recs, verdict)}: the inputs of k_hist_seq and k_hist_qual.  verdict "ok" or "bad" """
    out = {}

    def add(name, reads, verdict="ok"):
        assert name not in out
        raw, recs = block_of(reads)
        out[name] = (raw, recs, verdict)

    g = _Reads(2)
    # lengths: around the 64 symbols of a step, and the reads the encoder refuses (the analysis takes them)
    for n in LENGTHS:
        add("lengths:%d-alone" % n, [g.read(n, 0.05)])
    add("lengths:mixed", [g.read(n, 0.05) for n in LENGTHS + LENGTHS[::-1]])

    # N places in a read of 200 bases (steps 0..63, 64..127, 128..191, 192..199)
    places = {"at-0": [0], "at-3": [3], "at-63": [63], "at-64": [64], "run-60-67": range(60, 68), "run-62-129": range(62, 130),
              "second-step-whole": range(64, 128)}
    for k in (1, 2, 3):   # k kept bases end the first step: the carry keeps 4 - k bases of the initial context
        places["%d-kept-before-64" % k] = range(0, 64 - k)
        places["%d-kept-before-128" % k] = range(64, 128 - k)   # ... and here of the first step's
    n_reads = []
    for name, where in places.items():
        read = (_with_n(g.seq(200), where), g.qual(200))
        assert read[0].count(b"N") == len(where) and all(read[0][p] == 0x4E for p in where)
        add("n_places:" + name, [read])
        n_reads.append(read)
    for k in (1, 2, 3):
        s = out["n_places:%d-kept-before-64" % k][0]
        assert s[3: 3 + 64].count(b"N") == 64 - k and b"N" not in s[3 + 64 - k: 3 + 200]
    assert out["n_places:second-step-whole"][0][3 + 64: 3 + 128] == b"N" * 64
    all_n = (b"N" * 200, g.qual(200))
    add("n_places:all-N-then-a-read", [all_n, g.read(200)])
    add("n_places:all-N-alone", [all_n])
    add("n_places:combined", n_reads + [all_n] + n_reads[::-1])

    # quality cells: how many lanes of a step share the leading lane's cell
    for n in (64, 100):
        shapes = {"constant": bytes([ord("I")]) * n, "alternating": (b"I5" * n)[:n], "period-3": (b"I5#" * n)[:n],
                  "random": g.qual(n), "Q0": bytes([33]) * n, "Q63": bytes([33 + 63]) * n}
        for name, q in shapes.items():
            prof = fold_profile(q)
            last = min(n, 128) - 64 if n > 64 else None
            if name in ("constant", "Q0", "Q63") and n > 64:
                assert prof[1] == (last, 0, 0), prof           # one cell: the first round takes the whole step
            if name == "alternating" and n > 64:
                assert prof[1] == (last // 2, last // 2, 0), prof   # two cells: both rounds, nothing left
            if name in ("period-3", "random"):
                assert prof[-1][2] > 0, prof                   # three cells and more: atomics are left over
            add("qual_cells:%s-%d" % (name, n), [(g.seq(n), q)])
    add("qual_cells:combined", [(g.seq(100), q) for q in (bytes([ord("I")]) * 100, (b"I5" * 50), (b"I5#" * 34)[:100], bytes([33]) * 100,
                                                           bytes([96]) * 100)])

    # record counts: one more record than the 16384 waves of the largest grid (4096 workgroups of four)
    add("records:one", [g.read(100, 0.05)])
    add("records:16385-of-3-bases", _many_reads(g, 16385, 3, p_n=0.05))

    # refusals: a byte that is no base, a quality outside 0..63; behind the read's length the same bytes are nobody's
    good = g.read(70)
    for name, ch in (("lowercase-base", b"a"), ("dot", b"."), ("zero-byte", b"\0"), ("lowercase-n", b"n")):
        for at in (0, 64, 69):
            s = bytearray(good[0])
            s[at: at + 1] = ch
            add("refusals:%s-at-%d" % (name, at), [g.read(10), (bytes(s), good[1]), g.read(10)], "bad")
        add("refusals:%s-behind-the-read" % name, [g.read(10), (good[0] + ch, good[1] + b"I", 70), g.read(10)])
    for name, ch in (("quality-32", bytes([32])), ("quality-97", bytes([97]))):
        for at in (0, 64, 69):
            q = bytearray(good[1])
            q[at: at + 1] = ch
            add("refusals:%s-at-%d" % (name, at), [g.read(10), (good[0], bytes(q)), g.read(10)], "bad")
        add("refusals:%s-behind-the-read" % name, [g.read(10), (good[0] + b"A", good[1] + ch, 70), g.read(10)])

    # the switch between the encoder's sort and the atomics kernel: min_len >= 3 && n_bases >= 2^20
    g = _Reads(3)
    exact = _many_reads(g, 8192, 128)
    add("switch:8192-reads-of-128", exact)
    add("switch:last-read-127", exact[:-1] + [(exact[-1][0][:127], exact[-1][1][:127])])
    add("switch:2^20-and-a-read-of-2", exact + [g.read(2)])
    bases = {k: int(out[k][1]["len"].sum()) for k in out if k.startswith("switch:")}
    assert sorted(bases.values()) == [SWITCH_BASES - 1, SWITCH_BASES, SWITCH_BASES + 2], bases
    assert int(out["switch:2^20-and-a-read-of-2"][1]["len"].min()) == 2
    return out


READ_FAMILIES = ("lengths", "n_places", "qual_cells", "records", "refusals", "switch")


@functools.lru_cache(maxsize=None)
def shared_read_cases():
    return read_cases()


def read_names(family):
    return [k for k in shared_read_cases() if k.split(":")[0] == family]


@functools.lru_cache(maxsize=None)
def read_reference(name):
    """-> (verdict, seq counts, qual counts) by the byte loops, computed once a case"""
    raw, recs, verdict = shared_read_cases()[name]
    sc, qc = seq_counts(raw, recs), qual_counts(raw, recs)
    got = "bad" if isinstance(sc, str) or isinstance(qc, str) else "ok"
    assert got == verdict, (name, got, verdict)
    if got == "ok":
        sc.setflags(write=False)
        qc.setflags(write=False)
    return got, sc, qc
