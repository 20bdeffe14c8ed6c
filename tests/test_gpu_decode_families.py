"""The chain walk of fqcomp28_amd/csrc/decode.hip -- walk_positions with its plain and RUN step forms and its stores,
LdsBits, WalkT<COMPACT>, decode_chunk / seed_history / decode_stream<SNAP>, k_gather_ncount and k_npatch, and the launch
placements of fq_decode_launch -- at the edges its own comments name: every case of tests/decode_ref.py's families is
decoded from the ORACLE's streams through the C ABI and the whole restored buffer compared with the input; damaged
streams get the oracle's verdict and, when accepted, the oracle's bytes.  Which kernel form ran is not assumed: every
placement is proven by Context.decode_forms(), and the batch sizes come from the n_cus it reports.
tests/test_decode_families_host.py holds the same cases to the oracle and to the reference's compiled decoder."""
import struct

import numpy as np
import pytest

import decode_ref as D
import headers_ref as H
import oracle_lib as O
import ref_pin as R

pytestmark = pytest.mark.gpu

E_CORRUPT = -3
CASES = D.families()
GOOD = [c for c in CASES if c.kind == "ok"]
DAMAGED = [c for c in CASES if c.kind == "damage"]
IX_HEAD = 32


def ids(cases):
    return [D.case_id(c) for c in cases]


@pytest.fixture(scope="module")
def F():
    import fqcomp28_amd as F
    assert F.device_count() >= 1, "no GPU visible: the product path has no CPU fallback"
    return F


@pytest.fixture(scope="module")
def handles(F):
    """one handle per named table set, made when first asked for; "own" tables: a handle of the case's own, closed by the
    caller"""
    made = {}

    def get(case):
        if case.tables == "own":
            return F.Context(*D.case_tables(case))
        if case.tables not in made:
            made[case.tables] = F.Context(*D.tables(case.tables))
        return made[case.tables]

    yield get
    for c in made.values():
        c.close()


def release(case, ctx):
    if case.tables == "own":
        ctx.close()


def forms_of(F):
    """the module that holds the DEC_FORM_* bits"""
    from fqcomp28_amd import binding
    return binding


def host_decode(ctx, case):
    """fqgpu_decode_block over the oracle's streams into the blanked block -> (rc, bytes)"""
    e = D.coded(case)
    return ctx.decode_block(e["seq"], e["qual"], e["n_count"], e["n_pos"], case.recs, O.blank_skeleton(case.raw, case.recs))


def loaded(ctx, case):
    """a device block of the case's shape holding the oracle's streams, its sequence and quality bytes wiped"""
    e = D.coded(case)
    b = ctx.dblock(case.raw, case.recs)
    b.load_streams(e["seq"], e["qual"], e["n_count"], e["n_pos"])
    b.wipe()
    return b


def assert_restored(b, case, what=""):
    assert b.status()[0] == 0, (what, D.case_id(case), b.status()[0])
    got = b.fetch_raw()
    assert got.tobytes() == case.raw.tobytes(), (what, D.case_id(case), int(np.argmax(got != case.raw)))


# ---------------------------------------------------------------------------------------------------------- one block
@pytest.mark.parametrize("case", GOOD, ids=ids(GOOD))
def test_one_block_restores_in_one_launch(F, handles, case):
    """k_decode_both: through the host-pointer call and through a device block"""
    B = forms_of(F)
    ctx = handles(case)
    try:
        rc, out = host_decode(ctx, case)
        assert rc == 0
        assert out.tobytes() == case.raw.tobytes(), int(np.argmax(out != case.raw))
        d = ctx.decode_forms()
        assert d["forms"] == B.DEC_FORM_BOTH and (d["qual_chains"], d["qual_strides"]) == (1, 0), d
        b = loaded(ctx, case)
        ctx.decode_dblocks([b])
        assert_restored(b, case, "device block")
        assert ctx.decode_forms()["forms"] == B.DEC_FORM_BOTH
        b.close()
    finally:
        release(case, ctx)


# ------------------------------------------------------------------------------------------------------------ batches
def batch_groups():
    """(label, cases): what one batch repeats -- the cases of a family that share a table set; a case with tables of its
    own makes a batch of its own"""
    groups = []
    for family in ("lengths", "runs", "window", "n", "strides"):
        by_tables = {}
        for c in D.of_family(family):
            by_tables.setdefault(c.tables if c.tables != "own" else D.case_id(c), []).append(c)
        for key, cases in by_tables.items():
            groups.append(("%s-%s" % (family, key.split("/")[-1]), cases))
    return groups


GROUPS = batch_groups()


def run_batch(F, ctx, cases, n_blocks):
    """n_blocks device blocks, the cases in turn, decoded in one call -> the diagnostic; every block restored"""
    blocks = [loaded(ctx, cases[i % len(cases)]) for i in range(n_blocks)]
    ctx.decode_dblocks(blocks)
    ctx.sync()
    d = ctx.decode_forms()
    for i, b in enumerate(blocks):
        assert_restored(b, cases[i % len(cases)], "block %d of %d" % (i, n_blocks))
        b.close()
    return d


@pytest.mark.parametrize("placement", ["separate-resident", "separate-compact"])
@pytest.mark.parametrize("group", GROUPS, ids=[g[0] for g in GROUPS])
def test_batches_beyond_one_launch(F, handles, group, placement):
    """n_cus + 1 blocks: the two streams in separate launches, the resident quality walk (k_decode<Qual, resident>);
    2 * n_cus + 1 blocks: the compact whole-stream walk (k_decode<Qual, compact>).  The record arrays are batch-wide:
    every block but the first has rec_base > 0."""
    B = forms_of(F)
    cases = group[1]
    ctx = handles(cases[0])
    try:
        n_cus = ctx.decode_forms()["n_cus"]
        assert n_cus >= 1
        n = n_cus + 1 if placement == "separate-resident" else 2 * n_cus + 1
        d = run_batch(F, ctx, cases, n)
        want = B.DEC_FORM_QUAL_RESIDENT if placement == "separate-resident" else B.DEC_FORM_QUAL_COMPACT
        assert d["forms"] == want | B.DEC_FORM_SEQ and (d["qual_chains"], d["qual_strides"]) == (n, 0), d
        # and as many as still go out as one launch
        d = run_batch(F, ctx, cases, min(n_cus, len(cases)))
        assert d["forms"] == B.DEC_FORM_BOTH, d
    finally:
        release(cases[0], ctx)


# ------------------------------------------------------------------------------------------------------------ strides
STRIDES = D.of_family("strides")


def index_header(ix, stream):
    magic, s, stride, n_snap, n_sym, _ = struct.unpack_from("<IIIIQQ", bytes(ix[:IX_HEAD]), 0)
    assert magic == 0x58495146 and s == stream
    return stride, n_snap, n_sym


def built_index(F, ctx, case, cache={}):
    """both decode indexes of a strides case, from the indexing decode of the oracle's streams (k_decode_both<SNAP>), made
    once; the decode that builds them restores the block"""
    B = forms_of(F)
    key = D.case_id(case)
    if key not in cache:
        ctx.set_index_stride(D.STRIDE)
        b = loaded(ctx, case)
        ctx.decode_dblocks_indexing([b])
        assert_restored(b, case, "indexing decode")
        d = ctx.decode_forms()
        assert d["forms"] == B.DEC_FORM_BOTH | B.DEC_FORM_SNAP and d["qual_chains"] == 1, d
        ix = (b.fetch_index(0), b.fetch_index(1))
        for s in (0, 1):
            assert index_header(ix[s], s) == (D.STRIDE, case.extra["n_strides"] - 1, int(case.recs["len"].sum()))
        # the walk in pieces stopped where the generator says: the bytes the model has seen in front of every boundary
        # (p - 1 first, 0xFF in front of the read), which seed_history starts the stride below from
        raw = case.raw.tobytes()
        for s in (0, 1):
            for k, (r, i1) in enumerate(D.boundary_places(case.recs)):
                at = IX_HEAD + k * (16 + 2 * (256, 8192)[s])
                line = int(case.recs[r][("seq_off", "qual_off")[s]])
                if i1 == int(case.recs[r]["len"]):  # between two reads: the stride below begins with the read in front
                    i1 = 0
                want = bytes(raw[line + i1 - 1 - i] if i1 >= i + 1 else 0xFF for i in range(4))
                assert bytes(ix[s][at + 8: at + 12]) == want, (s, k, r, i1)
        b.close()
        cache[key] = ix
    return cache[key]


def indexed(F, ctx, case):
    b = loaded(ctx, case)
    ix = built_index(F, ctx, case)
    for s in (0, 1):
        assert b.load_index(s, ix[s]) == 0
    return b


@pytest.mark.parametrize("case", STRIDES, ids=ids(STRIDES))
def test_strides_from_the_index_the_decode_built(F, handles, case):
    """decode_stream<SNAP> in pieces, then decode_chunk / seed_history from its snapshots: k_decode_chunks<Qual, resident>
    and k_decode_chunks<Seq>; then the windows next to every boundary through fqgpu_decode_chunk_range"""
    B = forms_of(F)
    ctx = handles(case)
    b = indexed(F, ctx, case)
    ctx.decode_dblocks([b])
    assert_restored(b, case, "indexed")
    d = ctx.decode_forms()
    n_strides = case.extra["n_strides"]
    assert d["forms"] == B.DEC_FORM_CHUNKS_QUAL_RESIDENT | B.DEC_FORM_CHUNKS_SEQ and (d["qual_chains"], d["qual_strides"]) == (0, n_strides), d
    b.close()
    # the host-pointer call with the same indexes
    e, ix = D.coded(case), built_index(F, ctx, case)
    rc, out = ctx.decode_block(e["seq"], e["qual"], e["n_count"], e["n_pos"], case.recs, O.blank_skeleton(case.raw, case.recs), index=ix)
    assert rc == 0 and out.tobytes() == case.raw.tobytes()
    assert ctx.decode_forms()["qual_strides"] == n_strides
    # record windows beside the boundaries: only the strides that hold them are walked
    hdrs = R.headers_of(case.raw, case.recs)
    fields = R.oracle_fields(hdrs)[2]
    fmt = H.fmt_of(hdrs[0])
    n = len(case.recs)
    raw = case.raw.tobytes()
    starts = [int(r["seq_off"]) - len(h) - 1 for r, h in zip(case.recs, hdrs)] + [len(raw)]
    seen = set()
    for r, _ in D.boundary_places(case.recs):
        for a, z in ((r, r + 1), (r - 1, r), (r + 1, r + 2), (r - 2, r + 3), (0, r + 1), (r, n)):
            if not 0 <= a < z <= n:
                continue
            got = ctx.decode_chunk_range(fmt, fields, e["readlens"], e["seq"], e["qual"], e["n_count"], e["n_pos"], len(raw), a, z, index=ix)
            assert got["rc"] == 0 and got["raw"].tobytes() == raw[starts[a]: starts[z]], (a, z, got["rc"])
            d = ctx.decode_forms()
            assert d["forms"] == B.DEC_FORM_CHUNKS_QUAL_RESIDENT | B.DEC_FORM_CHUNKS_SEQ and 1 <= d["qual_strides"] <= n_strides, d
            seen.add(d["qual_strides"])
    assert 1 in seen and max(seen) >= 2, "windows inside one stride and windows across a boundary"


def test_more_quality_strides_than_places_take_the_compact_stride_walk(F, handles):
    """k_decode_chunks<Qual, compact>: the indexed strides blocks repeated until their quality strides exceed 2 * n_cus"""
    B = forms_of(F)
    ctx = handles(STRIDES[0])
    n_cus = ctx.decode_forms()["n_cus"]
    blocks, which, strides = [], [], 0
    while strides <= 2 * n_cus:
        case = STRIDES[len(blocks) % len(STRIDES)]
        blocks.append(indexed(F, ctx, case))
        which.append(case)
        strides += case.extra["n_strides"]
    ctx.decode_dblocks(blocks)
    ctx.sync()
    d = ctx.decode_forms()
    assert d["forms"] == B.DEC_FORM_CHUNKS_QUAL_COMPACT | B.DEC_FORM_CHUNKS_SEQ and (d["qual_chains"], d["qual_strides"]) == (0, strides), d
    assert strides > 2 * n_cus
    for b, case in zip(blocks, which):
        assert_restored(b, case, "compact stride walk")
    # indexed and plain blocks in one batch: the stride kernels beside the whole-stream ones
    plain = [loaded(ctx, c) for c in D.of_family("n") if c.tables == "sample"]
    for b in blocks[:3]:
        b.wipe()
    ctx.decode_dblocks(plain + blocks[:3])
    d = ctx.decode_forms()
    assert d["forms"] == B.DEC_FORM_BOTH | B.DEC_FORM_CHUNKS_QUAL_RESIDENT | B.DEC_FORM_CHUNKS_SEQ, d
    assert (d["qual_chains"], d["qual_strides"]) == (len(plain), sum(c.extra["n_strides"] for c in which[:3]))
    for b, case in zip(plain + blocks[:3], [c for c in D.of_family("n") if c.tables == "sample"] + which[:3]):
        assert_restored(b, case, "mixed batch")
    for b in blocks + plain:
        b.close()


# ------------------------------------------------------------------------------------------------------ sequence only
FASTA = [c for c in D.of_family("lengths", "runs", "n")]


@pytest.mark.parametrize("case", FASTA, ids=ids(FASTA))
def test_sequence_only_path(F, handles, case):
    """fqgpu_decode_chunk_fasta: k_decode<Seq> alone on the handle's main stream, the N pass behind it; no quality byte
    is given"""
    B = forms_of(F)
    ctx = handles(case)
    try:
        e = D.coded(case)
        hdrs = R.headers_of(case.raw, case.recs)
        fields = R.oracle_fields(hdrs)[2]
        n = len(case.recs)
        raw = case.raw.tobytes()
        want = b"".join(b">" + h[1:] + b"\n" + raw[int(r["seq_off"]): int(r["seq_off"]) + int(r["len"])] + b"\n" for h, r in zip(hdrs, case.recs))
        got = ctx.decode_chunk_fasta(H.fmt_of(hdrs[0]), fields, e["readlens"], e["seq"], e["n_count"], e["n_pos"], len(raw), 0, n)
        assert got["rc"] == 0 and got["raw"].tobytes() == want
        d = ctx.decode_forms()
        assert d["forms"] == B.DEC_FORM_SEQ and (d["qual_chains"], d["qual_strides"]) == (0, 0), d
    finally:
        release(case, ctx)


# ------------------------------------------------------------------------------------------------------------- damage
def oracle_verdict(case):
    rc, out = D.oracle_decode(case)
    return (None if rc else out)


@pytest.mark.parametrize("case", DAMAGED, ids=ids(DAMAGED))
def test_damaged_streams_get_the_oracles_verdict(F, handles, case):
    """refused (FQGPU_E_CORRUPT) where the oracle refuses, the oracle's bytes where it accepts.  (Every read of the walk
    stays inside its buffers whatever the stream holds: LdsBits::fill reads no dword at or behind n_dw, dword() gives zero
    below dword 0, slide() flags the underflow and the walk ends with the read it is in; open_at_end refuses a last byte
    of zero and an end mark below the state flush before peek_bits reads; a table offset is new state + bits, below
    2^log for every cell; stores go where the record table says.)"""
    ctx = handles(case)
    want = oracle_verdict(case)
    rc, out = host_decode(ctx, case)
    if want is None:
        assert rc == E_CORRUPT
    else:
        assert rc == 0 and out.tobytes() == want.tobytes(), int(np.argmax(out != want))
    # the handle restores the undamaged block right afterwards
    rc, out = host_decode(ctx, case.extra["base"])
    assert rc == 0 and out.tobytes() == case.raw.tobytes()


def _refused_per_base():
    picked = {}
    for c in DAMAGED:
        key = (D.case_id(c.extra["base"]), c.extra["damage"][0])
        if key not in picked and oracle_verdict(c) is None and not c.extra["damage"][1].startswith("last-byte"):
            picked[key] = c
    return list(picked.values())


REFUSED = _refused_per_base()


@pytest.mark.parametrize("case", REFUSED, ids=ids(REFUSED))
def test_one_damaged_block_among_good_ones(F, handles, case):
    """exactly that block reports FQGPU_E_CORRUPT, every other block restores, and the handle decodes a good batch
    afterwards"""
    ctx = handles(case)
    base = case.extra["base"]
    others = [c for c in D.of_family(base.family) if c.tables == base.tables][:4] or [base]
    batch = [others[0], base, case, others[-1], base]
    blocks = [loaded(ctx, c) for c in batch]
    ctx.decode_dblocks(blocks)
    ctx.sync()
    for i, (b, c) in enumerate(zip(blocks, batch)):
        if c is case:
            assert b.status()[0] == E_CORRUPT, i
        else:
            assert_restored(b, c, "beside a damaged block")
    good = [b for b, c in zip(blocks, batch) if c is not case]
    for b in good:
        b.wipe()
    ctx.decode_dblocks(good)
    for b, c in zip(good, [c for c in batch if c is not case]):
        assert_restored(b, c, "after a damaged batch")
    for b in blocks:
        b.close()


# ------------------------------------------------------------------------------------------------- behind the streams
@pytest.mark.parametrize("family", ["lengths", "window"])
def test_nothing_depends_on_the_bytes_behind_a_stream(F, family):
    """peek_bits and LdsBits::fill read the dword behind a stream's last byte: every case once more with every scratch
    byte of the handle, the staging block's stream buffers included, set to 0xFF before the call"""
    ctxs = {}
    try:
        for case in D.of_family(family):
            if case.tables not in ctxs:
                ctxs[case.tables] = F.Context(*D.tables(case.tables))
                assert host_decode(ctxs[case.tables], case)[0] == 0  # (a handle that has done nothing owns no scratch)
            ctx = ctxs[case.tables]
            buffers, n_bytes = ctx.fill_scratch(0xFF)
            assert buffers > 0 and n_bytes > 0
            rc, out = host_decode(ctx, case)
            assert rc == 0 and out.tobytes() == case.raw.tobytes(), D.case_id(case)
    finally:
        for c in ctxs.values():
            c.close()
