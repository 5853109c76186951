"""The pair-merge tile kernel (k_tile_merge, csrc/ksh_pair.hip) over tile sizes, 16-byte phases and tie positions:
the sheets of tests/pair_tile_cases.py through every call that runs the kernel -- ksh_pair_plan / ksh_pair_write,
ksh_pair_algebra, ksh_pair_algebra_batch, ksh_set_union_plan / _write, ksh_set_diff and ksh_pair_weights -- for
u16, u32 and u64 keys.  Expected values are numpy's intersect1d / setdiff1d / union1d on the 64-bit k-mers, brought
to bucket offsets and keys by synth.to_bucketed; everything is exact.  Which classes of tile, split, lane and phase
the sheets hold is asserted on the CPU (tests/test_pair_tile_model_cpu.py)."""
import numpy as np
import pytest

import pair_tile_cases as ptc
from kmersets import capi, synth

pytestmark = pytest.mark.gpu
U = np.uint64
WIDTHS = (2, 4, 8)
CELLS = [(kb, name) for kb in WIDTHS for name in ptc.sheet_names(kb)]
CELL_IDS = ["u%d-%s" % (8 * kb, name) for kb, name in CELLS]
WIDTH_IDS = ["u%d" % (8 * kb) for kb in WIDTHS]
GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


class Want:
    """The numpy answers for one ordered pair of k-mer arrays: k-mers, and (offsets, keys) per result."""

    def __init__(self, g, x, y):
        self.kmers = {"i": np.intersect1d(x, y, assume_unique=True), "amb": np.setdiff1d(x, y, assume_unique=True),
                      "bma": np.setdiff1d(y, x, assume_unique=True), "u": np.union1d(x, y)}
        self.bucketed = {name: synth.to_bucketed(v, g.k, g.n_bucket_bits, g.key_bytes) for name, v in self.kmers.items()}
        self.sizes = [self.kmers[name].size for name in ("i", "amb", "bma")]

    def trio(self):
        return [self.bucketed[name] for name in ("i", "amb", "bma")]


class World:
    """One key width: its sheets on the device and the numpy answers (each computed once and left unchanged)."""

    def __init__(self, ctx, kb):
        self.kb = kb
        self.g = capi.geom(*ptc.GEOMS[kb])
        assert self.g.key_bytes == kb
        self.cfg = ptc.constants()[kb]
        self.sheets = ptc.sheets(kb)
        self.dev = {name: (capi.DeviceSet.from_kmers(self.g, s.a, ctx.device), capi.DeviceSet.from_kmers(self.g, s.b, ctx.device))
                    for name, s in self.sheets.items()}
        self.empty = capi.DeviceSet.from_kmers(self.g, np.zeros(0, dtype=U), ctx.device)
        self._want = {}

    def want(self, name):
        if name not in self._want:
            s = self.sheets[name]
            self._want[name] = Want(self.g, s.a, s.b)
        return self._want[name]


@pytest.fixture(scope="module")
def worlds(ctx):
    cache = {}

    def get(kb):
        if kb not in cache:
            cache[kb] = World(ctx, kb)
        return cache[kb]

    return get


class Guarded:
    """A key buffer of exactly n bytes: a slice of a larger tensor at a 64-byte offset, with 64 bytes of 0xA5 before
    it and 64 after it (and 0xA5 in it, so a key that is not written shows too)."""

    def __init__(self, n_bytes, device):
        import torch

        self.n = int(n_bytes)
        self.big = torch.full((GUARD + self.n + GUARD,), FILL, dtype=torch.uint8, device=device)
        self.buf = self.big[GUARD:GUARD + self.n]
        assert self.big.data_ptr() % 64 == 0 and (self.n == 0 or self.buf.data_ptr() == self.big.data_ptr() + GUARD)

    def body(self):
        """The buffer's bytes, after checking that the guard bytes are as they were."""
        h = self.big.cpu().numpy()
        assert (h[:GUARD] == FILL).all(), "bytes before the result were written"
        assert (h[GUARD + self.n:] == FILL).all(), "bytes after the result were written"
        return h[GUARD:GUARD + self.n]


def same_set(d, bucketed):
    """A DeviceSet against numpy's (offsets, keys)."""
    off, keys = d.to_numpy()
    assert d.n_keys == bucketed[1].size
    assert np.array_equal(off, bucketed[0])
    assert np.array_equal(keys, bucketed[1])


def two_call(ctx, w, a, b, want, keep=(True, True, True)):
    """ksh_pair_plan, then ksh_pair_write into guarded exact-size buffers (keep[r] False: output r passed as None).
    Returns the bytes written per output."""
    outs = [capi.DeviceSet.empty_like_offsets(w.g, 0, ctx.device) for _ in range(3)]
    totals = ctx.pair_plan(a, b, *outs)
    assert totals == want.sizes
    for o, (off, _) in zip(outs, want.trio()):
        assert np.array_equal(o.offsets.cpu().numpy(), off)
    guards = [Guarded(n * w.kb, ctx.device) for n in totals]
    for o, gd, n in zip(outs, guards, totals):
        o.keys, o.n_keys = gd.buf, n
    ctx.pair_write(a, b, *[o if k else None for o, k in zip(outs, keep)])
    ctx.sync()
    bodies = []
    for gd, (_, keys), k in zip(guards, want.trio(), keep):
        body = gd.body()
        if k:
            assert np.array_equal(body.view(capi.KEY_DTYPE[w.kb]), keys)
        else:
            assert (body == FILL).all(), "an output passed as None was written"
        bodies.append(body.copy())
    return bodies


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_two_call_form(ctx, worlds, cell):
    """Plan totals, the three offset arrays and the keys; then every choice of outputs left out of the write."""
    kb, name = cell
    w = worlds(kb)
    a, b = w.dev[name]
    want = w.want(name)
    full = two_call(ctx, w, a, b, want)
    for keep in ((False, True, True), (True, False, True), (True, True, False),
                 (True, False, False), (False, True, False), (False, False, True)):
        part = two_call(ctx, w, a, b, want, keep)
        for r in range(3):
            if keep[r]:
                assert np.array_equal(part[r], full[r])


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_one_call_form(ctx, worlds, cell):
    kb, name = cell
    w = worlds(kb)
    a, b = w.dev[name]
    for d, bucketed in zip(ctx.pair_algebra_onepass(a, b), w.want(name).trio()):
        same_set(d, bucketed)


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_batch_form(ctx, worlds, cell):
    """(A, B), (B, A), (A, A), (A, {}), ({}, B) and another sheet's pair in one launch: tiles of different pairs
    sit next to each other."""
    kb, name = cell
    w = worlds(kb)
    names = ptc.sheet_names(kb)
    other = names[(names.index(name) + 1) % len(names)]
    a, b = w.dev[name]
    a2, b2 = w.dev[other]
    want, want2 = w.want(name), w.want(other)
    s = w.sheets[name]
    none = synth.to_bucketed(np.zeros(0, dtype=U), w.g.k, w.g.n_bucket_bits, kb)
    whole_a = synth.to_bucketed(s.a, w.g.k, w.g.n_bucket_bits, kb)
    whole_b = synth.to_bucketed(s.b, w.g.k, w.g.n_bucket_bits, kb)
    i_, amb, bma = want.trio()
    got = ctx.pair_algebra_batch([(a, b), (b, a), (a, a), (a, w.empty), (w.empty, b), (a2, b2)])
    expect = [(i_, amb, bma), (i_, bma, amb), (whole_a, none, none), (none, whole_a, none), (none, none, whole_b),
              tuple(want2.trio())]
    assert got.totals == [[t[1].size for t in trio] for trio in expect]
    for trio, want_trio in zip(got, expect):
        for d, bucketed in zip(trio, want_trio):
            same_set(d, bucketed)


@pytest.mark.parametrize("cell", CELLS, ids=CELL_IDS)
def test_union_and_diff(ctx, worlds, cell):
    kb, name = cell
    w = worlds(kb)
    a, b = w.dev[name]
    want = w.want(name)
    off, keys = want.bucketed["u"]
    plan = ctx.set_union_plan(a, b)
    assert plan.n_keys == keys.size
    assert np.array_equal(plan.out.offsets.cpu().numpy(), off)
    gd = Guarded(plan.n_keys * kb, ctx.device)
    ctx.set_union_write(plan, keys=gd.buf)
    ctx.sync()
    assert np.array_equal(gd.body().view(capi.KEY_DTYPE[kb]), keys)
    assert ctx.set_diff(a, b) == want.sizes[1] + want.sizes[2] == ctx.set_diff(b, a)
    assert ctx.set_diff(a, a) == 0 and ctx.set_diff(b, b) == 0


def bucket_counts(w, x, y):
    """Common k-mers of two k-mer arrays per bucket (numpy)."""
    common = np.intersect1d(x, y, assume_unique=True)
    return np.bincount((common >> U(ptc.key_bits(w.kb))).astype(np.int64), minlength=ptc.N_BUCKETS)


@pytest.mark.parametrize("kb", WIDTHS, ids=WIDTH_IDS)
@pytest.mark.parametrize("names", [("s0", "s1"), ("tight", "single")], ids=["s0+s1", "tight+single"])
def test_pair_weights(ctx, worlds, kb, names):
    """ksh_pair_weights over the four sets of two sheets, every ordered pair of them (self pairs and reversed pairs
    included): all buckets, only the buckets that hold a tile of kCap keys, and the first and the last bucket."""
    w = worlds(kb)
    dsets = [d for name in names for d in w.dev[name]]
    kmers = [x for name in names for x in (w.sheets[name].a, w.sheets[name].b)]
    pairs = [(i, j) for i in range(4) for j in range(4)]
    per_bucket = {}
    for i, j in pairs:
        per_bucket[i, j] = per_bucket[j, i] if (j, i) in per_bucket else bucket_counts(w, kmers[i], kmers[j])
    full = sorted({bk for name in names for bk in ptc.full_tile_buckets(w.sheets[name], w.cfg)})
    if names == ("s0", "s1"):
        assert len(full) >= w.cfg.kPer  # (the cross puts a full tile at every phase pair, spread over the sheets)
    id_lists = [list(range(ptc.N_BUCKETS)), [0, ptc.N_BUCKETS - 1], [ptc.SINGLE_BUCKET]] + ([full] if full else [])
    for ids in id_lists:
        got = ctx.pair_weights(dsets, ids, pairs)
        want = [int(per_bucket[p][ids].sum()) for p in pairs]
        assert got.tolist() == want, (names, len(ids))
    assert per_bucket[0, 1].sum() > 0


@pytest.mark.parametrize("kb", WIDTHS, ids=WIDTH_IDS)
def test_repeatable_with_other_plans_between(ctx, worlds, kb):
    """The first sheet twice on one context, with another sheet's pair plan and union plan in between: the same
    bytes -- the splits one plan saved do not leak into another."""
    w = worlds(kb)
    a, b = w.dev["s0"]
    a2, b2 = w.dev["s1"]
    first = two_call(ctx, w, a, b, w.want("s0"))
    outs = [capi.DeviceSet.empty_like_offsets(w.g, 0, ctx.device) for _ in range(3)]
    assert ctx.pair_plan(a2, b2, *outs) == w.want("s1").sizes
    second = two_call(ctx, w, a, b, w.want("s0"))
    assert ctx.set_union_plan(b2, a2).n_keys == w.want("s1").kmers["u"].size
    third = two_call(ctx, w, a, b, w.want("s0"))
    for x, y, z in zip(first, second, third):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # and the union of the first sheet after a pair plan of the second
    plan = ctx.set_union_plan(a, b)
    ctx.pair_plan(a2, b2, *outs)
    plan = ctx.set_union_plan(a, b)
    gd = Guarded(plan.n_keys * kb, ctx.device)
    ctx.set_union_write(plan, keys=gd.buf)
    ctx.sync()
    assert np.array_equal(gd.body().view(capi.KEY_DTYPE[kb]), w.want("s0").bucketed["u"][1])


def test_misaligned_keys_are_refused(ctx, worlds):
    """d_keys off a 16-byte boundary: KSH_INVALID_ARGUMENT before anything runs (the tile loads are whole 16-byte
    vectors)."""
    w = worlds(4)
    a, b = w.dev["s0"]
    bad = capi.DeviceSet(w.g, a.offsets, a.keys[4:], a.n_keys - 1)
    assert bad.keys.data_ptr() % 16 == 4
    outs = [capi.DeviceSet.empty_like_offsets(w.g, 0, ctx.device) for _ in range(3)]
    for x, y in ((bad, b), (b, bad)):
        with pytest.raises(capi.KshError, match="16-byte aligned") as e:
            ctx.pair_plan(x, y, *outs)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT
