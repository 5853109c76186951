"""CPU checks of the per-bucket sort sweep (tests/bucket_sort_cases.py): the constants read from ksh_decode.hip, the
branch list -- which branches of k_bucket_sort the cases reach, per sorted type, as conditions computed by the
model -- the thresholds, the numpy reference against the oracle's KmerCounter, and the input builder.
tests/test_gpu_bucket_sort.py runs the cases."""
import numpy as np
import pytest

import bucket_sort_cases as bsc
import oracle_lib as ol
from kmersets import synth

U = np.uint64
GEOM_IDS = [bsc.geom_id(g) for g in bsc.GEOMS]
SORTED_TYPES = (2, 4, 8)
UNREACHABLE = {2: set(), 4: set(), 8: {"stream"}}  # kCap of an 8-byte type is below kSortRegs * kSortThreads


@pytest.fixture(scope="module")
def cfg():
    return bsc.constants()


def case_named(g, family, name):
    (c,) = [c for c in bsc.cases(g, family) if c.name == name]
    return c


def test_constants_read_from_the_kernel(cfg):
    assert [bsc.k_cap(sb, cfg) for sb in SORTED_TYPES] == [31744, 15872, 7936]
    assert cfg.kSortRegs * cfg.kSortThreads == 8192
    assert cfg.sub_limit == 64 and cfg.part_div == 4 and cfg.kCoarseBits == 14 and cfg.kMaxSubBits == 11
    assert bsc.k_cap(8, cfg) < cfg.kSortRegs * cfg.kSortThreads < bsc.k_cap(4, cfg)
    assert bsc.big_size(cfg) == 2048 * 1984 + 1
    # the sorted types of the geometries: u16, u32 and u64 on the plain route; the composite on the wide one
    assert [bsc.sorted_bytes(g, cfg) for g in bsc.GEOMS] == [2, 4, 4, 8, 8, 4, 4, 8]
    assert [bsc.sort_key_bits(g, cfg) for g in bsc.GEOMS] == [14, 30, 32, 42, 48, 32, 20, 48]
    # a changed constant is noticed, a missing one refused
    text = open(bsc.DECODE_HIP).read()
    assert bsc.k_cap(4, bsc.constants(text.replace("kSortLdsBytes = 63488;", "kSortLdsBytes = 32768;"))) == 8192
    assert bsc.constants(text.replace("if (s1 - s0 > 64) {", "if (s1 - s0 > 32) {")).sub_limit == 32
    for gone in ("constexpr int kSortRegs = 8;", "if (s1 - s0 > 64) {", "kCap / 4 &&", "if (pc <= kCap) {"):
        with pytest.raises(AssertionError):
            bsc.constants(text.replace(gone, "//"))


def test_model_plans():
    """The two `bits` loops at their edges."""
    assert [bsc.lds_plan(cnt, 30)[0] for cnt in (1, 4, 5, 8, 9, 1024, 1025, 8192, 8193, 15872)] == [0, 0, 1, 1, 2, 8, 9, 11, 11, 11]
    assert bsc.lds_plan(3000, 3) == (3, 0) and bsc.lds_plan(3000, 14) == (10, 4)
    cap = bsc.k_cap(4)
    assert bsc.partition_plan(cap + 1, 30, 4) == (2, 28) and bsc.partition_plan(4 * (cap // 4) + 4, 30, 4) == (3, 27)
    assert bsc.partition_plan(bsc.big_size(), 48, 8) == (11, 37) and bsc.partition_plan(10 ** 9, 48, 8) == (11, 37)
    assert bsc.partition_plan(5 * bsc.k_cap(2), 14, 2) == (5, 9)


@pytest.mark.parametrize("g", bsc.GEOMS, ids=GEOM_IDS)
def test_every_case_is_what_it_says(g):
    """The model finds the branches each case aims at (and none of those it must avoid) in its target bucket; the
    target's neighbours are in place with key 0 and the all-ones key."""
    kbw = bsc.sort_key_bits(g)
    names = [c.name for c in bsc.all_cases(g)]
    assert len(set(names)) == len(names)
    for c in bsc.all_cases(g):
        got = c.branches()
        assert c.expect <= got and not (c.forbid & got), (c.name, sorted(got))
        assert c.kmers.size < 1 << 20 and int(c.kmers.max()) < 1 << (2 * g.k)
        if c.kmers.size > 160000:
            assert c.name == "uniform-%d" % (5 * bsc.k_cap(bsc.sorted_bytes(g)))
        if c.family != "reads":
            buckets = c.kmers >> U(kbw)
            for nb in (c.target - 1, c.target + 1):
                if 0 <= nb < 1 << bsc.sort_bucket_bits(g):
                    assert np.array_equal(np.sort(c.kmers[buckets == U(nb)] & U((1 << kbw) - 1)), bsc._neighbour_keys(kbw))
            assert set(np.unique(buckets).tolist()) <= {c.target - 1, c.target, c.target + 1}
            # equal keys do not arrive adjacent (a handful may, by chance)
            dup = c.kmers[1:] == c.kmers[:-1]
            assert c.family == "heavy" or dup.mean() < 0.2, c.name
    assert {c.target for c in bsc.all_cases(g) if c.family != "reads"} == {0, (1 << bsc.sort_bucket_bits(g)) // 2 + 2,
                                                                            (1 << bsc.sort_bucket_bits(g)) - 1}


@pytest.mark.parametrize("sb", SORTED_TYPES, ids=["u16", "u32", "u64"])
def test_every_branch_is_reached(sb):
    """A condition on the case list: for each sorted type, every branch name at some case and cutoff -- except
    `stream` for 8-byte types, whose LDS holds fewer keys than the registers of a workgroup."""
    reached = set()
    geoms = [g for g in bsc.GEOMS if bsc.sorted_bytes(g) == sb]
    assert geoms
    for g in geoms:
        for c in bsc.all_cases(g):
            for cutoff in sorted({1, c.at_cutoff}):
                reached |= c.branches(cutoff)
    assert set(bsc.BRANCHES) - reached == UNREACHABLE[sb]
    if sb == 8:
        assert "stream" not in bsc.big_case().branches() and {"partition", "regs"} <= bsc.big_case().branches()


@pytest.mark.parametrize("g", bsc.GEOMS, ids=GEOM_IDS)
def test_thresholds_split_the_cases(g):
    """64 | 65 keys in a sub-bin, 8192 | 8193 keys, kCap | kCap + 1 keys: the two cases of each pair fall on
    different sides."""
    sb = bsc.sorted_bytes(g)
    cap, lim = bsc.k_cap(sb), bsc.cfg().sub_limit
    kbw = bsc.sort_key_bits(g)
    for c in bsc.cases(g, "threshold"):
        n_in = int(c.name.split("-")[1])
        counts = np.sort(bsc.sub_bin_counts(c.target_keys(), kbw))
        assert counts[-1] == n_in and counts[-2] <= 3, c.name
        assert ("lds_bitonic" in c.branches()) == (n_in > lim), c.name
    assert {int(c.name.split("-")[1]) for c in bsc.cases(g, "threshold")} == {lim, lim + 1}
    regs = bsc.cfg().kSortRegs * bsc.cfg().kSortThreads
    at, above = case_named(g, "uniform", "uniform-%d" % regs).branches(), case_named(g, "uniform", "uniform-%d" % (regs + 1)).branches()
    if sb == 8:  # both beyond kCap: the one pair that cannot be split
        assert "partition" in at and "partition" in above and cap < regs
    else:
        assert "regs" in at and "stream" not in at and "stream" in above and "regs" not in above
    at, above = case_named(g, "uniform", "uniform-%d" % cap).branches(), case_named(g, "uniform", "uniform-%d" % (cap + 1)).branches()
    assert "partition" not in at and "partition" in above
    assert case_named(g, "uniform", "uniform-%d" % cap).target_keys().size == cap


@pytest.mark.parametrize("g", bsc.GEOMS, ids=GEOM_IDS)
def test_family_arithmetic(g):
    """What the families were sized by: uniform keys at kCap stay below 30 per sub-bin, kCap + 1 gives 4 parts that
    all fit, the 3000-key cluster overflows, kCap + 5 heavy keys give exactly one part for the global network."""
    sb, kbw = bsc.sorted_bytes(g), bsc.sort_key_bits(g)
    cap = bsc.k_cap(sb)
    assert bsc.sub_bin_counts(case_named(g, "uniform", "uniform-%d" % cap).target_keys(), kbw).max() < 30
    keys = case_named(g, "uniform", "uniform-%d" % (cap + 1)).target_keys()
    bits, shift = bsc.partition_plan(keys.size, kbw, sb)
    parts = np.bincount((keys >> U(shift)).astype(np.int64), minlength=1 << bits)
    assert bits == 2 and parts.size == 4 and parts.min() > 0 and parts.max() <= cap
    for c in bsc.cases(g, "clustered"):
        if c.name.startswith("cluster-3000"):
            assert bsc.sub_bin_counts(c.target_keys(), kbw).max() > bsc.cfg().sub_limit
        elif c.name.startswith("cluster-pair"):
            keys = c.target_keys()
            bits, shift = bsc.partition_plan(keys.size, kbw, sb)
            parts = np.bincount((keys >> U(shift)).astype(np.int64), minlength=1 << bits)
            assert keys.size == cap + 100 and (parts > 0).sum() == 2 and parts.max() <= cap
            assert (parts[:parts.size // 2] > 0).sum() == 1  # one cluster in each half of the key range
    for c in bsc.cases(g, "heavy"):
        keys = c.target_keys()
        if keys.size > cap:
            bits, shift = bsc.partition_plan(keys.size, kbw, sb)
            parts = np.bincount((keys >> U(shift)).astype(np.int64), minlength=1 << bits)
            assert (parts > cap).sum() == 1 and c.name.startswith("heavy-%d-" % (cap + 5))
    # where a case aims at the network in LDS, the overflowing sub-bin holds more than one value, so a network that
    # does nothing leaves keys out of order (the one exception: two clusters of a 14-bit key, whose parts have one
    # value per sub-bin -- that geometry has `cluster-part` for it)
    for c in bsc.cases(g, "threshold") + bsc.cases(g, "clustered") + bsc.cases(g, "heavy"):
        keys = c.target_keys()
        if "lds_bitonic" in c.expect:
            assert bsc.needs_network(keys, kbw), c.name
        elif "part_lds_bitonic" in c.expect and not (kbw == 14 and c.name.startswith("cluster-pair")):
            bits, shift = bsc.partition_plan(keys.size, kbw, sb)
            part = (keys >> U(shift)).astype(np.int64)
            assert any(bsc.needs_network(keys[part == p], shift) for p in np.unique(part)), c.name
    assert ("cluster-part" in [c.name for c in bsc.cases(g, "clustered")]) == (kbw == 14)
    if kbw == 14:
        # a cluster on the low 12 bits of a 14-bit key spreads over 256 sub-bins and does not overflow: these
        # geometries cluster on the low 3 bits, with repeats
        wide_cluster = np.random.default_rng(1).permutation(4096)[:3000].astype(U)
        assert "lds_bitonic" not in bsc.bucket_branches(wide_cluster, kbw, sb)
        assert bsc.cluster_bits(g) == 3
    else:
        assert bsc.cluster_bits(g) == 12
    # the runs: per = 1, 2 and 9, the last key the largest of its bucket with the occurrences its name says
    threads = bsc.cfg().kSortThreads
    seen = set()
    for c in bsc.cases(g, "runs"):
        keys = np.sort(c.target_keys())
        per, last = int(c.name.split("-")[1][3:]), int(c.name.split("-")[2][4:])
        assert (keys.size + threads - 1) // threads == per and (keys == keys[-1]).sum() == last
        assert keys[-1] == U((1 << kbw) - 1)
        seen.add((per, last))
    assert seen == {(p, m) for p in bsc.RUN_PERS for m in bsc.RUN_LAST}
    assert set(bsc.RUN_LAST) >= {c + d for c in bsc.CUTOFFS if c > 1 for d in (-1, 0, 1)}


def kmer_text(kmers, k):
    """One line of k bases per k-mer."""
    kmers = np.asarray(kmers, dtype=U)
    lines = np.full((kmers.size, k + 1), ord("\n"), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        lines[:, j] = letters[((kmers >> U(2 * (k - 1 - j))) & U(3)).astype(np.int64)]
    return lines.tobytes()


@pytest.mark.parametrize("g", bsc.GEOMS, ids=GEOM_IDS)
def test_reference_is_the_oracles_counter(g):
    """np.unique with counts == KmerCounter::FromReads + ToKmerSet(cutoff) of the oracle, set and cut count, on every
    case of at most ORACLE_MAX occurrences fed as reads, at every cutoff -- so the GPU test needs no oracle.  (With
    2^20 buckets the oracle spends a third of a second per case on building empty buckets: half a minute.)"""
    n_checked = 0
    for c in bsc.all_cases(g):
        if c.kmers.size > bsc.ORACLE_MAX:
            continue
        counter = ol.Counter(g.k, g.n, g.kb)
        if c.strings is not None:
            counter.from_reads(c.strings, canonical=c.canonical)
        else:
            text = kmer_text(c.kmers, g.k)
            ol.lib().ko_counter_from_reads(counter.h, text, len(text), int(c.canonical))
        for cutoff in bsc.CUTOFFS:
            want_set, want_cut = counter.to_set(cutoff)
            kept, n_cut, offsets = bsc.reference(c.counted(), g, cutoff)
            assert n_cut == want_cut and np.array_equal(kept, want_set.kmers()), (c.name, cutoff)
            assert int(offsets[-1]) == kept.size
        n_checked += 1
    assert n_checked >= 50


def test_pack_kmers_round_trip():
    rng = np.random.default_rng(3)
    for k in (1, 5, 11, 16, 17, 31, 32):
        for n in (0, 1, 2, 31, 32, 33, 1000):
            top = (1 << (2 * k)) - 1
            kmers = rng.integers(0, top, size=n, dtype=np.uint64, endpoint=True)
            if n > 1:
                kmers[0], kmers[-1] = 0, top
            words, lens = bsc.pack_kmers(kmers, k)
            assert words.dtype == U and words.size == (n * k + 31) // 32 and lens.size == n and not lens.any()
            strings = synth.unpack_strings(words, lens, k)
            assert strings == [s.decode() for s in kmer_text(kmers, k).split(b"\n")[:-1]]
            if n:
                back = np.concatenate([synth.kmers_of_bases(synth.bases_of_string(s), k) for s in strings])
                assert np.array_equal(back, kmers)
            want_words, want_lens = synth.pack_strings(strings, k)
            assert np.array_equal(words, want_words) and np.array_equal(lens, want_lens)
