"""The cases of tests/probe_cases.py and their model, on the CPU: every case is what it says, the cases together reach
every branch of the staged neighbour probe that the model names, what is asserted about fits / batches / routes is
asserted both ways, the unitigs that follow from the model's neighbour verdicts are the oracle's, the plan arithmetic
is pinned, and the lines and constants of ksh_encode.hip that the model restates still stand there."""
import numpy as np
import pytest

import oracle_lib as ol
import probe_cases as pc


def each(fn):
    """fn once per family of cases, over every case of it."""
    return pytest.mark.parametrize("family", list(pc.FAMILIES))(fn)


def test_restated_lines_and_constants_stand():
    text = open(pc.ENCODE_HIP).read()
    c = pc.constants(text)
    # what the cases rely on: a stream is cut at twice the window, a window's cut moves by at most three k-mers, sixteen
    # ranges per group, the bucket table of k_adj_fwd_targets is shorter than a window can span
    assert c.chunk == c.chunk64 and c.segs == 16 and c.span == 16 and c.sg_bits == 7 and c.l2_tile == 2048
    assert c.window_bytes == 78 << 10 and c.rows_max == 512 and c.off_cap == 1024
    for line in pc.LINES:
        assert text.count(line) >= 1
        with pytest.raises(AssertionError):
            pc.constants(text.replace(line, line[:len(line) // 2] + " " + line[len(line) // 2:]))
    with pytest.raises(AssertionError):
        pc.constants(text.replace("constexpr int kTgtSpan", "constexpr int kTgtSpam"))


def test_plan_arithmetic_pinned():
    assert {kb: pc.rc1_kcap(kb) for kb in (2, 4, 8)} == {2: 8128, 4: 8128, 8: 4640} == pc.RC1_CAP
    # the sizes the older route tests pin (tests/test_gpu_bench_routes.py)
    p = pc.plan(19, 8, 4, 1_400_000)
    assert (p.per_group, p.threads, p.rc1_cap) == (5468, 1024, 7552) == pc.rc_shape(1_400_000, 8, 4)[:1] + (1024, 7552)
    assert pc.plan(25, 8, 8, 1_100_000).rc1_cap == 4640 and pc.plan(19, 8, 4, 5_000_000).cap == 7976
    # small sets: the window holds 1024 keys, k_adj_rc1 between 256 and about 1000 records
    p = pc.plan(15, 8, 4, 6259)
    assert (p.staged, p.rows, p.per_row, p.two_level, p.gbits, p.per_group, p.threads) == (True, 1, 6144 + 1024, False, 8, 24, 64)
    assert (p.cap, p.rc1_cap, p.pass1_cap, p.rc1_sbits, p.rest_bits, p.e_sbits) == (1024, 288, 288, 8, 18, 8)
    assert (p.chunk, p.stream_max, p.n_chunks) == (2048, 4096, 4)
    p = pc.plan(23, 14, 4, 16383)
    assert (p.per_group, p.cap, p.rc1_cap, p.rc1_sbits, p.threads) == (0, 1024, 256, 8, 64)
    for n in range(0, 600 * 256, 997):
        p = pc.plan(15, 8, 4, n)
        assert p.cap == 1024 and 256 <= p.rc1_cap <= 1064 and p.cap % 8 == 0 and p.rc1_cap % 8 == 0
    # the thread variants at their thresholds (N = 2)
    assert [pc.plan(15, 2, 4, n).threads for n in (1027, 1028, 4099, 4100, 16387, 16388)] == [64, 256, 256, 512, 512, 1024]
    assert [pc.plan(15, 2, 4, n).rc1_sbits for n in (700, 1028, 4100, 6975, 16388)] == [8, 9, 10, 11, 12]
    # 2-byte keys: cap takes both parities that & ~7 leaves, and the LDS bound
    assert [pc.plan(9, 2, 2, n).cap for n in (4 * 621, 4 * 628, 31200)] == [1032, 1040, 9976]
    assert (78 * 1024 - 64) // 8 == 9976 and (78 * 1024 - 64) // 10 == 7980 and (78 * 1024 - 64) // 14 == 5700
    # KSH_RC1=marks: no group is k_adj_rc1's; KSH_RC_GROUPS=half: two levels from 2^12 k-mers, half groups at N = 14
    # with 18 key bits; KSH_RC_SCATTER=direct takes both back
    p = pc.plan(15, 8, 4, 6259, pc.ENVS["marks"])
    assert (p.rc1_cap, p.pass1_cap) == (0, -1)
    assert [pc.plan(17, 14, 4, n, pc.ENVS["half"]).two_level for n in (4095, 4096)] == [False, True]
    p = pc.plan(17, 14, 4, 5000, pc.ENVS["half"])
    assert (p.extra, p.gbits, p.ng, p.cap) == (1, 15, 32768, 1024)
    assert pc.plan(15, 14, 2, 5000, pc.ENVS["half"]).extra == 0 and pc.plan(17, 8, 4, 5000, pc.ENVS["half"]).extra == 0
    p = pc.plan(17, 14, 4, 5000, pc.ENVS["half+direct"])
    assert (p.two_level, p.extra) == (False, 0) and not pc.plan(17, 7, 4, 5000, pc.ENVS["half"]).two_level
    # 2K = N + 4 is staged at N = 2 only; a geometry with rest_bits below sbits
    assert pc.plan(3, 2, 2, 28).staged and pc.plan(3, 2, 2, 28).rest_bits == 0
    assert not pc.plan(5, 6, 2, 300).staged and not pc.plan(9, 14, 2, 3000).staged
    assert pc.plan(5, 2, 2, 300).rest_bits == 4 and pc.plan(7, 6, 2, 1500).rest_bits == 4
    assert not pc.plan(15, 8, 4, 6000, {"KSH_ADJACENCY": "probe"}).staged


def test_batch_planner_model():
    # the first-batch rule: everything at once when the (clamped) lengths add up to at most cap
    assert pc.rc_batches([1024], 1024) == (True, [(1024, {0: 1024})], False)
    fits, batches, take0 = pc.rc_batches([1025], 1024)
    assert not fits and [u for u, _ in batches] == [1024, 1] and not take0
    assert [u for u, _ in pc.rc_batches([2053], 1024)[1]] == [1024, 1024, 5]
    # a batch that ends at a range's end leaves take = 0 in the next non-empty range
    fits, batches, take0 = pc.rc_batches([600, 424, 0, 100] + [0] * 12, 1024)
    assert not fits and take0 and batches == [(1024, {0: 600, 1: 424}), (100, {3: 100})]
    fits, batches, take0 = pc.rc_batches([600, 423, 0, 100] + [0] * 12, 1024)
    assert not fits and not take0 and batches == [(1024, {0: 600, 1: 423, 3: 1}), (99, {3: 99})]
    # the slice-index space: a batch's slices take at most its keys and one bound per range and slice index
    for lens in ([1024] + [0] * 15, [64] * 16, [1] * 16, [3, 5, 1000] + [0] * 13):
        fits, batches, _ = pc.rc_batches(lens, 1024)
        assert fits
        space = sum((1 << (int(x).bit_length() - 1) if x >= 2 else 1) + 1 for x in lens)
        assert space <= 1024 + 2 * 16


@each
def test_case_is_what_it_says(family):
    for case in pc.family(family):
        assert case.env in pc.ENVS and all(e in pc.ENVS for e in case.also), case.name
        km = case.kmers
        assert (np.diff(km.astype(np.int64)) > 0).all() and (km < pc.synth.revcomp(km, case.k)).all(), case.name
        assert case.kb >= (2 if 2 * case.k - case.nbits <= 16 else 4 if 2 * case.k - case.nbits <= 32 else 8)
        got = case.branches()
        assert case.expect <= got and not (case.forbid & got), (case.name, sorted(case.expect - got), sorted(case.forbid & got))
        assert (case.expect | case.forbid) <= set(pc.BRANCHES) | set(pc.COMBOS) | {"fwd:target_in_table", "fwd:stream_buckets_in_table",
                                                                               "fwd:empty_window_and_stream"}, case.name
        for env in case.envs():
            assert case.model(env).plan.staged, (case.name, env)


def test_the_cases_cover_every_branch():
    expected, reached = set(), set()
    for case in pc.all_cases():
        expected |= case.expect
        for env in case.envs():
            reached |= case.branches(env)
    assert set(pc.BRANCHES) <= reached, sorted(set(pc.BRANCHES) - reached)
    # every branch of A - D is expected by some case under its home switches; E's come with the switches
    assert set(pc.BRANCHES) - set(pc.E_BRANCHES) - {"part:direct"} <= expected, sorted(set(pc.BRANCHES) - expected)
    under = {env: set().union(*[c.branches(env) for c in pc.cases_under(env)]) for env in pc.ENVS}
    assert set(pc.E_BRANCHES) <= under["batched"] and "part:direct" in under["half+direct"]
    assert "part:two_level" in under["half"] and "part:two_level" not in under["half+direct"]
    assert not any(b.startswith("rc1:") for b in under["marks"]) and not any(b.startswith("rc:") for b in under["batched"])


def test_what_is_asserted_goes_both_ways():
    expected, forbidden = set(), set()
    for case in pc.all_cases():
        expected |= case.expect
        forbidden |= case.forbid
    for yes, no in pc.OPPOSITES:
        event = no if yes.endswith("_fits") else yes  # (some group's pass fits in every set: the batched side is the event)
        assert event in expected and event in forbidden, event
        assert yes in expected and no in expected, (yes, no)
    # the same base, one k-mer apart, on the two sides of every edge
    by_name = {c.name: c for c in pc.all_cases()}
    for a, b in (("a-group-at-rc1-cap", "a-group-rc1-cap+1"), ("b-pass0-at-cap", "b-pass0-cap+1"),
                 ("b-pass1-at-cap", "b-pass1-cap+1"), ("d-stream-at-max", "d-stream-max+1")):
        assert by_name[b].kmers.size == by_name[a].kmers.size + 1 and np.isin(by_name[a].kmers, by_name[b].kmers).all()


def test_routes_asserted_both_ways():
    must, never = set(), set()
    for case in pc.all_cases():
        for env in case.envs():
            m, n = case.routes(env)
            assert not (m & n)
            must |= m
            never |= n
    both = {"rc_64", "rc_256", "rc_512", "rc_1024", "rc_batched", "rc_marks_groups", "scatter_two_level", "fwd_targets",
            "fwd_staged", "rc1_streamed", "tgt_parts"}
    assert both <= must and both <= never and "probe_staged" in must
    # per switch set: what it is there for
    def routes_under(env):
        m, n = set(), set()
        for case in pc.cases_under(env):
            mm, nn = case.routes(env)
            m |= mm
            n |= nn
        return m, n
    m, n = routes_under("batched")
    assert "rc_batched" in m and "rc_batched" in n and "rc_marks_groups" not in m
    m, n = routes_under("marks")
    assert "rc1_streamed" not in m and "rc_marks_groups" not in m and {"rc_batched"} <= m & n
    assert "scatter_two_level" in routes_under("half")[0] and "scatter_two_level" not in routes_under("half+direct")[0]
    assert "fwd_staged" in routes_under("staged")[0] and not ({"fwd_staged", "fwd_targets", "tgt_parts"} & routes_under("probe")[0])


@each
def test_model_verdicts_give_the_oracles_unitigs(family):
    """Two k-mers are linked where each is the other's single neighbour on the facing sides, by the model's combined
    verdicts; the chains cut elsewhere are the oracle's unitigs, string for string."""
    for case in pc.family(family):
        want = ol.Set.from_kmers(case.k, case.nbits, case.kb, case.kmers).unitigs()
        assert case.model().unitig_strings() == want, case.name


def test_verdict_classes_and_self_hits_on_a_known_set():
    # K = 3: ATA's prefix AT is its own reverse complement, and so is the suffix of the TAT it would be read as
    k = 3
    names = ["AAA", "AAC", "ATA", "CAT", "ACA"]
    km = pc.finish(np.array([ol.kmer(s) for s in names], dtype=np.uint64), k)
    m = pc.Probe(km, k, 2, 2)
    v = m.verdicts()
    at = {s: int(np.searchsorted(km, np.uint64(ol.kmer(s)))) for s in ("AAA", "ATA")}
    assert v["self_direct"][:, at["AAA"]].all() and v["self_rc"][0][at["ATA"]]
    assert "self:next_is_itself" in m.branches() and "self:prefix_is_its_own_rc" in m.branches()
    # AAA -> AAC directly; a k-mer never counts itself
    assert v["nd"][1][at["AAA"]] == 1 and m.combined()[1][at["AAA"]] == int(np.searchsorted(km, np.uint64(ol.kmer("AAC"))))
