"""The cases of tests/chain_rank_cases.py and their model, on the CPU: every case is what it says, the cases together
reach every branch of the chain ranking and the log emit that the model names, the model's unitigs and its log emit
reproduce the oracle's strings, three deliberately wrong variants of the log emit fail, and the lines and constants
of ksh_encode.hip that the model restates still stand there."""
import numpy as np
import pytest

import chain_rank_cases as crc
import oracle_lib as ol
from model_encode import EncodeModel

FAMILIES = {"small": crc.small_cases, "medium": crc.medium_cases, "l2": crc.l2_cases}  # built when a test asks


def cases(*families):
    return [c for f in (families or FAMILIES) for c in FAMILIES[f]()]


def oracle_strings(case):
    n, kb = case.geom()
    o = ol.Set.from_kmers(case.k, n, kb, case.kmers)
    if case.canonical:
        return o.unitigs(), o.spss()
    return o.unitigs_directed(), o.spss_directed()


_ORACLE = {}


def oracle(case):
    if case.name not in _ORACLE:
        _ORACLE[case.name] = oracle_strings(case)
    return _ORACLE[case.name]


def test_restated_lines_and_constants_stand():
    text = open(crc.ENCODE_HIP).read()
    c = crc.constants(text)
    # what the cases rely on: a level-2 ruler is a ruler, the logs keep the same number of states for both kinds of
    # walker, the two-level floor lies below the default, and the hash of first_phase is a 32-bit odd multiplier
    assert c.ruler_shift >= 1 and c.l2_shift >= 1 and crc.l2_every(c) % crc.every(c) == 0
    assert c.mid_rulers == c.mid_heads >= 1 and c.jump_hops >= 1 and c.match_first >= 1 and c.match_batch >= 1
    assert c.l2_floor < c.l2_default and c.hash_mul % 2 == 1 and c.hash_mul < 1 << 32
    for line in crc.LINES:
        assert text.count(line) >= 1
        with pytest.raises(AssertionError):
            crc.constants(text.replace(line, line[:len(line) // 2] + " " + line[len(line) // 2:]))
    with pytest.raises(AssertionError):
        crc.constants(text.replace("#define KSH_JUMP_HOPS", "#define KSH_JUMP_HOPZ"))


def each(fn):
    """fn once per family of cases, over every case of it."""
    return pytest.mark.parametrize("family", list(FAMILIES))(fn)


@each
def test_case_is_what_it_says(family):
    for case in cases(family):
        _is_what_it_says(case)


def _is_what_it_says(case):
    got = case.branches()
    assert case.expect <= got and not (case.forbid & got), (case.name, sorted(case.expect - got), sorted(case.forbid & got))
    # the lone k-mers are on their own: no neighbour in the set, in either orientation
    links = case.profile().links
    at = np.searchsorted(case.kmers, case.lone)
    assert (case.kmers[at] == case.lone).all()
    assert (links.cnt[:, at] == 0).all(), case.name


def test_the_cases_cover_every_branch():
    covered = set()
    for case in cases():
        covered |= case.branches()
    # every branch but the two that no set reaches through the API (UNREACHABLE_BRANCHES gives the reasons;
    # test_matching_rounds and test_no_set_of_3_mers_has_logs_that_fit assert them)
    assert set(crc.BRANCHES) - covered == set(crc.UNREACHABLE_BRANCHES), sorted(set(crc.BRANCHES) ^ covered)
    # K = 5, where the rulers fall as they may: what the committed seeds reach
    for (k, canonical), want in crc.SMALL_K_BRANCHES.items():
        got = set()
        for case in cases("small"):
            if case.k == k and case.canonical == canonical and case.name.startswith("small-k"):
                got |= case.branches()
        assert want <= got, (k, canonical, sorted(want - got))


def test_every_k_and_both_kinds_of_set_run_the_stretches():
    for k in crc.STRETCH_KS:
        for canonical in (True, False):
            got = set()
            for case in cases("small"):
                if case.k == k and case.canonical == canonical:
                    got |= case.branches()
            assert set(crc.STRETCH_BRANCHES) <= got, (k, canonical, sorted(set(crc.STRETCH_BRANCHES) - got))
            assert {"lone_sampled", "lone_unsampled", "ruler_is_end", "self_only", "string_K", "string_K+1"} <= got
            assert set(crc.DIRECTION_BRANCHES) <= got, (k, canonical)


def test_routes_asserted_both_ways():
    must, never = set(), set()
    for case in cases():
        m, n = case.routes(l2=bool(case.env))
        must |= m
        never |= n
    assert {"emit_logs", "long_stretches", "jump_two_level", "rank_stamped", "match_more_rounds"} <= must
    assert {"emit_logs", "long_stretches", "match_more_rounds"} <= never


def test_log_fit_rule_both_sides():
    fits, over = crc.log_fit_cases()
    assert fits.kmers.size == over.kmers.size
    pf, po = fits.profile(), over.profile()
    assert crc.logs_fit(pf.n, pf.n_ends) and not crc.logs_fit(pf.n, pf.n_ends + 1)
    assert po.n_ends == pf.n_ends + 1
    assert max(crc.small_k_unreachable()[n] for n in range(1, 30)) < 2  # one chain has two end k-mers


def test_jump_rounds_suffice():
    """max_rounds of the host against what a chain of that many records needs."""
    c = crc.cfg()
    for case in cases("medium", "l2"):
        p = case.profile()
        chains, _ = p.ruler_chains()
        if case.env:
            n_jump = (((p.n_dense - 1) >> (c.l2_shift + 1)) << 1) + 2
            longest = max(sum(p.level2(i) for i in ch) for ch in chains)
        else:
            n_jump, longest = p.n_dense, max(len(ch) for ch in chains)
        assert crc.rounds_needed(longest) <= crc.jump_rounds(n_jump), case.name


@each
def test_model_unitigs_equal_the_oracles(family):
    for case in cases(family):
        unitigs, _ = oracle(case)
        assert case.profile().unitig_strings() == unitigs, case.name


def test_links_equal_the_encode_models():
    for case in [c for c in cases("small") if c.canonical and c.kmers.size <= 3000][:12]:
        m = EncodeModel(case.kmers, case.k)
        m.build_links()
        assert [m.succ(s) for s in range(2 * m.n)] == case.profile().succ, case.name
        assert m.unitigs() == oracle(case)[0], case.name


@each
def test_log_emit_model_writes_the_oracles_unitigs(family):
    rc = str.maketrans("ACGT", "TGCA")
    for case in cases(family):
        if "route:stamped" in case.expect:
            continue
        unitigs, _ = oracle(case)
        p = case.profile()
        for policy in ("all", "first", "second"):
            assert p.log_emit_strings(policy) == unitigs, (case.name, policy)
        assert p.log_emit_strings("first", flip=True) == [u[::-1].translate(rc) for u in unitigs], case.name


def _fails(case, variant):
    unitigs, _ = oracle(case)
    for policy in ("all", "first", "second"):  # (with both mirror images walking, each end of a chain starts a walk)
        try:
            if case.profile().log_emit_strings(policy, variant=variant) != unitigs:
                return True
        except AssertionError:
            return True
    return False


@pytest.mark.parametrize("variant", ["steps_over_k", "long_ge", "no_arrival"])
def test_wrong_log_emit_models_fail(variant):
    """steps / K instead of (steps - 1) / K reads a log entry no walk wrote where a walk arrives at a ruler after a
    multiple of K steps; >= instead of > in the emit's is_long leaves a stretch of exactly (n_mid + 1) K steps to a
    list it is not on; without the arrival the end of a chain is never written."""
    picked = [c for c in cases("small") if c.name.startswith(("stretch-k15-", "stretch-k31-directed"))]
    failing = [c.name for c in picked if _fails(c, variant)]
    assert failing, variant
    if variant == "long_ge":
        assert "stretch-k15-canonical-top" in failing and "stretch-k31-directed-top" in failing


def test_the_cover_flips_unitigs_with_boundary_lengths():
    for case in cases("small"):
        if not (case.canonical and case.name.startswith("stretch-") and case.name.split("-")[-1] in crc.boundary_lengths(case.k)):
            continue
        unitigs, spss = oracle(case)
        flipped = crc.flipped_unitigs(unitigs, spss, case.k)
        p = case.profile()
        g = crc.boundary_lengths(case.k)[case.name.split("-", 3)[3]]
        with_length = {p.place[w.u >> 1][0] for w in p.walkers if w.steps == g}
        assert any(flipped[u] for u in with_length), case.name


def test_matching_rounds():
    c = crc.cfg()
    full, plain = crc.junction_case(full=True), crc.junction_case(full=False)
    assert full.model_rounds() == c.match_first + 1 and plain.model_rounds() <= c.match_first
    # No set takes more (UNREACHABLE_BRANCHES): a side's edges all run through one junction, and every live round
    # matches the pair of the junction's live edge of smallest priority.  So the live rounds of any set are at most
    # the sides a side of its fullest junction -- four bases, four sides -- and the empty round after them is the fifth.
    assert 4 + 1 <= c.match_first + c.match_batch
    m = EncodeModel(full.kmers, full.k)
    m.spss()
    for v in range(2 * m.n_unitigs):
        across = [w for w in m.edges[v] if w != -1]
        assert len(across) <= 4 and all(sorted(x for x in m.edges[w] if x != -1) == sorted(
            x for x in m.edges[across[0]] if x != -1) for w in across), "the sides across a side see the same sides"


def test_no_set_of_3_mers_has_logs_that_fit():
    """UNREACHABLE_BRANCHES["log_emit@run0"]: sets as read by counting, canonical sets one by one."""
    import itertools

    fit = crc.small_k_unreachable()
    assert all(fit[n] < 2 for n in range(1, 30))  # a chain has two end k-mers; a set without end k-mers is loops
    assert all(fit[n] < n - 16 for n in range(30, 65))  # as read: n edges out of 16 2-mers, n - 16 end k-mers at least
    full = np.unique(crc.synth.canonical(np.arange(64, dtype=np.uint64), 3))
    assert full.size == 32
    for drop in range(3):  # the canonical sets of 32, 31 and 30 3-mers
        for out in itertools.combinations(range(32), drop):
            kmers = np.delete(full, list(out))
            assert not crc.logs_fit(kmers.size, crc.Links(kmers, 3, True).ends.size)


def test_placement_gives_every_k_mer_its_kind():
    """Builder.place and _fill on their own: at K = 9, where the gap below a k-mer rarely holds the lone k-mers it
    needs and the gaps further down take the rest, every k-mer with a wanted kind and phase has it in the set, the
    other k-mers of the sequences are all there, and the lone k-mers have no neighbour."""
    c = crc.cfg()
    ev, ev2 = crc.every(c), crc.l2_every(c)
    for k, kinds, pad, canonical in ((9, ("ruler", "ruler"), 2500, True), (9, ("ruler", "ruler"), 2500, False),
                                     (15, ("ruler", "l2"), 0, True), (15, ("ruler", "l2"), 0, False)):
        placed = 0
        for seed in range(6):
            b = crc.Builder(k, canonical, 1000 + seed)
            seqs = [b.grow(n) for n in (300, 200, 150, 90)]
            rng = np.random.default_rng(seed)
            for seq in seqs:
                for j in range(seq.size):
                    b.want(seq, j, "none" if j % 2 else "free")
                for j in rng.choice(seq.size, size=3, replace=False):
                    b.want(seq, int(j), kinds[int(rng.integers(0, 2))], int(rng.integers(0, 2)))
            seqs.append(b.grow(400))  # "any"
            try:
                kmers = b.place("any", pad_to=pad)
            except crc.PlacementError:
                continue
            placed += 1
            assert kmers.size >= pad and (np.diff(kmers.astype(np.int64)) > 0).all()
            base = np.concatenate(seqs)
            base = crc.synth.canonical(base, k) if canonical else base
            assert np.isin(base, kmers).all() and not np.isin(b.lone, base).any()
            assert kmers.size == base.size + b.lone.size
            for x, (kind, phase) in b.status.items():
                t = int(np.searchsorted(kmers, np.uint64(x)))
                assert int(kmers[t]) == x
                assert {"none": t % ev != 0, "ruler": t % ev == 0 and t % ev2 != 0, "l2": t % ev2 == 0,
                        "free": t % ev2 != 0, "any": True}[kind], (kind, t)
                assert phase is None or crc.first_phase(2 * t, c) == phase
            links = crc.Links(kmers, k, canonical)
            assert (links.cnt[:, np.searchsorted(kmers, b.lone)] == 0).all()
        assert placed >= 4, "the seeds of this test no longer place"
