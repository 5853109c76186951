"""The model of tests/cover_graph_cases.py against the oracle, on every case of every family (no GPU): the model's
strings equal cover_oracle.cover under every mode of the case (and the oracle's own C API where the canonical fast
cover applies); every case reaches what it expects and nothing it forbids, with exactly its designed edges; every
family reaches, between its cases, exactly the branches its docstring lists; the walk allowance covers the worst
schedule; the anchors in the kernels' text each stand there once."""
import pytest

import cover_graph_cases as cg
import cover_oracle

FAMILY_NAMES = [f.__name__ for f in cg.FAMILIES]


def test_anchors_match_once():
    for what, found, wanted in cg.anchor_counts():
        assert found == wanted, (what, found, wanted)
    c = cg.constants()
    assert c == cg.C and c.match_first >= 2 and c.match_batch >= 1 and c.jump_hops >= 1 and c.emit_run >= 2


def test_table_sizing_rule():
    for n in list(range(1, 70)) + [3000, 4096, 4097]:
        cap = cg.table_cap(n)
        assert cap & (cap - 1) == 0 and cap >= 4 * n and (cap == 1 or cap // 2 < 4 * n)
    assert [cg.table_cap(n) for n in (1, 2, 3, 4, 5)] == [4, 8, 16, 16, 32]


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_model_equals_oracle(name):
    for case in cg.cases(name):
        res = cg.check_case(case)  # designed edges, expect, forbid
        assert set(res) == set(case.modes) and case.strings
        for mode, r in res.items():
            want = cover_oracle.cover(case.strings, case.k, **cg.ARGS[mode])
            assert r.strings == want, (case.name, mode)
            if mode == cg.FAST:
                assert r.strings == cover_oracle.oracle_capi_cover(case.strings, case.k), case.name
            # the model's (sid, koff, flip) spell the same strings, base by base, as k_cover_emit places them
            assert sorted(set(r.sid.tolist())) == list(range(len(want)))
            for u in range(0, len(case.strings), max(1, len(case.strings) // 50)):
                s = cg.revcomp_string(case.strings[u]) if r.flip[u] else case.strings[u]
                at = int(r.koff[u])
                assert want[int(r.sid[u])][at:at + len(s)] == s, (case.name, mode, u)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_family_reaches_its_branches(name):
    fn = {f.__name__: f for f in cg.FAMILIES}[name]
    listed = set(fn.__doc__.split("Branches: ")[1].split(", "))
    reached = cg.tracked_branches(name)
    assert reached == listed, (sorted(reached - listed), sorted(listed - reached))


def test_families_cover_what_the_issue_lists():
    c = cg.C
    rounds = cg.FAMILY_BRANCHES["matching_rounds"]
    assert {"rounds=%d" % r for r in range(1, c.match_first + 2)} <= rounds  # 1 .. R + 1, R = kMatchFirst
    assert {"first_batch_full_less_one", "second_batch"} <= rounds and "third_batch" not in rounds
    loops = cg.FAMILY_BRANCHES["cover_loops"]
    assert {"loop_len=%d" % n for n in (2, 3, 4, 63, 64, 65, 4096, 10 ** 4 + 1)} <= loops
    kernels = cg.FAMILY_BRANCHES["cover_kernels"]
    assert {"%s_phase=%d" % (e, p) for e in ("first", "last") for p in range(32)} <= kernels
    assert {"table_wrap", "run_crosses_in_flipped", "run_spans=3"} <= kernels
    p = c.jump_hops + 1
    lengths, powers = cg.walk_lengths(), cg.step_powers()
    assert lengths[:4] == [(p - 1) // 2, (p - 1) // 2 + 1, (p * p - 1) // 2, (p * p - 1) // 2 + 1]
    assert 2 * lengths[-2] + 1 > 7 * 10 ** 4 > 2 * lengths[-4] + 1
    assert powers[0] == p and all(b == a * p for a, b in zip(powers, powers[1:]))
    assert powers[-1] > 7 * 10 ** 4 > powers[-2]
    singles = {case.name for case in cg.cases("walk_allowance_paths")}
    for n in lengths + [x for q in powers for x in (q - 1, q)] + [q + 1 for q in powers if q < 2 * 10 ** 4]:
        assert {"walk-%d" % n, "walk-%d-reversed" % n, "walk-%d/shuffled" % n, "walk-%d/shuffled+rc" % n} <= singles
    # every phase sweep runs at every k the issue names
    names = {case.name for case in cg.cases("cover_kernels")}
    assert {"phase-k%d-%d" % (k, p) for k in (2, 3, 16, 17, 31) for p in range(32)} <= names


def test_walk_allowance_covers_the_worst_schedule():
    """One path through all n_u strings is the longest walk n_u strings can hold: its worst-case need (every hop
    reads a successor not yet updated, so a record's reach grows (kJumpHops + 1)-fold per launch, plus the launch
    that changes nothing) stays within the host's walk_rounds -- for n_u = 1 .. 2000 and at every L of the family.
    With one launch to spare at least: the need is at most ceil(log(L)) + 1 launches (logarithms to the base
    kJumpHops + 1), the allowance at least floor(log(2 L)) + 3 >= ceil(log(L)) + 2."""
    base = cg.C.jump_hops + 1
    for n_u in list(range(1, 2001)) + cg.WALK_SINGLES:
        need, allow = cg.walk_need(n_u), cg.walk_allowance(n_u)
        assert need + 1 <= allow, (n_u, need, allow)
        # the need in closed form: the first state is n_u - 1 hops from the last; r launches finish the states up
        # to base^r - 1 hops away (the hop after the one that arrives reads the last state's done flag), and one
        # launch more finds nothing to change
        r, reach = 0, 1
        while reach < n_u:
            reach *= base
            r += 1
        assert need == r + 1, (n_u, need, r)
    # where the host's formula steps, and where the need does
    for p in cg.step_powers():
        assert cg.walk_allowance(p) == cg.walk_allowance(p - 1) + 1, p
        assert cg.walk_allowance(p + 1) == cg.walk_allowance(p), p
        assert cg.walk_need(p + 1) == cg.walk_need(p) + 1 and cg.walk_need(p) == cg.walk_need(p - 1) or p == base, p
    powers = cg.step_powers()
    assert all(cg.walk_allowance(n + 1) == cg.walk_allowance(n) for n in range(1, 2000) if n + 1 not in powers)
    # the issue's L (2 L about a power) lie between two steps: the same allowance on both sides
    for lo, hi in zip(cg.walk_lengths()[0::2], cg.walk_lengths()[1::2]):
        assert hi == lo + 1 and cg.walk_allowance(hi) == cg.walk_allowance(lo)


def test_every_encoded_family_has_unitig_sets_of_their_own():
    """The cases that are the unitigs of their own k-mer set also go through the encode on the GPU: every family
    but the loops has some, at the small k too."""
    ks = set()
    for name in cg.FAMILY_BRANCHES:
        own = [case for case in cg.cases(name) if cg.FAST in case.modes and cg.own_unitig_set(case) is not None]
        assert bool(own) == (name in cg.ENCODED), (name, len(own))
        ks |= {case.k for case in own}
    assert ks >= {2, 3, 4, 5, cg.K, 16, 17, 31}


def test_refusal_inputs_violate_what_they_say():
    good, refusals = cg.refusal_inputs()
    k = cg.REFUSAL_K
    assert len(good) == 14 and cg.violations(good, k, True) == {} and cg.violations(good, k, False) == {}
    kinds = set()
    for r in refusals:
        v = cg.violations(r.strings, k, r.canonical)
        if r.bases_off:
            assert r.kind == cg.BASES
        else:
            # what the host reports: the first kind, in its order, that some string violates
            assert [kind for kind in cg.HOST_ORDER[r.canonical] if kind in v][0] == r.kind, r.name
            own_fault = r.kind in (cg.PALINDROME, cg.SAME_ENDS)
            assert r.named == ({min(v[r.kind])} if own_fault else v[r.kind]), r.name
        kinds.add((r.kind, len(v)))
    assert {kind for kind, _ in kinds} == set(cg.MESSAGE)
    assert any(n >= 3 for kind, n in kinds if kind == cg.BASES)  # several kinds beside a wrong n_bases
    several = [r for r in refusals if len(cg.violations(r.strings, k, r.canonical).get(r.kind, ())) >= 3]
    assert {r.kind for r in several} >= {cg.PALINDROME, cg.SAME_ENDS, cg.DUP_END, cg.DUP_FIRST, cg.DUP_LAST}
