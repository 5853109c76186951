"""The chain ranking and the log emit of the SPSS encode (k_rank_walk, k_rank_heads, k_ruler_jump, k_l2_*,
k_choose_ends, k_rulers_done, emit_logged and its callers, the stamped pass after a loop; csrc/ksh_encode.hip) over
the cases of tests/chain_rank_cases.py: rulers placed so that every stretch length, arrival kind, walker, level-2
configuration, loop and side of the log-fit rule that the model names is present.  Expected values are the oracle's
strings, string for string and in order (unitigs for mode 1, the path cover for mode 0), and the decode of the result
is the input set; everything is exact.  Before a case runs, the model's branches are asserted, and after each encode
the routes it reports (ksh_spss_encode_routes), so a case cannot silently test something else.

The default route runs in the test process.  KSH_RANK_PHASES=1, KSH_RANK_PHASES=2, KSH_L2_MIN=4096 and the last two
together are read once per process: each runs once, in a child (tests/chain_rank_worker.py) that is handed the cases,
the oracle's strings and the expected routes, all made and asserted here."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import chain_rank_cases as crc
import oracle_lib as ol
from kmersets import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


_PREPARED = {}
_ORACLE = {}


def prepared(case, l2=False):
    """What a run of the case needs: the set, the oracle's strings, the routes, the rounds -- after the model's
    branches have been asserted."""
    key = (case.name, l2)
    if key not in _PREPARED:
        if case.name not in _ORACLE:  # (once per case: the strings do not depend on the switches)
            got = case.branches()
            assert case.expect <= got and not (case.forbid & got), (case.name, sorted(case.expect - got), sorted(case.forbid & got))
            n, kb = case.geom()
            o = ol.Set.from_kmers(case.k, n, kb, case.kmers)
            _ORACLE[case.name] = (n, o.unitigs(), o.spss()) if case.canonical else (n, o.unitigs_directed(), o.spss_directed())
        n, unitigs, spss = _ORACLE[case.name]
        must, never = case.routes(l2)
        _PREPARED[key] = dict(name=case.name, k=case.k, n=n, canonical=case.canonical, kmers=case.kmers, unitigs=unitigs,
                              spss=spss, must=must, never=never, rounds=case.model_rounds() if case.want_rounds else None)
    return _PREPARED[key]


def run_prepared(ctx, p):
    """Both modes of one prepared case against the oracle's strings, with the routes, n_bases and the decode."""
    g = capi.geom(p["k"], p["n"])
    d = capi.DeviceSet.from_kmers(g, p["kmers"], ctx.device)
    for mode, want in ((1, p["unitigs"]), (0, p["spss"])):
        sp = ctx.spss_encode(d, mode=mode, canonical=p["canonical"])
        routes = ctx.spss_encode_routes()
        must = p["must"] - ({"match_more_rounds"} if mode == 1 else set())
        assert must <= routes and not (p["never"] & routes), (p["name"], mode, sorted(must - routes), sorted(p["never"] & routes))
        if mode == 0 and p["rounds"] is not None:
            assert ctx.spss_encode_stats()["rounds"] == p["rounds"], (p["name"], ctx.spss_encode_stats())
        assert sp.n_strings == len(want) and sp.n_bases == sum(len(s) for s in want), (p["name"], mode)
        got = sp.to_strings()
        assert got == want, (p["name"], mode, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b))
        back = ctx.spss_decode(sp, canonical=p["canonical"])
        assert back.n_keys == p["kmers"].size and np.array_equal(back.kmers(), p["kmers"]), (p["name"], mode)


def small_groups():
    groups = {}
    for case in crc.small_cases():
        key = "k%d" % case.k if case.name.startswith(("stretch-", "small-k")) else "strings-and-rounds"
        groups.setdefault(key, []).append(case)
    return groups


GROUPS = ["k3", "k5"] + ["k%d" % k for k in crc.STRETCH_KS] + ["strings-and-rounds"]


@pytest.mark.parametrize("group", GROUPS)
def test_stretches_default_route(ctx, group):
    """Items 1, 2, 3 and 7 and the matching rounds, on the default route (both phases of the ranking walks, as
    under KSH_RANK_PHASES=2: these sets are below the size at which one launch takes all walkers)."""
    cases = small_groups()[group]
    assert cases
    for case in cases:
        run_prepared(ctx, prepared(case))


def test_jumping_log_fit_and_loops_default_route(ctx):
    """Item 6, the single-level jumping of item 4 and the loops of item 5 without KSH_L2_MIN; the sets built for
    KSH_L2_MIN run here too, on the single-level route (chains of some 1800 ruler records through k_ruler_jump)."""
    for case in crc.medium_cases() + crc.l2_cases():
        run_prepared(ctx, prepared(case))


def test_the_asserted_routes_go_both_ways():
    must, never = set(), set()
    for case in crc.all_cases():
        p = prepared(case, l2=bool(case.env))
        must |= p["must"]
        never |= p["never"]
    assert {"emit_logs", "long_stretches", "jump_two_level", "rank_stamped", "match_more_rounds"} <= must
    assert {"emit_logs", "long_stretches", "match_more_rounds"} <= never


CHILDREN = {"KSH_RANK_PHASES=1": {"KSH_RANK_PHASES": "1"}, "KSH_RANK_PHASES=2": {"KSH_RANK_PHASES": "2"},
            "KSH_L2_MIN=4096": {"KSH_L2_MIN": "4096"},
            "KSH_L2_MIN=4096,KSH_RANK_PHASES=2": {"KSH_L2_MIN": "4096", "KSH_RANK_PHASES": "2"}}


@pytest.mark.parametrize("knobs", list(CHILDREN))
def test_other_routes_in_a_child(gpu, knobs, tmp_path):
    """The one-launch ranking walks, the two phases forced, and the two-level jumping at its floor (with it, the sets
    of items 4 and 5 that need it), each in a process of its own."""
    env = CHILDREN[knobs]
    l2 = "KSH_L2_MIN" in env
    # the cases a switch applies to: below 4096 ruler records KSH_L2_MIN changes nothing, so its children take the
    # sets built for it and the other children all the rest; the one-launch race of mirror images also gets two of
    # the large sets (chains of some 1800 ruler records, the loops of 3000 k-mers)
    cases = crc.l2_cases() if l2 else crc.small_cases() + crc.medium_cases()
    if env == {"KSH_RANK_PHASES": "1"}:
        cases = cases + [c for c in crc.l2_cases() if c.name in ("l2-chains", "loops-l2")]
        assert len(cases) == len(crc.small_cases() + crc.medium_cases()) + 2
    work = [prepared(case, l2) for case in cases]
    assert all(("jump_two_level" in p["must"]) != ("rank_stamped" in p["must"]) for p in work) or not l2
    if l2:
        assert any("jump_two_level" in p["must"] for p in work) and any("rank_stamped" in p["must"] for p in work)
    path = tmp_path / "cases.pickle"
    with open(path, "wb") as f:
        pickle.dump(work, f)
    r = subprocess.run([sys.executable, os.path.join(HERE, "chain_rank_worker.py"), str(path)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "chain rank ok: %d cases" % len(work) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
