"""The staged neighbour probe of the SPSS encode (the rc partition k_rc_*, k_adj_rc1, k_adj_rc, k_tgt_bounds / _split /
_subcuts, k_adj_fwd_targets; csrc/ksh_encode.hip) over the cases of tests/probe_cases.py: sets with a group of exactly
rc1_cap records and of one more, buckets and range sums of exactly `cap` keys and of one more, batches that end at a
range's end, every thread variant at every key width, prefix runs across a window cut, streams of exactly kStreamMax
k-mers and of one more, parts with empty windows, every class of direct and through-rc neighbours, and the k-mers
that would find themselves.  Expected values are the oracle's strings, string for string and in order (unitigs for
mode 1 -- the direct image of the neighbour table -- and the path cover for mode 0), n_strings, n_bases, and the decode
of the result is the input set; everything is exact.  Before a case runs, the model's branches are asserted, and
after each encode the routes it reports (ksh_spss_encode_routes), so a case cannot silently test something else.

The default route runs in the test process.  KSH_RC1, KSH_RC_GROUPS, KSH_RC_SCATTER and KSH_FWD are read once per
process: each switch set runs once, in a child (tests/probe_worker.py) that is handed the cases, the oracle's strings
and the expected routes, all made and asserted here.  The children run one after another; one that dies or times out
fails its test and is not run again."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import probe_cases as pc
from kmersets import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


_ORACLE = {}


def prepared(case, env):
    """What a run of the case under the switch set env needs: the set, the oracle's strings, the routes -- after the
    model's branches (under the case's home switches) have been asserted."""
    if case.name not in _ORACLE:  # (once per case: the strings do not depend on the switches)
        got = case.branches()
        assert case.expect <= got and not (case.forbid & got), (case.name, sorted(case.expect - got), sorted(case.forbid & got))
        o = ol.Set.from_kmers(case.k, case.nbits, case.kb, case.kmers)
        _ORACLE[case.name] = (o.unitigs(), o.spss())
    unitigs, spss = _ORACLE[case.name]
    must, never = case.routes(env)
    return dict(name=case.name, env=env, k=case.k, n=case.nbits, kb=case.kb, kmers=case.kmers, unitigs=unitigs, spss=spss,
                must=must, never=never)


def run_prepared(ctx, p):
    """Both modes of one prepared case against the oracle's strings, with the routes, the counts and the decode."""
    g = capi.geom(p["k"], p["n"], p["kb"])
    d = capi.DeviceSet.from_kmers(g, p["kmers"], ctx.device)
    for mode, want in ((1, p["unitigs"]), (0, p["spss"])):
        sp = ctx.spss_encode(d, mode=mode)
        routes = ctx.spss_encode_routes()
        tag = (p["name"], p["env"], mode)
        assert p["must"] <= routes and not (p["never"] & routes), (tag, sorted(p["must"] - routes), sorted(p["never"] & routes))
        assert sp.n_strings == len(want) and sp.n_bases == sum(len(s) for s in want), tag
        got = sp.to_strings()
        assert got == want, (tag, next(i for i, (a, b) in enumerate(zip(got, want)) if a != b))
        back = ctx.spss_decode(sp)
        assert back.n_keys == p["kmers"].size and np.array_equal(back.kmers(), p["kmers"]), tag


def group_of(case):
    name = case.name
    if name.startswith("a-threads"):
        return "a-threads-kb" + name[-1]
    if name.startswith("d-"):
        return "d-cuts" if name.startswith(("d-first", "d-window", "d-n", "d-run")) else \
            "d-streams" if name.startswith(("d-stream", "d-part", "d-tie", "d-one", "d-slots")) else "d-verdicts"
    return name[0]


GROUPS = ("a", "a-threads-kb2", "a-threads-kb4", "a-threads-kb8", "b", "c", "d-cuts", "d-streams", "d-verdicts")


@pytest.mark.parametrize("group", GROUPS)
def test_default_route(ctx, group):
    """The cases whose home is the default route: k_adj_rc1 for the groups that fit it and k_adj_rc for the others, the
    one-level scatter, k_adj_fwd_targets."""
    cases = [c for c in pc.cases_under("default") if group_of(c) == group]
    assert cases and {group_of(c) for c in pc.cases_under("default")} == set(GROUPS)
    for case in cases:
        run_prepared(ctx, prepared(case, "default"))


def test_the_asserted_routes_go_both_ways():
    must, never = set(), set()
    for case in pc.all_cases():
        for env in case.envs():
            p = prepared(case, env)
            must |= p["must"]
            never |= p["never"]
    both = {"rc_64", "rc_256", "rc_512", "rc_1024", "rc_batched", "rc_marks_groups", "scatter_two_level", "fwd_targets",
            "fwd_staged", "rc1_streamed", "tgt_parts"}
    assert both <= must and both <= never and "probe_staged" in must


CHILDREN = ("marks", "batched", "half", "half+direct", "staged", "probe")


@pytest.mark.parametrize("switches", CHILDREN)
def test_other_routes_in_a_child(gpu, switches, tmp_path):
    """KSH_RC1=marks (every group is k_adj_rc's: only the range sizes matter), KSH_RC1=batched (every group is
    k_adj_rc1's, a crowded one in batches), KSH_RC_GROUPS=half (the two-level scatter from 2^12 k-mers, half-bucket
    groups at N = 14), with KSH_RC_SCATTER=direct (the one-pass form at the same sizes), KSH_FWD=staged and =probe
    (the other forward forms on the forward cases), each in a process of its own."""
    env = pc.ENVS[switches]
    work = [prepared(case, switches) for case in pc.cases_under(switches)]
    assert work
    if switches == "batched":
        assert any("rc_batched" in p["must"] for p in work) and not any("rc_marks_groups" in p["must"] for p in work)
    if switches in ("staged", "probe"):
        assert all("fwd_targets" in p["never"] and "tgt_parts" in p["never"] for p in work)
        assert all(("fwd_staged" in p["must"]) == (switches == "staged") for p in work)
    path = tmp_path / "cases.pickle"
    with open(path, "wb") as f:
        pickle.dump(work, f)
    r = subprocess.run([sys.executable, os.path.join(HERE, "probe_worker.py"), str(path)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "probe ok: %d cases" % len(work) in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
