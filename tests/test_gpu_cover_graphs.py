"""The unitig-level stage of the path cover (cover_stage in csrc/ksh_encode.hip) and the kernels of csrc/ksh_cover.hip
on the designed unitig graphs of tests/cover_graph_cases.py: every case through Context.spss_cover under each of its
modes, string for string and in order against the oracle, with the sizes, the stats and the number of matching rounds
the model counts; the cases whose strings are the unitigs of their own k-mer set also through ksh_spss_encode (k_edges
builds the same graph from the set).  Then the refusals of ksh_spss_cover_plan on inputs with several violations."""
import re

import numpy as np
import pytest

import cover_graph_cases as cg
import cover_oracle
from kmersets import capi

pytestmark = pytest.mark.gpu

# (family, parts): the cases of a family run in `parts` tests, case i in test i % parts
PARTS = (("matching_rounds", 2), ("cover_loops", 8), ("walk_allowance_paths", 13), ("classes_and_order", 1),
         ("cover_kernels", 6), ("dense_fuzz", 4))


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


geom_bits = cg.geom_bits


def device_strings(ctx, k, strings):
    return capi.DeviceSpss.from_strings(capi.geom(k, geom_bits(k)), strings, ctx.device)


def run_cover(ctx, k, sp, n_in, want, rounds, **args):
    out = ctx.spss_cover(sp, **args)
    assert out.to_strings() == want
    n_bases = sum(len(s) for s in want)
    assert out.n_strings == len(want) and out.n_bases == n_bases
    assert ctx.spss_size(out) == sum(len(s) - k + 1 for s in want)
    assert ctx.spss_cover_stats() == {"unitigs": n_in, "rounds": rounds, "strings": len(want), "bases": n_bases}


def run_encode(ctx, k, oset, kmers):
    """The same graph from the k-mer set: k_edges instead of k_cover_edges, then the shared stage."""
    d = capi.DeviceSet.from_kmers(capi.geom(k, geom_bits(k)), kmers, ctx.device)
    rounds = cg.model(oset.unitigs(), k, cg.FAST).rounds  # the encode numbers its unitigs as the oracle does
    assert ctx.spss_encode(d, mode=0).to_strings() == oset.spss()
    assert ctx.spss_encode_stats()["rounds"] == rounds
    assert ("match_more_rounds" in ctx.spss_encode_routes()) == (rounds > cg.C.match_first)
    assert ctx.spss_encode(d, mode=2).to_strings() == oset.spss_slow()
    return rounds


@pytest.mark.parametrize("name,part", [(name, i) for name, parts in PARTS for i in range(parts)])
def test_cover_graphs(ctx, name, part):
    parts = dict(PARTS)[name]
    encoded = 0
    for case in cg.cases(name)[part::parts]:
        res = cg.check_case(case)  # the designed edges, expect and forbid: the case is what it says
        sp = device_strings(ctx, case.k, case.strings)
        for mode in case.modes:
            want = cover_oracle.cover(case.strings, case.k, **cg.ARGS[mode])
            run_cover(ctx, case.k, sp, len(case.strings), want, res[mode].rounds, **cg.ARGS[mode])
        own = cg.own_unitig_set(case) if cg.FAST in case.modes else None
        if own is not None:  # the strings are the unitigs of their own k-mer set: the same graph through k_edges
            run_encode(ctx, case.k, *own)
            encoded += 1
    # (tests/test_cover_graph_model_cpu.py: every family of cg.ENCODED has such cases; a part of one may have none)
    assert encoded == 0 or name in cg.ENCODED


def test_encode_takes_the_second_batch_of_rounds(ctx):
    """A K(4, 4) junction whose k-mer set the oracle spells with every predecessor before every successor: the
    encode's matching needs kMatchFirst live rounds, one more than its first batch answers."""
    k = cg.K
    strings, _ = cg.junction(np.random.default_rng(0), k, "ACGT", "ACGT")
    case = cg.Case("encode-K44", "matching_rounds", k, strings, (cg.FAST,))
    oset, kmers = cg.own_unitig_set(case)
    assert cg.model(oset.unitigs(), k, cg.FAST).rounds == cg.C.match_first + 1
    assert run_encode(ctx, k, oset, kmers) == cg.C.match_first + 1
    # and below the boundary: kMatchFirst - 1 live rounds are answered inside the first batch
    less = "ACGT"[:cg.C.match_first - 1]
    strings, _ = cg.junction(np.random.default_rng(0), k, less, less)
    oset, kmers = cg.own_unitig_set(cg.Case("encode-K33", "matching_rounds", k, strings, (cg.FAST,)))
    assert run_encode(ctx, k, oset, kmers) == cg.C.match_first


# ---------------------------------------------------------------------------------------------------- refusals
def test_cover_refusals_with_several_violations(ctx):
    """Several violations of one kind and of several kinds in one input: the kind follows the host's order (bases,
    palindrome, same ends, duplicate end; directed: duplicate first before duplicate last), a string's own fault
    names the smallest index, a repeated k-mer one of the strings that share it; sum(lens + K) one above and one
    below n_bases; and after every refusal the context still serves a good cover."""
    k = cg.REFUSAL_K
    good, refusals = cg.refusal_inputs()
    want = {c: cover_oracle.cover(good, k, canonical=c) for c in (True, False)}
    good_sp = device_strings(ctx, k, good)
    for r in refusals:
        sp = device_strings(ctx, k, r.strings)
        if r.bases_off:
            sp = capi.DeviceSpss(sp.g, sp.words, sp.lens, sp.n_strings, sp.n_bases + r.bases_off)
        with pytest.raises(capi.KshError, match=cg.MESSAGE[r.kind]) as e:
            ctx.spss_cover(sp, canonical=r.canonical)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT, r.name
        if r.named is not None:
            assert int(re.search(r"string (\d+)", str(e.value)).group(1)) in r.named, (r.name, str(e.value))
        assert ctx.spss_cover(good_sp, canonical=r.canonical).to_strings() == want[r.canonical], r.name
