"""The degenerate loop families (tests/loop_families.py) still are what they are there for -- asserted on the oracle
alone, so that a later change to synth cannot hollow test_gpu_loop_families.py out.  These are conditions on the
inputs, not tolerances: ties at the arg-max, empty nodes, a check whose improvement is negative, an interval of 3
or more, a loop that ends on weight 0 after some merges."""
import numpy as np
import pytest

import loop_families as lf
import oracle_lib as ol


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lf.oracle_build(ol, name)
        return cache[name]

    return get


def test_family_list():
    assert len(set(lf.FAMILIES)) == len(lf.FAMILIES) == 14
    assert set(lf.MIN_EMPTY_NODES) <= set(lf.FAMILIES) and set(lf.TIED) <= set(lf.FAMILIES)
    for name in lf.FAMILIES:
        k, n, kb, sets, ids = lf.family(name)
        assert 2 * k - n <= 8 * kb
        for s in sets:
            assert s.dtype == np.uint64 and np.all(s[1:] > s[:-1])              # sorted, distinct
            assert np.array_equal(s, lf.synth.canonical(s, k))
        if name not in ("sampled_23", "dups_31"):
            assert (k, n, kb) == (15, 10, 4) and np.array_equal(ids, np.arange(1 << 10))   # every bucket sampled
        else:
            assert 0 < ids.size < (1 << n) // 40


@pytest.mark.parametrize("name", lf.FAMILIES)
def test_family_is_what_its_row_says(built, name):
    k, n, kb, sets, ids, osets, ocompacts, okss = built(name)
    n0 = len(sets)
    for i in range(n0):
        assert np.array_equal(okss.get(i).kmers(), sets[i]), "Get(%d)" % i
    it = okss.iterations()
    cp, imp = okss.checkpoints()
    w0 = okss.initial_weights(n0)
    empty = sum(okss.node(i).size() == 0 for i in range(okss.size()))
    assert okss.size() == n0 + len(it)
    if name in lf.MIN_EMPTY_NODES:
        assert empty >= lf.MIN_EMPTY_NODES[name], empty
    if name in lf.TIED:
        assert w0.max() > 0 and int((w0 == w0.max()).sum()) >= 2
    if name == "one_input":
        assert okss.size() == 1 and len(it) == 0 and len(cp) == 0
    if name == "all_empty":
        assert okss.size() == 3 and len(it) == 0 and len(cp) == 0 and empty == 3
    if name == "two_identical":
        assert okss.size() == 3 and len(it) == 1
    if name == "star":
        assert w0.size == 36 and np.all(w0 == w0[0]) and len(it) == 8
    if name == "permuted_ties":
        pairs = [(a, b) for a in range(n0) for b in range(a + 1, n0)]
        assert w0[pairs.index((1, 4))] == w0[pairs.index((2, 3))] == w0.max() == 1000
        assert [(int(r[0]), int(r[1])) for r in it] == [(1, 4), (2, 3)]
        # it ended on weight 0: before the structure was exhausted, and no check said "stop"
        assert okss.size() < 2 * n0 - 1 and not np.any(cp[:, 3])
    if name in ("nested_chain", "many_small_24"):
        assert len(imp) > 0 and float(imp.min()) < 0.0, imp
        assert cp[int(np.argmin(imp)), 3] == 1                   # ... and that check stops the loop
    if name.startswith("many_small_"):
        assert n0 // 8 + 1 >= 3 and len(cp) >= 2
        assert [int(c) for c in cp[:, 0]] == [(q + 1) * (n0 // 8 + 1) for q in range(len(cp))]
    if name in ("sampled_23", "dups_31"):
        assert empty >= 1 and len(it) >= 1                     # the same kinds of edge behind the 2 % sample
