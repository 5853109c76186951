"""The bubbles of the coloured graph of a KmerSetSet (capi.KssIndex.colored_bubbles), on the two oracle-built
structures of tests/test_gpu_colored_graph.py, a borrowed and an owned index, the inputs as columns and the permuted
subset with inner nodes.  The first six values are colored_graph's; the bubbles are the host reference's on the
downloaded links; the carriers are the AND taken on the host; every allele pair begins with the last K - 1 bases of
the oriented source and ends with the first K - 1 of the oriented sink.

The expected number of bubbles at max_arm = 8, worked out without a GPU from the oracle's node sets, the coloured
unitigs of link_bubbles_cases.colored_unitigs_of, spss_links_reference.links and link_bubbles_reference.bubbles (the
number does not depend on how the strings are numbered or oriented: every bubble is reported once):

    (9, 10),  inputs 0 .. 5:        491 strings, 1632 links,   8 bubbles, every arm one string
    (9, 10),  columns [13, 1, 12, 0]: 325 strings, 1106 links,   5 bubbles, one arm of two strings (4 at max_arm = 1)
    (23, 14), inputs 0 .. 7:       2449 strings, 6568 links, 258 bubbles, every arm one string
    (23, 14), columns [21, 1, 20, 0]: 468 strings, 1162 links, 111 bubbles, 21 arms of two strings and 3 of three
                                    (87 at max_arm = 1, 108 at max_arm = 2)

Each is above 0, so each is asserted as it stands."""
import numpy as np
import pytest
import torch

import link_bubbles_reference as ref
from test_gpu_paint import CASES, build_both
from kmersets import capi

pytestmark = pytest.mark.gpu

PICKS = [c for c in CASES if (c[0], c[1]) in ((9, 10), (23, 14))]
# (k, n) -> bubbles with the inputs as columns, with the permuted subset, and the subset's at max_arm = 1
EXPECTED = {(9, 10): (8, 5, 4), (23, 14): (258, 111, 87)}


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", PICKS, ids=["k%d-n%d" % (c[0], c[1]) for c in PICKS])
def test_colored_bubbles(ctx, case):
    k, n, kb, n_sets, size, seed = case
    assert len(PICKS) == 2
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    n_nodes = okss.size()
    g = capi.geom(k, n)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    inner = list(range(n_sets, n_nodes))[::-1]
    column_lists = (list(range(n_sets)), [inner[0], 1, inner[1], 0])
    try:
        for cols, expected in zip(column_lists, EXPECTED[(k, n)][:2]):
            for idx in (borrowed, owned):
                check_bubbles(k, idx, cols, 8, expected)
        check_bubbles(k, borrowed, column_lists[1], 1, EXPECTED[(k, n)][2])
    finally:  # (the structure goes before its context does, also when a check fails)
        owned.close()
        borrowed.close()
        dkss.close()


def check_bubbles(k, idx, cols, max_arm, expected):
    out = idx.colored_bubbles(cols, max_arm=max_arm)
    assert len(out) == 10
    spss, string_class, rows, counts, off, to, ends, arm_off, arm, arm_rows = out
    # the first six values are colored_graph's
    g_spss, g_class, g_rows, g_counts, g_off, g_to = idx.colored_graph(cols)
    strings = spss.to_strings()
    assert strings == g_spss.to_strings() and torch.equal(string_class, g_class)
    assert np.array_equal(rows, g_rows) and np.array_equal(counts, g_counts)
    assert torch.equal(off, g_off) and torch.equal(to, g_to)
    # the bubbles are the reference's on the downloaded links
    cls = string_class.cpu().numpy()
    want = ref.bubbles(off.cpu().numpy(), to.cpu().numpy(), max_arm, cls, rows)
    assert ends.dtype == arm_off.dtype == arm.dtype == torch.int64 and arm_rows.dtype == torch.uint64
    got = [x.cpu().numpy() for x in (ends, arm_off, arm, arm_rows)]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    nb = len(got[0])
    assert nb == expected > 0
    # the carriers: the AND of the rows of the arm's strings, taken here
    table = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, 2)
    for a in range(2 * nb):
        members = table[cls[got[2][got[1][a]:got[1][a + 1]] >> 1]]
        assert np.array_equal(got[3][a], np.bitwise_and.reduce(members, axis=0))
        assert ref.carriers(got[3][a]) == ref.carriers(got[3][a], len(cols))
    # the alleles, textually
    alleles = capi.bubble_alleles(strings, k, ends, arm_off, arm)
    assert len(alleles) == nb
    for b, (v, w, a0, a1) in enumerate(alleles):
        assert (v, w) == (int(got[0][b, 0]), int(got[0][b, 1])) and a0 != a1
        assert a0 == ref.spell(strings, k, got[2][got[1][2 * b]:got[1][2 * b + 1]])  # (the overlaps are asserted)
        assert a1 == ref.spell(strings, k, got[2][got[1][2 * b + 1]:got[1][2 * b + 2]])
        assert a0[:k - 1] == a1[:k - 1] == ref.oriented(strings, v)[-(k - 1):]
        assert a0[-(k - 1):] == a1[-(k - 1):] == ref.oriented(strings, w)[:k - 1]
        assert a0[k - 1] < a1[k - 1]  # arm 0 is the arm of the lower base
    parsed = ref.parse_bubble_lines(capi.bubble_lines(strings, k, ends, arm_off, arm, arm_rows, len(cols)))
    assert [(p[0], p[1], p[2], p[3]) for p in parsed] == alleles
    assert [p[4] for p in parsed] == [ref.carriers(got[3][2 * b]) for b in range(nb)]
