"""The coloured compacted de Bruijn graph of a KmerSetSet (capi.KssIndex.colored_graph): on oracle-built structures, a
borrowed and an owned index, the inputs as columns and a permuted subset with inner nodes.  Its strings, classes, rows
and counts are those of colored_unitigs(cols, mode=1); its links are the host reference's on the downloaded strings,
twin-symmetric, and together with the k-mer pairs inside the strings exactly the edges of the de Bruijn graph of the
selected k-mers, found by brute force; the GFA text of it verifies link by link.

Something to show: every run has links between strings of different classes, and the graph has exactly as many strings
as the host reference's painting (tests/paint_reference.py) gives the unitigs runs.  That is more strings than unitigs
wherever a class changes inside a unitig: with the permuted subset (10 changes in 315 unitigs at (9, 10), 129 in 339 at
(23, 14), by the CPU oracle's unitigs) and with the inputs at (9, 10) (1 in 490).  With the inputs of (23, 14) it is
not: the family's members differ by substitutions, every change of class along the union's graph is a branch, and none
of the oracle's 2449 unitigs holds two classes -- there the test asserts equality with the unitigs, and that the other
column list of the case does cut."""
import numpy as np
import pytest
import torch

import paint_reference as pr
import spss_links_reference as ref
from index_reference import IndexReference
from test_gpu_paint import CASES, build_both, kmer_strings
from kmersets import capi

pytestmark = pytest.mark.gpu

PICKS = [c for c in CASES if (c[0], c[1]) in ((9, 10), (23, 14))]
UNITIGS_OF_ONE_CLASS = {(23, 14)}  # with the inputs as columns no unitig holds two classes: the docstring


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", PICKS, ids=["k%d-n%d" % (c[0], c[1]) for c in PICKS])
def test_colored_graph(ctx, case):
    k, n, kb, n_sets, size, seed = case
    assert len(PICKS) == 2
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    n_nodes = okss.size()
    g = capi.geom(k, n)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    inner = list(range(n_sets, n_nodes))[::-1]
    assert len(inner) >= 2
    try:
        check_graphs(ctx, k, okss, (borrowed, owned), (list(range(n_sets)), [inner[0], 1, inner[1], 0]),
                     (k, n) not in UNITIGS_OF_ONE_CLASS)
    finally:  # (the structure goes before its context does, also when a check fails)
        owned.close()
        borrowed.close()
        dkss.close()


def check_graphs(ctx, k, okss, indexes, column_lists, inputs_cut):
    n_nodes = okss.size()
    iref = IndexReference(k, [okss.get(i).kmers() for i in range(n_nodes)], [[] for _ in range(n_nodes)])
    cut_somewhere = []
    for cols in column_lists:
        edges = None  # the brute-force edges of the selection, once per column list
        for idx in indexes:
            assert idx.canonical is True
            spss, string_class, rows, counts, off, to = idx.colored_graph(cols)
            # the nodes are those of colored_unitigs(cols, mode=1)
            u_spss, u_class, u_rows, u_counts = idx.colored_unitigs(cols, mode=1)
            strings = spss.to_strings()
            assert strings == u_spss.to_strings() and spss.n_bases == u_spss.n_bases
            assert torch.equal(string_class, u_class)
            assert np.array_equal(rows, u_rows) and np.array_equal(counts, u_counts)
            # the links are the host reference's
            assert off.dtype == to.dtype == torch.int64 and off.is_cuda and to.is_cuda
            h_off, h_to = off.cpu().numpy(), to.cpu().numpy()
            want_off, want_to = ref.links(strings, k, True)
            assert np.array_equal(h_off, want_off) and np.array_equal(h_to, want_to)
            assert ref.twin_symmetric(h_off, h_to)
            assert int(np.diff(h_off).max()) <= 4
            # something to show: the painting has cut unitigs, and links join strings of different classes
            selection = idx.select(cols)
            unitigs = ctx.spss_encode(selection, mode=1)
            _, h_start, _, h_missing = pr.class_runs(iref, unitigs.to_strings(), cols, rows, True)
            assert h_missing == 0 and spss.n_strings == len(h_start) >= unitigs.n_strings
            cut_somewhere.append(spss.n_strings > unitigs.n_strings)
            cls = string_class.cpu().numpy()
            source = np.repeat(np.arange(2 * len(strings)), np.diff(h_off))
            assert int((cls[source >> 1] != cls[h_to >> 1]).sum()) > 0
            # complete: links and inner pairs are the de Bruijn edges of the selected k-mers, each once
            if edges is None:
                edges = ref.graph_edges(kmer_strings(selection.kmers(), k), k, True)
            between = ref.link_pairs(strings, k, h_off, h_to)
            inside = ref.inner_pairs(strings, k, True)
            assert len(set(between)) == len(between) and len(set(inside)) == len(inside)
            assert not set(between) & set(inside)
            assert set(between) | set(inside) == edges
            # GFA
            lines = capi.gfa_lines(strings, k, off, to, string_class)
            pairs = ref.gfa_links_verify(lines, k)
            assert pairs == list(zip(source.tolist(), h_to.tolist()))
            segments, _ = ref.parse_gfa(lines)
            assert segments == {str(r): (s, int(c)) for r, (s, c) in enumerate(zip(strings, cls))}
    # more strings than unitigs: with the permuted subset always, with the inputs unless no unitig holds two classes
    assert all(cut_somewhere[len(indexes):]) and len(set(cut_somewhere[:len(indexes)])) == 1
    assert cut_somewhere[0] == inputs_cut
