"""Coloured unitigs of a KmerSetSet (capi.KssIndex.colored_unitigs): on oracle-built structures, a borrowed and an
owned index, the inputs as columns and a permuted subset with an inner node.  The strings hold the union selection
and nothing else, each paints as one run of its own class, the positions per class are the class counts, there are as
many strings as the uncut strings have runs, and they are the host reference's cut of the uncut strings at the runs of
the host reference's painting.

The counts: the table of color_classes(cols) has the zero row where some k-mer of the structure lies outside every
column.  No column holds such a k-mer, so it is in no string: the positions of every class with a non-zero row equal
its count, and the zero row, if the table has it, has no string."""
import numpy as np
import pytest
import torch

import paint_reference as pr
from index_reference import IndexReference
from spss_cut_reference import cut
from test_gpu_paint import CASES, build_both
from kmersets import capi

pytestmark = pytest.mark.gpu

PICKS = [c for c in CASES if (c[0], c[1]) in ((9, 10), (23, 14), (23, 18))]


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", PICKS, ids=["k%d-n%d" % (c[0], c[1]) for c in PICKS])
def test_colored_unitigs(ctx, case):
    k, n, kb, n_sets, size, seed = case
    assert len(PICKS) == 3
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    n_nodes = okss.size()
    ref = IndexReference(k, [okss.get(i).kmers() for i in range(n_nodes)], [[] for _ in range(n_nodes)])
    g = capi.geom(k, n)
    comps = [capi.DeviceSpss.from_strings(g, dkss.node_strings(i), ctx.device) for i in range(n_nodes)]
    owned = capi.KssIndex.from_nodes(ctx, comps, [dkss.children(i) for i in range(n_nodes)])
    borrowed = capi.KssIndex.from_kss(dkss)
    inner = list(range(n_sets, n_nodes))[::-1]
    assert len(inner) >= 2
    for cols in (list(range(n_sets)), [inner[0], 1, inner[1], 0]):
        want_rows, want_counts = ref.color_classes(cols)
        for idx in (borrowed, owned):
            spss, string_class, rows, counts = idx.colored_unitigs(cols)
            assert string_class.dtype == torch.int32 and string_class.is_cuda
            assert string_class.numel() == spss.n_strings
            assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts)
            # the structure's own answer has something to show
            selection = idx.select(cols)
            uncut = ctx.spss_encode(selection, mode=0)
            off, start, cls, missing = idx.class_runs(uncut, rows, cols)
            n_runs = int(start.numel())
            assert rows.shape[0] >= 3 and n_runs > uncut.n_strings and missing == 0
            # same set
            back = ctx.spss_decode(spss)
            got_off, got_keys = back.to_numpy()
            want_off, want_keys = selection.to_numpy()
            assert back.n_keys == selection.n_keys > 0
            assert np.array_equal(got_off, want_off) and np.array_equal(got_keys, want_keys)
            # monochrome
            m_off, m_start, m_cls, m_missing = idx.class_runs(spss, rows, cols)
            assert m_missing == 0 and m_start.numel() == spss.n_strings and not bool(m_start.any())
            assert torch.equal(m_off.cpu(), torch.arange(spss.n_strings + 1, dtype=torch.int64))
            assert torch.equal(m_cls, string_class)
            # counts
            lens = spss.lens[:spss.n_strings].cpu().numpy().view(np.uint32).astype(np.int64)
            per_class = np.bincount(string_class.cpu().numpy(), weights=None, minlength=rows.shape[0])
            positions = np.zeros(rows.shape[0], dtype=np.int64)
            np.add.at(positions, string_class.cpu().numpy(), lens + 1)
            zero = ~rows.any(axis=1)
            assert np.array_equal(positions[~zero], counts[~zero]) and not positions[zero].any()
            assert per_class[~zero].all() and int(positions.sum()) == selection.n_keys
            # string count
            assert spss.n_strings == n_runs
            # against the host
            strings = uncut.to_strings()
            h_off, h_start, h_cls, h_missing = pr.class_runs(ref, strings, cols, rows, True)
            assert h_missing == 0
            want_strings, want_lens, want_bases = cut(strings, k, h_off, h_start)
            assert len(want_strings) > len(strings) and max(len(s) for s in want_strings) > k
            assert spss.to_strings() == want_strings and spss.n_bases == want_bases
            assert np.array_equal(lens, want_lens.astype(np.int64))
            assert np.array_equal(string_class.cpu().numpy(), h_cls)
    owned.close()
    borrowed.close()
    dkss.close()
