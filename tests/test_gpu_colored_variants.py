"""The coloured graph placed on a reference (capi.KssIndex.colored_variants), on the two oracle-built structures of
tests/test_gpu_colored_bubbles.py with the inputs as columns.  An input's own path-cover strings serve as the
reference, given once as a DeviceSpss and once as a list of strings.  The first ten values are colored_bubbles'; the
located ends are the host reference's (tests/seq_locate_reference.py) on the downloaded strings; the bubbles are
placed by capi.place_bubbles and every record is checked against the reference's text.

Worked out without a GPU from the input sets, the coloured unitigs of link_bubbles_cases.colored_unitigs_of,
spss_links_reference.links, link_bubbles_reference.bubbles, seq_locate_reference.locate and capi.place_bubbles, with
the oracle's path cover of the input as the reference (the numbers do not depend on how the strings are numbered or
oriented; every located end occurs exactly once, an input's path cover holds each of its k-mers once):

    (9, 10),  input 0:  26 reference strings,  766 of  982 ends located,   8 bubbles placed, none unplaced
    (9, 10),  input 1:  32 reference strings,  778 of  982 ends located,   8 placed, none unplaced
    (23, 14), input 0:   1 reference string,  2820 of 4898 ends located, 255 placed, 3 unplaced: anchor
    (23, 14), input 1:   1 reference string,  2876 of 4898 ends located, 256 placed, 2 unplaced: anchor

An anchor is missing where the input holds neither k-mer next to the site."""
import numpy as np
import pytest
import torch

import seq_locate_reference as locate_ref
from test_gpu_paint import CASES, build_both
from kmersets import capi

pytestmark = pytest.mark.gpu

PICKS = [c for c in CASES if (c[0], c[1]) in ((9, 10), (23, 14))]
# (k, n) -> per input 0, 1: (located ends, placed bubbles, unplaced for want of an anchor)
EXPECTED = {(9, 10): ((766, 8, 0), (778, 8, 0)), (23, 14): ((2820, 255, 3), (2876, 256, 2))}


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


@pytest.mark.parametrize("case", PICKS, ids=["k%d-n%d" % (c[0], c[1]) for c in PICKS])
def test_colored_variants(ctx, case, tmp_path):
    k, n, kb, n_sets, size, seed = case
    assert len(PICKS) == 2
    sets, ocompacts, okss, dkss = build_both(ctx, k, n, kb, n_sets, size, seed)
    idx = capi.KssIndex.from_kss(dkss)
    cols = list(range(n_sets))
    try:
        bubbles = idx.colored_bubbles(cols, max_arm=8)
        strings = bubbles[0].to_strings()
        for which, (located, n_placed, n_anchor) in enumerate(EXPECTED[(k, n)]):
            reference = ocompacts[which].strings()
            as_spss = capi.DeviceSpss.from_strings(idx.g, reference, ctx.device)
            out = idx.colored_variants(as_spss, cols, max_arm=8)
            assert len(out) == 12
            # the first ten values are colored_bubbles'
            assert out[0].to_strings() == strings
            for a, b in zip(out[1:10], bubbles[1:]):
                assert np.array_equal(host(a), host(b))
            where, count = out[10], out[11]
            assert where.dtype == torch.int64 and count.dtype == torch.uint32 and where.is_cuda
            # the located ends are the reference's on the downloaded strings
            want = locate_ref.locate(strings, reference, k, idx.canonical)
            assert np.array_equal(where.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])
            assert int((want[1] > 0).sum()) == located and int((want[1] > 1).sum()) == 0
            # a list of strings as the reference gives the same
            again = idx.colored_variants(reference, cols, max_arm=8)
            assert np.array_equal(host(again[10]), want[0]) and np.array_equal(host(again[11]), want[1])
            # placed: every record spells the reference, and its ALT is no text of the reference there
            recs = capi.place_bubbles(strings, k, out[6], out[7], out[8], where, count, reference, out[9], len(cols))
            lines, counts = capi.vcf_lines(recs, ["r%d" % i for i in range(len(reference))],
                                           [len(t) for t in reference])
            assert counts == {"placed": n_placed, "anchor": n_anchor, "apart": 0, "order": 0, "off": 0}
            assert len(recs) == out[6].shape[0] == n_placed + n_anchor
            for r in recs:
                if "unplaced" in r:
                    continue
                t, at = reference[r["seq"]], r["pos"] - 1
                assert t[at:at + len(r["ref"])] == r["ref"] and r["alt"] != r["ref"]
                assert r["gt"][which] in ("0", "0/1") and len(r["gt"]) == len(cols)  # the input carries its own text
            path = tmp_path / ("input%d.vcf" % which)
            assert capi.write_vcf(str(path), recs, ["r%d" % i for i in range(len(reference))],
                                  [len(t) for t in reference]) == counts
            assert path.read_text().splitlines() == lines
    finally:  # (the structure goes before its context does, also when a check fails)
        idx.close()
        dkss.close()
