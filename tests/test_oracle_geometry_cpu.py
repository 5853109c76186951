"""The oracle's strings do not depend on the bucket geometry (CPU only).

test_gpu_geometry.py compares the GPU encode at some thirty (k, N, key width) cells with ONE oracle run per family,
made at the reference geometry (N = min(14, 2k - 1), the narrowest key; geometry_families.ref_geom).  That is
sound only because the oracle iterates a set in ascending k-mer order (oracle/ko_kmer_set.h, find()), and
bucket-major order is numeric order whatever N and the key width are.  This file pins the premise: for small
seeded families, SPSS fast and slow, unitigs, and the directed SPSS and unitigs are the same lists at every
N in {1, 2, 8, 14, 16, 20, 2k - 1} and every key width the key bits fit, and the hash is the XOR of the k-mers."""
import numpy as np
import pytest

import geometry_families as gf
import oracle_lib as ol

U = np.uint64
PREMISE = ("the oracle's strings changed with the bucket geometry: test_gpu_geometry.py compares every cell with "
           "one oracle run at the reference geometry and has lost its expected answers")


def geometries(k):
    for n in sorted({1, 2, 8, 14, 16, 20, 2 * k - 1}):
        if n >= 2 * k or n > 24:
            continue
        for kb in (1, 2, 4, 8):
            if 2 * k - n <= 8 * kb:
                yield n, kb


@pytest.mark.parametrize("k", [3, 5, 8, 11, 15, 19, 24, 25, 31])
def test_strings_do_not_depend_on_geometry(k):
    size = 3000
    for name in gf.FAMILIES:
        kmers = gf.family(name, k, size, seed=100 + k)
        assert kmers.size > 0
        want = gf.oracle_answers(ol, name, k, kmers)
        xor = int(np.bitwise_xor.reduce(kmers)) if kmers.size else 0
        for n, kb in geometries(k):
            got = gf.oracle_answers(ol, name, k, kmers, n, kb)
            for variant in want:
                assert got[variant] == want[variant], "%s: family %s, k = %d, (N, key bytes) = (%d, %d), %s" % (
                    PREMISE, name, k, n, kb, variant)
            o = ol.Set.from_kmers(k, n, kb, kmers)
            assert o.hash() == xor and np.array_equal(o.kmers(), kmers), (name, k, n, kb)


def test_geometry_list_covers_the_edges():
    """k = 3 reaches N = 5 (one key bit) with every key width; k = 31 reaches N = 20 with 8-byte keys only."""
    assert set(geometries(3)) == {(n, kb) for n in (1, 2, 5) for kb in (1, 2, 4, 8)}
    assert (20, 8) in set(geometries(31)) and (20, 4) not in set(geometries(31))
    assert (17, 1) in set(geometries(9))


def test_family_shapes():
    """The families the GPU sweep runs have the shapes their names promise at a genome-sized k."""
    k = 23
    fam = {name: gf.family(name, k, 20000, seed=7) for name in gf.FAMILIES}
    ans = {name: gf.oracle_answers(ol, name, k, x) for name, x in fam.items()}
    assert len(ans["genome"]["spss"]) < 5
    assert len(ans["difference"]["spss"]) > 300
    assert len(ans["repeats"]["unitigs"]) > 2 * len(ans["repeats"]["spss"]) > 10
    assert len(ans["random"]["spss"]) > 0.9 * fam["random"].size
    assert not np.array_equal(np.unique(gf.synth.canonical(fam["directed"], k)), fam["directed"])
    for name in gf.CANONICAL:
        assert np.array_equal(gf.synth.canonical(fam[name], k), fam[name])
        assert np.array_equal(gf.kmers_of_strings(ans[name]["spss"], k, canonical=True), fam[name])
    assert np.array_equal(gf.kmers_of_strings(ans["directed"]["spss_directed"], k, canonical=False), fam["directed"])
