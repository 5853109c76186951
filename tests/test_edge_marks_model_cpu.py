"""CPU twin of tests/test_gpu_edge_marks.py: on the arrays of the encode's model (tests/model_encode.py) for the same
generators, a unitig side whose link entry is `none` and that never had a neighbour has no edge in the model's edge
table -- what lets k_edges (csrc/ksh_encode.hip) store four `none` for it without a search -- and the cases hold
sides of every branch k_edges takes.

The model's state of a side: cnt == 0: never had a neighbour; link None and cnt > 0: the side k_link_cut marks."""
import numpy as np
import pytest

import edge_marks_cases as emc
import oracle_lib as ol
from model_encode import NONE, EncodeModel

_M = (1 << 64) - 1


def _revcomp(x, k):
    x = ~x & _M
    x = ((x >> 2) & 0x3333333333333333) | ((x & 0x3333333333333333) << 2)
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0F) | ((x & 0x0F0F0F0F0F0F0F0F) << 4)
    return int.from_bytes(x.to_bytes(8, "little"), "big") >> (64 - 2 * k)


class Model(EncodeModel):
    """(the model with a reverse complement that does not loop over the bases)"""

    def canon(self, x):
        return min(x, _revcomp(x, self.k))

    def oriented(self, t, d):
        return self.km[t] if d == 0 else _revcomp(self.km[t], self.k)


def branch_counts(kmers, k):
    """{"dead", "cut", "live"} -> unitig sides of that branch; asserts that a dead end has no edge."""
    m = Model(kmers, k)
    m.build_links()
    m.build_unitigs()
    m.build_edges()
    counts = {"dead": 0, "cut": 0, "live": 0}
    for u in range(m.n_unitigs):
        for side in (0, 1):
            t, d = m.u_members[u][0] if side == 0 else m.u_members[u][-1]
            # the side of the k-mer the state enters through (left end) or leaves through (right end)
            ks = "LR"[d ^ side]
            if m.link[ks][t] is not None:
                counts["live"] += 1
            elif m.cnt[ks][t] > 0:
                counts["cut"] += 1
            else:
                counts["dead"] += 1
                assert m.edges[2 * u + side] == [NONE] * 4, (u, side)
    return counts, m


def test_revcomp_matches_the_model():
    from model_encode import revcomp1
    rng = np.random.default_rng(1)
    for k in (15, 23, 31):
        for x in rng.integers(0, 4 ** k, size=50, dtype=np.uint64).tolist():
            assert _revcomp(x, k) == revcomp1(x, k)


@pytest.mark.parametrize("geom", emc.GEOMS)
def test_chains_are_all_dead_ends(geom):
    k = geom[0]
    kmers = emc.chains(k)
    assert 2000 <= kmers.size <= 20000
    counts, m = branch_counts(kmers, k)
    assert m.n_unitigs == 200 and counts == {"dead": 400, "cut": 0, "live": 0}


@pytest.mark.parametrize("geom", emc.GEOMS)
@pytest.mark.parametrize("name", ["tips", "bubbles"])
def test_fork_sets_have_dead_and_cut_ends(geom, name):
    k = geom[0]
    kmers = emc.fork(k, name)
    assert 2000 <= kmers.size <= 20000
    counts, m = branch_counts(kmers, k)
    assert counts["dead"] > 20 and counts["cut"] > 60 and counts["live"] == 0, counts
    # the incoming stretches: a last k-mer whose single neighbour has two on the facing side, cut by that neighbour
    pieces = emc.fork_pieces(k, name)
    seen = 0
    for piece in pieces[-24:]:
        y = m.index[m.canon(int(emc.synth.kmers_of_bases(piece, k)[-1]))]
        for ks in "LR":
            if m.cnt[ks][y] == 1 and m.link[ks][y] is None:
                x, same = m.single[ks][y]
                seen += m.cnt[ks if same else "LR"[ks == "L"]][x] >= 2
    assert seen >= 20, seen


@pytest.mark.parametrize("geom", emc.GEOMS)
def test_remainder_and_intersection_end_in_dead_ends(geom):
    k = geom[0]
    rem, inter = emc.mutated_pair(k)
    for kmers in (rem, inter):
        assert 2000 <= kmers.size <= 20000
        counts, m = branch_counts(kmers, k)
        # (a subset of one sequence's k-mers forks only where the sequence repeats a (k - 1)-mer)
        assert counts["dead"] >= 0.95 * 2 * m.n_unitigs and m.n_unitigs > 150 and counts["live"] == 0, counts


def test_loop_ends_hold_live_links():
    k = 23
    kmers = emc.loop_with_tails_elsewhere(k)
    assert 2000 <= kmers.size <= 20000
    counts, m = branch_counts(kmers, k)
    assert counts["live"] == 2 and counts["dead"] > 20 and counts["cut"] > 60, counts
    assert sorted(m.uclass.values()).count(3) == 1 and max(m.u_len) >= 3000
    assert m.spss() == ol.Set.from_kmers(k, 14, 4, kmers).spss()
