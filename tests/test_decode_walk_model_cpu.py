"""CPU checks of the decode walk sweep (tests/decode_walk_cases.py): the constants and restated lines read from
ksh_decode.hip, the model's arithmetic at its edges, the branch list -- every name is some case's expectation and
every case's expectations hold --, the numpy reference against the oracle on the small cases, and the windows the
decoder must not emit against the k-mers it must.  tests/test_gpu_decode_walk.py runs the cases."""
import numpy as np
import pytest

import decode_walk_cases as dw
import oracle_lib as ol
from kmersets import synth

U = np.uint64
ALL = dw.all_cases()
IDS = [c.name for c in ALL]
SMALL = [c for c in ALL if c.n_occ <= dw.ORACLE_MAX]


def test_constants_read_from_the_kernel():
    cfg = dw.constants()
    assert cfg == dw.Cfg(kDecThreads=1024, kDecSgBits=7, kDecL1Threads=1024, per_narrow=8, per_wide=4,
                         kDecL2Threads=256, kDecL2Per=8, kColTeams=16, kCoarseBits=14, max_groups=512,
                         group_words=256, l2_min_floor=1024, l2_min_default_bits=20, max_two_level_bits=15)
    assert [dw.l1_tile_positions(g, cfg) for g in (dw.Geom(16, 14, 4), dw.Geom(31, 14, 8), dw.Geom(16, 20, 2),
                                                   dw.Geom(31, 20, 8))] == [8192, 4096, 8192, 4096]
    # a changed constant is noticed, a missing constant or restated line refused
    text = open(dw.DECODE_HIP).read()
    assert dw.constants(text.replace("constexpr int kDecSgBits = 7;", "constexpr int kDecSgBits = 6;")).kDecSgBits == 6
    assert dw.constants(text.replace("std::min<int64_t>(512, (*n_words + 255) / 256)",
                                     "std::min<int64_t>(256, (*n_words + 511) / 512)"))[9:11] == (256, 512)
    assert dw.constants(text.replace(": int64_t(1) << 20;", ": int64_t(1) << 21;")).l2_min_default_bits == 21
    assert dw.constants(text.replace("nbits_w <= 15 &&", "nbits_w <= 14 &&")).max_two_level_bits == 14
    assert dw.constants(text.replace("== 8 ? 4 : 8;", "== 8 ? 2 : 8;")).per_wide == 2
    for gone in ("constexpr int kDecL2Per = 8;", "constexpr int kColTeams = 16;", "(*n_words + 255) / 256", "atoll(e)",
                 "nbits_w > kDecSgBits") + dw.RESTATED:
        with pytest.raises(AssertionError):
            dw.constants(text.replace(gone, "//"))


def test_geometry_edges():
    geo = dw.geometry
    assert geo(1) == (1, 2, 1, 1) and geo(32) == (1, 2, 1, 1) and geo(33) == (2, 2, 1, 2) and geo(64)[1] == 2
    assert geo(65)[1] == 3 and geo(256 * 32) == (256, 129, 1, 256) and geo(256 * 32 + 1) == (257, 130, 2, 129)
    assert [geo(w * 32)[2:] for w in (3840, 3841, 4096, 4097)] == [(15, 256), (16, 241), (16, 256), (17, 241)]
    assert geo(131072 * 32)[2:] == (512, 256) and geo(131073 * 32)[2:] == (512, 257)
    # 512 groups of 257 words: group 510 holds the last three words, group 511 starts past the end
    assert 510 * 257 == 131070 and 511 * 257 > 131073
    assert "empty_last_group" in dw.case_named("group-cap").branches()


def test_l2_spans():
    tile = 2048
    counts = np.zeros(128, dtype=np.int64)
    counts[[5, 6, 9, 127]] = (tile + 10, tile - 10, 5, tile + 1)
    # tile 0 in 5; tile 1: 10 of 5 and all of 6; tile 2: 9 and 127 (far: 119 wide); tile 3: the last key, in 127
    assert dw.l2_spans(counts) == [(5, 1), (5, 2), (9, 119), (127, 1)]
    assert dw.l2_spans(np.full(128, 16)) == [(0, 128)]
    counts[:] = 0
    counts[127] = 2 * tile
    assert dw.l2_spans(counts) == [(127, 1), (127, 1)]


def test_routes():
    """Which cases scatter in two levels in each of the three processes; the pair on the default switch."""
    below, at = dw.case_named("switch-1048575"), dw.case_named("switch-1048576")
    assert (below.n_occ, at.n_occ) == ((1 << 20) - 1, 1 << 20)
    assert dw.route(below, dw.ENVS["default"]) == "direct" and dw.route(at, dw.ENVS["default"]) == "two_level"
    assert dw.route(below, dw.ENVS["l2min"]) == "two_level" and dw.route(at, dw.ENVS["direct"]) == "direct"
    # KSH_DECODE_L2_MIN has a floor
    assert dw.two_level_min({"KSH_DECODE_L2_MIN": "5"}) == 1024 and dw.two_level_min({"KSH_DECODE_L2_MIN": "4096"}) == 4096
    by_env = {env: [c.name for c in ALL if dw.route(c, dw.ENVS[env]) == "two_level"] for env in dw.ENVS}
    assert by_env["default"] == ["group-cap", "switch-1048576"] and by_env["direct"] == []
    still_direct = [c for c in ALL if dw.route(c, dw.ENVS["l2min"]) == "direct"]
    assert len(by_env["l2min"]) == len(ALL) - len(still_direct) >= 40
    assert all(c.n_occ < 1024 or c.g.n <= 7 for c in still_direct) and len(still_direct) == 9


def test_every_branch_is_reached():
    names = [c.name for c in ALL]
    assert len(set(names)) == len(names)
    aimed = set()
    for c in ALL:
        aimed |= c.expect
    assert set(dw.BRANCHES) - aimed == set()
    assert len(dw.BRANCHES) == len(set(dw.BRANCHES))


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_every_case_is_what_it_says(case):
    """The model finds the branches the case aims at, and none of those it must avoid; its validity test (the
    kernels' end-bit window) marks exactly the positions the reference keeps (the strings' own last K - 1 bases)."""
    got = case.branches()
    assert case.expect <= got and not (case.forbid & got), (sorted(case.expect - got), sorted(case.forbid & got))
    valid, _ = dw.valid_positions(case)
    starts = np.cumsum(case.lens) - case.lens
    want = np.zeros(valid.size, dtype=bool)
    for s, ln in zip(starts.tolist(), case.lens.tolist()):
        want[s:s + ln - case.g.k + 1] = True
    assert np.array_equal(valid, want)
    assert case.occurrences(False).size == case.n_occ == int(valid.sum())
    assert case.n_bases < 1 << 23 and (case.n_bases <= 200000 or case.family in ("groups", "switch"))
    words, lens = case.words_and_lens()
    assert words.size == dw.geometry(case.n_bases).n_words and synth.unpack_strings(words, lens, case.g.k) == case.strings
    pad = -case.n_bases % 32
    if pad:
        assert int(words[-1]) & ((1 << (2 * pad)) - 1) == ((1 << (2 * pad)) - 1 if case.pad_ones else 0)


def test_tiles_of_the_aimed_cases():
    """What the tile cases were sized by."""
    tile_words, tiles = dw.l1_tiles(dw.case_named("poly-a-tile"))
    assert tile_words == 256 and [t[:3] for t in tiles] == [(0, 0, 256), (1, 256, 256)] and tiles[0][3] == 8192
    assert np.all(dw.case_named("poly-a-tile").occurrences(True)[:8192] == 0)
    tile_words, tiles = dw.l1_tiles(dw.case_named("group-cap"))
    assert tile_words == 256 and [t[:3] for t in tiles[:2]] == [(0, 0, 256), (0, 256, 1)]
    assert tiles[-1][:3] == (510, 510 * 257, 3) and len(tiles) == 510 * 2 + 1
    tile_words, tiles = dw.l1_tiles(dw.case_named("groups-4096-words"))
    assert tile_words == 128 and len(tiles) == 32 and all(t[2] == 128 for t in tiles)
    for name, want in (("l2-one-16-14-4", [(37, 1), (37, 1), (37, 1)]), ("l2-seam-16-14-4", [(37, 2), (38, 1)]),
                       ("l2-last-16-14-4", [(126, 1), (126, 2), (127, 1)]), ("l2-last-31-20-8", [(126, 1), (126, 2), (127, 1)])):
        c = dw.case_named(name)
        sg = (c.occurrences(False) >> U(2 * c.g.k - 7)).astype(np.int64)
        assert dw.l2_spans(np.bincount(sg, minlength=128)) == want, name
    assert sorted({dw.scatter_bytes(g) for g in dw.WIDE_GEOMS}) == [2, 4, 8]
    assert [dw.scatter_bytes(g) for g in dw.WIDE_GEOMS] == [2, 4, 4, 8]


@pytest.mark.parametrize("case", SMALL, ids=[c.name for c in SMALL])
def test_reference_is_the_oracle(case):
    """np.unique of walk_reference == GetKmerSetFromSPSS of the oracle for both canonical flags, and with counts ==
    KmerCounter::FromReads + ToKmerSet at cutoffs 1 and 2 -- so the GPU test needs no oracle."""
    g = case.g
    for canonical in (False, True):
        occ = dw.walk_reference(case.strings, g.k, canonical)
        assert np.array_equal(occ, case.occurrences(canonical))
        vals, counts = np.unique(occ, return_counts=True)
        want = ol.Set.from_spss(case.strings, g.k, g.n, g.kb, canonical=canonical)
        assert np.array_equal(vals, want.kmers())
        counter = ol.Counter(g.k, g.n, g.kb)
        counter.from_reads(case.strings, canonical=canonical)
        for cutoff in dw.CUTOFFS:
            want_set, want_cut = counter.to_set(cutoff)
            kept, n_cut, offsets, keys = dw.expected_at(vals, counts, g, cutoff)
            assert n_cut == want_cut and np.array_equal(kept, want_set.kmers()), cutoff
            assert int(offsets[-1]) == kept.size == keys.size


def test_reference_on_known_strings():
    assert dw.walk_reference(["ACGT", "TTT"], 3, False).tolist() == [0b000110, 0b011011, 0b111111]
    assert dw.walk_reference(["ACGT", "TTT"], 3, True).tolist() == [0b000110, 0b000110, 0]
    assert dw.walk_reference(["AT"], 2, True).tolist() == [0b0011]
    rng = np.random.default_rng(4)
    for k in (2, 9, 16, 31):
        strings = dw.occurrence_strings(rng, k, 500, k, k + 40)
        want = np.concatenate([synth.kmers_of_bases(synth.bases_of_string(s), k) for s in strings])
        assert np.array_equal(dw.walk_reference(strings, k, False), want)
        assert np.array_equal(dw.walk_reference(strings, k, True), synth.canonical(want, k))


@pytest.mark.parametrize("case", [c for c in ALL if c.g.k >= dw.PHANTOM_MIN_K],
                         ids=[c.name for c in ALL if c.g.k >= dw.PHANTOM_MIN_K])
def test_phantom_windows_are_no_real_kmers(case):
    """Every window across a string end or across the tail (into the padding bits as the case sets them and the
    zero word behind) is absent from the case's k-mers, for both flags: a wrong end mask or tail test shows as an
    extra key, never as one more copy of a key that is there anyway."""
    n_phantoms = int(((case.g.k - 1) * len(case.strings)))
    for canonical in (False, True):
        ph = dw.phantom_windows(case, canonical)
        assert 0 < ph.size <= n_phantoms
        assert np.intersect1d(ph, case.counted(canonical)[0]).size == 0, canonical
