"""CPU checks of the pair-tile sweep (tests/pair_tile_cases.py): the numpy model of the tile plan against brute
force, and the class list -- which tiles, splits, lanes, phases and sizes the built sheets contain, per key width.
The classes are conditions on the case list, computed by the model; tests/test_gpu_pair_tiles.py runs the sheets."""
import os

import numpy as np
import pytest

import pair_tile_cases as ptc

U = np.uint64
WIDTHS = (2, 4, 8)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cfgs():
    return ptc.constants()


@pytest.fixture(scope="module")
def modelled(cfgs):
    """kb -> (sheets, the modelled tiles of all of them)"""
    cache = {}

    def get(kb):
        if kb not in cache:
            sh = ptc.sheets(kb)
            cache[kb] = (sh, [t for s in sh.values() for t in ptc.sheet_tiles(s, cfgs[kb])])
        return cache[kb]

    return get


def test_constants_read_from_the_kernel(cfgs):
    for kb, c in cfgs.items():
        assert c.kThreads == 64 and c.kVT % 2 == 1 and c.kPer == 16 // kb
        assert c.kTile == c.kThreads * c.kVT - 1 and c.kCap == c.kTile + 1
        assert c.kTile < ptc.N_BUCKETS < 2 * c.kTile  # the tight sheet's arithmetic (tight_sheet's docstring)
    assert cfgs[2].kVT == cfgs[4].kVT
    # a changed constant is noticed: the same text with another kVT gives another plan
    text = open(ptc.PAIR_HIP).read().replace("#define KSH_VT32 %d" % cfgs[4].kVT, "#define KSH_VT32 %d" % (cfgs[4].kVT + 2))
    assert ptc.constants(text)[4].kTile == cfgs[4].kTile + 2 * 64
    with pytest.raises(AssertionError):
        ptc.constants(text.replace("kTile = kThreads * kVT - 1;", "kTile = kThreads * kVT - 2;"))


# ---- the model against brute force ---------------------------------------------------------------------------------
def brute_split(a, b, diag):
    """Merge with ties A first, cut at diag; the cut moves one to the right when it falls inside an "a, b" pair."""
    keys = np.concatenate([a, b])
    order = np.argsort(keys, kind="stable")  # A's keys come first in `keys`: stable = A first on ties
    from_a = order < a.size
    i = int(from_a[:diag].sum())
    j = diag - i
    moved = bool(0 < diag < keys.size and from_a[diag - 1] and not from_a[diag] and keys[order[diag - 1]] == keys[order[diag]])
    return i, j + int(moved), moved


def small_inputs():
    rng = np.random.default_rng(99)
    out = []
    for t in range(300):
        na, nb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        span = (8, 30, 200, 1 << 40)[t % 4]  # tie-heavy to tie-free
        a = np.unique(rng.integers(0, span, size=na).astype(U))
        b = np.unique(rng.integers(0, span, size=nb).astype(U))
        if t % 7 == 0:
            b = a.copy()
        out.append((a, b))
    return out


def test_model_split_matches_brute_force():
    moved_seen = 0
    for a, b in small_inputs():
        for diag in range(a.size + b.size + 1):
            got = ptc.merge_path_split(a, b, diag)
            assert got == brute_split(a, b, diag), (a, b, diag)
            moved_seen += got[2]
    assert moved_seen > 100


def test_model_tiles_match_brute_force():
    for a, b in small_inputs():
        for k_tile in (1, 3, 7, 20):
            n = a.size + b.size
            n_tiles = -(-n // k_tile)
            assert ptc.seg_tiles(n, k_tile) == n_tiles
            tiles = ptc.tile_split(a, b, k_tile)
            assert len(tiles) == n_tiles
            cuts = [brute_split(a, b, q * n // n_tiles)[:2] for q in range(1, n_tiles)]
            want = list(zip([(0, 0)] + cuts, cuts + [(a.size, b.size)])) if n_tiles else []
            assert [((t.a0, t.b0), (t.a1, t.b1)) for t in tiles] == want
            # a tile holds at most k_tile + 1 keys, and a common pair is never cut; a tile is never empty once
            # k_tile >= 3 (the diagonals are then at least 2 apart and a fix-up takes one key): the kernel's
            # staging relies on that
            for t in tiles:
                assert (k_tile >= 3) <= (t.a1 - t.a0) + (t.b1 - t.b0) <= k_tile + 1
                assert not (t.a0 > 0 and t.b0 < b.size and a[t.a0 - 1] == b[t.b0])


def test_model_lanes_match_brute_force():
    cfg = ptc.Cfg(8, 64, 3, 191, 192, 2)
    rng = np.random.default_rng(5)
    seen = 0
    for t in range(120):
        na, nb = int(rng.integers(0, 120)), int(rng.integers(0, 70))
        span = (40, 150, 1 << 30)[t % 3]
        a = np.unique(rng.integers(0, span, size=na).astype(U))
        b = np.unique(rng.integers(0, span, size=nb).astype(U))
        n = a.size + b.size
        ns, d0, i, straddle = ptc.lane_plan(a, b, cfg)
        assert ns == min(3, (-(-n // 64)) | 1)
        for lane in range(64):
            assert d0[lane] == min(lane * ns, n)
            bi, bj, moved = brute_split(a, b, int(d0[lane]))
            assert i[lane] == bi and straddle[lane] == moved, (t, lane)
            seen += moved
    assert seen > 50


# ---- the class list ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kb", WIDTHS)
def test_axes_are_all_there(kb, cfgs, modelled):
    cfg = cfgs[kb]
    sh, _ = modelled(kb)
    assert list(sh) == ptc.sheet_names(kb)
    t, p = cfg.kTile, cfg.kPer
    lengths = {1, 2, 3, p - 1, p, p + 1, 63, 64, 65, 127, 128, 129, t - 1, t, t + 1, t + 2, 2 * t - 1, 2 * t, 2 * t + 1,
               3 * t, 3 * t + 1, 5 * t + 7}
    assert set(ptc.merged_lengths(cfg)) == lengths
    cases = [pl.case for name in sh if name.startswith("s") and name != "single" for pl in sh[name].placed]
    have = {(c.length, c.a.size, c.kind) for c in cases}
    for length in lengths:
        half = (length + 1) // 2
        for na in {0, 1, half, length - 1, length}:
            if 0 <= na <= length:
                assert (length, na, "interleaved") in have, (length, na)
                if 0 < na < length:
                    for kind in ("a_below_b", "b_below_a", "random"):
                        assert (length, na, kind) in have, (length, na, kind)
        if length > 1:
            assert (length, half, "identical") in have
    # the sliding runs: every r and every offset at the tile boundaries of every multi-tile size and at lane boundaries
    names = {c.name for c in cases}
    for length in lengths:
        if ptc.seg_tiles(length, t) > 1:
            for r in ptc.RUNS:
                for d in ptc.DELTAS:
                    assert "L%d-tile-run%d%+d" % (length, r, d) in names
    for r in ptc.RUNS:
        for d in ptc.DELTAS:
            assert "L%d-lane-run%d%+d" % (t, r, d) in names
    # the cross: both patterns at every phase pair of every size from kTile - 1 up
    for length in (v for v in lengths if v >= t - 1):
        for kinds in (("identical",), ("tile_run", "lane_run")):
            got = {(c.pa, c.pb) for c in cases if c.length == length and c.kind in kinds and "-p" in c.name}
            assert got == {(x, y) for x in range(p) for y in range(p)}, (length, kinds)
    # every case sits at the phase it asked for
    for name in sh:
        for pl in sh[name].placed:
            if pl.case.pa is not None:
                assert (pl.a_start % p, pl.b_start % p) == (pl.case.pa, pl.case.pb)
    # a few million keys per width, so that the numpy references stay at seconds
    assert sum(s.a.size + s.b.size for s in sh.values()) < 6_000_000


@pytest.mark.parametrize("kb", WIDTHS)
def test_tile_classes(kb, cfgs, modelled):
    cfg = cfgs[kb]
    sh, tiles = modelled(kb)
    p = cfg.kPer
    # a full tile at the worst phase of both ranges
    assert any(t.ca + t.cb == cfg.kCap and t.phase_a == p - 1 and t.phase_b == p - 1 for t in tiles)
    assert any(t.ca + t.cb == cfg.kCap and t.q > 0 for t in tiles)  # and one that does not start its bucket
    assert max(t.ca + t.cb for t in tiles) == cfg.kCap
    # one-sided tiles inside a multi-tile segment
    assert any(t.ca == 0 and t.n_tiles > 1 for t in tiles) and any(t.cb == 0 and t.n_tiles > 1 for t in tiles)
    # every phase pair at a tile of at least kTile - 1 keys
    big = {(t.phase_a, t.phase_b) for t in tiles if t.ca + t.cb >= cfg.kTile - 1}
    assert big == {(x, y) for x in range(p) for y in range(p)}
    full = {(t.phase_a, t.phase_b) for t in tiles if t.ca + t.cb == cfg.kCap}
    assert full == big  # (the cross at 2 kTile and 3 kTile takes the fix-up at every phase pair)
    # single-tile segments of 1, 2 and 3 keys
    assert {1, 2, 3} <= {t.ca + t.cb for t in tiles if t.n_tiles == 1}
    # n_steps takes every odd value up to kVT
    assert {t.n_steps for t in tiles} == set(range(1, cfg.kVT + 1, 2))


@pytest.mark.parametrize("kb", WIDTHS)
def test_split_classes(kb, cfgs, modelled):
    """The unadjusted split of a tile boundary falls inside an "a, b" pair (the j += 1 branch), just before one
    and just after one."""
    _, tiles = modelled(kb)
    inside = before = after = 0
    for t in tiles:
        if t.q == 0:
            continue
        a, b = t.case.a, t.case.b
        i, j = t.tile.a0, t.tile.b0 - int(t.tile.moved)  # the split as searched
        assert i + j == t.tile.diag
        inside += t.tile.moved
        if not t.tile.moved:
            before += bool(i < a.size and j < b.size and a[i] == b[j])
            after += bool(i > 0 and j > 0 and a[i - 1] == b[j - 1])
    assert inside >= 10 and before >= 10 and after >= 10, (inside, before, after)


@pytest.mark.parametrize("kb", WIDTHS)
def test_lane_classes(kb, cfgs, modelled):
    """A lane whose first merged key is the B half of a common pair: in the first lane that can be one (lane 0
    starts its tile, and a tile never starts inside a pair), in a middle lane and in the last active lane."""
    _, tiles = modelled(kb)
    assert not any(0 in t.straddle_lanes for t in tiles)
    first = sum(1 in t.straddle_lanes for t in tiles)
    last = sum(t.last_lane > 1 and t.last_lane in t.straddle_lanes for t in tiles)
    middle = sum(any(1 < lane < t.last_lane for lane in t.straddle_lanes) for t in tiles)
    assert first >= 5 and middle >= 5 and last >= 5, (first, middle, last)
    # ... at every n_steps, and in a full tile
    assert {t.n_steps for t in tiles if t.straddle_lanes} == set(range(1, cfgs[kb].kVT + 1, 2))
    assert any(t.straddle_lanes and t.ca + t.cb == cfgs[kb].kCap for t in tiles)


@pytest.mark.parametrize("kb", WIDTHS)
def test_bound_sheets(kb, cfgs, modelled):
    cfg = cfgs[kb]
    sh, tiles = modelled(kb)
    tight = sh["tight"]
    lengths = np.array([pl.case.length for pl in tight.placed])
    assert lengths.size == ptc.N_BUCKETS and (lengths % cfg.kTile == 1).all() and (lengths > 1).sum() > 300
    n_tiles = sum(1 for t in tiles if t.sheet == "tight")
    assert n_tiles == sum(ptc.seg_tiles(int(v), cfg.kTile) for v in lengths)
    bound = ptc.N_BUCKETS + (tight.a.size + tight.b.size) // cfg.kTile + 1
    # as tight as 1024 buckets allow: tight_sheet's docstring has the arithmetic
    assert n_tiles == bound - 2
    single = sh["single"]
    assert [pl.bucket for pl in single.placed] == [ptc.SINGLE_BUCKET]
    shift = U(ptc.key_bits(kb))
    assert set((single.a >> shift).tolist()) == {ptc.SINGLE_BUCKET} == set((single.b >> shift).tolist())
    assert single.a.size == ptc.SINGLE_KEYS[kb] and 0 < np.intersect1d(single.a, single.b).size < single.b.size


@pytest.mark.parametrize("kb", WIDTHS)
def test_extreme_keys(kb, modelled):
    sh, _ = modelled(kb)
    bits = ptc.key_bits(kb)
    assert bits == 8 * kb or kb == 8  # u16 and u32 at full key width: the all-ones key is the type's largest
    ones = U(((ptc.N_BUCKETS - 1) << bits) | ((1 << bits) - 1))
    for key in (U(0), ones):
        forms = {(bool((s.a == key).any()), bool((s.b == key).any())) for s in sh.values()}
        assert {(True, True), (True, False), (False, True)} <= forms, key


def test_the_indirect_pins_are_still_there():
    parity = open(os.path.join(HERE, "test_gpu_parity.py")).read()
    assert "def test_pair_algebra_edge_cases(ctx, geom):" in parity and "dense[:30000], dense[10000:]" in parity
    geometry = open(os.path.join(HERE, "test_gpu_geometry.py")).read()
    assert "def test_geometry_cell(ctx, families, cell):" in geometry and "(31, 24, 8)" in geometry
    assert "ctx.pair_algebra(d, e)" in geometry and "ctx.set_union(d, e)" in geometry
