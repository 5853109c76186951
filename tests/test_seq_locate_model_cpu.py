"""The designed cases of tests/seq_locate_cases.py hold what they claim, on the reference alone: no GPU needed."""
import numpy as np
import pytest

import hash_table_cases as hc
import seq_locate_cases as cases
import seq_locate_reference as ref


def test_constants_parse_from_the_kernels_text():
    r, threads = cases.kernel_constants()
    assert r in (8, 16, 32, 64) and threads == 256 and cases.BLOCK == r * threads
    assert cases.kernel_constants("constexpr int kLocRun = 64;\nconstexpr int kLocThreads = 128;\n") == (64, 128)
    with pytest.raises(AssertionError):
        cases.kernel_constants("constexpr int kLocRun = 64;\n")
    text = open(cases.SOURCE).read()
    assert "launch_scan<%d>" % r in text  # the run the library states is one it builds


def test_every_builder_at_every_k():
    assert {c["k"] for c in cases.CASES} == set(cases.KS) == {15, 16, 23, 31}
    for build in cases.BUILDERS:
        assert {c["k"] for c in cases.CASES if c["id"].startswith(build(15)["id"][:-4])} == set(cases.KS)
    assert sum(c["id"].startswith("self-rc") for c in cases.CASES) == 1
    assert all(c["edge"] and len(c["strings"]) <= 300 for c in cases.CASES)


@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "directed"])
@pytest.mark.parametrize("case", cases.CASES, ids=[c["id"] for c in cases.CASES])
def test_case_holds_its_claim(case, canonical):
    k = case["k"]
    where, count = ref.locate(case["strings"], case["reference"], k, canonical)
    assert where.shape == count.shape == (2 * len(case["strings"]),)
    got = ref.split(where, case["reference"], k)
    claims = case["expect"][canonical]
    assert claims or not case["strings"]
    for e, (r, p, strand, c) in claims.items():
        assert got[e] == (r, p, strand) and count[e] == c, (case["id"], e, got[e], int(count[e]))
    assert ((where >= 0) == (count > 0)).all()


def test_boundaries_fall_where_the_case_says():
    for k in cases.KS:
        c = next(x for x in cases.CASES if x["id"] == "boundaries-k%d" % k)
        ps = ref.pstart(c["reference"], k)
        r, block = cases.R, cases.BLOCK
        assert {r - 1, r, r + 1, block - 1, block, block + 1} <= set(ps.tolist())
        assert ps[-1] > block + 2 * r  # more than one workgroup, and a partial last one
        c = next(x for x in cases.CASES if x["id"] == "one-position-runs-k%d" % k)
        ps = ref.pstart(c["reference"], k)
        assert (np.diff(ps)[1:-1] == 1).all() and np.diff(ps)[1:-1].size == 3 * r
        c = next(x for x in cases.CASES if x["id"] == "across-boundary-k%d" % k)
        a, b = c["reference"]
        assert c["strings"][0] in a + b and c["strings"][0] not in a and c["strings"][0] not in b


def test_table_cases_against_the_model_of_link_slot():
    """The colliding ends share a home, the run behind it is full, the absent k-mer of the reference has that home
    too and is no end; the wrap's home is the last slot."""
    for c in cases.CASES:
        if "table" not in c:
            continue
        t, k = c["table"], c["k"]
        slots = t["slots"]
        assert slots == cases.slots_of(len(c["strings"])) == hc.link_slots(len(c["strings"])) == 32
        keys = np.array([hc.kmer_int(min(y, ref.rc(y))) for y in c["strings"]], dtype=np.uint64)
        assert all(y < ref.rc(y) for y in c["strings"] + [t["absent"]])  # the key is the k-mer in both modes
        homes = hc.link_homes(keys, slots)
        assert (homes[:t["run"]] == t["home"]).all() and len(set(homes[t["run"]:].tolist())) == len(homes) - t["run"]
        occ = hc.occupied(homes, slots)
        start, length = hc.run_of(occ, t["home"])
        assert (start, length) == (t["home"], t["run"])
        assert int(hc.link_homes(np.array([hc.kmer_int(t["absent"])], dtype=np.uint64), slots)[0]) == t["home"]
        assert t["absent"] not in c["strings"] and any(t["absent"] in s for s in c["reference"])
        if c["id"].startswith("wrap"):
            assert t["home"] == slots - 1 and hc.wrapped(homes, slots) == t["run"] - 1
    assert sum("table" in c for c in cases.CASES) == 2 * len(cases.KS)
    one = next(c for c in cases.CASES if c["id"] == "n1-k23")
    assert cases.slots_of(len(one["strings"])) == 4


def test_homopolymer_key_is_zero():
    assert hc.kmer_int("A" * 31) == 0
    for k in cases.KS:
        c = next(x for x in cases.CASES if x["id"] == "homopolymer-k%d" % k)
        assert c["strings"][0] == "A" * k and sum(len(t) - k + 1 for t in c["reference"]) == 51


@pytest.mark.parametrize("canonical", [True, False], ids=["canonical", "directed"])
def test_reference_agrees_with_brute_force(canonical):
    assert len(cases.SMALL) >= 40
    for c in cases.SMALL:
        a = ref.locate(c["strings"], c["reference"], c["k"], canonical)
        b = ref.brute(c["strings"], c["reference"], c["k"], canonical)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), c["id"]


def test_reference_refusals_in_the_devices_order():
    k = 23
    with pytest.raises(ValueError, match=r"req->strings: lens\[1\] = UINT32_MAX"):
        ref.check_request([3, ref.UINT32_MAX, ref.UINT32_MAX], 0, [ref.UINT32_MAX], 0, k)
    with pytest.raises(ValueError, match=r"req->strings: sum\(lens \+ K\) = 49 but n_bases = 50"):
        ref.check_request([3, 0], 50, [ref.UINT32_MAX], 0, k)
    with pytest.raises(ValueError, match=r"req->reference: lens\[0\] = UINT32_MAX"):
        ref.check_request([3, 0], 49, [ref.UINT32_MAX, 1], 7, k)
    with pytest.raises(ValueError, match=r"req->reference: sum\(lens \+ K\) = 47 but n_bases = 7"):
        ref.check_request([3, 0], 49, [0, 1], 7, k)
    with pytest.raises(ValueError, match=r"req->reference: sum\(lens \+ K\) = 0 but n_bases = 7"):
        ref.check_request([3, 0], 50, [], 7, k)
    ref.check_request([3, 0], 49, [0, 1], 47, k)
    ref.check_request([3, 0], 49, [], 0, k)
