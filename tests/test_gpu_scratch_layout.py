"""Device scratch of every stage, in bytes, against the figures recorded before the stages' layouts were declared
as one list per block (tests/golden/scratch_bytes.json; csrc/ksh_layout.h).

Each case runs one operation of the public Python API on a fresh Context and reads Context.mem_stats(): `scratch`
(the three slots, the arena and the pair plan together) and the pool's peak.  The pool rounds a request to a size
class, so its peak must be what it was; a slot, the arena or the pair plan may have become smaller by less than 4 KiB
per block where several alignment roundings merged into one, never larger, and every such case is entered in the
golden file under "allowed" with its reason.

`python tests/test_gpu_scratch_layout.py [out.json]` records the figures of the tree it runs on (the golden file is
that output for the commit before the change; the "allowed" entries are written by hand)."""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # (under pytest, conftest.py has done this)
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "tests"), os.path.join(_root, "kmer-sets-compression_amd")]

import geometry_families as gf
from kmersets import capi

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scratch_bytes.json")
# A reserve maps its request plus at most a quarter of it (csrc/ksh_core.hip: arena_reserve, plan_reserve; the slots an
# eighth), so a request smaller by less than 4 KiB moves a block's mapped size by less than this.
BLOCK_SLACK = 4096 + 4096 // 4
SEED = 900
SIZE = 4000

# (k, N, device key bytes): one geometry per key width at N = 14 -- the encode's arena bound is above 64 MiB there, far
# past the context's first 8 MiB arena, and 4000 < 4 * 2^14 --, and one with 4000 >= 4 * 2^8 (the coarse index's rule)
ENCODE_GEOMS = [(15, 14, 2), (23, 14, 4), (31, 14, 8), (19, 8, 4)]
FAMILY_OF = {15: "random", 23: "repeats", 31: "genome", 19: "difference"}

_cache = {}


def kmers_of(k, size=SIZE):
    key = ("kmers", k, size)
    if key not in _cache:
        _cache[key] = gf.family(FAMILY_OF[k], k, size, SEED + k)
    return _cache[key]


def strings_of(k, n_bits, mode):
    """The encode's strings for the family of k (made on a context of their own, once)."""
    key = ("strings", k, n_bits, mode)
    if key not in _cache:
        ctx = capi.Context(0)
        g = capi.geom(k, n_bits)
        _cache[key] = ctx.spss_encode(capi.DeviceSet.from_kmers(g, kmers_of(k), ctx.device), mode=mode).to_strings()
        ctx.close()
    return _cache[key]


def text_on(ctx, raw):
    import torch

    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(ctx.device)


def two_sets(ctx, g, k):
    x = kmers_of(k)
    return (capi.DeviceSet.from_kmers(g, x[: 3 * x.size // 4], ctx.device),
            capi.DeviceSet.from_kmers(g, x[x.size // 4:], ctx.device))


# ---- the operations: each takes a fresh context
def op_encode(k, n_bits, kb, mode):
    def run(ctx):
        g = capi.geom(k, n_bits, kb)
        ctx.spss_encode(capi.DeviceSet.from_kmers(g, kmers_of(k), ctx.device), mode=mode)
    return run


def op_cover(ctx):
    g = capi.geom(23, 14)
    unitigs = capi.DeviceSpss.from_strings(g, strings_of(23, 14, 1), ctx.device)
    ctx.spss_cover_write(ctx.spss_cover_plan(unitigs))


def op_decode(k, n_bits):
    def run(ctx):
        g = capi.geom(k, n_bits)
        sp = capi.DeviceSpss.from_strings(g, strings_of(k, 14, 0), ctx.device)
        ctx.spss_decode_write(ctx.spss_decode_plan(sp))
    return run


def op_pair_plan(ctx):
    g = capi.geom(23, 14)
    a, b = two_sets(ctx, g, 23)
    ctx.pair_algebra(a, b)


def op_union_plan(ctx):
    g = capi.geom(23, 14)
    a, b = two_sets(ctx, g, 23)
    ctx.set_union(a, b)


def op_pair_onepass(ctx):
    g = capi.geom(23, 14)
    a, b = two_sets(ctx, g, 23)
    ctx.pair_algebra_onepass(a, b)


def op_set_diff(ctx):
    g = capi.geom(23, 14)
    a, b = two_sets(ctx, g, 23)
    ctx.set_diff(a, b)


def op_pair_batch(ctx):
    g = capi.geom(23, 14)  # 64 jobs of 2^14 segments each: the batch's arena request passes 8 MiB
    a, b = two_sets(ctx, g, 23)
    ctx.pair_algebra_batch([(a, b)] * 64)


def op_pair_weights(ctx):
    g = capi.geom(23, 14)
    x = kmers_of(23)
    sets = [capi.DeviceSet.from_kmers(g, x[i::2], ctx.device) for i in range(2)] + list(two_sets(ctx, g, 23))
    ids = np.arange(0, 1 << 14, 50, dtype=np.int32)
    ctx.pair_weights(sets, ids, [(i, j) for i in range(4) for j in range(i + 1, 4)])


def op_from_text(ctx):
    g = capi.geom(23, 14)
    raw = "".join(s + "\n" for s in strings_of(23, 14, 0)).encode()
    ctx.spss_from_text(g, text_on(ctx, raw))


def op_fasta(ctx):
    g = capi.geom(23, 14)
    raw = "".join(">r%d\n%s\n" % (i, s) for i, s in enumerate(strings_of(23, 14, 0))).encode()
    ctx.fasta_fragments(g, text_on(ctx, raw))


CASES = {"encode-k%d-N%d-u%d-mode%d" % (k, n, 8 * kb, mode): op_encode(k, n, kb, mode)
         for k, n, kb in ENCODE_GEOMS for mode in (0, 1, 2)}
CASES.update({
    "cover-k23-N14": op_cover,
    "decode-k23-N14": op_decode(23, 14),
    "decode-k23-N16": op_decode(23, 16),
    "pair-plan": op_pair_plan,
    "union-plan": op_union_plan,
    "pair-onepass": op_pair_onepass,
    "set-diff-onepass": op_set_diff,
    "pair-batch-64": op_pair_batch,
    "pair-weights": op_pair_weights,
    "from-text": op_from_text,
    "fasta": op_fasta,
})


def measure(name):
    ctx = capi.Context(0)
    try:
        ctx.mem_stats(reset_peak=True)
        CASES[name](ctx)
        ctx.sync()
        st = ctx.mem_stats()
        return {"scratch": st["scratch"], "pool_peak": st["pool_peak"]}
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def golden(gpu):
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_the_cases(golden):
    assert set(golden["cases"]) == set(CASES)
    assert set(golden["allowed"]) <= set(CASES)
    for name, entry in golden["allowed"].items():
        was = golden["cases"][name]["scratch"]
        assert entry["reason"] and entry["blocks"] >= 1
        assert 0 < was - entry["scratch"] < entry["blocks"] * BLOCK_SLACK, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_are_what_they_were(golden, name):
    was, got = golden["cases"][name], measure(name)
    print(name, "was", was, "is", got)
    assert got["pool_peak"] == was["pool_peak"]
    allowed = golden["allowed"].get(name)
    assert got["scratch"] == (allowed["scratch"] if allowed else was["scratch"])


def test_a_smaller_set_does_not_regrow_the_scratch(gpu):
    """A lane's slot is reserved once at the largest n (csrc/ksh_kss.hip): every smaller plan must find it large
    enough, or a build pays a hipFree and a stream synchronise in its middle."""
    ctx = capi.Context(0)
    g = capi.geom(23, 14)
    big = gf.family("genome", 23, 20000, SEED)
    seen = []
    for x in (big, big[:3000]):
        ctx.spss_encode(capi.DeviceSet.from_kmers(g, x, ctx.device), mode=0)
        seen.append(ctx.mem_stats()["scratch"])
    ctx.close()
    print("scratch after 20 000 and after 3 000 k-mers:", seen)
    assert seen[1] == seen[0]


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    allowed = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            allowed = json.load(f).get("allowed", {})
    result = {"cases": {name: measure(name) for name in sorted(CASES)}, "allowed": allowed}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
