"""Oracle string equality on inputs that PROVABLY take the kernel variants the headline bench runs
("What's weak" 1): k_adj_rc<KeyT, 1024> with windows staged in several batches, the
two-level rc scatter, two-level pointer jumping, the one-launch ranking walks -- each test asserts
the route through ksh_spss_encode_routes, so a case cannot silently take another variant -- and a
route differential at 10^8 k-mers: the default staged route against the size-independent in-place
probe + stamping walks + emit by walking (independent algorithms; the latter oracle-checked at
small sizes by test_encode_alternative_paths).  Reference: lib/core/spss.h:230-615,1358-1829."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
from kmersets import capi, synth
from probe_cases import RC1_CAP, rc_shape, records_per_group

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    yield c
    c.close()


def encode_vs_oracle(ctx, k, n, kmers, must, must_not=()):
    g = capi.geom(k, n)
    d = capi.DeviceSet.from_kmers(g, kmers, ctx.device)
    sp = ctx.spss_encode(d, mode=0)
    routes = ctx.spss_encode_routes()
    stats = ctx.spss_encode_stats()
    missing = set(must) - routes
    assert not missing and not (set(must_not) & routes), (sorted(routes), must, must_not)
    want = ol.Set.from_kmers(k, n, g.key_bytes, kmers).spss()
    got = sp.to_strings()
    assert len(got) == len(want) and got == want
    assert sp.n_bases == sum(len(x) for x in want)
    back = ctx.spss_decode(sp)
    assert back.n_keys == d.n_keys and ctx.set_diff(back, d) == 0
    return routes, stats


def test_u32_1024_threads_batched_windows(ctx):
    """(19, 8, uint32_t), 5 x 10^6 k-mers: 19 500 records per group, more than k_adj_rc1's LDS holds -> k_adj_rc<u32,
    1024>; a window holds 7 976 keys, so every group's pass 0 (and pass 1 for most) takes several batches; N = 8 >
    kSgBits and n >= 2^20 -> the two-level rc scatter; 3 x 10^5 ruler walkers >= 2^18 -> all of them in one launch."""
    k, n = 19, 8
    a = synth.phylogeny_sets(k, 1, 5_000_000, seed=41)[0]
    encode_vs_oracle(ctx, k, n, a, {"probe_staged", "rc_1024", "rc_marks_groups", "rc_batched", "scatter_two_level",
                                    "fwd_targets", "rank_one_launch", "emit_logs"}, {"rank_stamped"})


def test_u32_fragmented_heads_one_launch(ctx):
    """The intersection of two 5 %-diverged genomes of 10^7 bases, (19, 8, uint32_t): 3.8 x 10^6 k-mers in some
    1.9 x 10^5 unitigs, so the chain-start walkers pass 2^18 and go in one launch too, the matching has work at
    every junction and the path cover stitches multi-unitig strings -- on the 1024-thread, batched route."""
    k, n = 19, 8
    a, b = synth.phylogeny_sets(k, 2, 10_000_000, seed=43, rate=0.025)
    inter = np.intersect1d(a, b)
    assert 3_000_000 < inter.size < 4_500_000
    routes, stats = encode_vs_oracle(ctx, k, n, inter, {"probe_staged", "rc_1024", "rc_batched", "scatter_two_level",
                                                       "heads_one_launch"}, {"rank_stamped"})
    assert stats["unitigs"] > 150_000


def test_u64_1024_threads_batched_windows(ctx):
    """(23, 8, uint64_t), 2.5 x 10^6 k-mers: 9 800 records per group (k_adj_rc1 holds 4 644 of an 8-byte key's) ->
    k_adj_rc<u64, 1024>, a window of 5 700 8-byte keys -> several batches; 16-byte records through the two-level
    scatter (the intermediate records borrow nbr + link)."""
    k, n = 23, 8
    a = synth.phylogeny_sets(k, 1, 2_500_000, seed=47)[0]
    encode_vs_oracle(ctx, k, n, a, {"probe_staged", "rc_1024", "rc_marks_groups", "rc_batched", "scatter_two_level",
                                    "fwd_targets", "emit_logs"}, {"rank_stamped"})


def test_bench_geometry_two_level_jumping(ctx):
    """One (23, 14, uint32_t) set of 1.7 x 10^7 k-mers against the oracle: the bench's geometry with 2^20 ruler
    records, i.e. two-level pointer jumping, the one-launch ranking, the two-level scatter at N = 14 (128
    groups per super-group) and the emit from the logs with its long-stretch list."""
    k, n = 23, 14
    a = synth.phylogeny_sets(k, 1, 17_000_000, seed=53)[0]
    encode_vs_oracle(ctx, k, n, a, {"probe_staged", "rc_512", "scatter_two_level", "fwd_targets", "rank_one_launch",
                                    "jump_two_level", "emit_logs"}, {"rank_stamped"})


# (RC1_CAP, rc_shape and records_per_group live in tests/probe_cases.py, beside the model of the probe that uses them)


def test_rc1_cap_arithmetic():
    assert RC1_CAP == {2: 8128, 4: 8128, 8: 4640}
    assert rc_shape(1_400_000, 8, 4) == (5468, "rc_1024", 7552)
    assert rc_shape(1_100_000, 8, 8)[1:] == ("rc_1024", 4640)


@pytest.mark.parametrize("k,n,kb,size,threads,marks", [
    (19, 8, 4, 1_400_000, "rc_1024", False),   # the bench's k_adj_rc1<u32, 1024>, every group in LDS
    (11, 8, 2, 1_800_000, "rc_1024", False),   # its 2-byte twin on a dense 11-mer graph
    (25, 8, 8, 600_000, "rc_512", False),      # k_adj_rc1<u64, 512> alone
    (25, 8, 8, 1_100_000, "rc_1024", True),    # u64: kCap 4640 splits the groups between k_adj_rc1 and k_adj_rc
])
def test_rc1_does_the_work(ctx, k, n, kb, size, threads, marks):
    """VERDICT "What next" 4a: inputs sized so that k_adj_rc1 -- not k_adj_rc -- probes every group (or, in the
    last case, the groups that fit its LDS while k_adj_rc takes the rest in the same encode), against the oracle.
    The group sizes are counted here with numpy, so the expected routes follow from the set, not from hope."""
    if k == 11:  # uniform canonical 11-mers: over half of the 2.1 x 10^6 canonical 11-mers, a dense graph
        kmers = synth.uniform_pair(k, size, 0.0, seed=73)[0]
    else:
        kmers = synth.phylogeny_sets(k, 1, size, seed=71 + k)[0]
    assert capi.geom(k, n).key_bytes == kb
    # the staged probe's conditions (csrc/ksh_encode.hip, encode plan)
    assert n <= 14 and 2 * k >= n + 4 and 2 * k - n >= n + 2 + (n & 1)
    assert kmers.size >> n <= 4 * ((78 * 1024 - 4 * 16) // (kb + 6))
    per_group, want_threads, rc1_cap = rc_shape(kmers.size, n, kb)
    assert want_threads == threads
    counts = records_per_group(kmers, k, n)
    assert (counts.max() > rc1_cap) == marks, (counts.max(), rc1_cap)
    if marks:
        assert (counts <= rc1_cap).sum() > 0
    must = {"probe_staged", threads, "rc1_streamed", "fwd_targets"} | ({"rc_marks_groups"} if marks else set())
    encode_vs_oracle(ctx, k, n, kmers, must, set() if marks else {"rc_marks_groups"})


def stream_parts(kmers, k, chunk=2048, stream_max=4096):
    """Parts beyond the first that k_tgt_split makes (tests/test_model_probe_partition.py, cuts_of): a window of
    `chunk` k-mers, cut where the (K-1)-base prefix changes, streams the k-mers whose suffix lies in its prefix
    range, and a stream longer than stream_max is cut into ceil(stream / stream_max) parts."""
    from probe_cases import cuts_of

    _, v = cuts_of(kmers, k, chunk)
    v = np.array(v, dtype=np.uint64)
    stream = sum(np.diff(np.searchsorted(kmers, np.uint64(a << (2 * k - 2)) + v)) for a in range(4))
    return int(np.maximum((stream + stream_max - 1) // stream_max - 1, 0).sum())


def t_heavy_set(k, length, p_t, seed):
    """Canonical k-mers of a genome whose bases are T with probability p_t: canonical k-mers that start with T are
    rare, so the last windows span wide prefix ranges, while k-mers with a T second base are common -- long streams."""
    idx = np.arange(length, dtype=np.uint64)
    r = (synth.mix64(idx + np.uint64(seed)) >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    b = np.where(r < p_t, 3, synth.mix64(idx + np.uint64(seed + 1)) % np.uint64(3)).astype(np.uint8)
    return synth.canonical_set_of_bases(b, k)


def test_target_windows_cut_into_parts(ctx):
    """VERDICT "What next" 4b: KSH_ROUTE_TGT_PARTS reports that k_tgt_split / k_tgt_subcuts cut some window of
    k_adj_fwd_targets into parts.  For each set the numpy model says whether a stream exceeds kStreamMax, and the
    bit must agree; the strings must be the oracle's either way.  A T-heavy set cuts its last windows into many
    parts; a 2 x 10^5-k-mer genome set already cuts one (its last window streams about 12 600 k-mers); a set of
    fewer k-mers than kStreamMax cannot."""
    k, n = 23, 14
    cases = [("t_heavy", t_heavy_set(k, 600_000, 0.55, 97)),
             ("genome", synth.phylogeny_sets(k, 1, 200_000, seed=83)[0]),
             ("small", synth.phylogeny_sets(k, 1, 4000, seed=89)[0])]
    parts = {name: stream_parts(km, k) for name, km in cases}
    assert parts["t_heavy"] >= 10 and parts["genome"] > 0 and parts["small"] == 0, parts
    for name, km in cases:
        want = {"probe_staged", "fwd_targets"} | ({"tgt_parts"} if parts[name] else set())
        encode_vs_oracle(ctx, k, n, km, want, set() if parts[name] else {"tgt_parts"})


ROUTE_WORKER = r"""
import hashlib, json, sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
from kmersets import capi, synth_torch
k, n, size = 23, 14, int(sys.argv[1])
ctx = capi.Context(0)
g = capi.geom(k, n)
a, b = [synth_torch.device_set(g, x) for x in synth_torch.phylogeny_sets(k, 2, size, 61, ctx.device)]
inter, amb, _ = ctx.pair_algebra(a, b)
out = {}
for name, s in (("genome", a), ("intersection", inter), ("difference", amb)):
    sp = ctx.spss_encode(s, mode=0)
    routes = sorted(ctx.spss_encode_routes())
    torch.cuda.synchronize()
    n_words = (sp.n_bases + 31) // 32
    h = hashlib.sha256()
    h.update(sp.words[:n_words].cpu().numpy().tobytes())
    h.update(sp.lens[:sp.n_strings].cpu().numpy().tobytes())
    back = ctx.spss_decode(sp)
    ok = back.n_keys == s.n_keys and ctx.set_diff(back, s) == 0
    out[name] = {"n": s.n_keys, "strings": sp.n_strings, "bases": sp.n_bases, "sha256": h.hexdigest(),
                 "routes": routes, "roundtrip": bool(ok)}
    del sp, back
print("ROUTE_RESULT " + json.dumps(out))
"""


def _run_route(env_add, size):
    env = dict(os.environ)
    env.update(env_add)
    code = ROUTE_WORKER % (os.path.join(os.path.dirname(HERE), "kmer-sets-compression_amd"), HERE)
    r = subprocess.run([sys.executable, "-c", code, str(size)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("ROUTE_RESULT ")][-1]
    return json.loads(line[len("ROUTE_RESULT "):])


def test_route_differential_1e8(gpu):
    """At the bench's size -- a 10^8-k-mer genome set, its intersection with a sibling and the difference set --
    the default route (k_adj_rc1<u32, 1024>: the groups' records chained in LDS, their ranges streamed; k_adj_rc for
    the groups that do not fit; k_adj_fwd_targets; two-level scatter and jumping,
    one-launch ranking, strings from the walk logs) and the route of independent, size-independent kernels
    (k_adjacency probing in global memory, stamping walks + k_choose, k_emit) write the same SPSS words and
    lengths, byte for byte -- and so does round 3's probe (k_adj_rc with two batches of windows for the dense groups,
    k_adj_fwd_staged).  The switches are read once per process: three processes."""
    size = 100_000_000
    default = _run_route({}, size)
    other = _run_route({"KSH_ADJACENCY": "probe", "KSH_RANK": "stamp", "KSH_EMIT": "walk"}, size)
    round3 = _run_route({"KSH_RC1": "marks", "KSH_FWD": "staged"}, size)
    r = set(default["genome"]["routes"])
    assert {"probe_staged", "rc_1024", "rc1_streamed", "scatter_two_level", "fwd_targets", "rank_one_launch",
            "jump_two_level", "emit_logs"} <= r, sorted(r)
    assert "probe_staged" not in other["genome"]["routes"] and "rank_stamped" in other["genome"]["routes"]
    r3 = set(round3["genome"]["routes"])
    assert {"rc_1024", "rc_batched", "fwd_staged"} <= r3 and not ({"rc1_streamed", "fwd_targets"} & r3), sorted(r3)
    for name in ("genome", "intersection", "difference"):
        d = default[name]
        for o in (other[name], round3[name]):
            assert d["roundtrip"] and o["roundtrip"], name
            assert (d["n"], d["strings"], d["bases"], d["sha256"]) == (o["n"], o["strings"], o["bases"], o["sha256"]), name
    assert default["difference"]["strings"] > 1000 and default["genome"]["n"] > 99_000_000
