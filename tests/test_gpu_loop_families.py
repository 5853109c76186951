"""The KmerSetSet build on the degenerate families of tests/loop_families.py against the oracle, by every route:
the default ksh_kss_build on one lane and on four, KSH_KSS_LOOP=ahead, KSH_REWEIGH=full, the owned build over rank
threads (with fewer inputs than ranks too) and over gloo processes, the sharded build over gloo, and the index on
the structures that come out.  What the families are there for -- ties at the arg-max, empty nodes inside the loop,
a check whose improvement is negative, a loop that ends on weight 0 after some merges, an interval of 4 and 6,
one input, every bucket in the sample -- is pinned on the oracle alone by test_loop_families_cpu.py; here every
comparison is the full compare() of tests/kss_compare.py (the workers keep their own checks).  And n_inputs = 0:
KSH_OK and a structure of 0 nodes on all three entry points (include/kmersets_hip.h)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import loop_families as lf
import oracle_lib as ol
from kmersets import capi, synth
from kss_compare import compare

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = {}


def oracle(name):
    """The oracle's structure of a family, built once per session and left unchanged."""
    if name not in _ORACLE:
        _ORACLE[name] = lf.oracle_build(ol, name)
    return _ORACLE[name]


def build_device(ctx, name):
    k, n, kb, sets, ids, osets, ocompacts, okss = oracle(name)
    g = capi.geom(k, n)
    dcompacts = [capi.DeviceSpss.from_strings(g, c.strings(), ctx.device) for c in ocompacts]
    return sets, osets, okss, capi.DeviceKmerSetSet(ctx, dcompacts, ids)


@pytest.fixture(scope="module")
def ctx(gpu):
    c = capi.Context(0)
    c.set_lanes(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", lf.FAMILIES)
def test_family_default_build(ctx, name):
    sets, osets, okss, dkss = build_device(ctx, name)
    try:
        assert compare(sets, osets, okss, dkss) == len(okss.iterations())
    finally:
        dkss.close()


def test_families_four_lanes(gpu):
    """Every family twice on one fresh context with four lanes: the empty nodes are encoded on a lane like any
    other, the lanes and their scratch are reused from family to family."""
    c = capi.Context(0)
    c.set_lanes(4)
    try:
        for name in lf.FAMILIES:
            for rep in range(2):
                sets, osets, okss, dkss = build_device(c, name)
                try:
                    compare(sets, osets, okss, dkss)
                except AssertionError as e:
                    raise AssertionError("%s, build %d: %s" % (name, rep, e)) from e
                finally:
                    dkss.close()
    finally:
        c.close()


@pytest.mark.parametrize("switch", ["KSH_KSS_LOOP=ahead", "KSH_REWEIGH=full"])
def test_families_switch(gpu, switch):
    """The control loop ahead of the sets (the weight-only plan of an empty node, merged_again over an interval of 4
    and 6) and the reweigh of all three families instead of the subtraction: every family, in a process of its own
    per switch (they are read once)."""
    key, value = switch.split("=")
    env = dict(os.environ)
    env[key] = value
    r = subprocess.run([sys.executable, os.path.join(HERE, "loop_families_worker.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "loop families ok %d" % len(lf.FAMILIES) in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    if key == "KSH_KSS_LOOP":      # the route was taken: some node was only weighed somewhere
        assert any(" (0 weighed)" not in line for line in r.stdout.splitlines() if "merges" in line), r.stdout


def run_threads(name, world, env=None):
    k, n, kb, sets, ids = lf.family(name)
    cmd = [sys.executable, os.path.join(HERE, "owned_threads_worker.py"), str(k), str(n), str(kb), str(len(sets)), "0",
           "0", str(world), "striped", "family=" + name]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    _, _, _, _, _, _, _, okss = oracle(name)
    assert res["ok"] and res["world"] == world
    assert res["iterations"] == len(okss.iterations()) and res["nodes"] == okss.size()
    assert res["checks"] == len(okss.checkpoints()[0])
    assert sum(res["nodes_per_rank"]) == res["nodes"]
    assert res["bytes_sent"] == res["bytes_received"]
    return res, len(sets)


@pytest.mark.parametrize("name", lf.FAMILIES)
def test_family_owned_threads(gpu, name):
    """ksh_kss_build_owned, four rank threads, striped owners, the weight tables dealt out by pair list and
    all-gathered (the default): the gathered table is searched in the order of the reference's std::map, empty sets
    travel and are handed over, and with fewer inputs than ranks (one_input, two_identical, three_identical,
    all_empty) some ranks own nothing.  The worker checks the oracle on every rank and that each node is held by
    exactly one."""
    res, n0 = run_threads(name, 4)
    # the initial table (one pair or more) + one per iteration that has a third node to weigh the new one against
    if n0 >= 3:
        assert res["weight_gathers"] >= res["iterations"] + 1
    elif n0 == 2:
        assert res["weight_gathers"] >= 1


@pytest.mark.parametrize("name", ["permuted_ties", "star", "dups_of_two"])
def test_family_owned_threads_replicated(gpu, name):
    """... and with every rank weighing its own replica of the samples: the same ties, no exchange."""
    res, _ = run_threads(name, 4, env=dict(os.environ, KSH_OWNED_WEIGHTS="replicated"))
    assert res["weight_gathers"] == 0


GLOO_FAMILIES = ["dups_of_two", "permuted_ties", "one_input"]


def run_gloo(worker, name, port, extra=()):
    k, n, kb, sets, ids = lf.family(name)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(HERE, worker), str(k), str(n), str(kb), str(len(sets)), "0", "0", *extra, "family=" + name]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    _, _, _, _, _, _, _, okss = oracle(name)
    assert res["ok"] and res["iterations"] == len(okss.iterations()) and res["nodes"] == okss.size()
    return res


@pytest.mark.parametrize("name", GLOO_FAMILIES)
def test_family_owned_gloo(gpu, name):
    """ksh_kss_build_owned with two processes over gloo, striped: one_input leaves rank 1 with nothing."""
    res = run_gloo("dist_owned_worker.py", name, 29621 + GLOO_FAMILIES.index(name), extra=("striped",))
    assert sum(res["nodes_per_rank"]) == res["nodes"] and res["bytes_sent"] == res["bytes_received"]


@pytest.mark.parametrize("name", GLOO_FAMILIES)
def test_family_sharded_gloo(gpu, name):
    """ksh_kss_build_sharded with two processes over gloo: empty nodes in the deal of the encodes, pair lists shorter
    than the exchange is worth."""
    run_gloo("dist_kss_worker.py", name, 29631 + GLOO_FAMILIES.index(name))


@pytest.mark.parametrize("name", ["dups_of_two", "star", "nested_chain", "all_empty", "sampled_23"])
def test_family_index(ctx, name):
    """KssIndex.from_kss on these structures (empty nodes, duplicate inputs): pair_counts == |Get(a) & Get(b)| from
    the oracle's Get, jaccard of duplicates exactly 1.0, query == the oracle's Contains columns, seq_hits == the column
    sums of the query of the same positions."""
    k, n, kb, sets, ids, osets, ocompacts, okss = oracle(name)
    _, _, _, dkss = build_device(ctx, name)
    index = capi.KssIndex.from_kss(dkss)
    try:
        n_nodes = okss.size()
        gets = [okss.get(i).kmers() for i in range(n_nodes)]
        for i in range(len(sets)):
            assert np.array_equal(gets[i], sets[i])
        want = np.array([[len(np.intersect1d(gets[a], gets[b], assume_unique=True)) for b in range(n_nodes)]
                         for a in range(n_nodes)], dtype=np.int64)
        assert index.n_nodes == n_nodes
        assert np.array_equal(index.pair_counts(), want)
        jac = index.jaccard()
        n_dups = 0
        for a in range(len(sets)):
            for b in range(a + 1, len(sets)):
                if np.array_equal(sets[a], sets[b]):
                    assert jac[a, b] == 1.0 and jac[b, a] == 1.0, (a, b)
                    n_dups += 1
        if name in ("dups_of_two", "all_empty", "sampled_23"):
            assert n_dups >= 1
        q = np.concatenate([s[:200] for s in sets])
        if q.size:
            cols = np.stack([np.isin(q, gets[i], assume_unique=False) for i in range(n_nodes)], axis=1)
            assert np.array_equal(index.query(q), cols)
        seqs = ocompacts[0].strings()[:5]
        if seqs:
            hits = index.seq_hits(seqs)
            assert hits.shape == (len(seqs), n_nodes)
            for row, s in zip(hits, seqs):
                positions = synth.kmers_of_bases(synth.bases_of_string(s), k)
                assert np.array_equal(row, index.query(positions).sum(axis=0).astype(np.uint32))
                pos_c = synth.canonical(positions, k)
                assert np.array_equal(row, np.array([np.isin(pos_c, gets[i]).sum() for i in range(n_nodes)], dtype=np.uint32))
    finally:
        index.close()
        dkss.close()


# --------------------------------------------------------------------------------------------- n_inputs = 0
class _NoExchange:
    """A transport of two ranks that must never be used: a build of no inputs exchanges nothing."""

    def __init__(self, rank):
        self.rank = rank

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return 2

    def get_backend(self):
        return "none"

    def _refuse(self, *args):
        raise AssertionError("a build of no inputs exchanged something")

    all_gather = all_reduce = send = recv = barrier = _refuse


def check_zero_nodes(dkss):
    assert dkss.size() == 0
    it, cp, imp = dkss.trace()
    assert it.shape == (0, 5) and cp.shape == (0, 4) and imp.shape == (0,)
    assert dkss.initial_weights().size == 0
    assert dkss.meta() == "0"
    st = dkss.stats()
    for key in ("initial_total_size", "final_total_size", "initial_spss_weight", "n_processed", "final_spss_weight",
                "packed_bytes", "length_bytes", "nodes", "n_encodes", "n_weighed"):
        assert st[key] == 0, key
    assert dkss.children(0) == []
    for reader in (dkss.node_size, dkss.node_strings, dkss.node_kmers, dkss.node_holder, dkss.get_kmers):
        with pytest.raises(capi.KshError) as e:
            reader(0)
        assert e.value.code == capi.KSH_INVALID_ARGUMENT


@pytest.mark.parametrize("route", ["build", "sharded", "owned"])
def test_zero_inputs(ctx, route):
    """n_inputs = 0 is KSH_OK and a structure of 0 nodes whose accessors work, on all three entry points, with and
    without bucket ids; the multi-rank builds exchange nothing (include/kmersets_hip.h)."""
    g = capi.geom(15, 10)
    for ids in (np.arange(1 << 10, dtype=np.int32), np.zeros(0, dtype=np.int32)):
        if route == "build":
            dkss = capi.DeviceKmerSetSet(ctx, [], ids, g=g)
        elif route == "sharded":
            dkss = capi.DeviceKmerSetSet(ctx, [], ids, dist=_NoExchange(1), g=g)
        else:
            dkss = capi.OwnedKmerSetSet(ctx, [], ids, _NoExchange(1), "cpu", owners=[], g=g)
        try:
            check_zero_nodes(dkss)
        finally:
            dkss.close()


def test_zero_inputs_null_arrays_and_bad_counts(ctx):
    """inputs and bucket_ids may be NULL with a count of 0; a negative count, or NULL with a positive one, is
    KSH_INVALID_ARGUMENT."""
    g = capi.geom(15, 10)
    L = capi.lib()
    h = C.c_void_p()
    assert L.ksh_kss_build(ctx.h, C.byref(g), None, 0, None, 0, 1, -1, C.byref(h)) == capi.KSH_OK
    n = C.c_int32(-1)
    assert L.ksh_kss_size(h, C.byref(n)) == capi.KSH_OK and n.value == 0
    assert L.ksh_kss_destroy(h) == capi.KSH_OK
    one = (C.c_int32 * 1)(0)
    for n_inputs, ids, n_ids in ((-1, one, 1), (0, one, -1), (0, None, 1), (1, one, 1)):   # (the last: inputs NULL)
        h = C.c_void_p()
        assert L.ksh_kss_build(ctx.h, C.byref(g), None, n_inputs, ids, n_ids, 1, -1, C.byref(h)) == capi.KSH_INVALID_ARGUMENT
        assert not h.value
