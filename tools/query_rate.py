"""Membership queries over the bench's KmerSetSet (64 sets of 10^8 k-mers, k = 23, (23, 14, uint32), inputs made as
bench.py makes them: synth_torch.phylogeny_sets on the device, synth.sample_bucket_ids): index creation from the
structure and from its node containers, then batches of 10^4 .. 10^8 query k-mers (half members, half random) on
the per-query search (route 1), the bucket join (route 2) and auto, and the only way to answer the question without
the index: 64 x (ksh_kss_get + ksh_set_contains).  Prints one JSON line and writes profiles/query_rate.json.

    python tools/query_rate.py [--sets 64] [--size 1e8] [--batches 1e4,1e6,1e7,1e8] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth, synth_torch  # noqa: E402


class NodeSpss:
    """A node's container as the structure holds it (no copy), in the shape KssIndex.from_nodes reads."""

    def __init__(self, g, view):
        self.g, self._view = g, view

    def view(self):
        return self._view


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        times.append((start.elapsed_time(stop), (time.perf_counter() - t0) * 1e3))
    times.sort()
    return times[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--size", type=float, default=1e8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--batches", default="1e4,1e6,1e7,1e8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-batch", type=float, default=1e7)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "query_rate.json"))
    args = ap.parse_args()
    k, nbits = 23, 14
    g = capi.geom(k, nbits)
    ctx = capi.Context(0)
    dev = ctx.device
    ids = synth.sample_bucket_ids(nbits, seed=args.seed + 1)
    kmers = synth_torch.phylogeny_sets(k, args.sets, int(args.size), args.seed, dev)
    batches = [int(float(x)) for x in args.batches.split(",")]
    gen = torch.Generator(device=dev).manual_seed(7)
    per_set = (max(batches) // 2 + args.sets - 1) // args.sets
    members = torch.cat([km[torch.randint(0, km.numel(), (per_set,), device=dev, generator=gen)] for km in kmers])
    members = members[torch.randperm(members.numel(), device=dev, generator=gen)]
    compacts = []
    for i, km in enumerate(kmers):
        compacts.append(ctx.spss_encode(synth_torch.device_set(g, km), mode=0))
        kmers[i] = None
    del kmers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dkss = capi.DeviceKmerSetSet(ctx, compacts, ids)
    build_s = time.perf_counter() - t0
    n_nodes = dkss.size()
    res = {"tool": "query_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "key_bytes": g.key_bytes, "nodes": n_nodes, "build_s": round(build_s, 3), "reps": args.reps}

    (_, create_ms), idx = timed(lambda: capi.KssIndex.from_kss(dkss), 1)
    info = idx.info()
    res["index"] = dict(info, from_kss_ms=round(create_ms, 3))
    total_keys = sum(dkss.node_size(i) for i in range(n_nodes))
    res["index"]["total_keys"] = total_keys
    res["index"]["floor_ms_at_6TBps"] = round(total_keys * g.key_bytes / 6e12 * 1e3, 3)
    nodes = []
    for i in range(n_nodes):
        sv = capi.SpssView()
        capi.check(capi.lib().ksh_kss_node(dkss.h, i, C.byref(sv), None, None))
        nodes.append(NodeSpss(g, sv))
    children = [dkss.children(i) for i in range(n_nodes)]
    (_, nodes_ms), idx2 = timed(lambda: capi.KssIndex.from_nodes(ctx, nodes, children), 1)
    res["index"]["from_nodes_ms"] = round(nodes_ms, 3)

    rows = []
    for n in batches:
        half = n // 2
        q = torch.cat([members[:half], torch.randint(0, 1 << (2 * k), (n - half,), device=dev, generator=gen)])
        ref = None
        for route in (1, 2, 0):
            reps = 1 if (route == 1 and n >= 10 ** 8) else args.reps
            (ms, wall), out = timed(lambda: idx.query(q, route=route, packed=True), reps)
            bits = idx.routes()
            same = ref is None or bool(torch.equal(out, ref))
            ref = out if ref is None else ref
            rows.append({"queries": n, "route": route, "routes_bits": bits, "ms": round(ms, 3),
                         "wall_ms": round(wall, 3), "mq_per_s": round(n / ms / 1e3, 1), "same_rows": same})
            print(json.dumps(rows[-1]), file=sys.stderr)
        if n == max(batches):
            same2 = bool(torch.equal(idx2.query(q, route=0, packed=True), ref))
            res["index"]["from_nodes_rows_equal"] = same2
        del ref, out, q
    res["queries"] = rows
    idx2.close()

    # the route without an index: Get(i) materialised for every input i, then ksh_set_contains on it
    n = int(args.baseline_batch)
    q = torch.cat([members[: n // 2], torch.randint(0, 1 << (2 * k), (n - n // 2,), device=dev, generator=gen)])
    found = torch.empty(n, dtype=torch.uint8, device=dev)
    qc = torch.minimum(q, synth_torch.revcomp(q, k))  # canonicalised once, outside the timed region
    L = capi.lib()

    def baseline():
        for i in range(args.sets):
            d_off, d_keys, nk = C.c_void_p(), C.c_void_p(), C.c_int64()
            capi.check(L.ksh_kss_get(dkss.h, i, C.byref(d_off), C.byref(d_keys), C.byref(nk)))
            v = capi.SetView(d_off.value, d_keys.value, nk.value)
            capi.check(L.ksh_set_contains(ctx.h, C.byref(g), C.byref(v), qc.data_ptr(), n, found.data_ptr()))
            L.ksh_free(dev.index, d_off)  # (waits for the device: the probe is done before Get(i)'s buffers go)
            L.ksh_free(dev.index, d_keys)

    baseline()  # warm-up: the pool holds Get(i)'s buffers from then on
    (bms, bwall), _ = timed(baseline, args.reps)
    # both sides in wall-clock ms from a synchronised start to the end of their last kernel
    res["baseline"] = {"queries": n, "inputs": args.sets, "wall_ms": round(bwall, 3), "event_ms": round(bms, 3)}
    auto = [r for r in rows if r["queries"] == n and r["route"] == 0]
    if auto:
        res["baseline"]["auto_wall_ms"] = auto[0]["wall_ms"]
        res["baseline"]["auto_speedup"] = round(bwall / auto[0]["wall_ms"], 1)
    idx.close()
    dkss.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
