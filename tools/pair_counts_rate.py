"""Pairwise intersection counts over the bench's KmerSetSet (64 sets of 10^8 k-mers, k = 23, (23, 14, uint32), inputs
made as bench.py makes them): KssIndex.pair_counts with cols = the inputs, against the route to the same table that
exists without the call: ksh_kss_get for every input, then the totals of ksh_pair_plan for every pair.  Both sides
are timed the same way: wall clock from a synchronised start to a synchronised end, median of --reps after one
warm-up.  Prints one JSON line and writes profiles/pair_counts_rate.json.

    python tools/pair_counts_rate.py [--sets 64] [--size 1e8] [--reps 3] [--profile]

--profile: afterwards, a child process runs the call alone (--call-only) under rocprofv3 --kernel-trace --stats (no
counters) and the call's kernels' rows of the stats go into the JSON.
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth, synth_torch  # noqa: E402


def wall_ms(fn, reps):
    fn()  # warm-up: the pool holds the scratch from then on
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return times[len(times) // 2], out


def baseline(ctx, dkss, g, n_inputs, offs):
    """ksh_kss_get for every input, ksh_pair_plan totals for every pair; the table on the host."""
    lib = capi.lib()
    dev = ctx.device.index
    views, held = [], []
    table = np.zeros((n_inputs, n_inputs), dtype=np.int64)
    try:
        for i in range(n_inputs):
            d_off, d_keys, n = C.c_void_p(), C.c_void_p(), C.c_int64()
            capi.check(lib.ksh_kss_get(dkss.h, i, C.byref(d_off), C.byref(d_keys), C.byref(n)))
            held += [d_off, d_keys]
            views.append(capi.SetView(d_off.value, d_keys.value, n.value))
            table[i, i] = n.value
        totals = (C.c_int64 * 3)()
        for a in range(n_inputs):
            for b in range(a + 1, n_inputs):
                capi.check(lib.ksh_pair_plan(ctx.h, C.byref(g), C.byref(views[a]), C.byref(views[b]),
                                             offs[0].data_ptr(), offs[1].data_ptr(), offs[2].data_ptr(), totals))
                table[a, b] = table[b, a] = totals[0]
    finally:
        for p in held:
            lib.ksh_free(dev, p)
    return table


def kernel_stats(argv):
    """The call alone in a child process under rocprofv3 --kernel-trace --stats; rows of the k_pair_* kernels."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "pair_counts",
               "--", sys.executable, os.path.abspath(__file__), "--call-only"] + argv
        run = subprocess.run(cmd, capture_output=True, text=True)
        if run.returncode != 0:
            return {"error": "rocprofv3 run failed with %d" % run.returncode, "stderr_tail": run.stderr[-400:]}
        rows = []
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as f:
                for r in csv.DictReader(f):
                    if "k_pair_" in r.get("Name", ""):
                        rows.append({"name": r["Name"].split("(")[0], "calls": int(r["Calls"]),
                                     "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3),
                                     "average_ms": round(float(r["AverageNs"]) / 1e6, 3)})
        return {"kernels": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--size", type=float, default=1e8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--call-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "pair_counts_rate.json"))
    args = ap.parse_args()
    k, nbits = 23, 14
    g = capi.geom(k, nbits)
    ctx = capi.Context(0)
    dev = ctx.device
    ids = synth.sample_bucket_ids(nbits, seed=args.seed + 1)
    kmers = synth_torch.phylogeny_sets(k, args.sets, int(args.size), args.seed, dev)
    compacts = []
    for i, km in enumerate(kmers):
        compacts.append(ctx.spss_encode(synth_torch.device_set(g, km), mode=0))
        kmers[i] = None
    del kmers
    dkss = capi.DeviceKmerSetSet(ctx, compacts, ids)
    idx = capi.KssIndex.from_kss(dkss)
    cols = list(range(args.sets))
    if args.call_only:
        idx.pair_counts(cols=cols, with_distinct=True)
        idx.pair_counts(cols=cols, with_distinct=True)
        idx.close()
        dkss.close()
        ctx.close()
        return
    info = idx.info()
    res = {"tool": "pair_counts_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "nodes": idx.n_nodes, "resident_bytes": info["resident_bytes"], "reps": args.reps}
    new_ms, (got, distinct) = wall_ms(lambda: idx.pair_counts(cols=cols, with_distinct=True), args.reps)
    res.update({"pair_counts_wall_ms": round(new_ms, 3), "routes_bits": idx.routes(), "distinct_kmers": int(distinct)})
    print(json.dumps(res), file=sys.stderr)
    offs = [torch.empty((1 << nbits) + 1, dtype=torch.int64, device=dev) for _ in range(3)]
    base_ms, want = wall_ms(lambda: baseline(ctx, dkss, g, args.sets, offs), args.reps)
    res.update({"baseline_wall_ms": round(base_ms, 3), "baseline_over_pair_counts": round(base_ms / new_ms, 3),
                "same_table": bool(np.array_equal(got, want))})
    idx.close()
    dkss.close()
    ctx.close()
    del compacts, offs
    torch.cuda.empty_cache()
    if args.profile:
        res["rocprofv3_kernel_stats"] = kernel_stats(["--sets", str(args.sets), "--size", str(args.size),
                                                      "--seed", str(args.seed)])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
