"""Selections over the bench's KmerSetSet (64 sets of 10^8 k-mers, k = 23, (23, 14, uint32), inputs made as
bench.py makes them), with cols = the inputs: the core (ksh_kss_select_count + ksh_kss_select_keys) and the
multiplicity spectrum, against the route to the same core that exists without the calls: ksh_kss_get for every input,
then a chain of ksh_pair_algebra intersections.  Both sides are timed the same way: wall clock from a synchronised
start to a synchronised end, median of --reps after one warm-up.  Prints one JSON line and writes
profiles/select_rate.json.  No ratio is a pass condition: the figures are what they are.

    python tools/select_rate.py [--sets 64] [--size 1e8] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
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


class Got:
    """Get(i) as ksh_kss_get returns it: library-owned device buffers behind a DeviceSet's pointers."""

    def __init__(self, ctx, dkss, i):
        self.dev = ctx.device.index
        self.d_off, self.d_keys, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        capi.check(capi.lib().ksh_kss_get(dkss.h, i, C.byref(self.d_off), C.byref(self.d_keys), C.byref(n)))
        self.set = capi.DeviceSet.__new__(capi.DeviceSet)
        self.set.g, self.set.n_keys = dkss.g, n.value
        self.set._ptrs = (self.d_off.value, self.d_keys.value)

    def free(self):
        capi.lib().ksh_free(self.dev, self.d_off)
        capi.lib().ksh_free(self.dev, self.d_keys)


def baseline_core(ctx, dkss, n_inputs):
    """Get(0) & Get(1) & ...: one ksh_kss_get per input, one ksh_pair_algebra per step; (size, hash)."""
    first = Got(ctx, dkss, 0)
    core, held = first.set, first
    for i in range(1, n_inputs):
        nxt = Got(ctx, dkss, i)
        try:
            core_next = ctx.pair_algebra(core, nxt.set)[0]
        finally:
            nxt.free()
            if held is not None:
                held.free()
                held = None
        core = core_next
    out = (core.n_keys, ctx.set_hash(core))
    if held is not None:
        held.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--size", type=float, default=1e8)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(HERE, "..", "profiles", "select_rate.json"))
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
    info = idx.info()
    res = {"tool": "select_rate", "sets": args.sets, "size": int(args.size), "k": k, "n_bucket_bits": nbits,
           "nodes": idx.n_nodes, "resident_bytes": info["resident_bytes"], "reps": args.reps}

    def core():
        s = idx.select(cols, min_count=args.sets)
        return s.n_keys, ctx.set_hash(s)

    count_ms, (_, n_core, _) = wall_ms(lambda: idx.select_count(cols, min_count=args.sets), args.reps)
    core_ms, (n_core2, core_hash) = wall_ms(core, args.reps)
    spec_ms, spec = wall_ms(lambda: idx.spectrum(cols), args.reps)
    res.update({"core_count_wall_ms": round(count_ms, 3), "core_count_write_hash_wall_ms": round(core_ms, 3),
                "spectrum_wall_ms": round(spec_ms, 3), "routes_bits": idx.routes(), "core_kmers": int(n_core),
                "spectrum": [int(v) for v in spec]})
    print(json.dumps(res), file=sys.stderr)
    base_ms, (n_base, base_hash) = wall_ms(lambda: baseline_core(ctx, dkss, args.sets), args.reps)
    res.update({"baseline_wall_ms": round(base_ms, 3), "baseline_over_core": round(base_ms / core_ms, 3),
                "same_core": bool(n_base == n_core == n_core2 and base_hash == core_hash
                                  and int(spec[args.sets]) == n_core)})
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
