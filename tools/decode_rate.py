"""Time of the SPSS decode (ksh_spss_decode_plan + ksh_spss_decode_write, through Context.spss_decode) of one
genome-like set (synth_torch) at given (k, N), timed with HIP events; also the encode of the same set, which makes
the decode's input.  N > 14 takes the decode's wide route.  Prints one JSON line.

    python tools/decode_rate.py [--size 1e8] [--reps 5] [--geoms 23:14,23:16,23:20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth_torch  # noqa: E402


def timed(fn, reps):
    fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(reps):
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    times.sort()
    return times[len(times) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--geoms", default="23:14,23:16,23:20")
    args = ap.parse_args()
    ctx = capi.Context(0)
    rows = []
    for spec in args.geoms.split(","):
        k, n = (int(x) for x in spec.split(":"))
        g = capi.geom(k, n)
        d = synth_torch.device_set(g, synth_torch.phylogeny_sets(k, 1, int(args.size), 4, ctx.device)[0])
        enc_ms, sp = timed(lambda: ctx.spss_encode(d, mode=0), args.reps)
        dec_ms, back = timed(lambda: ctx.spss_decode(sp), args.reps)
        same = back.n_keys == d.n_keys and bool(torch.equal(back.offsets, d.offsets)) and bool(
            torch.equal(back.keys[: d.n_keys * g.key_bytes], d.keys[: d.n_keys * g.key_bytes]))
        rows.append({"k": k, "n_bucket_bits": n, "key_bytes": g.key_bytes, "kmers": d.n_keys,
                     "decode_ms": round(dec_ms, 3), "encode_ms": round(enc_ms, 3), "round_trip": same})
        del d, sp, back
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"tool": "decode_rate", "reps": args.reps, "rows": rows}))


if __name__ == "__main__":
    main()
