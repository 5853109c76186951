"""Time of the path cover from caller-supplied unitigs (Context.spss_cover, fast) against the whole encode of the
same set (spss_encode, mode 0), on synth_torch genome sets of 10^7 and 10^8 k-mers at (23, 14); the unitigs come from
spss_encode(mode=1).  Prints one JSON line; quoted in DESIGN.md."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kmer-sets-compression_amd"))
from kmersets import capi, synth_torch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ctx = capi.Context(0)
    rows = []
    for k, size in ((23, 10_000_000), (23, 100_000_000)):
        g = capi.geom(k, 14)
        d = synth_torch.device_set(g, synth_torch.phylogeny_sets(k, 1, size, 4, ctx.device)[0])
        unitigs = ctx.spss_encode(d, mode=1)
        enc_ms, enc = timed(lambda: ctx.spss_encode(d, mode=0), reps)
        cov_ms, cov = timed(lambda: ctx.spss_cover(unitigs), reps)
        st = ctx.spss_cover_stats()
        nw = (cov.n_bases + 31) // 32
        same = bool((cov.words[:nw] == enc.words[:nw]).all()) and cov.n_strings == enc.n_strings
        rows.append({"k": k, "kmers": d.n_keys, "unitigs": st["unitigs"], "rounds": st["rounds"],
                     "strings": st["strings"], "cover_ms": round(cov_ms, 3), "encode_ms": round(enc_ms, 3),
                     "ratio": round(cov_ms / enc_ms, 3), "same_as_encode": same})
        del d, unitigs, enc, cov
        torch.cuda.empty_cache()
    ctx.close()
    print(json.dumps({"tool": "cover_rate", "reps": reps, "rows": rows}))


if __name__ == "__main__":
    main()
