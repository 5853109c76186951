// What the calls that walk the k-mer positions of sequences share: ksh_seq_hits (ksh_seqhits.hip, which defines
// everything declared here), ksh_seq_class_runs (ksh_paint.hip) and ksh_seq_locate (ksh_locate.hip).  DESIGN.md 3.8b,
// 3.8g, 3.8m.  gfx950 only.
//
// The positions of all sequences are numbered in one line: sequence s owns positions pstart[s] .. pstart[s + 1)
// (pstart = exclusive scan of lens + 1), and the k-mer of position p of sequence s starts at base p + s (K - 1).
#ifndef KSH_SEQ_H_
#define KSH_SEQ_H_

#include "ksh_internal.h"

#include <algorithm>

namespace ksh {

constexpr int64_t kSeqPassBytes = int64_t(256) << 20;  // default pass: its scratch fits this
constexpr int64_t kSeqMaxPass = int64_t(1) << 28;

// The default pass of a call that keeps `bytes_per_position` of scratch per position: as many positions as fit
// kSeqPassBytes, at most the join's own pass of 2^24 queries.
inline int64_t seq_default_pass(int64_t bytes_per_position) {
  return std::min<int64_t>(int64_t(1) << 24, (kSeqPassBytes / bytes_per_position) & ~int64_t(4095));
}

// The last sequence of [lo, hi] whose first position is <= p.
__device__ __forceinline__ int64_t seq_of(const int64_t* __restrict__ pstart, int64_t lo, int64_t hi, int64_t p) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (pstart[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// What needs neither index nor device (seqs is not NULL): negative sizes, a negative pass_positions, a route
// outside 0..2, NULL words or lens with strings.
int seq_check_request(const ksh_spss_view* seqs, int route, int64_t pass_positions);

// pstart (n_strings + 1 values, already allocated) from the container's lens, and the container's sizes checked
// against n_bases before anything reads its words: synchronises the stream once.  *total = k-mer positions in all.
// Resets the arena (the scan's block sums).  n_strings >= 1.
int seq_positions(ksh_ctx* ctx, const ksh_spss_view* seqs, int k, int64_t* pstart, unsigned long long* d_bad,
                  int64_t* total);

// The 2K-bit patterns of positions p0 .. p0 + m into pat[0 .. m) (k_seq_extract).
int seq_extract(ksh_ctx* ctx, const ksh_spss_view* seqs, const int64_t* pstart, int64_t p0, int64_t m, int k,
                int canon, uint64_t* pat);

}  // namespace ksh

#endif
