// The toolkit of the calls that work on a packed 2-bit container and the line of its k-mer positions: ksh_seq_hits
// (ksh_seqhits.hip, which defines every host function declared here), ksh_seq_class_runs (ksh_paint.hip), ksh_spss_cut
// (ksh_cut.hip), ksh_spss_links (ksh_links.hip), ksh_link_bubbles (ksh_bubbles.hip) and ksh_seq_locate
// (ksh_locate.hip).  DESIGN.md 3.8b, 3.8g .. 3.8j, 3.8m.  gfx950 only.
//
// The positions of all sequences are numbered in one line: sequence s owns positions pstart[s] .. pstart[s + 1)
// (pstart = exclusive scan of lens + 1), and the k-mer of position p of sequence s starts at base p + s (K - 1).
#ifndef KSH_SEQ_H_
#define KSH_SEQ_H_

#include "ksh_internal.h"
#include "ksh_kmer.h"

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

// The K bases from base b of the stream on, as a 2K-bit pattern (a window spans at most two words; bits behind the
// window never count).
__device__ __forceinline__ uint64_t seq_window(const uint64_t* __restrict__ words, int64_t b, int k) {
  const int64_t w = b >> 5;
  const int o = int(b & 31);
  uint64_t x = words[w] << (2 * o);
  if (o + k > 32) x |= words[w + 1] >> (64 - 2 * o);  // (o >= 2 here: k <= 31)
  return x >> (64 - 2 * k);
}

// Both end k-mers of string s as written.  Returns whether the string is one k-mer: it then has one end, read once.
__device__ __forceinline__ bool seq_ends(const uint64_t* __restrict__ words, const uint32_t* __restrict__ lens,
                                         const int64_t* __restrict__ pstart, int64_t s, int k, uint64_t* first,
                                         uint64_t* last) {
  const int64_t b0 = pstart[s] + s * int64_t(k - 1);
  const uint32_t len = lens[s];
  *first = seq_window(words, b0, k);
  *last = len == 0 ? *first : seq_window(words, b0 + int64_t(len), k);
  return len == 0;
}

// The rolling walk over positions p0 .. p0 + m of the line, by a grid of workgroups of kThreads threads: f(p, fwd, rc)
// for every position p, fwd its k-mer as written and rc the reverse complement.  Thread t of the grid takes positions
// p0 + t * kR .. of them, finds the sequence of its first one (a search between the sequences of the workgroup's
// first and last position, which two threads look up among all sequences), reads that window whole and rolls it
// from there: two bits in at the low end, two out at the top, the reverse complement alongside.  A run that passes
// the end of its sequence reads the next sequence's first window whole: no window crosses from one sequence into
// the next.  Every thread of the workgroup calls it (it synchronises the workgroup once).
template <int kR, int kThreads, class F>
__device__ __forceinline__ void seq_walk(const uint64_t* __restrict__ words, const int64_t* __restrict__ pstart,
                                         int64_t n_seqs, int64_t p0, int64_t m, int k, F f) {
  __shared__ int64_t s_range[2];
  const int64_t blk0 = int64_t(blockIdx.x) * (kThreads * kR);
  if (threadIdx.x < 2) {
    const int64_t i = threadIdx.x == 0 ? blk0 : min(blk0 + int64_t(kThreads * kR), m) - 1;
    s_range[threadIdx.x] = seq_of(pstart, 0, n_seqs - 1, p0 + i);
  }
  __syncthreads();
  const int64_t i0 = blk0 + int64_t(threadIdx.x) * kR;
  if (i0 >= m) return;
  const int64_t i1 = min(i0 + int64_t(kR), m);
  int64_t s = seq_of(pstart, s_range[0], s_range[1], p0 + i0);
  int64_t s_end = pstart[s + 1];
  const uint64_t mask = kmer_mask(k);
  uint64_t fwd = 0, rc = 0, cur = 0;
  int64_t cur_w = -1;
  bool whole = true;
  for (int64_t i = i0; i < i1; i++) {
    const int64_t p = p0 + i;
    if (p >= s_end) {  // every sequence has a position: the next one starts here
      s++;
      s_end = pstart[s + 1];
      whole = true;
    }
    const int64_t b = p + s * int64_t(k - 1);  // first base of the position's k-mer
    if (whole) {
      fwd = seq_window(words, b, k);
      rc = revcomp(fwd, k);
      whole = false;
    } else {
      const int64_t j = b + k - 1;  // the base that enters
      if ((j >> 5) != cur_w) {
        cur_w = j >> 5;
        cur = words[cur_w];
      }
      const uint64_t c = (cur >> (62 - 2 * int(j & 31))) & 3;
      fwd = ((fwd << 2) | c) & mask;
      rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)));
    }
    f(p, fwd, rc);
  }
}

// The refusals that need neither index nor device.  `name` stands in front of the message: "" or "req->x: ".
// seq_check_sizes: negative sizes of a container (v is not NULL).  seq_check_request: seq_check_sizes(seqs, ""), a
// negative pass_positions, a route outside 0..2, NULL words or lens with strings ("NULL argument": ksh_seq_locate
// words that refusal otherwise and later, so it calls seq_check_sizes alone).  seq_check_k: K < 4.
// seq_check_empty: a container without strings that claims bases.
int seq_check_sizes(const ksh_spss_view* v, const char* name);
int seq_check_request(const ksh_spss_view* seqs, int route, int64_t pass_positions);
int seq_check_k(int k, const char* name);
int seq_check_empty(const ksh_spss_view* v, const char* name);

// pstart (n_strings + 1 values, already allocated) from the container's lens, and the container's sizes checked
// against n_bases before anything reads its words: synchronises the stream once.  *total = k-mer positions in all.
// Resets the arena (the scan's block sums).  n_strings >= 1.  A refusal of the container stands behind `name`.
int seq_positions(ksh_ctx* ctx, const ksh_spss_view* seqs, int k, int64_t* pstart, unsigned long long* d_bad,
                  int64_t* total, const char* name = "");

// The 2K-bit patterns of positions p0 .. p0 + m into pat[0 .. m) (k_seq_extract).
int seq_extract(ksh_ctx* ctx, const ksh_spss_view* seqs, const int64_t* pstart, int64_t p0, int64_t m, int k,
                int canon, uint64_t* pat);

}  // namespace ksh

#endif
