// The strings of an SPSS container cut at given k-mer positions (ksh_spss_cut): every run of a run list
// as ksh_seq_class_runs writes it becomes a string of its own, the K - 1 bases behind a cut repeated, so that the
// k-mers of the output in order are the k-mers of the input in order.  Cut at the runs of a painting, the strings are
// monochromatic: the coloured unitigs of the structure.
//
// Positions are numbered as in ksh_seq.h: string s owns positions pstart[s] .. pstart[s + 1) and begins at base
// pstart[s] + s (K - 1).  Run r of string s starts at position q[r] = pstart[s] + start[r] of that line, and output
// string r begins at OUTPUT base B[r] = q[r] + r (K - 1): the position line does not move, every string before r has
// added K - 1 bases.  So the output bases B[r] .. B[r + 1) are the input bases at the same index minus
// (r - s)(K - 1), and the output is one gather over the input stream.
//   check  : k_cut_check, a thread a string and a run: the run list against the container's lens, the first offender
//            of every kind by atomicMin.  It reads nothing at an index the list itself names without a range check.
//   runs   : k_cut_runs, a thread a run: its owner (a search of run_offsets), q[r] and lens_out[r].
//   gather : k_cut_gather, a thread an output word.  Two threads of a workgroup find the runs and owners of its first
//            and last base among all; every thread then searches that narrow range for the run of its word's first
//            base and walks on through the runs that begin inside the word (eight at K = 4), taking each piece from
//            two adjacent input words by 64-bit shifts.  The word is written once.
#include "ksh_rowtile.h"
#include "ksh_seq.h"

using ksh::pc::PoolBuf;
using ksh::pc::pool_array;

namespace {

constexpr int kCutThreads = 256;
// What k_cut_check reports, a word each: the smallest offending string or run, ~0 if none.
enum { kBadFirst = 0, kBadLast, kBadEmpty, kBadStartZero, kBadOrder, kBadBeyond, kBadCount, kBadLens = 7 };

}  // namespace

namespace ksh {

__global__ __launch_bounds__(kCutThreads) void k_cut_check(const uint32_t* __restrict__ lens, int64_t n_strings,
                                                           const int64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ start, int64_t n_runs,
                                                           unsigned long long* __restrict__ bad) {
  const int64_t i = int64_t(blockIdx.x) * kCutThreads + threadIdx.x;
  if (i < n_strings) {
    const int64_t a = off[i], b = off[i + 1];
    if (i == 0 && a != 0) atomicMin(&bad[kBadFirst], 0ull);
    if (i == n_strings - 1 && b != n_runs) atomicMin(&bad[kBadLast], static_cast<unsigned long long>(i));
    if (a >= b) atomicMin(&bad[kBadEmpty], static_cast<unsigned long long>(i));
    if (a >= 0 && a < n_runs && start[a] != 0) atomicMin(&bad[kBadStartZero], static_cast<unsigned long long>(i));
  }
  if (i < n_runs) {
    // (with offsets that one of the checks above refuses the owner is meaningless, and so is what follows: the
    // offsets are reported first.  The search reads off[0 .. n_strings) whatever it finds there.)
    const int64_t s = seq_of(off, 0, n_strings - 1, i);
    const int64_t at = start[i];
    if (at > int64_t(lens[s])) atomicMin(&bad[kBadBeyond], static_cast<unsigned long long>(i));
    if (i > 0 && i > off[s] && at <= int64_t(start[i - 1])) atomicMin(&bad[kBadOrder], static_cast<unsigned long long>(i));
  }
}

__global__ __launch_bounds__(kCutThreads) void k_cut_runs(const int64_t* __restrict__ pstart, int64_t n_strings,
                                                          const int64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ start, int64_t n_runs,
                                                          int64_t* __restrict__ q, uint32_t* __restrict__ lens_out) {
  const int64_t r = int64_t(blockIdx.x) * kCutThreads + threadIdx.x;
  if (r >= n_runs) return;
  const int64_t s = seq_of(off, 0, n_strings - 1, r);
  const int64_t a = start[r];
  const int64_t e = r + 1 < off[s + 1] ? int64_t(start[r + 1]) : pstart[s + 1] - pstart[s];
  q[r] = pstart[s] + a;
  lens_out[r] = uint32_t(e - a - 1);
}

// The last run of [lo, hi] whose first output base is <= b.
__device__ __forceinline__ int64_t cut_run_of(const int64_t* __restrict__ q, int64_t k1, int64_t lo, int64_t hi,
                                              int64_t b) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (q[mid] + mid * k1 <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kCutThreads) void k_cut_gather(const uint64_t* __restrict__ words,
                                                            const int64_t* __restrict__ off, int64_t n_strings,
                                                            const int64_t* __restrict__ q, int64_t n_runs, int64_t k1,
                                                            int64_t n_out, uint64_t* __restrict__ out) {
  __shared__ int64_t s_run[2], s_seq[2];
  const int64_t blk0 = int64_t(blockIdx.x) * (kCutThreads * 32);
  if (threadIdx.x < 2) {
    const int64_t b = threadIdx.x == 0 ? blk0 : min(blk0 + int64_t(kCutThreads * 32), n_out) - 1;
    const int64_t r = cut_run_of(q, k1, 0, n_runs - 1, b);
    s_run[threadIdx.x] = r;
    s_seq[threadIdx.x] = seq_of(off, 0, n_strings - 1, r);
  }
  __syncthreads();
  int64_t b = blk0 + int64_t(threadIdx.x) * 32;
  if (b >= n_out) return;
  const int64_t w0 = b, w_end = min(b + 32, n_out);
  int64_t r = cut_run_of(q, k1, s_run[0], s_run[1], b);
  int64_t s = seq_of(off, s_seq[0], s_seq[1], r);
  int64_t s_last = off[s + 1];  // the first run of the next string
  uint64_t word = 0;
  while (b < w_end) {
    const int64_t next = r + 1 < n_runs ? q[r + 1] + (r + 1) * k1 : n_out;  // where output string r ends
    const int64_t stop = min(next, w_end);
    const int cnt = int(stop - b);                                         // 1 .. 32 bases of run r
    const int64_t in = b - (r - s) * k1;
    const int64_t w = in >> 5;
    const int o = int(in & 31);
    uint64_t x = words[w] << (2 * o);
    if (o + cnt > 32) x |= words[w + 1] >> (64 - 2 * o);  // (o >= 1 here)
    if (cnt < 32) x &= ~uint64_t(0) << (64 - 2 * cnt);
    word |= x >> (2 * int(b - w0));
    b = stop;
    if (b == next) {
      r++;
      if (r >= s_last) {
        s++;
        if (r < n_runs) s_last = off[s + 1];
      }
    }
  }
  out[w0 >> 5] = word;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_spss_cut(const ksh_spss_view* seqs, ksh_ctx* ctx, const ksh_geom* g, const int64_t* d_run_offsets,
                            const uint32_t* d_run_start, int64_t n_runs, uint64_t* d_words, uint32_t* d_lens,
                            int64_t* n_bases) {
  if (!seqs) return fail(KSH_INVALID_ARGUMENT, "seqs is NULL");
  if (!ctx) return fail(KSH_INVALID_ARGUMENT, "ctx is NULL");
  if (!g) return fail(KSH_INVALID_ARGUMENT, "g is NULL");
  KSH_TRY(check_geom(g));
  KSH_TRY(seq_check_request(seqs, 0, 0));
  const int k = g->k;
  KSH_TRY(seq_check_k(k, ""));
  const int64_t n = seqs->n_strings;
  if (n_runs < 0) return fail(KSH_INVALID_ARGUMENT, "n_runs = %lld is negative", (long long)n_runs);
  if (n_runs < n)
    return fail(KSH_INVALID_ARGUMENT, "n_runs = %lld but n_strings = %lld: every string has a run", (long long)n_runs,
                (long long)n);
  if (n == 0) {
    if (n_runs != 0) return fail(KSH_INVALID_ARGUMENT, "n_runs = %lld with no strings", (long long)n_runs);
    KSH_TRY(seq_check_empty(seqs, ""));
    if (n_bases) *n_bases = 0;
    return KSH_OK;
  }
  if (!d_run_offsets) return fail(KSH_INVALID_ARGUMENT, "d_run_offsets is NULL");
  if (!d_run_start) return fail(KSH_INVALID_ARGUMENT, "d_run_start is NULL");
  if (!d_words) return fail(KSH_INVALID_ARGUMENT, "d_words is NULL");
  if (!d_lens) return fail(KSH_INVALID_ARGUMENT, "d_lens is NULL");
  KSH_HIP(hipSetDevice(ctx->device));

  // 1. the run list against the container's lens, and the container's own sizes: one synchronisation for both
  PoolBuf pstart_buf(ctx), bad_buf(ctx), q_buf(ctx);
  int64_t *pstart, *q;
  unsigned long long* bad;
  KSH_TRY(pool_array(ctx, size_t(n + 1), &pstart_buf, &pstart));
  KSH_TRY(pool_array(ctx, 8, &bad_buf, &bad));
  KSH_TRY(pool_array(ctx, size_t(n_runs), &q_buf, &q));
  KSH_HIP(hipMemsetAsync(bad, 0xFF, 64, ctx->stream));
  hipLaunchKernelGGL(k_cut_check, dim3(unsigned((n_runs + kCutThreads - 1) / kCutThreads)), dim3(kCutThreads), 0,
                     ctx->stream, seqs->d_lens, n, d_run_offsets, d_run_start, n_runs, bad);
  KSH_HIP(hipGetLastError());
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned + 8, bad, kBadCount * 8, hipMemcpyDeviceToHost, ctx->stream));
  int64_t total = 0;  // k-mer positions in all
  KSH_TRY(seq_positions(ctx, seqs, k, pstart, bad + kBadLens, &total));
  const int64_t* h = ctx->h_pinned + 8;
  if (h[kBadFirst] != -1) return fail(KSH_INVALID_ARGUMENT, "d_run_offsets[0] is not 0");
  if (h[kBadLast] != -1)
    return fail(KSH_INVALID_ARGUMENT, "d_run_offsets[%lld] (the last) is not n_runs = %lld", (long long)n,
                (long long)n_runs);
  if (h[kBadEmpty] != -1)
    return fail(KSH_INVALID_ARGUMENT, "d_run_offsets[%lld] >= d_run_offsets[%lld]: string %lld has no run",
                (long long)h[kBadEmpty], (long long)h[kBadEmpty] + 1, (long long)h[kBadEmpty]);
  if (h[kBadStartZero] != -1)
    return fail(KSH_INVALID_ARGUMENT, "d_run_start: the first run of string %lld does not start at position 0",
                (long long)h[kBadStartZero]);
  if (h[kBadOrder] != -1)
    return fail(KSH_INVALID_ARGUMENT, "d_run_start[%lld] is not above d_run_start[%lld] of the same string",
                (long long)h[kBadOrder], (long long)h[kBadOrder] - 1);
  if (h[kBadBeyond] != -1)
    return fail(KSH_INVALID_ARGUMENT, "d_run_start[%lld] is beyond the last position of its string",
                (long long)h[kBadBeyond]);

  // 2. the runs' places, and the gather
  const int64_t k1 = k - 1;
  const int64_t n_out = seqs->n_bases + (n_runs - n) * k1;
  hipLaunchKernelGGL(k_cut_runs, dim3(unsigned((n_runs + kCutThreads - 1) / kCutThreads)), dim3(kCutThreads), 0,
                     ctx->stream, pstart, n, d_run_offsets, d_run_start, n_runs, q, d_lens);
  const int64_t per_block = int64_t(kCutThreads) * 32;
  hipLaunchKernelGGL(k_cut_gather, dim3(unsigned((n_out + per_block - 1) / per_block)), dim3(kCutThreads), 0,
                     ctx->stream, seqs->d_words, d_run_offsets, n, q, n_runs, k1, n_out, d_words);
  KSH_HIP(hipGetLastError());
  KSH_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch goes back to the pool: nothing of the call is in flight)
  if (n_bases) *n_bases = n_out;
  return KSH_OK;
}
