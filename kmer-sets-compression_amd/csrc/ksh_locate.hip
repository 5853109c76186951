// Where the string ends of one container occur in another (ksh_seq_locate): the first and the last
// k-mer of each of n strings looked for among all k-mer positions of m reference sequences.
// End e = 2 s is the first k-mer of string s as written, e = 2 s + 1 its last.  The reference's positions are
// numbered in one line as in ksh_seq.h; position g with k-mer x matches end k-mer y when x == y (strand 0) or, in
// canonical mode only, x == rc(y) (strand 1; a k-mer that is its own reverse complement reads strand 0).
// count[e] is the number of matching positions, where[e] = (g << 1) | strand of the one with the smallest g, -1 if
// there is none.
//   ends  : k_loc_ends, a thread a string, as k_link_ends: both end k-mers into ends[2 n], and their keys (the k-mer,
//           in canonical mode its canonical form) claimed in the end table by atomicCAS from 0, in the probe order of
//           link_insert.  A key that is there already is simply found: ends need not be distinct.
//   table : open addressing, the next power of two >= 4 n slots, three arrays: the key word (kValid set, so that the
//           all-A k-mer is not "empty"), a 64-bit minimum word that starts as all ones, a 32-bit count.  The scan's
//           misses touch the key words only.
//   scan  : k_loc_scan<R>, the hot path.  A thread owns R consecutive positions of the line, finds its sequence,
//           reads its first window whole and rolls it and its reverse complement by a base per position (afresh at a
//           sequence boundary inside the run).  Every position probes the table with plain loads, a miss ends at the
//           first empty slot; a hit does atomicMin of (g << 1) | (x != key) on the slot's minimum word and atomicAdd
//           on its count, both relaxed at agent scope.  Minimum and sum do not depend on the order of arrival.
//   write : k_loc_write, a thread an end: its key's slot found again, the count copied, the minimum copied with the
//           strand bit XORed by "this end as written is not its key".
// The result is a function of the two containers alone.
#include "ksh_clstable.h"
#include "ksh_seq.h"

#include <cstdlib>

using ksh::pc::PoolBuf;
using ksh::pc::pool_array;

namespace {

constexpr int kLocThreads = 256;
// Positions per thread of the scan.  8, 16, 32 and 64 are built; KSH_LOCATE_RUN picks another one of them for a
// measurement (tools/locate_rate.py), this one is what the library runs: 8, 16 and 32 measured within 3 % of each
// other and 64 slower, so it is the run of k_seq_extract.
constexpr int kLocRun = 16;
// The report words: the smallest string an end of which found no slot (~0 if none), the word of the sizes' check
// (seq_positions), the number of located ends.
enum { kBadNoSlot = 0, kBadLens = 1, kLocated = 2, kReportWords = 3 };

}  // namespace

namespace ksh {

// (link_slot of ksh_links.hip: the same hash, so the tables fill alike)
__device__ __forceinline__ uint64_t loc_slot(uint64_t key, uint64_t mask) { return pc::pc_mix(key) & mask; }

__device__ __forceinline__ uint64_t loc_key(uint64_t x, int k, int canon) { return canon ? canonical(x, k) : x; }

__device__ __forceinline__ void loc_insert(unsigned long long* __restrict__ keys, uint64_t mask, uint64_t key,
                                           int64_t s, unsigned long long* __restrict__ bad) {
  const unsigned long long kw = key | kValid;
  uint64_t h = loc_slot(key, mask);
  for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    const unsigned long long prev = atomicCAS(keys + h, 0ull, kw);
    if (prev == 0 || prev == kw) return;
  }
  atomicMin(&bad[kBadNoSlot], static_cast<unsigned long long>(s));  // (cannot happen: at most half load)
}

// The slot of `key` in the finished table, mask + 1 if it has none.  Plain loads, the probe order of loc_insert: a
// key's slot lies between its hash and the first empty slot behind it.
__device__ __forceinline__ uint64_t loc_find(const unsigned long long* __restrict__ keys, uint64_t mask,
                                             uint64_t key) {
  const unsigned long long kw = key | kValid;
  uint64_t h = loc_slot(key, mask);
  for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    const unsigned long long got = keys[h];
    if (got == 0) break;
    if (got == kw) return h;
  }
  return mask + 1;
}

__global__ __launch_bounds__(kLocThreads) void k_loc_ends(const uint64_t* __restrict__ words,
                                                          const uint32_t* __restrict__ lens,
                                                          const int64_t* __restrict__ pstart, int64_t n_strings, int k,
                                                          int canon, uint64_t* __restrict__ ends,
                                                          unsigned long long* __restrict__ keys, uint64_t mask,
                                                          unsigned long long* __restrict__ bad) {
  const int64_t s = int64_t(blockIdx.x) * kLocThreads + threadIdx.x;
  if (s >= n_strings) return;
  uint64_t first, last;
  const bool single = seq_ends(words, lens, pstart, s, k, &first, &last);
  ends[2 * s] = first;
  ends[2 * s + 1] = last;
  loc_insert(keys, mask, loc_key(first, k, canon), s, bad);
  if (!single) loc_insert(keys, mask, loc_key(last, k, canon), s, bad);
}

// seq_walk over the whole line, kR positions per thread and kLocThreads * kR per workgroup: every position's key
// looked up with plain loads (loc_find's loop, the hit's two atomics inside it: a lane that has found its slot does
// not wait for the wave's last lane to end its probe), a hit recorded in the slot's minimum word and count.
template <int kR>
__global__ __launch_bounds__(kLocThreads) void k_loc_scan(const uint64_t* __restrict__ words,
                                                          const int64_t* __restrict__ pstart, int64_t n_seqs,
                                                          int64_t total, int k, int canon,
                                                          const unsigned long long* __restrict__ keys, uint64_t mask,
                                                          unsigned long long* __restrict__ mins,
                                                          uint32_t* __restrict__ counts) {
  seq_walk<kR, kLocThreads>(words, pstart, n_seqs, 0, total, k, [=](int64_t p, uint64_t fwd, uint64_t rc) {
    const uint64_t key = canon && rc < fwd ? rc : fwd;
    const unsigned long long kw = key | kValid;
    uint64_t h = loc_slot(key, mask);
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
      const unsigned long long got = keys[h];
      if (got == 0) break;  // almost every position ends here, at its first probe
      if (got == kw) {
        const unsigned long long v = (static_cast<unsigned long long>(p) << 1) | (fwd != key ? 1ull : 0ull);
        __hip_atomic_fetch_min(mins + h, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(counts + h, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  });
}

__global__ __launch_bounds__(kLocThreads) void k_loc_write(const uint64_t* __restrict__ ends, int64_t n_ends, int k,
                                                           int canon, const unsigned long long* __restrict__ keys,
                                                           uint64_t mask, const unsigned long long* __restrict__ mins,
                                                           const uint32_t* __restrict__ counts,
                                                           int64_t* __restrict__ where, uint32_t* __restrict__ count,
                                                           unsigned long long* __restrict__ bad) {
  const int64_t e = int64_t(blockIdx.x) * kLocThreads + threadIdx.x;
  if (e >= n_ends) return;
  const uint64_t x = ends[e];
  const uint64_t key = loc_key(x, k, canon);
  const uint64_t h = loc_find(keys, mask, key);
  int64_t at = -1;
  uint32_t c = 0;
  if (h <= mask) {  // (always: k_loc_ends inserted it)
    c = counts[h];
    const unsigned long long m = mins[h];
    if (m != ~0ull) at = int64_t(m ^ (x != key ? 1ull : 0ull));
  }
  where[e] = at;
  count[e] = c;
  if (c != 0) atomicAdd(&bad[kLocated], 1ull);
}

template <int kR>
static void launch_scan(hipStream_t st, const ksh_spss_view* ref, const int64_t* pstart, int64_t total, int k,
                        int canon, const unsigned long long* keys, uint64_t mask, unsigned long long* mins,
                        uint32_t* counts) {
  const int64_t per_block = int64_t(kLocThreads) * kR;
  hipLaunchKernelGGL((k_loc_scan<kR>), dim3(unsigned((total + per_block - 1) / per_block)), dim3(kLocThreads), 0, st,
                     ref->d_words, pstart, ref->n_strings, total, k, canon, keys, mask, mins, counts);
}

// The run of this call: kLocRun, or the one of 8, 16, 32, 64 that KSH_LOCATE_RUN names.
static int loc_run() {
  const char* e = std::getenv("KSH_LOCATE_RUN");
  const int r = e ? std::atoi(e) : 0;
  return r == 8 || r == 16 || r == 32 || r == 64 ? r : kLocRun;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_seq_locate(const ksh_seq_locate_req* req) {
  if (!req) return fail(KSH_INVALID_ARGUMENT, "req is NULL");
  if (req->struct_size < sizeof(ksh_seq_locate_req))
    return fail(KSH_INVALID_ARGUMENT, "req->struct_size = %zu is smaller than ksh_seq_locate_req (%zu)",
                req->struct_size, sizeof(ksh_seq_locate_req));
  ksh_ctx* ctx = req->ctx;
  if (!ctx) return fail(KSH_INVALID_ARGUMENT, "req->ctx is NULL");
  if (!req->g) return fail(KSH_INVALID_ARGUMENT, "req->g is NULL");
  KSH_TRY(check_geom(req->g));
  const int k = req->g->k;
  KSH_TRY(seq_check_k(k, "req->g: "));
  const ksh_spss_view* strings = req->strings;
  const ksh_spss_view* ref = req->reference;
  if (!strings) return fail(KSH_INVALID_ARGUMENT, "req->strings is NULL");
  KSH_TRY(seq_check_sizes(strings, "req->strings: "));
  if (ref) KSH_TRY(seq_check_sizes(ref, "req->reference: "));
  const int64_t n = strings->n_strings;
  if (n == 0) {
    KSH_TRY(seq_check_empty(strings, "req->strings: "));
    if (req->n_located) *req->n_located = 0;
    return KSH_OK;
  }
  if (!ref) return fail(KSH_INVALID_ARGUMENT, "req->reference is NULL with %lld strings", (long long)n);
  if (!strings->d_words || !strings->d_lens)
    return fail(KSH_INVALID_ARGUMENT, "req->strings: NULL words or lens with %lld strings", (long long)n);
  const int64_t m = ref->n_strings;
  if (m > 0 && (!ref->d_words || !ref->d_lens))
    return fail(KSH_INVALID_ARGUMENT, "req->reference: NULL words or lens with %lld sequences", (long long)m);
  if (!req->d_where) return fail(KSH_INVALID_ARGUMENT, "req->d_where is NULL with %lld strings", (long long)n);
  if (!req->d_count) return fail(KSH_INVALID_ARGUMENT, "req->d_count is NULL with %lld strings", (long long)n);
  if (n > (INT64_MAX >> 6))
    return fail(KSH_INVALID_ARGUMENT, "req->strings: n_strings = %lld is more than any device holds", (long long)n);
  KSH_TRY(seq_check_empty(ref, "req->reference: "));
  KSH_HIP(hipSetDevice(ctx->device));
  const int canon = req->canonical ? 1 : 0;

  // 1. the sizes of both containers, before anything reads their words (a synchronisation each)
  uint64_t slots = 1;
  while (slots < 4 * uint64_t(n)) slots <<= 1;
  PoolBuf spos_buf(ctx), rpos_buf(ctx), bad_buf(ctx), ends_buf(ctx), keys_buf(ctx), mins_buf(ctx), counts_buf(ctx);
  int64_t *spos, *rpos;
  unsigned long long *bad, *keys, *mins;
  uint64_t* ends;
  uint32_t* counts;
  KSH_TRY(pool_array(ctx, size_t(n + 1), &spos_buf, &spos));
  KSH_TRY(pool_array(ctx, size_t(m + 1), &rpos_buf, &rpos));
  KSH_TRY(pool_array(ctx, 8, &bad_buf, &bad));
  KSH_TRY(pool_array(ctx, size_t(2 * n), &ends_buf, &ends));
  KSH_TRY(pool_array(ctx, size_t(slots), &keys_buf, &keys));
  KSH_TRY(pool_array(ctx, size_t(slots), &mins_buf, &mins));
  KSH_TRY(pool_array(ctx, size_t(slots), &counts_buf, &counts));
  int64_t own = 0, total = 0;  // k-mer positions of the strings, of the reference
  KSH_TRY(seq_positions(ctx, strings, k, spos, bad + kBadLens, &own, "req->strings: "));
  if (m > 0) KSH_TRY(seq_positions(ctx, ref, k, rpos, bad + kBadLens, &total, "req->reference: "));
  if (total >= (int64_t(1) << 32))
    return fail(KSH_INVALID_ARGUMENT, "req->reference: %lld k-mer positions: the counts are exact below 2^32",
                (long long)total);

  // 2. ends, scan, write (the last synchronisation)
  const int64_t n_ends = 2 * n;
  const dim3 grid_strings(unsigned((n + kLocThreads - 1) / kLocThreads));
  const dim3 grid_ends(unsigned((n_ends + kLocThreads - 1) / kLocThreads));
  KSH_HIP(hipMemsetAsync(bad + kBadNoSlot, 0xFF, 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(bad + kLocated, 0, 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(keys, 0, size_t(slots) * 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(mins, 0xFF, size_t(slots) * 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(counts, 0, size_t(slots) * 4, ctx->stream));
  hipLaunchKernelGGL(k_loc_ends, grid_strings, dim3(kLocThreads), 0, ctx->stream, strings->d_words, strings->d_lens,
                     spos, n, k, canon, ends, keys, slots - 1, bad);
  if (total > 0) {
    const int run = loc_run();
    if (run == 8) launch_scan<8>(ctx->stream, ref, rpos, total, k, canon, keys, slots - 1, mins, counts);
    if (run == 16) launch_scan<16>(ctx->stream, ref, rpos, total, k, canon, keys, slots - 1, mins, counts);
    if (run == 32) launch_scan<32>(ctx->stream, ref, rpos, total, k, canon, keys, slots - 1, mins, counts);
    if (run == 64) launch_scan<64>(ctx->stream, ref, rpos, total, k, canon, keys, slots - 1, mins, counts);
  }
  hipLaunchKernelGGL(k_loc_write, grid_ends, dim3(kLocThreads), 0, ctx->stream, ends, n_ends, k, canon, keys,
                     slots - 1, mins, counts, req->d_where, req->d_count, bad);
  KSH_HIP(hipGetLastError());
  int64_t* h = ctx->h_pinned + 8;
  KSH_HIP(hipMemcpyAsync(h, bad, kReportWords * 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch goes back to the pool: nothing of the call is in flight)
  if (h[kBadNoSlot] != -1) return fail(KSH_INTERNAL, "ksh_seq_locate: an end found no slot in the end table");
  if (req->n_located) *req->n_located = h[kLocated];
  return KSH_OK;
}
