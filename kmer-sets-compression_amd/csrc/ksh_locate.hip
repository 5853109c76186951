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
#include "ksh_kmer.h"
#include "ksh_seq.h"

#include <cstdlib>

using ksh::pc::PoolBuf;

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

// The K bases from base b of the stream on (a window spans at most two words; bits behind the window never count).
__device__ __forceinline__ uint64_t loc_window(const uint64_t* __restrict__ words, int64_t b, int k) {
  const int64_t w = b >> 5;
  const int o = int(b & 31);
  uint64_t x = words[w] << (2 * o);
  if (o + k > 32) x |= words[w + 1] >> (64 - 2 * o);  // (o >= 2 here: k <= 31)
  return x >> (64 - 2 * k);
}

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
  const int64_t b0 = pstart[s] + s * int64_t(k - 1);
  const uint32_t len = lens[s];
  const uint64_t first = loc_window(words, b0, k);
  const uint64_t last = len == 0 ? first : loc_window(words, b0 + int64_t(len), k);
  ends[2 * s] = first;
  ends[2 * s + 1] = last;
  loc_insert(keys, mask, loc_key(first, k, canon), s, bad);
  if (len != 0) loc_insert(keys, mask, loc_key(last, k, canon), s, bad);
}

// Positions i0 .. i0 + kR of the line per thread, kLocThreads * kR per workgroup; the sequence of a thread's first
// position is searched between the sequences of the workgroup's first and last position, which two threads look up
// among all sequences (as k_seq_extract does).
template <int kR>
__global__ __launch_bounds__(kLocThreads) void k_loc_scan(const uint64_t* __restrict__ words,
                                                          const int64_t* __restrict__ pstart, int64_t n_seqs,
                                                          int64_t total, int k, int canon,
                                                          const unsigned long long* __restrict__ keys, uint64_t mask,
                                                          unsigned long long* __restrict__ mins,
                                                          uint32_t* __restrict__ counts) {
  __shared__ int64_t s_range[2];
  const int64_t blk0 = int64_t(blockIdx.x) * (kLocThreads * kR);
  if (threadIdx.x < 2) {
    const int64_t i = threadIdx.x == 0 ? blk0 : min(blk0 + int64_t(kLocThreads * kR), total) - 1;
    s_range[threadIdx.x] = seq_of(pstart, 0, n_seqs - 1, i);
  }
  __syncthreads();
  const int64_t i0 = blk0 + int64_t(threadIdx.x) * kR;
  if (i0 >= total) return;
  const int64_t i1 = min(i0 + int64_t(kR), total);
  int64_t s = seq_of(pstart, s_range[0], s_range[1], i0);
  int64_t s_end = pstart[s + 1];
  const uint64_t kmask = kmer_mask(k);
  uint64_t fwd = 0, rc = 0, cur = 0;
  int64_t cur_w = -1;
  bool whole = true;
  for (int64_t p = i0; p < i1; p++) {
    if (p >= s_end) {  // every sequence has a position: the next one starts here
      s++;
      s_end = pstart[s + 1];
      whole = true;
    }
    const int64_t b = p + s * int64_t(k - 1);  // first base of the position's k-mer
    if (whole) {
      fwd = loc_window(words, b, k);
      rc = revcomp(fwd, k);
      whole = false;
    } else {
      const int64_t j = b + k - 1;  // the base that enters
      if ((j >> 5) != cur_w) {
        cur_w = j >> 5;
        cur = words[cur_w];
      }
      const uint64_t c = (cur >> (62 - 2 * int(j & 31))) & 3;
      fwd = ((fwd << 2) | c) & kmask;
      rc = (rc >> 2) | ((3 - c) << (2 * (k - 1)));
    }
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
  }
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

// The sizes of one container checked on the device (seq_positions), the refusal prefixed with the container's name.
static int loc_positions(ksh_ctx* ctx, const char* name, const ksh_spss_view* v, int k, int64_t* pstart,
                         unsigned long long* bad, int64_t* total) {
  const int rc = seq_positions(ctx, v, k, pstart, bad, total);
  if (rc == KSH_INVALID_ARGUMENT) {
    const std::string why = ksh_last_error();
    return fail(rc, "%s: %s", name, why.c_str());
  }
  return rc;
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
  if (k < 4) return fail(KSH_INVALID_ARGUMENT, "req->g: k = %d: sequence queries need K >= 4", k);
  const ksh_spss_view* strings = req->strings;
  const ksh_spss_view* ref = req->reference;
  if (!strings) return fail(KSH_INVALID_ARGUMENT, "req->strings is NULL");
  if (strings->n_strings < 0 || strings->n_bases < 0)
    return fail(KSH_INVALID_ARGUMENT, "req->strings: negative size: %lld strings, %lld bases",
                (long long)strings->n_strings, (long long)strings->n_bases);
  if (ref && (ref->n_strings < 0 || ref->n_bases < 0))
    return fail(KSH_INVALID_ARGUMENT, "req->reference: negative size: %lld strings, %lld bases",
                (long long)ref->n_strings, (long long)ref->n_bases);
  const int64_t n = strings->n_strings;
  if (n == 0) {
    if (strings->n_bases != 0)
      return fail(KSH_INVALID_ARGUMENT, "req->strings: sum(lens + K) = 0 but n_bases = %lld",
                  (long long)strings->n_bases);
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
  if (m == 0 && ref->n_bases != 0)
    return fail(KSH_INVALID_ARGUMENT, "req->reference: sum(lens + K) = 0 but n_bases = %lld",
                (long long)ref->n_bases);
  KSH_HIP(hipSetDevice(ctx->device));
  const int canon = req->canonical ? 1 : 0;

  // 1. the sizes of both containers, before anything reads their words (a synchronisation each)
  uint64_t slots = 1;
  while (slots < 4 * uint64_t(n)) slots <<= 1;
  PoolBuf spos_buf(ctx), rpos_buf(ctx), bad_buf(ctx), ends_buf(ctx), keys_buf(ctx), mins_buf(ctx), counts_buf(ctx);
  KSH_TRY(pool_alloc(ctx, size_t(n + 1) * 8, &spos_buf.p));
  KSH_TRY(pool_alloc(ctx, size_t(m + 1) * 8, &rpos_buf.p));
  KSH_TRY(pool_alloc(ctx, 64, &bad_buf.p));
  KSH_TRY(pool_alloc(ctx, size_t(2 * n) * 8, &ends_buf.p));
  KSH_TRY(pool_alloc(ctx, size_t(slots) * 8, &keys_buf.p));
  KSH_TRY(pool_alloc(ctx, size_t(slots) * 8, &mins_buf.p));
  KSH_TRY(pool_alloc(ctx, size_t(slots) * 4, &counts_buf.p));
  auto* spos = static_cast<int64_t*>(spos_buf.p);
  auto* rpos = static_cast<int64_t*>(rpos_buf.p);
  auto* bad = static_cast<unsigned long long*>(bad_buf.p);
  auto* ends = static_cast<uint64_t*>(ends_buf.p);
  auto* keys = static_cast<unsigned long long*>(keys_buf.p);
  auto* mins = static_cast<unsigned long long*>(mins_buf.p);
  auto* counts = static_cast<uint32_t*>(counts_buf.p);
  int64_t own = 0, total = 0;  // k-mer positions of the strings, of the reference
  KSH_TRY(loc_positions(ctx, "req->strings", strings, k, spos, bad + kBadLens, &own));
  if (m > 0) KSH_TRY(loc_positions(ctx, "req->reference", ref, k, rpos, bad + kBadLens, &total));
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
