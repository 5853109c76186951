// Sequence queries on a KmerSetSet index (ksh_seq_hits): for every sequence s of a 2-bit stream and every
// node i, the number of k-mer positions of s whose k-mer is in Get(i).
//
// The positions of all sequences are numbered in one line: sequence s owns positions pstart[s] ..
// pstart[s + 1) (pstart = exclusive scan of lens + 1), and the k-mer of position p of sequence s starts at
// base p + s (K - 1) of the stream.  The line is cut into passes of `pass_positions`; a pass
//   1. extracts its 2K-bit patterns (k_seq_extract: a thread rolls the window over a run of positions),
//   2. looks them up with the index's own routes (search or bucket join, ksh_query.hip): rows in scratch,
//   3. sums the rows' columns per sequence (k_seq_count: a wave per run of positions, ballots and popcounts)
//      into d_hits, one atomicAdd per (run of one sequence, node) with a non-zero count.
// Patterns and rows live in the context's pool, not in its arena: the join resets the arena.
#include "ksh_kmer.h"
#include "ksh_seq.h"

#include <algorithm>

namespace {

constexpr int kRun = 16;              // extraction: consecutive positions per thread
constexpr int kExtractThreads = 256;
constexpr int kCountChunk = 512;      // counting: consecutive positions per wave
constexpr int kCountThreads = 256;

// The default pass: as many positions as keep the pass's patterns (8 bytes) and rows (8 W bytes) within
// kSeqPassBytes, at most the join's own pass of 2^24 queries: 2^24 positions at W = 1, about 1.9 * 10^6 at W = 16.
int64_t default_pass(int words) { return ksh::seq_default_pass(8 + 8 * words); }

struct PoolBuf {
  ksh_ctx* ctx;
  void* p = nullptr;
  explicit PoolBuf(ksh_ctx* c) : ctx(c) {}
  ~PoolBuf() {
    if (p) ksh::pool_free(ctx, p);  // (single stream: a later user of the block is ordered after this call's kernels)
  }
  PoolBuf(const PoolBuf&) = delete;
  PoolBuf& operator=(const PoolBuf&) = delete;
};

}  // namespace

namespace ksh {

// Positions per sequence, for the scan; bad[0] = the smallest s with lens[s] == UINT32_MAX (lens + 1 would wrap
// in the type of the container).
__global__ __launch_bounds__(256) void k_seq_sizes(const uint32_t* __restrict__ lens, int64_t n,
                                                   int64_t* __restrict__ cnt, unsigned long long* __restrict__ bad) {
  const int64_t s = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t l = lens[s];
  cnt[s] = int64_t(l) + 1;
  if (l == 0xFFFFFFFFu) atomicMin(bad, static_cast<unsigned long long>(s));
}

// The K bases from base b of the stream on, as a 2K-bit pattern (a window spans at most two words).
__device__ __forceinline__ uint64_t seq_window(const uint64_t* __restrict__ words, int64_t b, int k) {
  const int64_t w = b >> 5;
  const int o = int(b & 31);
  uint64_t x = words[w] << (2 * o);
  if (o + k > 32) x |= words[w + 1] >> (64 - 2 * o);  // (o >= 2 here: k <= 31)
  return x >> (64 - 2 * k);
}

// Patterns of the pass's positions p0 .. p0 + m: thread t takes positions t * kRun .. of the pass, finds the
// sequence of its first one (a search between the sequences of the workgroup's first and last position, which
// two threads look up among all sequences), reads that window whole and rolls it from there: two bits in at
// the low end, two out at the top, the reverse complement alongside.  A run that passes the end of its
// sequence reads the next sequence's first window whole: no window crosses from one sequence into the next.
__global__ __launch_bounds__(kExtractThreads) void k_seq_extract(const uint64_t* __restrict__ words,
                                                                 const int64_t* __restrict__ pstart,
                                                                 int64_t n_strings, int64_t p0, int64_t m, int k,
                                                                 int canon, uint64_t* __restrict__ pat) {
  __shared__ int64_t s_range[2];
  const int64_t blk0 = int64_t(blockIdx.x) * (kExtractThreads * kRun);
  if (threadIdx.x < 2) {
    const int64_t i = threadIdx.x == 0 ? blk0 : min(blk0 + int64_t(kExtractThreads * kRun), m) - 1;
    s_range[threadIdx.x] = seq_of(pstart, 0, n_strings - 1, p0 + i);
  }
  __syncthreads();
  const int64_t i0 = blk0 + int64_t(threadIdx.x) * kRun;
  if (i0 >= m) return;
  const int64_t i1 = min(i0 + int64_t(kRun), m);
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
    pat[i] = canon && rc < fwd ? rc : fwd;
  }
}

__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v |= __shfl_xor(v, d, 64);
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
  return (uint64_t(hi) << 32) | lo;  // the same in every lane, and known to be
}

// Column sums of the pass's rows per sequence.  A wave takes kCountChunk consecutive positions of the pass and
// walks them sequence by sequence; of a run of one sequence it reads 64 rows at a time (a lane a row), and for
// every column some row of the 64 has set, a ballot and a popcount give the column's sum, kept by the lane
// whose number is the column's bit: WT counters per lane, 64 WT per wave.  When the run ends (the sequence or
// the chunk does) lane b adds its non-zero counters to d_hits[s][64 w + b].
template <int WT>
__global__ __launch_bounds__(kCountThreads) void k_seq_count(const uint64_t* __restrict__ rows, int words,
                                                             const int64_t* __restrict__ pstart, int64_t n_strings,
                                                             int64_t p0, int64_t m, int n_nodes,
                                                             uint32_t* __restrict__ hits) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = int64_t(blockIdx.x) * (kCountThreads / 64) + (threadIdx.x >> 6);
  int64_t i = wave * kCountChunk;
  if (i >= m) return;
  const int64_t i_end = min(i + int64_t(kCountChunk), m);
  int64_t s = seq_of(pstart, 0, n_strings - 1, p0 + i);
  while (i < i_end) {
    const int64_t run_end = min(i_end, pstart[s + 1] - p0);
    uint32_t cnt[WT];
#pragma unroll
    for (int w = 0; w < WT; w++) cnt[w] = 0;
    for (int64_t b = i; b < run_end; b += 64) {
      const int64_t q = b + lane;
#pragma unroll
      for (int w = 0; w < WT; w++) {
        if (w < words) {
          const uint64_t v = q < run_end ? rows[q * words + w] : 0;
          if (__ballot(v != 0) == 0) continue;
          uint64_t any = wave_or(v);
          while (any) {
            const int bit = __builtin_ctzll(any);
            any &= any - 1;
            const unsigned long long holders = __ballot((v >> bit) & 1);
            if (lane == bit) cnt[w] += uint32_t(__popcll(holders));
          }
        }
      }
    }
#pragma unroll
    for (int w = 0; w < WT; w++) {
      const int col = 64 * w + lane;
      if (w < words && cnt[w] != 0 && col < n_nodes) atomicAdd(&hits[s * n_nodes + col], cnt[w]);
    }
    i = run_end;
    s++;
  }
}

template <int WT>
static void launch_count(hipStream_t st, const uint64_t* rows, int words, const int64_t* pstart, int64_t n_strings,
                         int64_t p0, int64_t m, int n_nodes, uint32_t* hits) {
  const int64_t waves = (m + kCountChunk - 1) / kCountChunk;
  const int64_t blocks = (waves + kCountThreads / 64 - 1) / (kCountThreads / 64);
  hipLaunchKernelGGL((k_seq_count<WT>), dim3(unsigned(blocks)), dim3(kCountThreads), 0, st, rows, words, pstart,
                     n_strings, p0, m, n_nodes, hits);
}

int seq_check_request(const ksh_spss_view* seqs, int route, int64_t pass_positions) {
  if (seqs->n_strings < 0 || seqs->n_bases < 0)
    return fail(KSH_INVALID_ARGUMENT, "negative size: %lld strings, %lld bases", (long long)seqs->n_strings,
                (long long)seqs->n_bases);
  if (pass_positions < 0)
    return fail(KSH_INVALID_ARGUMENT, "pass_positions = %lld is negative", (long long)pass_positions);
  if (route < 0 || route > 2) return fail(KSH_INVALID_ARGUMENT, "route = %d (0 auto, 1 search, 2 join)", route);
  if (seqs->n_strings > 0 && (!seqs->d_words || !seqs->d_lens)) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  return KSH_OK;
}

int seq_positions(ksh_ctx* ctx, const ksh_spss_view* seqs, int k, int64_t* pstart, unsigned long long* bad,
                  int64_t* total_out) {
  const int64_t n = seqs->n_strings;
  KSH_TRY(arena_reserve(ctx, size_t(n) / 32 + (size_t(1) << 20)));  // the scan's block sums
  arena_reset(ctx);
  KSH_HIP(hipMemsetAsync(bad, 0xFF, 8, ctx->stream));
  hipLaunchKernelGGL(k_seq_sizes, dim3(unsigned((n + 255) / 256)), dim3(256), 0, ctx->stream, seqs->d_lens, n, pstart,
                     bad);
  KSH_HIP(hipGetLastError());
  KSH_TRY(scan_exclusive_i64(ctx, pstart, pstart, n, pstart + n));
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned, pstart + n, 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned + 1, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t total = ctx->h_pinned[0];
  if (ctx->h_pinned[1] != -1)
    return fail(KSH_INVALID_ARGUMENT, "lens[%lld] = UINT32_MAX: lens + 1 does not fit the container's type",
                (long long)ctx->h_pinned[1]);
  if (total + n * int64_t(k - 1) != seqs->n_bases)
    return fail(KSH_INVALID_ARGUMENT, "sum(lens + K) = %lld but n_bases = %lld", (long long)(total + n * int64_t(k - 1)),
                (long long)seqs->n_bases);
  *total_out = total;
  return KSH_OK;
}

int seq_extract(ksh_ctx* ctx, const ksh_spss_view* seqs, const int64_t* pstart, int64_t p0, int64_t m, int k,
                int canon, uint64_t* pat) {
  const int64_t per_block = int64_t(kExtractThreads) * kRun;
  hipLaunchKernelGGL(k_seq_extract, dim3(unsigned((m + per_block - 1) / per_block)), dim3(kExtractThreads), 0,
                     ctx->stream, seqs->d_words, pstart, seqs->n_strings, p0, m, k, canon, pat);
  KSH_HIP(hipGetLastError());
  return KSH_OK;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_seq_hits(const ksh_spss_view* seqs, ksh_kss_index* idx, int canonicalize, int route,
                            int64_t pass_positions, uint32_t* d_hits) {
  if (!seqs || !idx || !d_hits) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  KSH_TRY(seq_check_request(seqs, route, pass_positions));
  const IndexShape x = index_shape(idx);
  const int k = x.g.k;
  if (k < 4) return fail(KSH_INVALID_ARGUMENT, "k = %d: sequence queries need K >= 4", k);
  const int64_t n = seqs->n_strings;
  if (n == 0) {
    if (seqs->n_bases != 0)
      return fail(KSH_INVALID_ARGUMENT, "sum(lens + K) = 0 but n_bases = %lld", (long long)seqs->n_bases);
    index_set_routes(idx, 0);
    return KSH_OK;
  }
  ksh_ctx* ctx = x.ctx;
  KSH_HIP(hipSetDevice(ctx->device));

  // 1. positions per sequence, scanned; the container's sizes are checked before anything reads its words
  PoolBuf pstart_buf(ctx), bad_buf(ctx), pat_buf(ctx), rows_buf(ctx);
  KSH_TRY(pool_alloc(ctx, size_t(n + 1) * 8, &pstart_buf.p));
  KSH_TRY(pool_alloc(ctx, 16, &bad_buf.p));
  auto* pstart = static_cast<int64_t*>(pstart_buf.p);
  auto* bad = static_cast<unsigned long long*>(bad_buf.p);
  int64_t total = 0;  // k-mer positions in all
  KSH_TRY(seq_positions(ctx, seqs, k, pstart, bad, &total));

  // 2. the passes
  const int64_t pass = std::min(pass_positions > 0 ? pass_positions : default_pass(x.words), kSeqMaxPass);
  const int64_t cap = std::min(pass, total);
  KSH_TRY(pool_alloc(ctx, size_t(cap) * 8, &pat_buf.p));
  KSH_TRY(pool_alloc(ctx, size_t(cap) * size_t(x.words) * 8, &rows_buf.p));
  auto* pat = static_cast<uint64_t*>(pat_buf.p);
  auto* rows = static_cast<uint64_t*>(rows_buf.p);
  KSH_HIP(hipMemsetAsync(d_hits, 0, size_t(n) * size_t(x.n_nodes) * 4, ctx->stream));
  KSH_HIP(hipMemsetAsync(x.d_flags, 0, 16, ctx->stream));
  uint32_t routes = total > pass ? uint32_t(KSH_QROUTE_SEQ_PASSES) : 0u;
  index_set_routes(idx, 0);
  for (int64_t p0 = 0; p0 < total; p0 += pass) {
    const int64_t m = std::min(pass, total - p0);
    KSH_TRY(seq_extract(ctx, seqs, pstart, p0, m, k, canonicalize ? 1 : 0, pat));
    const bool join = route == 2 || (route == 0 && index_auto_joins(idx, m));
    routes |= join ? KSH_QROUTE_JOIN : KSH_QROUTE_SEARCH;
    KSH_TRY(index_lookup(idx, join, pat, m, 0, rows));  // (the patterns are canonical already, if asked)
    switch (x.wt) {
      case 1: launch_count<1>(ctx->stream, rows, x.words, pstart, n, p0, m, x.n_nodes, d_hits); break;
      case 2: launch_count<2>(ctx->stream, rows, x.words, pstart, n, p0, m, x.n_nodes, d_hits); break;
      case 4: launch_count<4>(ctx->stream, rows, x.words, pstart, n, p0, m, x.n_nodes, d_hits); break;
      case 8: launch_count<8>(ctx->stream, rows, x.words, pstart, n, p0, m, x.n_nodes, d_hits); break;
      default: launch_count<16>(ctx->stream, rows, x.words, pstart, n, p0, m, x.n_nodes, d_hits); break;
    }
    KSH_HIP(hipGetLastError());
  }
  index_set_routes(idx, routes);
  return KSH_OK;
}
