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
#include "ksh_rowtile.h"
#include "ksh_seq.h"

#include <algorithm>

using ksh::pc::PoolBuf;
using ksh::pc::pool_array;

namespace {

constexpr int kRun = 16;              // extraction: consecutive positions per thread
constexpr int kExtractThreads = 256;
constexpr int kCountChunk = 512;      // counting: consecutive positions per wave
constexpr int kCountThreads = 256;

// The default pass: as many positions as keep the pass's patterns (8 bytes) and rows (8 W bytes) within
// kSeqPassBytes, at most the join's own pass of 2^24 queries: 2^24 positions at W = 1, about 1.9 * 10^6 at W = 16.
int64_t default_pass(int words) { return ksh::seq_default_pass(8 + 8 * words); }

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

// Patterns of the pass's positions p0 .. p0 + m: seq_walk with kRun positions per thread, the pattern of position p
// (in canonical mode the smaller of the k-mer and its reverse complement) stored at pat[p - p0].
__global__ __launch_bounds__(kExtractThreads) void k_seq_extract(const uint64_t* __restrict__ words,
                                                                 const int64_t* __restrict__ pstart,
                                                                 int64_t n_strings, int64_t p0, int64_t m, int k,
                                                                 int canon, uint64_t* __restrict__ pat) {
  seq_walk<kRun, kExtractThreads>(words, pstart, n_strings, p0, m, k, [=](int64_t p, uint64_t fwd, uint64_t rc) {
    pat[p - p0] = canon && rc < fwd ? rc : fwd;
  });
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

int seq_check_sizes(const ksh_spss_view* v, const char* name) {
  if (v->n_strings < 0 || v->n_bases < 0)
    return fail(KSH_INVALID_ARGUMENT, "%snegative size: %lld strings, %lld bases", name, (long long)v->n_strings,
                (long long)v->n_bases);
  return KSH_OK;
}

int seq_check_k(int k, const char* name) {
  if (k < 4) return fail(KSH_INVALID_ARGUMENT, "%sk = %d: sequence queries need K >= 4", name, k);
  return KSH_OK;
}

int seq_check_empty(const ksh_spss_view* v, const char* name) {
  if (v->n_strings == 0 && v->n_bases != 0)
    return fail(KSH_INVALID_ARGUMENT, "%ssum(lens + K) = 0 but n_bases = %lld", name, (long long)v->n_bases);
  return KSH_OK;
}

int seq_check_request(const ksh_spss_view* seqs, int route, int64_t pass_positions) {
  KSH_TRY(seq_check_sizes(seqs, ""));
  if (pass_positions < 0)
    return fail(KSH_INVALID_ARGUMENT, "pass_positions = %lld is negative", (long long)pass_positions);
  if (route < 0 || route > 2) return fail(KSH_INVALID_ARGUMENT, "route = %d (0 auto, 1 search, 2 join)", route);
  if (seqs->n_strings > 0 && (!seqs->d_words || !seqs->d_lens)) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  return KSH_OK;
}

int seq_positions(ksh_ctx* ctx, const ksh_spss_view* seqs, int k, int64_t* pstart, unsigned long long* bad,
                  int64_t* total_out, const char* name) {
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
    return fail(KSH_INVALID_ARGUMENT, "%slens[%lld] = UINT32_MAX: lens + 1 does not fit the container's type", name,
                (long long)ctx->h_pinned[1]);
  if (total + n * int64_t(k - 1) != seqs->n_bases)
    return fail(KSH_INVALID_ARGUMENT, "%ssum(lens + K) = %lld but n_bases = %lld", name,
                (long long)(total + n * int64_t(k - 1)), (long long)seqs->n_bases);
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
  KSH_TRY(seq_check_k(k, ""));
  const int64_t n = seqs->n_strings;
  if (n == 0) {
    KSH_TRY(seq_check_empty(seqs, ""));
    index_set_routes(idx, 0);
    return KSH_OK;
  }
  ksh_ctx* ctx = x.ctx;
  KSH_HIP(hipSetDevice(ctx->device));

  // 1. positions per sequence, scanned; the container's sizes are checked before anything reads its words
  PoolBuf pstart_buf(ctx), bad_buf(ctx), pat_buf(ctx), rows_buf(ctx);
  int64_t* pstart;
  unsigned long long* bad;
  KSH_TRY(pool_array(ctx, size_t(n + 1), &pstart_buf, &pstart));
  KSH_TRY(pool_array(ctx, 2, &bad_buf, &bad));
  int64_t total = 0;  // k-mer positions in all
  KSH_TRY(seq_positions(ctx, seqs, k, pstart, bad, &total));

  // 2. the passes
  const int64_t pass = std::min(pass_positions > 0 ? pass_positions : default_pass(x.words), kSeqMaxPass);
  const int64_t cap = std::min(pass, total);
  uint64_t *pat, *rows;
  KSH_TRY(pool_array(ctx, size_t(cap), &pat_buf, &pat));
  KSH_TRY(pool_array(ctx, size_t(cap) * size_t(x.words), &rows_buf, &rows));
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
