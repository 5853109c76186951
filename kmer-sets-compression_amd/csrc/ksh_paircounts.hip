// Exact pairwise intersection counts on a KmerSetSet index (ksh_kss_pair_counts): for chosen nodes cols[0 .. n),
// counts[a][b] = |Get(cols[a]) & Get(cols[b])|.
//
// A k-mer q is in Get(i) iff some node that holds q is reachable from i, so the row of q over the chosen columns
// is the OR of proj[j] over the nodes j that hold q (proj[j] = anc[j] projected onto cols: two 64-bit words,
// whatever the index's row width), and the table is the Gram product of the bit matrix that has one such row per
// distinct k-mer of the structure.  One pass over the resident node sets forms it:
//   1. k_pair_project (ksh_rowtile.hip): proj from anc and cols;
//   2. k_pair_gram: the tile walk of ksh_rowtile.h with the Gram consumer.  A wave takes 64 slots of a tile's
//      table, turns the rows into one 64-bit ballot per column and adds popcount(mask[a] & mask[b]) for a <= b into
//      the workgroup's 32-bit counters in LDS, which are flushed to d_counts by 64-bit atomicAdd;
//   3. k_pair_mirror: the lower triangle from the upper.
#include "ksh_rowtile.h"

#include <algorithm>

using namespace ksh::pc;

namespace {

// Counters are 32 bits wide and a tile adds at most max(kTile, 1024) to one (a single key: one entry per node), so
// flushing once the rows since the last flush reach this keeps every counter below 2^31.
constexpr int64_t kFlushCap = (int64_t(1) << 31) - 2048;

constexpr int tri(int n) { return n * (n + 1) / 2; }

// LDS of k_pair_gram: the walk, a wave's column masks, the counters.
constexpr size_t gram_lds_bytes(int n_nodes, int n_cols) {
  return walk_lds_bytes(n_nodes) + size_t(kWaves) * kMaxCols * 8 + size_t(tri(n_cols)) * 4;
}
constexpr size_t kGramLdsMax = gram_lds_bytes(kMaxNodes, kMaxCols);  // what the kernel opts in to
static_assert(kGramLdsMax == 82248 && 2 * gram_lds_bytes(1007, kMaxCols) <= (160u << 10),
              "82248 bytes at 1024 nodes and 128 columns; two workgroups per CU up to 1007 nodes");

}  // namespace

namespace ksh {

// The Gram consumer of the walk.  flags[2]: the workgroup flushed before its last tile.
struct GramConsumer {
  int n_cols;
  int64_t flush_rows;
  unsigned long long *counts, *distinct;
  unsigned long long* s_mask = nullptr;  // LDS: kMaxCols words per wave
  uint32_t* s_cnt = nullptr;  // LDS: the counter of (a, b), a <= b: a * n_cols - a * (a - 1) / 2 - a + b
  unsigned long long my_distinct = 0;
  int64_t rows_acc = 0;   // entries counted since the last flush (at least the rows: every row is an entry's)
  bool pending = false;   // the counters are flushed before the next tile is counted (uniform: rows_acc is)

  // Adds the workgroup's counters to the table (upper triangle) and zeroes them.  Called behind a tile's closing
  // barrier (the counters are complete); a barrier follows before they are added to again.
  __device__ __forceinline__ void flush() {
    for (int a = 0; a < n_cols; a++) {
      const int base = a * n_cols - a * (a - 1) / 2 - a;
      for (int b = a + int(threadIdx.x); b < n_cols; b += kThreads) {
        const uint32_t v = s_cnt[base + b];
        if (v) {
          atomicAdd(&counts[size_t(a) * n_cols + b], static_cast<unsigned long long>(v));
          s_cnt[base + b] = 0;
        }
      }
    }
  }

  __device__ __forceinline__ void bind(const TileWalk&, OwnLds* own) {
    s_mask = pc_own<unsigned long long>(own, kWaves * kMaxCols);
    s_cnt = pc_own<uint32_t>(own, tri(n_cols));
  }
  __device__ __forceinline__ void bucket_next(int64_t) {}
  __device__ __forceinline__ Bucket bucket_begun(int64_t, int64_t) { return Bucket::kWalk; }
  __device__ __forceinline__ bool settle(int* flags) {
    if (!pending) return false;
    flush();
    if (threadIdx.x == 0) flags[2] = 1;
    pending = false;
    rows_acc = 0;
    return true;
  }
  // Gram of the 64 slots this wave holds in this round (an empty slot is a zero row)
  __device__ __forceinline__ void slot(const Slot& s) {
    const int lane = threadIdx.x & 63;
    unsigned long long* mask = s_mask + (threadIdx.x >> 6) * kMaxCols;
    if (s.occ) my_distinct++;
    if (__ballot((s.r0 | s.r1) != 0) == 0) return;
    uint64_t m0 = 0, m1 = 0;
    const int c0 = min(n_cols, 64);
    for (int c = 0; c < c0; c++) {
      const unsigned long long holders = __ballot((s.r0 >> c) & 1);
      if (lane == c) m0 = holders;
    }
    for (int c = 64; c < n_cols; c++) {
      const unsigned long long holders = __ballot((s.r1 >> (c - 64)) & 1);
      if (lane == c - 64) m1 = holders;
    }
    // (the masks are written and read by this wave only: its LDS operations complete in order)
    mask[lane] = m0;
    mask[64 + lane] = m1;
    __builtin_amdgcn_wave_barrier();
    for (int a = 0; a < n_cols; a++) {
      const uint64_t ma = pc_uniform(mask[a]);
      if (ma == 0) continue;
      const int base = a * n_cols - a * (a - 1) / 2 - a;
      for (int bb = a + lane; bb < n_cols; bb += 64) {
        const uint32_t v = uint32_t(__popcll(ma & mask[bb]));
        if (v) atomicAdd(&s_cnt[base + bb], v);
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void tile_done(int total) {
    rows_acc += total;
    if (rows_acc >= flush_rows) pending = true;
  }
  __device__ __forceinline__ void bucket_done(int64_t) {}
  __device__ __forceinline__ void finish() {
    if (rows_acc > 0) flush();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) my_distinct += __shfl_xor(my_distinct, d, 64);
    if ((threadIdx.x & 63) == 0 && my_distinct) atomicAdd(distinct, my_distinct);
  }
};

template <typename KeyT>
__global__ __launch_bounds__(kThreads) void k_pair_gram(WalkArgs a, GramConsumer c) {
  pc_walk<KeyT>(a, c);
}

__global__ __launch_bounds__(256) void k_pair_mirror(int64_t* __restrict__ counts, int n_cols) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cols * n_cols) return;
  const int a = i / n_cols, b = i % n_cols;
  if (a > b) counts[i] = counts[b * n_cols + a];
}

template <typename KeyT>
static int launch_gram(ksh_ctx* ctx, const IndexShape& x, const uint64_t* proj, int n_cols, int64_t flush_rows,
                       int64_t* d_counts, unsigned long long* distinct) {
  return walk_launch(ctx, x, proj, k_pair_gram<KeyT>, gram_lds_bytes(x.n_nodes, n_cols), kGramLdsMax,
                     lds_opt_in_bit<KeyT>(kLdsPairGram),
                     GramConsumer{n_cols, flush_rows, reinterpret_cast<unsigned long long*>(d_counts), distinct});
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_kss_pair_counts(const int32_t* cols, int32_t n_cols, ksh_kss_index* idx, int64_t flush_rows,
                                   int64_t* d_counts, int64_t* n_distinct) {
  if (!idx || !d_counts) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  if (flush_rows < 0) return fail(KSH_INVALID_ARGUMENT, "flush_rows = %lld is negative", (long long)flush_rows);
  KSH_TRY(check_col_count(cols, n_cols, "cols"));
  const IndexShape x = index_shape(idx);
  ColList list{};
  KSH_TRY(resolve_cols(cols, n_cols, x, "cols", &list, &n_cols));
  ksh_ctx* ctx = x.ctx;
  PoolBuf proj(ctx), distinct_buf(ctx);
  KSH_TRY(walk_prologue(idx, x, list, n_cols, &proj));
  KSH_TRY(pool_alloc(ctx, 16, &distinct_buf.p));
  auto* distinct = static_cast<unsigned long long*>(distinct_buf.p);
  KSH_HIP(hipMemsetAsync(distinct, 0, 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(d_counts, 0, size_t(n_cols) * size_t(n_cols) * 8, ctx->stream));
  const int64_t flush = flush_rows > 0 ? std::min(flush_rows, kFlushCap) : kFlushCap;
  KSH_TRY(KSH_BY_KEY(x.g.key_bytes, launch_gram, ctx, x, static_cast<const uint64_t*>(proj.p), n_cols, flush,
                     d_counts, distinct));
  hipLaunchKernelGGL(k_pair_mirror, dim3(unsigned((n_cols * n_cols + 255) / 256)), dim3(256), 0, ctx->stream,
                     d_counts, n_cols);
  KSH_HIP(hipGetLastError());
  if (n_distinct) {
    KSH_HIP(hipMemcpyAsync(ctx->h_pinned, distinct, 8, hipMemcpyDeviceToHost, ctx->stream));
    KSH_HIP(hipStreamSynchronize(ctx->stream));
    *n_distinct = ctx->h_pinned[0];
  }
  return KSH_OK;
}
