// Exact pairwise intersection counts on a KmerSetSet index (ksh_kss_pair_counts): for chosen nodes cols[0 .. n),
// counts[a][b] = |Get(cols[a]) & Get(cols[b])|.
//
// A k-mer q is in Get(i) iff some node that holds q is reachable from i, so the row of q over the chosen columns
// is the OR of proj[j] over the nodes j that hold q (proj[j] = anc[j] projected onto cols: two 64-bit words,
// whatever the index's row width), and the table is the Gram product of the bit matrix that has one such row per
// distinct k-mer of the structure.  One pass over the resident node sets forms it:
//   1. k_pair_project: proj from anc and cols (cols travel as a kernel argument: nothing of the caller's is read
//      after the call returns);
//   2. k_pair_gram: persistent workgroups stride over the buckets.  A bucket whose entries (all nodes together)
//      fit a tile is one tile; otherwise the workgroup walks the bucket's key range left to right and cuts it by
//      key: every tile is "all remaining entries with key <= c".  A tile's distinct keys and their rows are formed
//      in an LDS hash table (atomicCAS on the key, atomicOr on the row); a wave then takes 64 slots, turns the
//      rows into one 64-bit ballot per column and adds popcount(mask[a] & mask[b]) for a <= b into the
//      workgroup's 32-bit counters in LDS, which are flushed to d_counts by 64-bit atomicAdd;
//   3. k_pair_mirror: the lower triangle from the upper.
#include "ksh_rowtile.h"

#include <algorithm>

using namespace ksh::pc;

namespace {

// Counters are 32 bits wide and a tile adds at most max(kTile, 1024) to one (a single key: one entry per node), so
// flushing once the rows since the last flush reach this keeps every counter below 2^31.
constexpr int64_t kFlushCap = (int64_t(1) << 31) - 2048;

inline int tri(int n) { return n * (n + 1) / 2; }

// LDS of k_pair_gram: table keys and rows, a wave's column masks, per node {cur, end} and a prefix, the counters.
size_t gram_lds_bytes(int n_nodes, int n_cols) {
  return size_t(kSlots) * 24 + size_t(kWaves) * kMaxCols * 8 + size_t(n_nodes) * 16 + 8 * 8 +
         size_t((n_nodes + 2) & ~1) * 4 + size_t(tri(n_cols)) * 4;
}

}  // namespace

namespace ksh {

__global__ __launch_bounds__(256) void k_pair_project(const uint64_t* __restrict__ anc, int wt, int n_nodes,
                                                      ColList cols, int n_cols, uint64_t* __restrict__ proj) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_nodes) return;
  uint64_t w[2] = {0, 0};
  for (int c = 0; c < n_cols; c++) {
    const int id = cols.id[c];
    w[c >> 6] |= ((anc[size_t(j) * wt + (id >> 6)] >> (id & 63)) & 1) << (c & 63);
  }
  proj[2 * j] = w[0];
  proj[2 * j + 1] = w[1];
}

int pair_project(ksh_ctx* ctx, const IndexShape& x, const ColList& cols, int n_cols, uint64_t* proj) {
  hipLaunchKernelGGL(k_pair_project, dim3(unsigned((x.n_nodes + 255) / 256)), dim3(256), 0, ctx->stream, x.d_anc,
                     x.wt, x.n_nodes, cols, n_cols, proj);
  KSH_HIP(hipGetLastError());
  return KSH_OK;
}

// Adds the workgroup's counters to the table (upper triangle) and zeroes them.  Callers put a barrier before it
// (the counters are complete) and after it.
__device__ __forceinline__ void pc_flush(uint32_t* s_cnt, int n_cols, unsigned long long* __restrict__ counts) {
  for (int a = 0; a < n_cols; a++) {
    const int base = a * n_cols - a * (a - 1) / 2 - a;  // counter of (a, b), a <= b: base + b
    for (int b = a + int(threadIdx.x); b < n_cols; b += kThreads) {
      const uint32_t v = s_cnt[base + b];
      if (v) {
        atomicAdd(&counts[size_t(a) * n_cols + b], static_cast<unsigned long long>(v));
        s_cnt[base + b] = 0;
      }
    }
  }
}

// flags[1]: some bucket was cut by key range; flags[2]: some workgroup flushed before its last tile.
template <typename KeyT>
__global__ __launch_bounds__(kThreads) void k_pair_gram(const NodeRef* __restrict__ nodes, int n_nodes,
                                                        const uint64_t* __restrict__ proj, int n_cols, int64_t nb,
                                                        int key_bits, int64_t flush_rows,
                                                        unsigned long long* __restrict__ counts,
                                                        unsigned long long* __restrict__ distinct,
                                                        int* __restrict__ flags) {
  extern __shared__ unsigned long long pc_lds[];
  unsigned long long* t_key = pc_lds;
  unsigned long long* t_row = t_key + kSlots;
  unsigned long long* s_mask = t_row + 2 * kSlots;
  long long* s_cur = reinterpret_cast<long long*>(s_mask + kWaves * kMaxCols);
  long long* s_end = s_cur + n_nodes;
  unsigned long long* s_red = reinterpret_cast<unsigned long long*>(s_end + n_nodes);
  int* s_pre = reinterpret_cast<int*>(s_red + 8);
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_pre + ((n_nodes + 2) & ~1));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_cnt = n_cols * (n_cols + 1) / 2;
  const TileWalk w{t_key, t_row, s_cur, s_end, s_red, s_pre};
  pc_table_clear(w);
  for (int t = tid; t < n_cnt; t += kThreads) s_cnt[t] = 0;
  __syncthreads();

  const uint64_t key_max = (uint64_t(1) << key_bits) - 1;
  unsigned long long my_distinct = 0;
  int64_t rows_acc = 0;   // entries counted since the last flush (at least the rows: every row is an entry's)
  bool pending = false;   // the counters are flushed before the next tile is counted

  for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
    int64_t left = pc_bucket_begin(nodes, n_nodes, b, w);  // entries of the bucket not yet counted
    bool cut = false;
    while (left > 0) {
      const int total = pc_tile_cut<KeyT>(nodes, n_nodes, w, left, key_max, &cut, flags);

      if (pending) {  // (uniform: rows_acc is)
        pc_flush(s_cnt, n_cols, counts);
        if (tid == 0) flags[2] = 1;
        pending = false;
        rows_acc = 0;
        __syncthreads();
      }

      pc_tile_fill<KeyT>(nodes, n_nodes, proj, w, total);

      // Gram: a wave takes 64 slots, a lane a slot (an empty slot is a zero row), and leaves them empty
      unsigned long long* mask = s_mask + wave * kMaxCols;
      for (int g = wave; g < kSlots / 64; g += kWaves) {
        const int slot = g * 64 + lane;
        uint64_t r0 = 0, r1 = 0;
        if (t_key[slot] != kEmpty) {
          r0 = t_row[2 * slot];
          r1 = t_row[2 * slot + 1];
          t_key[slot] = kEmpty;
          t_row[2 * slot] = 0;
          t_row[2 * slot + 1] = 0;
          my_distinct++;
        }
        if (__ballot((r0 | r1) != 0) == 0) continue;
        uint64_t m0 = 0, m1 = 0;
        const int c0 = min(n_cols, 64);
        for (int c = 0; c < c0; c++) {
          const unsigned long long holders = __ballot((r0 >> c) & 1);
          if (lane == c) m0 = holders;
        }
        for (int c = 64; c < n_cols; c++) {
          const unsigned long long holders = __ballot((r1 >> (c - 64)) & 1);
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
      __syncthreads();

      left -= total;
      rows_acc += total;
      if (rows_acc >= flush_rows) pending = true;
    }
  }
  if (rows_acc > 0) pc_flush(s_cnt, n_cols, counts);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) my_distinct += __shfl_xor(my_distinct, d, 64);
  if (lane == 0 && my_distinct) atomicAdd(distinct, my_distinct);
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
  const size_t lds = gram_lds_bytes(x.n_nodes, n_cols);
  const uint32_t bit = 64u << (sizeof(KeyT) == 2 ? 0 : sizeof(KeyT) == 4 ? 1 : 2);
  if (!(ctx->lds_opt_in & bit)) {  // (more than the 64 KB a kernel gets without asking)
    KSH_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pair_gram<KeyT>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                int(gram_lds_bytes(1024, kMaxCols))));
    ctx->lds_opt_in |= bit;
  }
  int n_cu = 0;
  KSH_HIP(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int64_t nb = n_buckets(&x.g);
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, int64_t(160 << 10) / int64_t(lds)));
  const int64_t want = (x.total_keys + kRowsPerGroup - 1) / kRowsPerGroup;
  const int64_t grid = std::max<int64_t>(1, std::min({want, nb, per_cu * n_cu}));
  hipLaunchKernelGGL((k_pair_gram<KeyT>), dim3(unsigned(grid)), dim3(kThreads), lds, ctx->stream,
                     static_cast<const NodeRef*>(x.d_nodes), x.n_nodes, proj, n_cols, nb, key_bits(&x.g), flush_rows,
                     reinterpret_cast<unsigned long long*>(d_counts), distinct, x.d_flags);
  KSH_HIP(hipGetLastError());
  return KSH_OK;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_kss_pair_counts(const int32_t* cols, int32_t n_cols, ksh_kss_index* idx, int64_t flush_rows,
                                   int64_t* d_counts, int64_t* n_distinct) {
  if (!idx || !d_counts) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  if (flush_rows < 0) return fail(KSH_INVALID_ARGUMENT, "flush_rows = %lld is negative", (long long)flush_rows);
  if (cols && (n_cols < 1 || n_cols > kMaxCols))
    return fail(KSH_INVALID_ARGUMENT, "n_cols = %d is outside [1, %d]", n_cols, kMaxCols);
  const IndexShape x = index_shape(idx);
  ColList list{};
  if (!cols) {
    if (x.n_nodes > kMaxCols)
      return fail(KSH_INVALID_ARGUMENT, "cols is NULL (all nodes) but the index has %d nodes, more than %d columns: "
                                        "name the columns of each call", x.n_nodes, kMaxCols);
    n_cols = x.n_nodes;
    for (int32_t c = 0; c < n_cols; c++) list.id[c] = c;
  } else {
    std::vector<char> seen(size_t(x.n_nodes), 0);
    for (int32_t c = 0; c < n_cols; c++) {
      const int32_t id = cols[c];
      if (id < 0 || id >= x.n_nodes)
        return fail(KSH_INVALID_ARGUMENT, "cols[%d] = %d is outside [0, %d)", c, id, x.n_nodes);
      if (seen[size_t(id)]) return fail(KSH_INVALID_ARGUMENT, "cols[%d] = %d is repeated", c, id);
      seen[size_t(id)] = 1;
      list.id[c] = id;
    }
  }
  ksh_ctx* ctx = x.ctx;
  KSH_HIP(hipSetDevice(ctx->device));
  PoolBuf proj_buf(ctx), distinct_buf(ctx);
  KSH_TRY(pool_alloc(ctx, size_t(x.n_nodes) * 16, &proj_buf.p));
  KSH_TRY(pool_alloc(ctx, 16, &distinct_buf.p));
  auto* proj = static_cast<uint64_t*>(proj_buf.p);
  auto* distinct = static_cast<unsigned long long*>(distinct_buf.p);
  index_set_routes(idx, 0);
  KSH_HIP(hipMemsetAsync(x.d_flags, 0, 16, ctx->stream));
  KSH_HIP(hipMemsetAsync(distinct, 0, 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(d_counts, 0, size_t(n_cols) * size_t(n_cols) * 8, ctx->stream));
  KSH_TRY(pair_project(ctx, x, list, n_cols, proj));
  const int64_t flush = flush_rows > 0 ? std::min(flush_rows, kFlushCap) : kFlushCap;
  KSH_TRY(KSH_BY_KEY(x.g.key_bytes, launch_gram, ctx, x, proj, n_cols, flush, d_counts, distinct));
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
