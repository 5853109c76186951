// The tile walk over a KmerSetSet index that ksh_kss_pair_counts (ksh_paircounts.hip), ksh_kss_select_*
// (ksh_select.hip) and ksh_kss_color_classes (ksh_classes.hip) share.  gfx950 only.
//
// A workgroup of kThreads walks one bucket at a time.  A bucket whose entries (all nodes together) fit a tile is
// one tile; otherwise the workgroup walks the bucket's key range left to right and cuts it by key: every tile is
// "all remaining entries with key <= c", so the tiles of a bucket are ordered and no key straddles two of them.
// A tile's distinct keys and their rows over the chosen columns (the OR of proj[j] over the nodes j that hold the
// key) are formed in an LDS hash table: atomicCAS on the key, atomicOr on the row.  What is done with the occupied
// slots is the caller's; it leaves every slot empty (kEmpty, zero row) for the next tile.
//
// Callers rely on the barriers inside the walk: pc_bucket_begin and pc_tile_cut each pass at least one
// __syncthreads() in every thread, on every path (pc_block_sum, pc_prefix), and pc_tile_fill one between its two
// loops.  k_color_classes has thread 0 write an LDS flag ahead of pc_bucket_begin that all threads read after it,
// and reads its table's occupancy behind pc_tile_cut.  An edit that takes a barrier out of one of the three must
// give those callers one of their own.
#ifndef KSH_ROWTILE_H_
#define KSH_ROWTILE_H_

#include "ksh_internal.h"

namespace ksh {
namespace pc {

constexpr int kMaxCols = 128;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 512;             // entries of a tile that is not a single key
constexpr int kSlots = 2 * kTile;      // table slots: at most half load (a single-key tile fills one slot)
constexpr int64_t kRowsPerGroup = 8192;  // a workgroup is only started for this many entries (it zeroes and
                                         // flushes its counters whatever it counted)
constexpr unsigned long long kEmpty = ~0ull;  // no key: keys have at most 2K - N <= 62 bits

struct ColList {
  int32_t id[kMaxCols];
};

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

// The LDS of a walk, carved by the kernel: the table (kSlots keys, 2 * kSlots row words), per node the cursor and
// the end of its slice of the bucket, 8 words for the reductions, and n_nodes + 1 ints for the tile's prefix.
struct TileWalk {
  unsigned long long* t_key;
  unsigned long long* t_row;
  long long* s_cur;
  long long* s_end;
  unsigned long long* s_red;
  int* s_pre;
};
constexpr size_t walk_lds_bytes(int n_nodes) {
  return size_t(kSlots) * 24 + size_t(n_nodes) * 16 + 8 * 8 + size_t((n_nodes + 2) & ~1) * 4;
}

__device__ __forceinline__ uint64_t pc_uniform(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(uint32_t(v >> 32));
  return (uint64_t(hi) << 32) | lo;
}

// Sum of v over the workgroup, the same in every thread (two barriers; s_red: kWaves + 1 words).
__device__ __forceinline__ int64_t pc_block_sum(int64_t v, unsigned long long* s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = static_cast<unsigned long long>(v);
  __syncthreads();
  int64_t t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) t += static_cast<int64_t>(s_red[w]);
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint64_t pc_block_min(uint64_t v, unsigned long long* s_red) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t o = __shfl_xor(v, d, 64);
    v = o < v ? o : v;
  }
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t t = s_red[0];
#pragma unroll
  for (int w = 1; w < kWaves; w++) t = s_red[w] < t ? s_red[w] : t;
  __syncthreads();
  return t;
}

// s_pre[0 .. n) holds a count per node; on return s_pre[0 .. n] is their exclusive prefix (s_pre[n] = the sum,
// also returned).  Thread t scans the nodes t * per .. (t + 1) * per.
__device__ __forceinline__ int pc_prefix(int* s_pre, int n, unsigned long long* s_red) {
  const int per = (n + kThreads - 1) / kThreads;
  const int j0 = min(int(threadIdx.x) * per, n), j1 = min(j0 + per, n);
  int mine = 0;
  for (int j = j0; j < j1; j++) mine += s_pre[j];
  int inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (int(threadIdx.x & 63) >= d) inc += o;
  }
  if ((threadIdx.x & 63) == 63) s_red[threadIdx.x >> 6] = static_cast<unsigned long long>(inc);
  __syncthreads();
  int base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    const int s = int(s_red[w]);
    if (w < int(threadIdx.x >> 6)) base += s;
    total += s;
  }
  int run = base + inc - mine;
  for (int j = j0; j < j1; j++) {
    const int c = s_pre[j];
    s_pre[j] = run;
    run += c;
  }
  if (threadIdx.x == 0) s_pre[n] = total;
  __syncthreads();
  return total;
}

__device__ __forceinline__ uint64_t pc_mix(uint64_t x) {  // (keys of a tile share their high bits)
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 29;
  return x;
}

// Every slot empty: once, before the first tile.  Callers put a barrier after it.
__device__ __forceinline__ void pc_table_clear(const TileWalk& w) {
  for (int t = threadIdx.x; t < kSlots; t += kThreads) {
    w.t_key[t] = kEmpty;
    w.t_row[2 * t] = 0;
    w.t_row[2 * t + 1] = 0;
  }
}

// Bucket b: every node's slice into s_cur / s_end; returns the bucket's entries, the same in every thread.
__device__ __forceinline__ int64_t pc_bucket_begin(const NodeRef* __restrict__ nodes, int n_nodes, int64_t b,
                                                   const TileWalk& w) {
  int64_t mine = 0;
  for (int j = threadIdx.x; j < n_nodes; j += kThreads) {
    const int64_t* off = nodes[j].off;
    const int64_t c = off[b], e = off[b + 1];
    w.s_cur[j] = c;
    w.s_end[j] = e;
    mine += e - c;
  }
  return pc_block_sum(mine, w.s_red);
}

// The next tile of a bucket with `left` > 0 entries to go: s_pre[0 .. n_nodes] becomes the prefix of the entries
// each node gives to the tile; returns their number, the same in every thread.  *cut: the bucket has been cut by
// key range (flags[1] is set the first time).
template <typename KeyT>
__device__ __forceinline__ int pc_tile_cut(const NodeRef* __restrict__ nodes, int n_nodes, const TileWalk& w,
                                           int64_t left, uint64_t key_max, bool* cut, int* __restrict__ flags) {
  const int tid = threadIdx.x;
  int total;
  if (left <= kTile) {
    for (int j = tid; j < n_nodes; j += kThreads) w.s_pre[j] = int(w.s_end[j] - w.s_cur[j]);
    __syncthreads();
    total = pc_prefix(w.s_pre, n_nodes, w.s_red);
  } else {
    // the next cut: all remaining entries with key <= k_min + d.  d is guessed from the density of what is
    // left and halved while the tile does not fit; d == 0 is one key, at most one entry per node: accepted
    if (!*cut && tid == 0) flags[1] = 1;
    *cut = true;
    uint64_t m = ~uint64_t(0);
    for (int j = tid; j < n_nodes; j += kThreads) {
      if (w.s_cur[j] < w.s_end[j]) {
        const uint64_t v = static_cast<const KeyT*>(nodes[j].keys)[w.s_cur[j]];
        m = v < m ? v : m;
      }
    }
    const uint64_t k_min = pc_block_min(m, w.s_red);
    const uint64_t span = key_max - k_min;
    const double guess = (double(span) + 1.0) * (0.75 * kTile) / double(left);
    uint64_t d = guess >= double(span) ? span : uint64_t(guess);
    for (;;) {
      const uint64_t c = k_min + d;
      for (int j = tid; j < n_nodes; j += kThreads) {
        const KeyT* keys = static_cast<const KeyT*>(nodes[j].keys);
        const int64_t lo0 = w.s_cur[j];
        int64_t lo = lo0, hi = min(w.s_end[j], lo0 + kTile + 1);  // (more than kTile of one node: no fit anyway)
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (uint64_t(keys[mid]) <= c) lo = mid + 1; else hi = mid;
        }
        w.s_pre[j] = int(lo - lo0);
      }
      __syncthreads();
      total = pc_prefix(w.s_pre, n_nodes, w.s_red);
      if (total <= kTile || d == 0) break;
      d >>= 1;
    }
  }
  return total;
}

// The tile's entries into the table (entry e belongs to the node j with s_pre[j] <= e < s_pre[j + 1]), a barrier,
// and every node's cursor past what it gave.  The table is complete on return; s_cur is not read before the next
// barrier.
template <typename KeyT>
__device__ __forceinline__ void pc_tile_fill(const NodeRef* __restrict__ nodes, int n_nodes,
                                             const uint64_t* __restrict__ proj, const TileWalk& w, int total) {
  const int tid = threadIdx.x;
  for (int e = tid; e < total; e += kThreads) {
    int lo = 0, hi = n_nodes - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (w.s_pre[mid] <= e) lo = mid; else hi = mid - 1;
    }
    const int j = lo;
    const unsigned long long key = static_cast<const KeyT*>(nodes[j].keys)[w.s_cur[j] + (e - w.s_pre[j])];
    const uint64_t p0 = proj[2 * j], p1 = proj[2 * j + 1];
    uint32_t h = uint32_t(pc_mix(key)) & (kSlots - 1);
    for (;;) {
      const unsigned long long prev = atomicCAS(&w.t_key[h], kEmpty, key);
      if (prev == kEmpty || prev == key) break;
      h = (h + 1) & (kSlots - 1);
    }
    if (p0) atomicOr(&w.t_row[2 * h], static_cast<unsigned long long>(p0));
    if (p1) atomicOr(&w.t_row[2 * h + 1], static_cast<unsigned long long>(p1));
  }
  __syncthreads();
  for (int j = tid; j < n_nodes; j += kThreads) w.s_cur[j] += w.s_pre[j + 1] - w.s_pre[j];
}

}  // namespace pc

// Pinned words for the read-back of a call's results (the pair batch's buffer: every call that uses it has
// synchronised the stream before it returns, so none finds another's words in use).
inline int pinned_words(ksh_ctx* ctx, size_t n, int64_t** out) {
  if (ctx->h_batch_count < n) {
    if (ctx->h_batch) (void)hipHostFree(ctx->h_batch);
    ctx->h_batch = nullptr;
    ctx->h_batch_count = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&ctx->h_batch), n * sizeof(int64_t)) != hipSuccess)
      return fail(KSH_INTERNAL, "hipHostMalloc failed");
    ctx->h_batch_count = n;
  }
  *out = ctx->h_batch;
  return KSH_OK;
}

// proj[2 j], proj[2 j + 1] = anc[j] projected onto the n_cols columns of `cols`, for every node j, enqueued on the
// context's stream (ksh_paircounts.hip).  cols travel as a kernel argument: nothing of the caller's is read after
// the call returns.
int pair_project(ksh_ctx* ctx, const IndexShape& x, const pc::ColList& cols, int n_cols, uint64_t* proj);

}  // namespace ksh

#endif
