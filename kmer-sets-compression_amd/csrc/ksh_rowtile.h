// The tile walk over a KmerSetSet index that ksh_kss_pair_counts (ksh_paircounts.hip), ksh_kss_select_*
// (ksh_select.hip), ksh_kss_color_classes (ksh_classes.hip) and ksh_kss_select_class_ids (ksh_classids.hip) share
// (DESIGN.md 3.8c - 3.8f), and the host side of these calls (ksh_rowtile.hip).  gfx950 only.
//
// A workgroup of kThreads walks one bucket at a time.  A bucket whose entries (all nodes together) fit a tile is
// one tile; otherwise the workgroup walks the bucket's key range left to right and cuts it by key: every tile is
// "all remaining entries with key <= c", so the tiles of a bucket are ordered and no key straddles two of them.
// A tile's distinct keys and their rows over the chosen columns (the OR of proj[j] over the nodes j that hold the
// key) are formed in an LDS hash table: atomicCAS on the key, atomicOr on the row.
//
// The walk is one function, pc_walk: the loop over buckets, the loop over tiles and every __syncthreads() of the
// walk are in it, and a kernel is pc_walk with a consumer object whose hooks say what is done with the rows.  What
// each hook may rely on -- which barrier lies before it and which behind it -- is stated at pc_walk, hook by hook;
// a consumer that needs a barrier pc_walk does not promise there passes one of its own.  The walk's LDS is placed
// by walk_layout, for the launch's byte count and the kernel's pointers alike; a consumer's own LDS lies behind it.
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

// `count` elements of T from the context's pool into buf, *out typed on them.
template <class T>
int pool_array(ksh_ctx* ctx, size_t count, PoolBuf* buf, T** out) {
  KSH_TRY(pool_alloc(ctx, count * sizeof(T), &buf->p));
  *out = static_cast<T*>(buf->p);
  return KSH_OK;
}

// The LDS of a walk, first in every kernel's dynamic LDS: the table (kSlots keys, 2 * kSlots row words), per node
// the cursor and the end of its slice of the bucket, 8 words for the reductions, and n_nodes + 1 ints for the
// tile's prefix (rounded to whole 8-byte words).  Offsets in 8-byte words; `own` is where the consumer's region
// starts.
struct WalkLayout { size_t t_key, t_row, s_cur, s_end, s_red, s_pre, own; };
__host__ __device__ constexpr WalkLayout walk_layout(int n_nodes) {
  const size_t n = size_t(n_nodes), cur = 3 * size_t(kSlots), red = cur + 2 * n;
  return WalkLayout{0, kSlots, cur, cur + n, red, red + 8, red + 8 + (n + 2) / 2};
}
// A consumer's launch passes walk_lds_bytes(n_nodes) + the bytes of what it takes with pc_own.
constexpr size_t walk_lds_bytes(int n_nodes) { return walk_layout(n_nodes).own * 8; }
constexpr int kMaxNodes = 1024;  // the node count the LDS budgets are quoted at
static_assert(walk_lds_bytes(kMaxNodes) == 45128 && walk_lds_bytes(127) == 27184, "the walk's LDS: 24 KiB + 64 + "
              "20 bytes per node, the prefix rounded to 8");

struct TileWalk {
  unsigned long long* t_key;
  unsigned long long* t_row;
  long long* s_cur;
  long long* s_end;
  unsigned long long* s_red;
  int* s_pre;
};
// The consumer's region behind the walk's arrays, and the bytes of it that pc_own has handed out.
struct OwnLds { unsigned long long* base; size_t bytes; };
// The walk's arrays in the kernel's dynamic LDS; *own = the consumer's region, nothing of it taken.
__device__ __forceinline__ TileWalk walk_bind(unsigned long long* lds, int n_nodes, OwnLds* own) {
  const WalkLayout l = walk_layout(n_nodes);
  *own = OwnLds{lds + l.own, 0};
  return TileWalk{lds + l.t_key, lds + l.t_row, reinterpret_cast<long long*>(lds + l.s_cur),
                  reinterpret_cast<long long*>(lds + l.s_end), lds + l.s_red, reinterpret_cast<int*>(lds + l.s_pre)};
}
// The next n elements of type T of the consumer's region, from the next 8-byte boundary on.  at->bytes ends exactly
// behind them: what a consumer has taken is what its byte count adds to walk_lds_bytes, to the byte, provided the
// count lists the same arrays in the same order (an array of 4-byte elements that is not the last rounds to 8).
template <typename T>
__device__ __forceinline__ T* pc_own(OwnLds* at, size_t n) {
  const size_t from = (at->bytes + 7) & ~size_t(7);
  at->bytes = from + n * sizeof(T);
  return reinterpret_cast<T*>(at->base + from / 8);
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

// A slot of the complete table, taken: its key and row if it is occupied, and the slot left empty for the next tile.
struct Slot { bool occ; unsigned long long key; uint64_t r0, r1; };  // (r0, r1: zero where the slot was empty)
__device__ __forceinline__ Slot pc_take(const TileWalk& w, int slot) {
  Slot s{w.t_key[slot] != kEmpty, w.t_key[slot], 0, 0};
  if (s.occ) {
    s.r0 = w.t_row[2 * slot];
    s.r1 = w.t_row[2 * slot + 1];
    w.t_key[slot] = kEmpty;
    w.t_row[2 * slot] = w.t_row[2 * slot + 1] = 0;
  }
  return s;
}

// What a kernel of the walk is given besides its consumer's own arguments (walk_launch fills it).
struct WalkArgs {
  const NodeRef* nodes;
  int n_nodes;
  const uint64_t* proj;
  int64_t nb;
  int key_bits;
  int* flags;  // the index's d_flags: [1] is set by the walk when a bucket is cut by key range
};

enum class Bucket { kWalk, kSkip, kStop };

// The walk of a persistent workgroup: buckets blockIdx.x, blockIdx.x + gridDim.x, ..., each tile after tile.  A
// kernel of the walk is `pc_walk<KeyT>(a, c)` and nothing else: its consumer c travels as a kernel argument (what
// the host gives it first, then its LDS pointers and its state, which the device sets).  Every barrier of the
// walk is in this function or in the three steps it calls (pc_bucket_begin: two; pc_tile_cut: three for a bucket
// that fits a tile, otherwise two and three per halving of d; pc_tile_fill: one).  Consumer c's hooks, all called
// by every thread, and what lies round each:
//   c.bind(w, own)       takes its LDS arrays behind the walk's with pc_own, in the order its byte count lists
//                        them.  The driver zeroes exactly the bytes taken; behind that: barrier [A].
//   c.bucket_next(b)     before bucket b is begun.  Before it: [A], or the closing barrier [D] of the last tile
//                        walked.  Behind it: the two barriers of pc_bucket_begin, then bucket_begun.
//   c.bucket_begun(b, n) n = the bucket's entries, uniform.  Answers (uniformly) kWalk, kSkip (next bucket) or
//                        kStop (no more buckets: finish follows).  After kWalk with n > 0 at least one tile, and
//                        so at least five barriers, is passed before bucket_done and the next bucket_next.
//   c.settle(flags)      between a tile's cut and its fill; uniform.  Before it: the barriers of pc_tile_cut (at
//                        least three) and with them [D] of the tile before.  The consumer flushes or spills what
//                        it deferred, sets its route flag and answers whether it did; if so, and only then, [B] follows.
//   c.slot(s)            for each slot this thread takes (kSlots / kThreads rounds, slot = round * kThreads +
//                        thread: a wave takes 64 neighbours), in every lane of every round, so wave ballots are
//                        safe.  Before it: the barrier [C] inside pc_tile_fill: the table is complete.  Behind
//                        the last round: the tile's closing barrier [D].
//   c.tile_done(total)   behind [D]: what the slot rounds wrote is complete; total = the tile's entries, uniform.
//                        Before the next slot round of any thread lie the barriers of the next cut and [C].
//   c.bucket_done(b)     behind [D] of the bucket's last tile (or, for a bucket of no entries that was not
//                        skipped, behind pc_bucket_begin).  No barrier before bucket_next.
//   c.finish()           after the last bucket or kStop.  Before it: [D] of the last tile walked, or [A] if none
//                        was.  No barrier behind it.
// Per tile a workgroup passes: cut (3, or 2 + 3 per halving round) + [B] if settle answered true + [C] + [D],
// i.e. five for a bucket that fits a tile; per bucket two more for pc_bucket_begin.  Barriers inside a hook are
// the consumer's own and come on top.
template <typename KeyT, typename Consumer>
__device__ __forceinline__ void pc_walk(const WalkArgs& a, Consumer& c) {
  extern __shared__ unsigned long long pc_lds[];
  OwnLds own;
  const TileWalk w = walk_bind(pc_lds, a.n_nodes, &own);
  c.bind(w, &own);
  pc_table_clear(w);
  uint32_t* const zero = reinterpret_cast<uint32_t*>(own.base);  // (every element is 4 or 8 bytes wide)
  for (size_t t = threadIdx.x; t < own.bytes / 4; t += kThreads) zero[t] = 0;
  __syncthreads();  // [A]
  const uint64_t key_max = (uint64_t(1) << a.key_bits) - 1;
  for (int64_t b = blockIdx.x; b < a.nb; b += gridDim.x) {
    c.bucket_next(b);
    int64_t left = pc_bucket_begin(a.nodes, a.n_nodes, b, w);  // entries of the bucket not yet consumed
    const Bucket what = c.bucket_begun(b, left);
    if (what == Bucket::kStop) break;
    if (what == Bucket::kSkip) continue;
    bool cut = false;
    while (left > 0) {
      const int total = pc_tile_cut<KeyT>(a.nodes, a.n_nodes, w, left, key_max, &cut, a.flags);
      if (c.settle(a.flags)) __syncthreads();  // [B]
      pc_tile_fill<KeyT>(a.nodes, a.n_nodes, a.proj, w, total);  // [C] inside
      for (int slot = threadIdx.x; slot < kSlots; slot += kThreads) c.slot(pc_take(w, slot));
      __syncthreads();  // [D]
      c.tile_done(total);
      left -= total;
    }
    c.bucket_done(b);
  }
  c.finish();
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

// The host side of the calls (ksh_rowtile.hip).

// n_cols of a given column list: [1, kMaxCols].  Needs no index, so each entry point asks it before it
// dereferences its index; `name` is what the caller calls the list ("cols", "sel->cols").
int check_col_count(const int32_t* cols, int32_t n_cols, const char* name);
// The columns of a call whose count has passed check_col_count: cols == NULL is all nodes in order (refused above
// kMaxCols nodes), otherwise n_cols ids, each in [0, n_nodes) and none repeated.  *n_out = their number; col_of (if asked for) = per node its column or -1.
int resolve_cols(const int32_t* cols, int32_t n_cols, const IndexShape& x, const char* name, pc::ColList* list,
                 int* n_out, std::vector<int>* col_of = nullptr);

// What every call starts with: the context's device, proj from the pool (16 bytes per node), the index's route
// bits and d_flags cleared, proj formed (pair_project: proj[2 j], proj[2 j + 1] = anc[j] projected onto the n_cols
// columns, on the context's stream; cols travel as a kernel argument, so nothing of the caller's is read after the
// call returns).
int walk_prologue(ksh_kss_index* idx, const IndexShape& x, const pc::ColList& cols, int n_cols, pc::PoolBuf* proj);

// The grid of a walk whose workgroups take `lds` bytes: min(2 per CU by LDS, buckets, ceil(total_keys /
// kRowsPerGroup)), at least 1.  A kernel that can ask for more than the 64 KB it gets without asking (lds_max, its
// bytes at kMaxNodes) is granted lds_max once per context; opt_in is its bit of ksh_ctx::lds_opt_in.
int walk_grid(ksh_ctx* ctx, const IndexShape& x, const void* kernel, size_t lds, size_t lds_max, uint32_t opt_in,
              unsigned* grid);
template <typename Consumer>
int walk_launch(ksh_ctx* ctx, const IndexShape& x, const uint64_t* proj, void (*kernel)(pc::WalkArgs, Consumer),
                size_t lds, size_t lds_max, uint32_t opt_in, const Consumer& c) {
  unsigned grid = 0;
  KSH_TRY(walk_grid(ctx, x, reinterpret_cast<const void*>(kernel), lds, lds_max, opt_in, &grid));
  const pc::WalkArgs a{x.d_nodes, x.n_nodes, proj, n_buckets(&x.g), key_bits(&x.g), x.d_flags};
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(pc::kThreads), lds, ctx->stream, a, c);
  KSH_HIP(hipGetLastError());
  return KSH_OK;
}

}  // namespace ksh

#endif
