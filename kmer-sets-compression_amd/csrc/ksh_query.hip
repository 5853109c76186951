// Membership queries over a KmerSetSet (ksh_kss_index_*): for every query k-mer q, the nodes i
// with q in Get(i) (lib/core/kmer_set_set.h:433-454), as a row of bits over the nodes.
//
// Get(i) is the union of the sets of the nodes reachable from i, so q is in Get(i) iff some node j
// whose own resident set holds q is reachable from i.  The host closes the DAG once per index:
// anc[j] = the nodes from which j is reachable (j included), and row(q) = OR of anc[j] over the
// nodes j that hold q.  Two routes find those j:
//   * per-query search (small batches): one thread per query, a lower bound in the query's bucket
//     of every node;
//   * bucket join (large batches): the queries are grouped by bucket (histogram, scan, scatter),
//     one workgroup takes a tile of one bucket's queries into LDS and streams every node's slice of
//     that bucket through LDS once, so the node bytes read are about those of the touched slices.
#include "ksh_internal.h"
#include "ksh_kmer.h"

#include <algorithm>
#include <vector>

namespace {

using ksh::NodeRef;

constexpr int kMaxWords = 16;                  // rows up to 1024 nodes, in registers / LDS
constexpr int64_t kChunk = int64_t(1) << 24;   // join: queries per pass (bounds the scratch)
constexpr int kJoinThreads = 512;
constexpr int64_t kJoinMaxBlocks = 1 << 16;    // join grid cap: a pass can hold up to 2^24 tiles (N = 24)
constexpr int kSliceBytes = 32 << 10;          // LDS for one node's slice of a bucket
constexpr int kTileBytes = 24 << 10;           // LDS for a tile's query keys and hit rows
constexpr int kAncLdsBytes = 8 << 10;          // the anc table goes to LDS up to this size
constexpr int kSearchThreads = 256;
constexpr int64_t kCacheBytes = int64_t(256) << 20;  // MI355X Infinity Cache: auto never joins below it

int padded_words(int w) {
  int p = 1;
  while (p < w) p <<= 1;
  return p;
}

// Queries of one join tile: the keys (8 bytes) and a row of wt words each fit kTileBytes.
int join_tile(int wt) { return std::min(2048, (kTileBytes / (8 + 8 * wt)) & ~63); }

}  // namespace

struct ksh_kss_index {
  ksh_ctx* ctx = nullptr;
  ksh_geom g{};
  int32_t n_nodes = 0, words = 0, wt = 0;
  int64_t total_keys = 0, resident_bytes = 0;
  NodeRef* d_nodes = nullptr;   // pooled
  uint64_t* d_anc = nullptr;    // n_nodes * wt words, pooled
  int* d_flags = nullptr;       // int[4], see IndexShape
  std::vector<void*> owned;     // from nodes: the decoded sets (pooled)
  uint32_t routes = 0;
};

namespace ksh {

// Route 1: one thread per query; anc in LDS when it fits (anc_lds), else read through the cache.
template <typename KeyT, int WT>
__global__ __launch_bounds__(kSearchThreads) void k_query_search(const NodeRef* __restrict__ nodes, int n_nodes,
                                                                 const uint64_t* __restrict__ anc_g, int anc_lds,
                                                                 const uint64_t* __restrict__ kmers, int64_t n, int k,
                                                                 int key_bits, int canon, int words,
                                                                 uint64_t* __restrict__ rows) {
  extern __shared__ uint64_t s_anc[];
  if (anc_lds) {
    for (int t = threadIdx.x; t < n_nodes * WT; t += blockDim.x) s_anc[t] = anc_g[t];
    __syncthreads();
  }
  const uint64_t* anc = anc_lds ? s_anc : anc_g;
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t acc[WT];
#pragma unroll
  for (int w = 0; w < WT; w++) acc[w] = 0;
  uint64_t z = kmers[i];
  if ((z >> (2 * k)) == 0) {  // a pattern with bits at or above 2K is in no set
    if (canon) z = canonical(z, k);
    const int64_t b = int64_t(z >> key_bits);
    const KeyT key = KeyT(z & ((uint64_t(1) << key_bits) - 1));
    for (int j = 0; j < n_nodes; j++) {
      const int64_t* off = nodes[j].off;
      const KeyT* keys = static_cast<const KeyT*>(nodes[j].keys);
      int64_t lo = off[b], hi = off[b + 1];
      const int64_t end = hi;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      if (lo < end && keys[lo] == key) {
#pragma unroll
        for (int w = 0; w < WT; w++) acc[w] |= anc[j * WT + w];
      }
    }
  }
#pragma unroll
  for (int w = 0; w < WT; w++)
    if (w < words) rows[i * words + w] = acc[w];
}

// Join, pass 1: bucket histogram of the chunk's in-range queries; out-of-range rows are written here.
__global__ __launch_bounds__(256) void k_query_hist(const uint64_t* __restrict__ kmers, int64_t m, int k,
                                                    int key_bits, int canon, int words,
                                                    unsigned long long* __restrict__ cnt,
                                                    uint64_t* __restrict__ rows) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint64_t z = kmers[i];
  if (z >> (2 * k)) {
    for (int w = 0; w < words; w++) rows[i * words + w] = 0;
    return;
  }
  if (canon) z = canonical(z, k);
  atomicAdd(&cnt[z >> key_bits], 1ull);
}

// Tiles per bucket, in place of the counts (the bucket starts are already scanned).
__global__ __launch_bounds__(256) void k_query_tiles(int64_t* __restrict__ cnt, int64_t nb, int tile) {
  const int64_t b = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (b < nb) cnt[b] = (cnt[b] + tile - 1) / tile;
}

// Join, pass 2: (key, index in the chunk) into bucket order; `cursor` starts as the bucket starts.
__global__ __launch_bounds__(256) void k_query_scatter(const uint64_t* __restrict__ kmers, int64_t m, int k,
                                                       int key_bits, int canon,
                                                       unsigned long long* __restrict__ cursor,
                                                       uint64_t* __restrict__ pkey, uint32_t* __restrict__ pidx) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  uint64_t z = kmers[i];
  if (z >> (2 * k)) return;
  if (canon) z = canonical(z, k);
  const unsigned long long pos = atomicAdd(&cursor[z >> key_bits], 1ull);
  pkey[pos] = z & ((uint64_t(1) << key_bits) - 1);
  pidx[pos] = uint32_t(i);
}

// Join, pass 3: workgroup blockIdx.x takes tile r of bucket b (tstart: exclusive scan of the tiles per
// bucket).  Its queries' keys and hit rows sit in LDS; every node's slice of b is staged in LDS once
// and searched by all of them.  A slice longer than the staging buffer is searched in global memory.
template <typename KeyT, int WT>
__global__ __launch_bounds__(kJoinThreads) void k_query_join(const NodeRef* __restrict__ nodes, int n_nodes,
                                                             const uint64_t* __restrict__ anc_g, int anc_lds,
                                                             int64_t nb, const int64_t* __restrict__ start,
                                                             const int64_t* __restrict__ tstart, int64_t n_tiles,
                                                             int tile,
                                                             const uint64_t* __restrict__ pkey,
                                                             const uint32_t* __restrict__ pidx, int words,
                                                             uint64_t* __restrict__ rows, int* __restrict__ flags) {
  constexpr int kSliceKeys = kSliceBytes / int(sizeof(KeyT));
  extern __shared__ uint64_t lds[];
  KeyT* s_slice = reinterpret_cast<KeyT*>(lds);
  uint64_t* s_key = lds + kSliceBytes / 8;
  uint64_t* s_row = s_key + tile;
  uint64_t* s_anc = s_row + tile * WT;

  if (anc_lds)
    for (int t = threadIdx.x; t < n_nodes * WT; t += blockDim.x) s_anc[t] = anc_g[t];
  const uint64_t* anc = anc_lds ? s_anc : anc_g;

  // the grid is capped (kJoinMaxBlocks): a workgroup takes tiles blockIdx.x, + gridDim.x, ...
  for (int64_t blk = blockIdx.x; blk < n_tiles; blk += gridDim.x) {
    int64_t lo = 0, hi = nb - 1;  // the last bucket whose first tile is <= blk
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (tstart[mid] <= blk) lo = mid; else hi = mid - 1;
    }
    const int64_t b = lo;
    const int64_t q0 = start[b] + (blk - tstart[b]) * tile;
    const int nq = int(std::min<int64_t>(start[b + 1] - q0, tile));

    for (int t = threadIdx.x; t < nq; t += blockDim.x) s_key[t] = pkey[q0 + t];
    for (int t = threadIdx.x; t < nq * WT; t += blockDim.x) s_row[t] = 0;
    __syncthreads();

    for (int j = 0; j < n_nodes; j++) {
      const int64_t* off = nodes[j].off;
      const KeyT* keys = static_cast<const KeyT*>(nodes[j].keys);
      const int64_t s0 = off[b], len = off[b + 1] - s0;
      if (len <= 0) continue;
      if (len <= kSliceKeys) {
        for (int t = threadIdx.x; t < len; t += blockDim.x) s_slice[t] = keys[s0 + t];
        __syncthreads();
        for (int t = threadIdx.x; t < nq; t += blockDim.x) {
          const KeyT key = KeyT(s_key[t]);
          int a = 0, e = int(len);
          while (a < e) {
            const int mid = (a + e) >> 1;
            if (s_slice[mid] < key) a = mid + 1; else e = mid;
          }
          if (a < len && s_slice[a] == key) {
#pragma unroll
            for (int w = 0; w < WT; w++) s_row[t * WT + w] |= anc[j * WT + w];
          }
        }
        __syncthreads();  // the slice buffer is refilled for the next node
      } else {
        if (threadIdx.x == 0) flags[0] = 1;
        for (int t = threadIdx.x; t < nq; t += blockDim.x) {
          const KeyT key = KeyT(s_key[t]);
          int64_t a = s0, e = s0 + len;
          while (a < e) {
            const int64_t mid = (a + e) >> 1;
            if (keys[mid] < key) a = mid + 1; else e = mid;
          }
          if (a < s0 + len && keys[a] == key) {
#pragma unroll
            for (int w = 0; w < WT; w++) s_row[t * WT + w] |= anc[j * WT + w];
          }
        }
      }
    }
    // a query's row is ORed only by the thread that owns index t, which also writes it out here
    for (int t = threadIdx.x; t < nq; t += blockDim.x) {
      uint64_t* out = rows + int64_t(pidx[q0 + t]) * words;
      for (int w = 0; w < words; w++) out[w] = s_row[t * WT + w];
    }
    __syncthreads();  // the next tile refills s_key and s_row
  }
}

template <typename KeyT, int WT>
int launch_search(ksh_kss_index* x, const uint64_t* d_kmers, int64_t n, int canon, uint64_t* d_rows) {
  ksh_ctx* ctx = x->ctx;
  const size_t anc_bytes = size_t(x->n_nodes) * WT * 8;
  const int anc_lds = anc_bytes <= size_t(kAncLdsBytes) ? 1 : 0;
  hipLaunchKernelGGL((k_query_search<KeyT, WT>), dim3(unsigned((n + kSearchThreads - 1) / kSearchThreads)),
                     dim3(kSearchThreads), anc_lds ? anc_bytes : 0, ctx->stream, x->d_nodes, x->n_nodes, x->d_anc,
                     anc_lds, d_kmers, n, x->g.k, key_bits(&x->g), canon, x->words, d_rows);
  KSH_HIP(hipGetLastError());
  return KSH_OK;
}

template <typename KeyT, int WT>
int launch_join(ksh_kss_index* x, const uint64_t* d_kmers, int64_t n, int canon, uint64_t* d_rows) {
  ksh_ctx* ctx = x->ctx;
  const ksh_geom* g = &x->g;
  const int64_t nb = n_buckets(g);
  const int kbits = key_bits(g);
  const int tile = join_tile(WT);
  const int64_t chunk = std::min(n, kChunk);
  const size_t anc_bytes = size_t(x->n_nodes) * WT * 8;
  const int anc_lds = anc_bytes <= size_t(kAncLdsBytes) ? 1 : 0;
  const size_t lds = size_t(kSliceBytes) + size_t(tile) * (8 + 8 * WT) + (anc_lds ? anc_bytes : 0);

  int64_t *cnt = nullptr, *cursor = nullptr, *start = nullptr, *tstart = nullptr;
  uint64_t* pkey = nullptr;
  uint32_t* pidx = nullptr;
  const auto join_arena = [&](Carver& c) {
    cnt = c.take<int64_t>(size_t(nb));
    cursor = c.take<int64_t>(size_t(nb));
    start = c.take<int64_t>(size_t(nb + 1));
    tstart = c.take<int64_t>(size_t(nb + 1));
    pkey = c.take<uint64_t>(size_t(chunk));
    pidx = c.take<uint32_t>(size_t(chunk));
  };
  // Behind the arrays: the sums of the scans over nb.  The request stays the hand-written one -- the unrounded arrays,
  // 4 * 256 for their alignment, nb / 32 + 64 KiB for the sums: the list's roundings (under 1536 bytes) come out of those.
  const size_t was = 4 * 256 + size_t(nb) * 8 * 2 + size_t(nb + 1) * 8 * 2 + size_t(chunk) * 12 + size_t(nb) / 32 + (1u << 16);
  KSH_TRY(arena_layout(ctx, was - layout_bytes(join_arena), join_arena));
  const size_t scan_mark = ctx->arena_used;  // the scans below carve their own sums after this point

  for (int64_t base = 0; base < n; base += chunk) {
    const int64_t m = std::min(chunk, n - base);
    const unsigned blocks = unsigned((m + 255) / 256);
    KSH_HIP(hipMemsetAsync(cnt, 0, size_t(nb) * 8, ctx->stream));
    hipLaunchKernelGGL(k_query_hist, dim3(blocks), dim3(256), 0, ctx->stream, d_kmers + base, m, g->k, kbits, canon,
                       x->words, reinterpret_cast<unsigned long long*>(cnt), d_rows + base * x->words);
    KSH_HIP(hipGetLastError());
    ctx->arena_used = scan_mark;
    KSH_TRY(scan_exclusive_i64(ctx, cnt, start, nb, start + nb));
    KSH_HIP(hipMemcpyAsync(cursor, start, size_t(nb) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    hipLaunchKernelGGL(k_query_tiles, dim3(unsigned((nb + 255) / 256)), dim3(256), 0, ctx->stream, cnt, nb, tile);
    KSH_HIP(hipGetLastError());
    ctx->arena_used = scan_mark;
    KSH_TRY(scan_exclusive_i64(ctx, cnt, tstart, nb, tstart + nb));
    hipLaunchKernelGGL(k_query_scatter, dim3(blocks), dim3(256), 0, ctx->stream, d_kmers + base, m, g->k, kbits,
                       canon, reinterpret_cast<unsigned long long*>(cursor), pkey, pidx);
    KSH_HIP(hipGetLastError());
    KSH_HIP(hipMemcpyAsync(ctx->h_pinned, tstart + nb, 8, hipMemcpyDeviceToHost, ctx->stream));
    KSH_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t n_tiles = ctx->h_pinned[0];
    if (n_tiles > 0) {
      const unsigned grid = unsigned(std::min<int64_t>(n_tiles, kJoinMaxBlocks));
      hipLaunchKernelGGL((k_query_join<KeyT, WT>), dim3(grid), dim3(kJoinThreads), lds, ctx->stream, x->d_nodes,
                         x->n_nodes, x->d_anc, anc_lds, nb, start, tstart, n_tiles, tile, pkey, pidx, x->words,
                         d_rows + base * x->words, x->d_flags);
      KSH_HIP(hipGetLastError());
    }
  }
  if (n > chunk) x->routes |= KSH_QROUTE_CHUNKED;
  return KSH_OK;
}

template <typename KeyT>
int dispatch(ksh_kss_index* x, bool join, const uint64_t* d_kmers, int64_t n, int canon, uint64_t* d_rows) {
#define KSH_Q_W(WT) \
  return join ? launch_join<KeyT, WT>(x, d_kmers, n, canon, d_rows) : launch_search<KeyT, WT>(x, d_kmers, n, canon, d_rows)
  switch (x->wt) {
    case 1: KSH_Q_W(1);
    case 2: KSH_Q_W(2);
    case 4: KSH_Q_W(4);
    case 8: KSH_Q_W(8);
    default: KSH_Q_W(16);
  }
#undef KSH_Q_W
}

// auto: the join streams every touched slice once; the search costs each query about one 64-byte
// sector per node (the upper levels of its searches hit the cache).  Join once the search's sectors
// would outweigh one pass over the resident keys, and the batch fills the buckets: a join tile walks
// every node with two barriers whatever it holds, so at one query per tile the search is cheaper.
// Keys that fit the Infinity Cache serve the search's sectors from the cache: search.
bool index_auto_joins(const ksh_kss_index* idx, int64_t n) {
  const double key_bytes = double(idx->total_keys) * idx->g.key_bytes;
  return key_bytes > double(kCacheBytes) && double(n) * idx->n_nodes * 64.0 >= key_bytes &&
         n >= 2 * n_buckets(&idx->g);  // below two queries per bucket most tiles hold one query
}

IndexShape index_shape(const ksh_kss_index* idx) {
  return IndexShape{idx->ctx, idx->g,        idx->n_nodes, idx->words,     idx->wt,
                    idx->d_flags, idx->d_nodes, idx->d_anc,  idx->total_keys};
}

int index_lookup(ksh_kss_index* idx, bool join, const uint64_t* d_kmers, int64_t n, int canon, uint64_t* d_rows) {
  return KSH_BY_KEY(idx->g.key_bytes, dispatch, idx, join, d_kmers, n, canon, d_rows);
}

void index_set_routes(ksh_kss_index* idx, uint32_t routes) { idx->routes = routes; }

static void free_index(ksh_kss_index* x) {
  if (!x) return;
  if (x->ctx) {
    (void)hipSetDevice(x->ctx->device);
    (void)hipStreamSynchronize(x->ctx->stream);
    pool_free(x->ctx, x->d_nodes);
    pool_free(x->ctx, x->d_anc);
    pool_free(x->ctx, x->d_flags);
    for (void* p : x->owned) pool_free(x->ctx, p);
  }
  delete x;
}

// Ancestor closure of the DAG given as children CSR: anc[j * wt + w] bit i = j is reachable from i.
// Refuses out-of-range ids, self edges and cycles (Kahn's order must take every node).
static int close_dag(int32_t n, const int64_t* child_offsets, const int32_t* child_ids, int wt,
                     std::vector<uint64_t>* anc) {
  if (child_offsets[0] != 0) return fail(KSH_INVALID_ARGUMENT, "child_offsets[0] = %lld, not 0", (long long)child_offsets[0]);
  for (int32_t i = 0; i < n; i++)  // all offsets first: no edge is read before its range is known to be sound
    if (child_offsets[i + 1] < child_offsets[i])
      return fail(KSH_INVALID_ARGUMENT, "child_offsets decrease at node %d", i);
  if (child_offsets[n] > 0 && !child_ids) return fail(KSH_INVALID_ARGUMENT, "child_ids is NULL");
  std::vector<int32_t> indeg(size_t(n), 0);
  for (int32_t i = 0; i < n; i++) {
    for (int64_t e = child_offsets[i]; e < child_offsets[i + 1]; e++) {
      const int32_t c = child_ids[e];
      if (c < 0 || c >= n) return fail(KSH_INVALID_ARGUMENT, "node %d has child %d, outside [0, %d)", i, c, n);
      if (c == i) return fail(KSH_INVALID_ARGUMENT, "node %d is its own child (self edge)", i);
      indeg[size_t(c)]++;
    }
  }
  anc->assign(size_t(n) * wt, 0);
  std::vector<int32_t> order;
  order.reserve(size_t(n));
  for (int32_t i = 0; i < n; i++)
    if (indeg[size_t(i)] == 0) order.push_back(i);
  for (size_t h = 0; h < order.size(); h++) {
    const int32_t p = order[h];
    (*anc)[size_t(p) * wt + size_t(p) / 64] |= uint64_t(1) << (p % 64);
    for (int64_t e = child_offsets[p]; e < child_offsets[p + 1]; e++) {
      const int32_t c = child_ids[e];
      for (int w = 0; w < wt; w++) (*anc)[size_t(c) * wt + w] |= (*anc)[size_t(p) * wt + w];
      if (--indeg[size_t(c)] == 0) order.push_back(c);
    }
  }
  if (int32_t(order.size()) != n) return fail(KSH_INVALID_ARGUMENT, "the children lists hold a cycle");
  return KSH_OK;
}

// Shared tail of both constructors: node table, closure, flags on the device.
static int finish_index(ksh_kss_index* x, const std::vector<ksh_set_view>& sets, const int64_t* child_offsets,
                        const int32_t* child_ids) {
  ksh_ctx* ctx = x->ctx;
  std::vector<uint64_t> anc;
  KSH_TRY(close_dag(x->n_nodes, child_offsets, child_ids, x->wt, &anc));
  std::vector<NodeRef> refs(sets.size());
  const int64_t nb = n_buckets(&x->g);
  for (size_t i = 0; i < sets.size(); i++) {
    refs[i] = NodeRef{sets[i].d_offsets, sets[i].d_keys, sets[i].n_keys};
    x->total_keys += sets[i].n_keys;
    x->resident_bytes += sets[i].n_keys * x->g.key_bytes + (nb + 1) * 8;
  }
  KSH_TRY(pool_alloc(ctx, refs.size() * sizeof(NodeRef), reinterpret_cast<void**>(&x->d_nodes)));
  KSH_TRY(pool_alloc(ctx, anc.size() * 8, reinterpret_cast<void**>(&x->d_anc)));
  KSH_TRY(pool_alloc(ctx, 16, reinterpret_cast<void**>(&x->d_flags)));
  KSH_HIP(hipMemcpyAsync(x->d_nodes, refs.data(), refs.size() * sizeof(NodeRef), hipMemcpyHostToDevice, ctx->stream));
  KSH_HIP(hipMemcpyAsync(x->d_anc, anc.data(), anc.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  KSH_HIP(hipMemsetAsync(x->d_flags, 0, 16, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));  // the host vectors go out of scope
  return KSH_OK;
}

static int check_nodes(int32_t n_nodes) {
  if (n_nodes < 1) return fail(KSH_INVALID_ARGUMENT, "an index needs at least one node (n_nodes = %d)", n_nodes);
  if (n_nodes > 64 * kMaxWords)
    return fail(KSH_INVALID_ARGUMENT, "%d nodes: rows wider than %d words (%d nodes) are not supported", n_nodes,
                kMaxWords, 64 * kMaxWords);
  return KSH_OK;
}

}  // namespace ksh

using namespace ksh;

extern "C" {

int ksh_kss_index_from_kss(const ksh_kss* k, ksh_kss_index** out) {
  if (!k || !out) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  ksh_ctx* ctx = nullptr;
  ksh_geom g{};
  KSH_TRY(kss_context(k, &ctx, &g));
  int32_t n = 0;
  KSH_TRY(ksh_kss_size(k, &n));
  KSH_TRY(check_nodes(n));
  std::vector<ksh_set_view> sets(static_cast<size_t>(n));
  std::vector<int64_t> offsets(size_t(n) + 1, 0);
  std::vector<int32_t> ids;
  for (int32_t i = 0; i < n; i++) {
    int rc = ksh_kss_node(k, i, nullptr, &sets[size_t(i)], nullptr);
    if (rc != KSH_OK) return rc;  // (an owner-sharded node on another rank: KSH_FAILED_PRECONDITION)
    const int32_t* ch = nullptr;
    int32_t n_ch = 0;
    KSH_TRY(ksh_kss_children(k, i, &ch, &n_ch));
    ids.insert(ids.end(), ch, ch + n_ch);
    offsets[size_t(i) + 1] = int64_t(ids.size());
  }
  KSH_HIP(hipSetDevice(ctx->device));
  auto* x = new ksh_kss_index;
  x->ctx = ctx;
  x->g = g;
  x->n_nodes = n;
  x->words = (n + 63) / 64;
  x->wt = padded_words(x->words);
  const int rc = finish_index(x, sets, offsets.data(), ids.empty() ? nullptr : ids.data());
  if (rc != KSH_OK) {
    free_index(x);
    return rc;
  }
  *out = x;
  return KSH_OK;
}

int ksh_kss_index_create(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* nodes, int32_t n_nodes,
                         const int64_t* child_offsets, const int32_t* child_ids, int canonical, ksh_kss_index** out) {
  if (!ctx || !g || !nodes || !child_offsets || !out) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  *out = nullptr;
  KSH_TRY(check_geom(g));
  KSH_TRY(check_nodes(n_nodes));
  for (int32_t i = 0; i < n_nodes; i++) {
    const ksh_spss_view& v = nodes[i];
    if (v.n_strings < 0 || v.n_bases < 0 || (v.n_strings > 0 && (!v.d_words || !v.d_lens)))
      return fail(KSH_INVALID_ARGUMENT, "node %d: malformed container view", i);
  }
  {  // the DAG first: a bad one is refused before any device work
    std::vector<uint64_t> anc;
    const int wt = padded_words((n_nodes + 63) / 64);
    KSH_TRY(close_dag(n_nodes, child_offsets, child_ids, wt, &anc));
  }
  KSH_HIP(hipSetDevice(ctx->device));
  // (the decodes below run on ctx: the caller's pending decode plan ends here)
  const BorrowedPlans borrowed(ctx, kGroupDecode);
  auto* x = new ksh_kss_index;
  x->ctx = ctx;
  x->g = *g;
  x->n_nodes = n_nodes;
  x->words = (n_nodes + 63) / 64;
  x->wt = padded_words(x->words);
  const int64_t nb = n_buckets(g);
  std::vector<ksh_set_view> sets(static_cast<size_t>(n_nodes));
  int rc = KSH_OK;
  for (int32_t i = 0; i < n_nodes && rc == KSH_OK; i++) {
    int64_t* d_off = nullptr;
    void* d_keys = nullptr;
    int64_t nk = 0;
    rc = pool_alloc(ctx, size_t(nb + 1) * 8, reinterpret_cast<void**>(&d_off));
    if (rc != KSH_OK) break;
    x->owned.push_back(d_off);
    if (nodes[i].n_strings == 0) {
      rc = hipMemsetAsync(d_off, 0, size_t(nb + 1) * 8, ctx->stream) == hipSuccess
               ? KSH_OK : fail(KSH_INTERNAL, "hipMemsetAsync failed");
      if (rc == KSH_OK) rc = pool_alloc(ctx, 16, &d_keys);
      if (rc == KSH_OK) x->owned.push_back(d_keys);
    } else {
      rc = ksh_spss_decode_plan(ctx, g, &nodes[i], canonical, d_off, &nk);
      if (rc == KSH_OK) rc = pool_alloc(ctx, std::max<size_t>((size_t(nk) * g->key_bytes + 15) & ~size_t(15), 16), &d_keys);
      if (rc == KSH_OK) x->owned.push_back(d_keys);
      if (rc == KSH_OK) rc = ksh_spss_decode_write(ctx, g, &nodes[i], canonical, d_off, d_keys, &nk);
    }
    sets[size_t(i)] = ksh_set_view{d_off, d_keys, nk};
  }
  if (rc == KSH_OK) rc = finish_index(x, sets, child_offsets, child_ids);
  if (rc != KSH_OK) {
    free_index(x);
    return rc;
  }
  *out = x;
  return KSH_OK;
}

int ksh_kss_index_query(ksh_kss_index* idx, const uint64_t* d_kmers, int64_t n, int canonicalize, int route,
                        uint64_t* d_rows) {
  if (!idx) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  if (n < 0) return fail(KSH_INVALID_ARGUMENT, "n = %lld is negative", (long long)n);
  if (n > 0 && (!d_kmers || !d_rows)) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  if (route < 0 || route > 2) return fail(KSH_INVALID_ARGUMENT, "route = %d (0 auto, 1 search, 2 join)", route);
  idx->routes = 0;
  if (n == 0) return KSH_OK;
  ksh_ctx* ctx = idx->ctx;
  KSH_HIP(hipSetDevice(ctx->device));
  KSH_HIP(hipMemsetAsync(idx->d_flags, 0, 16, ctx->stream));
  const bool join = route == 2 || (route == 0 && index_auto_joins(idx, n));
  idx->routes = join ? KSH_QROUTE_JOIN : KSH_QROUTE_SEARCH;
  return index_lookup(idx, join, d_kmers, n, canonicalize ? 1 : 0, d_rows);
}

int ksh_kss_index_info(const ksh_kss_index* idx, int32_t* n_nodes, int32_t* words_per_row, int64_t* resident_bytes) {
  if (!idx) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  if (n_nodes) *n_nodes = idx->n_nodes;
  if (words_per_row) *words_per_row = idx->words;
  if (resident_bytes) *resident_bytes = idx->resident_bytes;
  return KSH_OK;
}

int ksh_kss_index_routes(const ksh_kss_index* idx, uint32_t* bits) {
  if (!idx || !bits) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  ksh_ctx* ctx = idx->ctx;
  KSH_HIP(hipSetDevice(ctx->device));
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned, idx->d_flags, 16, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  const int* flags = reinterpret_cast<const int*>(ctx->h_pinned);
  *bits = idx->routes | (flags[0] ? uint32_t(KSH_QROUTE_OVERSIZE) : 0u) |
          (flags[1] ? uint32_t(KSH_QROUTE_PAIR_SPLIT) : 0u) | (flags[2] ? uint32_t(KSH_QROUTE_PAIR_FLUSH) : 0u) |
          (flags[3] ? uint32_t(KSH_QROUTE_CLASS_SPILL) : 0u);
  return KSH_OK;
}

int ksh_kss_index_destroy(ksh_kss_index* idx) {
  if (!idx) return fail(KSH_INVALID_ARGUMENT, "NULL argument");
  free_index(idx);
  return KSH_OK;
}

}  // extern "C"
