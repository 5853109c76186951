// Core, shared and private k-mers of chosen sets on a KmerSetSet index (ksh_kss_select_count,
// ksh_kss_select_keys).
//
// For chosen nodes cols[0 .. n), the row of a k-mer q is bit a = (q in Get(cols[a])), formed as in
// ksh_kss_pair_counts: the OR of proj[j] over the nodes j that hold q (ksh_rowtile.h).  c(q) is the popcount of the
// row, and every selection is a predicate on it: min_count <= c(q) <= max_count, (row & require) == require,
// (row & exclude) == 0.  Two passes of one kernel, k_select, over the resident node sets:
//   count: per bucket the number of selected k-mers (a bucket is walked by one workgroup, tile after tile, so a
//          running count is enough), scanned to offsets by ksh_scan.h; the spectrum (k-mers per c(q), whatever the
//          predicate says) into the workgroup's 64-bit counters in LDS, added to the device array once at the end;
//   keys : the same walk; the selected keys of a tile come out of a hash table, so they are put in ascending order
//          in LDS (bitonic, at most kTile keys) and stored, narrowed to the key width, at offsets[b] + the bucket's
//          running count.  Tiles of a bucket are ordered by the cut, so the bucket comes out ascending.  Every store
//          is inside [offsets[b], offsets[b + 1]) and [0, n_keys); a bucket whose count is not
//          offsets[b + 1] - offsets[b] is reported.
#include "ksh_selection.h"

#include <algorithm>
#include <cstddef>

using namespace ksh::pc;

namespace {

constexpr int kSpecSlots = kMaxCols + 2;  // c(q) = 0 .. 128, padded to an even count
// device results of a call: [0] selected k-mers, [1] buckets that missed their offsets, [2 ..] the spectrum
constexpr int kAccWords = 2 + kSpecSlots;

// LDS of k_select: the walk, the tile's selected keys, the spectrum counters, the number of selected keys.
constexpr size_t select_lds_bytes(int n_nodes) {
  return walk_lds_bytes(n_nodes) + size_t(kTile) * 8 + size_t(kSpecSlots) * 8 + 8;
}
static_assert(select_lds_bytes(kMaxNodes) == 50272 && select_lds_bytes(kMaxNodes) <= (64u << 10),
              "49 KiB at 1024 nodes: under the 64 KB a kernel gets without asking");

}  // namespace

namespace ksh {

// The selecting consumer of the walk, in its two passes.  acc: see kAccWords.  kKeys == false: bucket_cnt (may be
// nullptr) receives each non-empty bucket's selected count (the caller zeroes it), spectrum != 0 asks for acc[2 ..].
// kKeys == true: offsets, out, cap.
template <typename KeyT, bool kKeys>
struct SelectConsumer {
  SelParams p;
  int spectrum;
  int64_t* bucket_cnt;
  const int64_t* offsets;
  KeyT* out;
  int64_t cap;
  unsigned long long* acc;
  unsigned long long* s_red = nullptr;   // LDS: the walk's reduction words
  unsigned long long* s_sort = nullptr;  // LDS: kTile keys, the selected keys of a tile
  unsigned long long* s_spec = nullptr;  // LDS: kSpecSlots counters
  int* s_n = nullptr;                    // LDS: keys in s_sort
  int64_t grand = 0;  // (thread 0) selected k-mers of this workgroup's buckets; buckets that missed their offsets
  int64_t my_sel = 0;               // count: what this thread selected in the bucket
  int64_t o0 = 0, o1 = 0, run = 0;  // keys: the bucket's range and the keys stored so far

  __device__ __forceinline__ void bind(const TileWalk& w, OwnLds* own) {
    s_red = w.s_red;
    s_sort = pc_own<unsigned long long>(own, kTile);
    s_spec = pc_own<unsigned long long>(own, kSpecSlots);
    s_n = pc_own<int>(own, 2);
  }
  __device__ __forceinline__ void bucket_next(int64_t) {}
  __device__ __forceinline__ Bucket bucket_begun(int64_t b, int64_t left) {
    if (left == 0 && !kKeys) return Bucket::kSkip;  // (its count stays zero)
    my_sel = run = 0;
    if (kKeys) {
      o0 = offsets[b];
      o1 = offsets[b + 1];
    }
    return Bucket::kWalk;
  }
  __device__ __forceinline__ bool settle(int*) { return false; }
  // a lane judges its slot
  __device__ __forceinline__ void slot(const Slot& s) {
    const int lane = threadIdx.x & 63;
    bool sel = false;
    int m = 0;
    if (s.occ) sel = sel_judge(p, s.r0, s.r1, &m);
    if (!kKeys) {
      my_sel += sel ? 1 : 0;
      if (spectrum) {  // one LDS add per wave and distinct multiplicity
        unsigned long long todo = __ballot(s.occ);
        while (todo) {
          const int leader = __ffsll(todo) - 1;
          const int mm = __shfl(m, leader, 64);
          const unsigned long long same = __ballot(s.occ && m == mm);
          if (lane == leader) atomicAdd(&s_spec[mm], static_cast<unsigned long long>(__popcll(same)));
          todo &= ~same;
        }
      }
    } else {
      const unsigned long long chosen = __ballot(sel);
      if (chosen) {
        const int leader = __ffsll(chosen) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(s_n, __popcll(chosen));
        base = __shfl(base, leader, 64);
        const int at = base + __popcll(chosen & ((1ull << lane) - 1));
        if (sel && at < kTile) s_sort[at] = s.key;  // (a tile has at most kTile distinct keys)
      }
    }
  }
  // keys: the tile's selected keys in ascending order (bitonic, barriers of its own) to their place in the bucket
  __device__ __forceinline__ void tile_done(int) {
    if (!kKeys) return;
    const int tid = threadIdx.x;
    const int n_sel = min(*s_n, kTile);
    if (n_sel > 1) {
      int width = 2;
      while (width < n_sel) width <<= 1;
      for (int t = n_sel + tid; t < width; t += kThreads) s_sort[t] = kEmpty;  // (above every key)
      __syncthreads();
      for (int k = 2; k <= width; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = tid; t < (width >> 1); t += kThreads) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const unsigned long long x = s_sort[i], y = s_sort[l];
            if ((x > y) == ((i & k) == 0)) {
              s_sort[i] = y;
              s_sort[l] = x;
            }
          }
          __syncthreads();
        }
      }
    }
    for (int t = tid; t < n_sel; t += kThreads) {
      const int64_t at = o0 + run + t;
      if (at >= o0 && at < o1 && at >= 0 && at < cap) out[at] = static_cast<KeyT>(s_sort[t]);
    }
    run += n_sel;
    __syncthreads();            // (every thread has read *s_n and its keys)
    if (tid == 0) *s_n = 0;     // (added to again in a slot round: behind the barriers of the next cut and fill)
  }
  __device__ __forceinline__ void bucket_done(int64_t b) {
    if (!kKeys) {
      const int64_t n_bucket = pc_block_sum(my_sel, s_red);
      if (threadIdx.x == 0) {
        if (bucket_cnt) bucket_cnt[b] = n_bucket;
        grand += n_bucket;
      }
    } else if (run != o1 - o0 || (run > 0 && (o0 < 0 || o1 > cap))) {
      grand += 1;
    }
  }
  __device__ __forceinline__ void finish() {
    if (threadIdx.x == 0 && grand) atomicAdd(&acc[kKeys ? 1 : 0], static_cast<unsigned long long>(grand));
    if (!kKeys && spectrum) {
      __syncthreads();  // (a barrier of its own: in count mode the last barrier was a bucket's block sum at best)
      for (int t = threadIdx.x; t < kSpecSlots; t += kThreads)
        if (s_spec[t]) atomicAdd(&acc[2 + t], s_spec[t]);
    }
  }
};

template <typename KeyT, bool kKeys>
__global__ __launch_bounds__(kThreads) void k_select(WalkArgs a, SelectConsumer<KeyT, kKeys> c) {
  pc_walk<KeyT>(a, c);
}

template <typename KeyT>
static int launch_select(ksh_ctx* ctx, const IndexShape& x, const uint64_t* proj, bool keys, const SelParams& p,
                         int spectrum, int64_t* bucket_cnt, const int64_t* offsets, void* out, int64_t cap,
                         unsigned long long* acc) {
  const size_t lds = select_lds_bytes(x.n_nodes), lds_max = select_lds_bytes(kMaxNodes);
  if (!keys)
    return walk_launch(ctx, x, proj, k_select<KeyT, false>, lds, lds_max, 0,
                       SelectConsumer<KeyT, false>{p, spectrum, bucket_cnt, offsets, static_cast<KeyT*>(out), cap, acc});
  return walk_launch(ctx, x, proj, k_select<KeyT, true>, lds, lds_max, 0,
                     SelectConsumer<KeyT, true>{p, spectrum, bucket_cnt, offsets, static_cast<KeyT*>(out), cap, acc});
}

// What does not need the index: refused before it is dereferenced.
int check_request(const ksh_kss_selection* sel, const ksh_kss_index* idx) {
  if (!sel) return fail(KSH_INVALID_ARGUMENT, "sel is NULL");
  if (!idx) return fail(KSH_INVALID_ARGUMENT, "idx is NULL");
  constexpr size_t kMinSize = offsetof(ksh_kss_selection, n_exclude) + sizeof(int32_t);
  if (sel->struct_size < kMinSize)
    return fail(KSH_INVALID_ARGUMENT, "sel->struct_size = %zu is smaller than the struct up to n_exclude (%zu)",
                sel->struct_size, kMinSize);
  KSH_TRY(check_col_count(sel->cols, sel->n_cols, "sel->cols"));
  if (sel->min_count < 1) return fail(KSH_INVALID_ARGUMENT, "sel->min_count = %d is below 1", sel->min_count);
  if (sel->max_count < 0) return fail(KSH_INVALID_ARGUMENT, "sel->max_count = %d is negative", sel->max_count);
  if (sel->max_count != 0 && sel->max_count < sel->min_count)
    return fail(KSH_INVALID_ARGUMENT, "sel->max_count = %d is below min_count = %d", sel->max_count, sel->min_count);
  if (sel->n_require < 0) return fail(KSH_INVALID_ARGUMENT, "sel->n_require = %d is negative", sel->n_require);
  if (sel->n_exclude < 0) return fail(KSH_INVALID_ARGUMENT, "sel->n_exclude = %d is negative", sel->n_exclude);
  if (sel->n_require > 0 && !sel->require)
    return fail(KSH_INVALID_ARGUMENT, "sel->require is NULL with n_require = %d", sel->n_require);
  if (sel->n_exclude > 0 && !sel->exclude)
    return fail(KSH_INVALID_ARGUMENT, "sel->exclude is NULL with n_exclude = %d", sel->n_exclude);
  return KSH_OK;
}

// What reads the index's host fields: the columns, the two masks and the thresholds of a checked request.
int resolve_request(const ksh_kss_selection* sel, const IndexShape& x, ColList* list, int* n_cols, SelParams* p) {
  std::vector<int> col_of;
  KSH_TRY(resolve_cols(sel->cols, sel->n_cols, x, "sel->cols", list, n_cols, &col_of));
  if (sel->max_count > *n_cols)
    return fail(KSH_INVALID_ARGUMENT, "sel->max_count = %d is above n_cols = %d", sel->max_count, *n_cols);
  if (sel->min_count > *n_cols)
    return fail(KSH_INVALID_ARGUMENT, "sel->min_count = %d is above n_cols = %d", sel->min_count, *n_cols);
  *p = SelParams{{0, 0}, {0, 0}, sel->min_count, sel->max_count ? sel->max_count : *n_cols};
  for (int side = 0; side < 2; side++) {
    const int32_t* ids = side ? sel->exclude : sel->require;
    const int32_t n = side ? sel->n_exclude : sel->n_require;
    const char* name = side ? "exclude" : "require";
    uint64_t* mask = side ? p->exclude : p->require;
    for (int32_t i = 0; i < n; i++) {
      const int32_t id = ids[i];
      if (id < 0 || id >= x.n_nodes)
        return fail(KSH_INVALID_ARGUMENT, "sel->%s[%d] = %d is outside [0, %d)", name, i, id, x.n_nodes);
      const int c = col_of[size_t(id)];
      if (c < 0) return fail(KSH_INVALID_ARGUMENT, "sel->%s[%d] = %d is not in cols", name, i, id);
      if (side && ((p->require[c >> 6] >> (c & 63)) & 1))
        return fail(KSH_INVALID_ARGUMENT, "sel->exclude[%d] = %d is in both require and exclude", i, id);
      mask[c >> 6] |= uint64_t(1) << (c & 63);
    }
  }
  return KSH_OK;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_kss_select_count(const ksh_kss_selection* sel, ksh_kss_index* idx, int64_t* d_offsets,
                                    int64_t* n_keys, int64_t* spectrum) {
  KSH_TRY(check_request(sel, idx));
  if (!d_offsets && !n_keys && !spectrum)
    return fail(KSH_INVALID_ARGUMENT, "d_offsets, n_keys and spectrum are all NULL: nothing is asked for");
  const IndexShape x = index_shape(idx);
  ColList list{};
  SelParams p{};
  int n_cols = 0;
  KSH_TRY(resolve_request(sel, x, &list, &n_cols, &p));
  ksh_ctx* ctx = x.ctx;
  PoolBuf proj(ctx), acc(ctx);
  KSH_TRY(walk_prologue(idx, x, list, n_cols, &proj));
  KSH_TRY(pool_alloc(ctx, size_t(kAccWords) * 8, &acc.p));
  KSH_HIP(hipMemsetAsync(acc.p, 0, size_t(kAccWords) * 8, ctx->stream));
  const int64_t nb = n_buckets(&x.g);
  if (d_offsets) KSH_HIP(hipMemsetAsync(d_offsets, 0, size_t(nb + 1) * 8, ctx->stream));
  auto* d_acc = static_cast<unsigned long long*>(acc.p);
  KSH_TRY(KSH_BY_KEY(x.g.key_bytes, launch_select, ctx, x, static_cast<const uint64_t*>(proj.p), false, p,
                     spectrum ? 1 : 0, d_offsets, nullptr, nullptr, 0, d_acc));
  if (d_offsets) {
    KSH_TRY(arena_reserve(ctx, size_t(nb / 256 + 1024) * 16));  // (the block sums of a scan of many buckets)
    arena_reset(ctx);
    KSH_TRY(scan_exclusive_i64(ctx, d_offsets, d_offsets, nb, d_offsets + nb));
  }
  int64_t* h = nullptr;
  KSH_TRY(pinned_words(ctx, kAccWords, &h));
  KSH_HIP(hipMemcpyAsync(h, d_acc, size_t(kAccWords) * 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  if (n_keys) *n_keys = h[0];
  if (spectrum)
    for (int m = 0; m <= n_cols; m++) spectrum[m] = h[2 + m];
  return KSH_OK;
}

extern "C" int ksh_kss_select_keys(const ksh_kss_selection* sel, ksh_kss_index* idx, const int64_t* d_offsets,
                                   int64_t n_keys, void* d_keys) {
  KSH_TRY(check_request(sel, idx));
  if (!d_offsets) return fail(KSH_INVALID_ARGUMENT, "d_offsets is NULL");
  if (n_keys < 0) return fail(KSH_INVALID_ARGUMENT, "n_keys = %lld is negative", (long long)n_keys);
  if (n_keys > 0 && !d_keys) return fail(KSH_INVALID_ARGUMENT, "d_keys is NULL with n_keys = %lld", (long long)n_keys);
  const IndexShape x = index_shape(idx);
  ColList list{};
  SelParams p{};
  int n_cols = 0;
  KSH_TRY(resolve_request(sel, x, &list, &n_cols, &p));
  ksh_ctx* ctx = x.ctx;
  PoolBuf proj(ctx), acc(ctx);
  KSH_TRY(walk_prologue(idx, x, list, n_cols, &proj));
  KSH_TRY(pool_alloc(ctx, size_t(kAccWords) * 8, &acc.p));
  KSH_HIP(hipMemsetAsync(acc.p, 0, size_t(kAccWords) * 8, ctx->stream));
  auto* d_acc = static_cast<unsigned long long*>(acc.p);
  KSH_TRY(KSH_BY_KEY(x.g.key_bytes, launch_select, ctx, x, static_cast<const uint64_t*>(proj.p), true, p, 0, nullptr,
                     d_offsets, d_keys, n_keys, d_acc));
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned, d_acc, 16, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  if (ctx->h_pinned[1] != 0)
    return fail(KSH_FAILED_PRECONDITION, "ksh_kss_select_keys: %lld buckets of the selection do not hold what "
                                         "d_offsets gives them within n_keys = %lld: the offsets are those of another "
                                         "selection or index (ksh_kss_select_count of the same request makes them)",
                (long long)ctx->h_pinned[1], (long long)n_keys);
  return KSH_OK;
}
