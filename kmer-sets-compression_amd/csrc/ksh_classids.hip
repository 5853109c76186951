// The colour class of every selected k-mer of a KmerSetSet index (ksh_kss_select_class_ids): the
// keys of ksh_kss_select_keys with, beside each key, the position of its row in a class table as
// ksh_kss_color_classes returns it.
//
// The rows are formed as in ksh_kss_select_*: the tile walk of ksh_rowtile.h.  Two kernels:
//   table  : the caller's class table (distinct rows, ascending) is uploaded and every row c is inserted into an
//            open-addressing table of 2^m >= 2 * n_classes slots in pool memory with the word c + 1 (cls_insert of
//            ksh_clstable.h: a row that is inserted once has its count word equal to what was added);
//   walk   : k_select_class_ids.  The selected lanes of a wave are grouped by equal row with ballots; a group's
//            leader finds its row in the table (cls_find: plain loads, the table is finished) and the group takes
//            the id by a shuffle.  Key and id go to two LDS arrays at the position the wave was given; behind the
//            tile's closing barrier the keys are put in ascending order (bitonic, as SelectConsumer) and every
//            exchange of two keys exchanges their ids, so each id stays beside its key; both are stored at
//            offsets[b] + the bucket's running count under the bounds checks of ksh_kss_select_keys.
#include "ksh_clstable.h"
#include "ksh_selection.h"

#include <algorithm>

using namespace ksh::pc;

namespace {

constexpr uint32_t kClassNone = KSH_CLASS_NONE;
// device results of a call: [0] selected k-mers whose row the table does not hold, [1] buckets that missed their
// offsets, [2] rows that found no slot when the table was built (cannot happen: at most half load)
constexpr int kAccWords = 4;

// LDS of k_select_class_ids: the walk, the tile's selected keys, their class ids, the number of selected keys.
constexpr size_t classids_lds_bytes(int n_nodes) {
  return walk_lds_bytes(n_nodes) + size_t(kTile) * 8 + size_t(kTile) * 4 + 8;
}
static_assert(classids_lds_bytes(kMaxNodes) == 51280 && classids_lds_bytes(kMaxNodes) <= (64u << 10),
              "50 KiB at 1024 nodes: under the 64 KB a kernel gets without asking");

}  // namespace

namespace ksh {

// Row c of rows[0 .. n) into the table with the word c + 1.  The rows are distinct (the host has checked that they
// ascend strictly), so each is inserted once and its slot's fourth word ends as c + 1.  *acc counts the rows that
// found no slot.
__global__ __launch_bounds__(256) void k_class_table(const uint64_t* __restrict__ rows, int64_t n,
                                                     unsigned long long* __restrict__ g_tab, uint32_t g_mask,
                                                     unsigned long long* __restrict__ acc) {
  const int64_t c = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (c >= n) return;
  int claims = 0;
  if (!cls_insert<4, 1>(g_tab, g_mask, rows[2 * c], rows[2 * c + 1], static_cast<unsigned long long>(c) + 1, &claims))
    atomicAdd(acc, 1ull);
}

int class_table_check_size(const uint64_t* rows, int64_t n_classes) {
  if (!rows) return fail(KSH_INVALID_ARGUMENT, "rows is NULL");
  if (n_classes < 1 || n_classes > kMaxClasses)
    return fail(KSH_INVALID_ARGUMENT, "n_classes = %lld is outside [1, %lld]", (long long)n_classes,
                (long long)kMaxClasses);
  return KSH_OK;
}

int class_table_check_order(const uint64_t* rows, int64_t n_classes) {
  for (int64_t c = 1; c < n_classes; c++) {
    const uint64_t a0 = rows[2 * c - 2], a1 = rows[2 * c - 1], b0 = rows[2 * c], b1 = rows[2 * c + 1];
    if (!(b1 > a1 || (b1 == a1 && b0 > a0)))
      return fail(KSH_INVALID_ARGUMENT, "rows[%lld] is not above rows[%lld]: rows must be strictly ascending by "
                                        "(rows[2 c + 1], rows[2 c]), as ksh_kss_color_classes returns them",
                  (long long)c, (long long)(c - 1));
  }
  return KSH_OK;
}

int class_table_check_cols(const uint64_t* rows, int64_t n_classes, int n_cols) {
  const uint64_t beyond[2] = {n_cols >= 64 ? 0 : ~uint64_t(0) << n_cols,
                              n_cols >= 128 ? 0 : n_cols <= 64 ? ~uint64_t(0) : ~uint64_t(0) << (n_cols - 64)};
  for (int64_t c = 0; c < n_classes; c++)
    if ((rows[2 * c] & beyond[0]) | (rows[2 * c + 1] & beyond[1]))
      return fail(KSH_INVALID_ARGUMENT, "rows[%lld] has a bit at or above n_cols = %d: the table is that of other "
                                        "columns", (long long)c, n_cols);
  return KSH_OK;
}

int class_table_build(ksh_ctx* ctx, const uint64_t* rows, int64_t n_classes, PoolBuf* tab, PoolBuf* up,
                      unsigned long long* d_noslot, int64_t* slots_out) {
  int64_t slots = 2;
  while (slots < 2 * n_classes) slots <<= 1;
  KSH_TRY(pool_alloc(ctx, size_t(slots) * 32, &tab->p));
  KSH_TRY(pool_alloc(ctx, size_t(n_classes) * 16, &up->p));
  auto* g_tab = static_cast<unsigned long long*>(tab->p);
  KSH_HIP(hipMemsetAsync(g_tab, 0, size_t(slots) * 32, ctx->stream));
  KSH_HIP(hipMemcpyAsync(up->p, rows, size_t(n_classes) * 16, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_class_table, dim3(unsigned((n_classes + 255) / 256)), dim3(256), 0, ctx->stream,
                     static_cast<const uint64_t*>(up->p), n_classes, g_tab, uint32_t(slots - 1), d_noslot);
  KSH_HIP(hipGetLastError());
  *slots_out = slots;
  return KSH_OK;
}

// The consumer of the walk that writes keys and class ids: SelectConsumer<KeyT, true> with an id beside every key.
// out may be nullptr (only the ids are asked for).  acc: see kAccWords.
template <typename KeyT>
struct ClassIdConsumer {
  SelParams p;
  const int64_t* offsets;
  KeyT* out;
  uint32_t* ids;
  int64_t cap;
  const unsigned long long* g_tab;
  uint32_t g_mask;
  unsigned long long* acc;
  unsigned long long* s_sort = nullptr;  // LDS: kTile keys, the selected keys of a tile
  uint32_t* s_id = nullptr;              // LDS: kTile ids, s_id[t] the class of s_sort[t]
  int* s_n = nullptr;                    // LDS: keys in s_sort
  int64_t missed = 0;                    // (thread 0) buckets that missed their offsets
  int64_t unmatched = 0;                 // selected k-mers this thread wrote with kClassNone
  int64_t o0 = 0, o1 = 0, run = 0;       // the bucket's range and the keys stored so far

  __device__ __forceinline__ void bind(const TileWalk&, OwnLds* own) {
    s_sort = pc_own<unsigned long long>(own, kTile);
    s_id = pc_own<uint32_t>(own, kTile);
    s_n = pc_own<int>(own, 2);
  }
  __device__ __forceinline__ void bucket_next(int64_t) {}
  __device__ __forceinline__ Bucket bucket_begun(int64_t b, int64_t) {
    run = 0;
    o0 = offsets[b];
    o1 = offsets[b + 1];
    return Bucket::kWalk;
  }
  __device__ __forceinline__ bool settle(int*) { return false; }
  // a lane judges its slot; the wave's selected lanes share one table look-up per distinct row
  __device__ __forceinline__ void slot(const Slot& s) {
    const int lane = threadIdx.x & 63;
    bool sel = false;
    int m = 0;
    if (s.occ) sel = sel_judge(p, s.r0, s.r1, &m);
    const unsigned long long chosen = __ballot(sel);
    if (chosen == 0) return;  // (uniform in the wave)
    int mine = lane;          // the first selected lane that holds my row
    unsigned long long todo = chosen;
    while (todo) {
      const int leader = __ffsll(todo) - 1;
      const uint64_t l0 = __shfl(static_cast<unsigned long long>(s.r0), leader, 64);
      const uint64_t l1 = __shfl(static_cast<unsigned long long>(s.r1), leader, 64);
      const bool like = sel && s.r0 == l0 && s.r1 == l1;
      const unsigned long long same = __ballot(like);
      if (like) mine = leader;
      todo &= ~same;
    }
    uint32_t id = kClassNone;
    if (sel && mine == lane) {  // the leaders look up side by side: cls_find never waits
      const unsigned long long v = cls_find<4, 1>(g_tab, g_mask, s.r0, s.r1);
      if (v) id = uint32_t(v - 1);
    }
    id = __shfl(id, mine, 64);
    const int first = __ffsll(chosen) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(s_n, __popcll(chosen));
    base = __shfl(base, first, 64);
    const int at = base + __popcll(chosen & ((1ull << lane) - 1));
    if (sel && at < kTile) {  // (a tile has at most kTile distinct keys)
      s_sort[at] = s.key;
      s_id[at] = id;
      unmatched += id == kClassNone ? 1 : 0;
    }
  }
  // the tile's selected keys in ascending order, each with its id (bitonic, barriers of its own), to their place
  // in the bucket
  __device__ __forceinline__ void tile_done(int) {
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
              const uint32_t xi = s_id[i], yi = s_id[l];
              s_sort[i] = y;
              s_sort[l] = x;
              s_id[i] = yi;
              s_id[l] = xi;
            }
          }
          __syncthreads();
        }
      }
    }
    for (int t = tid; t < n_sel; t += kThreads) {
      const int64_t at = o0 + run + t;
      if (at >= o0 && at < o1 && at >= 0 && at < cap) {
        if (out) out[at] = static_cast<KeyT>(s_sort[t]);
        ids[at] = s_id[t];
      }
    }
    run += n_sel;
    __syncthreads();         // (every thread has read *s_n, its keys and its ids)
    if (tid == 0) *s_n = 0;  // (added to again in a slot round: behind the barriers of the next cut and fill)
  }
  __device__ __forceinline__ void bucket_done(int64_t) {
    if (run != o1 - o0 || (run > 0 && (o0 < 0 || o1 > cap))) missed += 1;
  }
  __device__ __forceinline__ void finish() {
    if (threadIdx.x == 0 && missed) atomicAdd(&acc[1], static_cast<unsigned long long>(missed));
    int64_t v = unmatched;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&acc[0], static_cast<unsigned long long>(v));
  }
};

template <typename KeyT>
__global__ __launch_bounds__(kThreads) void k_select_class_ids(WalkArgs a, ClassIdConsumer<KeyT> c) {
  pc_walk<KeyT>(a, c);
}

template <typename KeyT>
static int launch_class_ids(ksh_ctx* ctx, const IndexShape& x, const uint64_t* proj, const SelParams& p,
                            const int64_t* offsets, void* out, uint32_t* ids, int64_t cap,
                            const unsigned long long* g_tab, int64_t slots, unsigned long long* acc) {
  return walk_launch(ctx, x, proj, k_select_class_ids<KeyT>, classids_lds_bytes(x.n_nodes),
                     classids_lds_bytes(kMaxNodes), 0,
                     ClassIdConsumer<KeyT>{p, offsets, static_cast<KeyT*>(out), ids, cap, g_tab, uint32_t(slots - 1),
                                           acc});
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_kss_select_class_ids(const ksh_kss_selection* sel, ksh_kss_index* idx, const uint64_t* rows,
                                        int64_t n_classes, const int64_t* d_offsets, int64_t n_keys, void* d_keys,
                                        uint32_t* d_class_ids, int64_t* n_unmatched) {
  KSH_TRY(check_request(sel, idx));
  if (!d_offsets) return fail(KSH_INVALID_ARGUMENT, "d_offsets is NULL");
  if (n_keys < 0) return fail(KSH_INVALID_ARGUMENT, "n_keys = %lld is negative", (long long)n_keys);
  KSH_TRY(class_table_check_size(rows, n_classes));
  if (n_keys > 0 && !d_class_ids)
    return fail(KSH_INVALID_ARGUMENT, "d_class_ids is NULL with n_keys = %lld", (long long)n_keys);
  KSH_TRY(class_table_check_order(rows, n_classes));
  const IndexShape x = index_shape(idx);
  ColList list{};
  SelParams p{};
  int n_cols = 0;
  KSH_TRY(resolve_request(sel, x, &list, &n_cols, &p));
  KSH_TRY(class_table_check_cols(rows, n_classes, n_cols));
  ksh_ctx* ctx = x.ctx;
  PoolBuf proj(ctx), acc(ctx), tab(ctx), up(ctx);
  KSH_TRY(walk_prologue(idx, x, list, n_cols, &proj));
  KSH_TRY(pool_alloc(ctx, size_t(kAccWords) * 8, &acc.p));
  auto* d_acc = static_cast<unsigned long long*>(acc.p);
  KSH_HIP(hipMemsetAsync(d_acc, 0, size_t(kAccWords) * 8, ctx->stream));
  int64_t slots = 0;
  KSH_TRY(class_table_build(ctx, rows, n_classes, &tab, &up, d_acc + 2, &slots));
  auto* g_tab = static_cast<unsigned long long*>(tab.p);
  KSH_TRY(KSH_BY_KEY(x.g.key_bytes, launch_class_ids, ctx, x, static_cast<const uint64_t*>(proj.p), p, d_offsets,
                     d_keys, d_class_ids, n_keys, g_tab, slots, d_acc));
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned, d_acc, size_t(kAccWords) * 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t* h = ctx->h_pinned;
  if (h[2] != 0) return fail(KSH_INTERNAL, "ksh_kss_select_class_ids: a row found no slot in the class table");
  if (h[1] != 0)
    return fail(KSH_FAILED_PRECONDITION, "ksh_kss_select_class_ids: %lld buckets of the selection do not hold what "
                                         "d_offsets gives them within n_keys = %lld: the offsets are those of another "
                                         "selection or index (ksh_kss_select_count of the same request makes them)",
                (long long)h[1], (long long)n_keys);
  if (n_unmatched) {
    *n_unmatched = h[0];
  } else if (h[0] != 0) {
    return fail(KSH_FAILED_PRECONDITION, "ksh_kss_select_class_ids: %lld selected k-mers have a row that rows does "
                                         "not hold: the class table is that of another request or index "
                                         "(ksh_kss_color_classes of the same cols makes it; pass n_unmatched to allow "
                                         "a partial table)", (long long)h[0]);
  }
  return KSH_OK;
}
