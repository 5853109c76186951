// Colour classes of a KmerSetSet on its index (ksh_kss_color_classes): for chosen nodes
// cols[0 .. n), every distinct row of column bits (bit a = the k-mer is in Get(cols[a])) with the number of distinct
// k-mers of the structure that have exactly that row.
//
// The rows are formed as in ksh_kss_pair_counts and ksh_kss_select_*: the tile walk of ksh_rowtile.h.  The consumer:
//   wave     : a lane takes a slot of the tile's table and empties it; the occupied lanes are grouped by equal row
//              with ballots (the leader's row, ballot(row == leader's), the leader carries the popcount), so a wave
//              has one (row, count) per distinct row among its 64 slots;
//   workgroup: the leaders add their pairs to a class table in LDS (kClsSlots slots of three key words and a 64-bit
//              count).  After a tile that leaves more than kClsSpill slots occupied the workgroup adds every entry
//              to the global table and clears its own before the next tile, and at its end what is left;
//   global   : an open-addressing table of 2^m >= 2 * capacity slots in pool memory, packed by k_class_pack; the
//              host sorts the packed classes.
// Both tables take a row by the same insertion, cls_insert (ksh_clstable.h): three set-once words per slot, each
// claimed by atomicCAS from 0, no lane ever waits for another, every probe loop is bounded by the table's slot count.
#include "ksh_clstable.h"

#include <algorithm>
#include <array>

using namespace ksh::pc;

namespace {

constexpr int kClsSlots = 1024;                       // slots of a workgroup's class table
constexpr int kClsSpill = kClsSlots * 3 / 4 - kTile;  // spill above this: the next tile's <= kTile new classes
                                                      // still fit at no more than 3/4 load
constexpr int64_t kMaxCapacity = int64_t(1) << 24;
constexpr int64_t kFirstCopy = 4096;  // classes read back with the call's one synchronisation (more: a second copy)
// device words of a call, in front of the packed classes: [0] slots of the global table that are taken, [1] non-zero:
// more than `capacity` classes, or a row found no slot, [2] the classes k_class_pack packed, [3] non-zero: a row
// found no slot in a workgroup's table (cannot happen: kClsSpill)
constexpr int kCtlWords = 4;

// LDS of k_color_classes: the walk, the class table (4 words per slot), occupancy and stop flag.
constexpr size_t classes_lds_bytes(int n_nodes) { return walk_lds_bytes(n_nodes) + size_t(kClsSlots) * 32 + 8; }
constexpr size_t kClassesLdsMax = classes_lds_bytes(kMaxNodes);  // what the kernel opts in to
static_assert(kClassesLdsMax == 77904 && 2 * kClassesLdsMax <= (160u << 10),
              "76 KiB at 1024 nodes (over 64 KiB from 406 nodes on): two workgroups per CU at any node count");

}  // namespace

namespace ksh {

// Every entry of the workgroup's table into the global one; the table is left empty.  Called behind a tile's
// closing barrier (the table is complete); a barrier follows before the table is inserted into again.  Once the call has failed (ctl[1]) nothing more is inserted.
__device__ __forceinline__ void cls_spill(unsigned long long* c_tab, unsigned long long* __restrict__ g_tab,
                                          uint32_t g_mask, int64_t capacity, unsigned long long* __restrict__ ctl) {
  for (int s = threadIdx.x; s < kClsSlots; s += kThreads) {
    const unsigned long long w0 = c_tab[s];
    if (w0 == 0) continue;
    const unsigned long long w1 = c_tab[kClsSlots + s], w2 = c_tab[2 * kClsSlots + s];
    const unsigned long long cnt = c_tab[3 * kClsSlots + s];
    c_tab[s] = 0;
    c_tab[kClsSlots + s] = 0;
    c_tab[2 * kClsSlots + s] = 0;
    c_tab[3 * kClsSlots + s] = 0;
    if (cls_peek(&ctl[1]) != 0) continue;
    const uint64_t r0 = (w0 & ~kValid) | ((w2 & 1) << 63), r1 = (w1 & ~kValid) | (((w2 >> 1) & 1) << 63);
    int claims = 0;
    if (!cls_insert<4, 1>(g_tab, g_mask, r0, r1, cnt, &claims)) atomicAdd(&ctl[1], 1ull);
    if (claims) {
      const unsigned long long taken = atomicAdd(&ctl[0], static_cast<unsigned long long>(claims)) + claims;
      if (taken > static_cast<unsigned long long>(capacity)) atomicAdd(&ctl[1], 1ull);
    }
  }
}

// The class consumer of the walk.  flags[3]: the workgroup spilled its class table before its last tile.
struct ClassConsumer {
  unsigned long long* g_tab;
  uint32_t g_mask;
  int64_t capacity;
  unsigned long long* ctl;
  unsigned long long* c_tab = nullptr;  // LDS: kClsSlots slots in four planes
  int* s_ctl = nullptr;                 // LDS: [0] slots of c_tab that are taken, [1] the call has failed
  bool pending = false;  // the class table is spilled before the next tile is counted (uniform: s_ctl[0] is read
                         // behind a tile's closing barrier)
  bool lost = false;     // (cannot happen) a row found no slot in c_tab

  __device__ __forceinline__ void bind(const TileWalk&, OwnLds* own) {
    c_tab = pc_own<unsigned long long>(own, 4 * kClsSlots);
    s_ctl = pc_own<int>(own, 2);
  }
  // (s_ctl[1] is written ahead of the barriers of the bucket's begin and read behind them; it is read only in a
  // bucket that has entries, so a tile, and with it a barrier, follows before thread 0 writes it again)
  __device__ __forceinline__ void bucket_next(int64_t) {
    if (threadIdx.x == 0) s_ctl[1] = cls_peek(&ctl[1]) != 0;
  }
  __device__ __forceinline__ Bucket bucket_begun(int64_t, int64_t left) {
    if (left == 0) return Bucket::kSkip;
    // more classes than capacity: the call fails whatever else is counted
    return s_ctl[1] ? Bucket::kStop : Bucket::kWalk;
  }
  __device__ __forceinline__ bool settle(int* flags) {
    if (!pending) return false;
    cls_spill(c_tab, g_tab, g_mask, capacity, ctl);
    if (threadIdx.x == 0) {
      flags[3] = 1;
      s_ctl[0] = 0;
    }
    pending = false;
    return true;
  }
  // one (row, count) per wave and distinct row of the round goes to c_tab
  __device__ __forceinline__ void slot(const Slot& s) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(s.occ);
    int mine = 0;  // leaders: the lanes of this round that hold my row
    while (todo) {
      const int leader = __ffsll(todo) - 1;
      const uint64_t l0 = __shfl(static_cast<unsigned long long>(s.r0), leader, 64);
      const uint64_t l1 = __shfl(static_cast<unsigned long long>(s.r1), leader, 64);
      const unsigned long long same = __ballot(s.occ && s.r0 == l0 && s.r1 == l1);
      if (lane == leader) mine = __popcll(same);
      todo &= ~same;
    }
    if (mine) {  // the leaders insert side by side: cls_insert never waits
      int claims = 0;
      if (!cls_insert<1, kClsSlots>(c_tab, kClsSlots - 1, s.r0, s.r1, static_cast<unsigned long long>(mine), &claims))
        lost = true;
      if (claims) atomicAdd(&s_ctl[0], claims);
    }
  }
  __device__ __forceinline__ void tile_done(int) { pending = s_ctl[0] > kClsSpill; }
  __device__ __forceinline__ void bucket_done(int64_t) {}
  // (the table is complete: the last barrier was a tile's closing one, or no tile was counted)
  __device__ __forceinline__ void finish() {
    cls_spill(c_tab, g_tab, g_mask, capacity, ctl);
    if (lost) atomicAdd(&ctl[3], 1ull);
  }
};

template <typename KeyT>
__global__ __launch_bounds__(kThreads) void k_color_classes(WalkArgs a, ClassConsumer c) {
  pc_walk<KeyT>(a, c);
}

// The occupied slots of the global table, packed as (r0, r1, count) in any order: out[3 c ..], c < capacity;
// ctl[2] = their number, whatever the capacity.  One atomicAdd per wave and round.
__global__ __launch_bounds__(256) void k_class_pack(const unsigned long long* __restrict__ g_tab, int64_t slots,
                                                    int64_t capacity, unsigned long long* __restrict__ ctl,
                                                    unsigned long long* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t step = int64_t(gridDim.x) * blockDim.x;
  for (int64_t base = int64_t(blockIdx.x) * blockDim.x; base < slots; base += step) {  // (uniform trip count)
    const int64_t s = base + threadIdx.x;
    unsigned long long w0 = 0;
    if (s < slots) w0 = g_tab[4 * s];
    const unsigned long long occ = __ballot(w0 != 0);
    if (occ == 0) continue;
    const int leader = __ffsll(occ) - 1;
    unsigned long long at = 0;
    if (lane == leader) at = atomicAdd(&ctl[2], static_cast<unsigned long long>(__popcll(occ)));
    at = __shfl(at, leader, 64) + __popcll(occ & ((1ull << lane) - 1));
    if (w0 != 0 && at < static_cast<unsigned long long>(capacity)) {
      const unsigned long long w1 = g_tab[4 * s + 1], w2 = g_tab[4 * s + 2];
      out[3 * at] = (w0 & ~kValid) | ((w2 & 1) << 63);
      out[3 * at + 1] = (w1 & ~kValid) | (((w2 >> 1) & 1) << 63);
      out[3 * at + 2] = g_tab[4 * s + 3];
    }
  }
}

template <typename KeyT>
static int launch_classes(ksh_ctx* ctx, const IndexShape& x, const uint64_t* proj, unsigned long long* g_tab,
                          int64_t slots, int64_t capacity, unsigned long long* ctl) {
  return walk_launch(ctx, x, proj, k_color_classes<KeyT>, classes_lds_bytes(x.n_nodes), kClassesLdsMax,
                     lds_opt_in_bit<KeyT>(kLdsClasses),
                     ClassConsumer{g_tab, uint32_t(slots - 1), capacity, ctl});
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_kss_color_classes(const int32_t* cols, int32_t n_cols, ksh_kss_index* idx, int64_t capacity,
                                     uint64_t* rows, int64_t* counts, int64_t* n_classes) {
  if (!idx) return fail(KSH_INVALID_ARGUMENT, "idx is NULL");
  if (!rows) return fail(KSH_INVALID_ARGUMENT, "rows is NULL");
  if (!counts) return fail(KSH_INVALID_ARGUMENT, "counts is NULL");
  if (!n_classes) return fail(KSH_INVALID_ARGUMENT, "n_classes is NULL");
  if (capacity < 1 || capacity > kMaxCapacity)
    return fail(KSH_INVALID_ARGUMENT, "capacity = %lld is outside [1, %lld]", (long long)capacity,
                (long long)kMaxCapacity);
  KSH_TRY(check_col_count(cols, n_cols, "cols"));
  const IndexShape x = index_shape(idx);
  ColList list{};
  KSH_TRY(resolve_cols(cols, n_cols, x, "cols", &list, &n_cols));
  ksh_ctx* ctx = x.ctx;
  PoolBuf proj(ctx), tab(ctx), res(ctx);
  KSH_TRY(walk_prologue(idx, x, list, n_cols, &proj));
  int64_t slots = 2;
  while (slots < 2 * capacity) slots <<= 1;
  KSH_TRY(pool_alloc(ctx, size_t(slots) * 32, &tab.p));
  KSH_TRY(pool_alloc(ctx, (size_t(kCtlWords) + 3 * size_t(capacity)) * 8, &res.p));
  auto* g_tab = static_cast<unsigned long long*>(tab.p);
  auto* ctl = static_cast<unsigned long long*>(res.p);
  KSH_HIP(hipMemsetAsync(g_tab, 0, size_t(slots) * 32, ctx->stream));
  KSH_HIP(hipMemsetAsync(ctl, 0, size_t(kCtlWords) * 8, ctx->stream));
  KSH_TRY(KSH_BY_KEY(x.g.key_bytes, launch_classes, ctx, x, static_cast<const uint64_t*>(proj.p), g_tab, slots,
                     capacity, ctl));
  const int64_t pack_grid = std::max<int64_t>(1, std::min<int64_t>((slots + 255) / 256, 4096));
  hipLaunchKernelGGL(k_class_pack, dim3(unsigned(pack_grid)), dim3(256), 0, ctx->stream, g_tab, slots, capacity, ctl,
                     ctl + kCtlWords);
  KSH_HIP(hipGetLastError());

  // the call's one synchronisation brings the control words and the first kFirstCopy classes
  const int64_t first = std::min(capacity, kFirstCopy);
  const size_t first_words = size_t(kCtlWords) + 3 * size_t(first);
  int64_t* h = nullptr;
  KSH_TRY(pinned_words(ctx, first_words, &h));
  KSH_HIP(hipMemcpyAsync(h, ctl, first_words * 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  if (h[3] != 0) return fail(KSH_INTERNAL, "ksh_kss_color_classes: a workgroup's class table was full");
  const int64_t n = h[2];
  if (h[1] != 0 || n > capacity) {
    *n_classes = capacity + 1;
    return fail(KSH_FAILED_PRECONDITION, "ksh_kss_color_classes: the chosen columns have more than capacity = %lld "
                                         "colour classes: call again with a larger capacity", (long long)capacity);
  }
  std::vector<std::array<uint64_t, 3>> got(static_cast<size_t>(n));
  const int64_t n_first = std::min(n, first);
  for (int64_t c = 0; c < n_first; c++)
    got[size_t(c)] = {uint64_t(h[kCtlWords + 3 * c]), uint64_t(h[kCtlWords + 3 * c + 1]),
                      uint64_t(h[kCtlWords + 3 * c + 2])};
  if (n > n_first) {  // a table of more than kFirstCopy classes: the rest, straight into the vector
    KSH_HIP(hipMemcpyAsync(got.data() + n_first, ctl + kCtlWords + 3 * n_first, size_t(n - n_first) * 24,
                           hipMemcpyDeviceToHost, ctx->stream));
    KSH_HIP(hipStreamSynchronize(ctx->stream));
  }
  // ascending by (r1, r0) as one 128-bit integer.  On the host on purpose: the table is small and the call has
  // synchronised.
  std::sort(got.begin(), got.end(), [](const std::array<uint64_t, 3>& a, const std::array<uint64_t, 3>& b) {
    return a[1] != b[1] ? a[1] < b[1] : a[0] < b[0];
  });
  for (int64_t c = 0; c < n; c++) {
    rows[2 * c] = got[size_t(c)][0];
    rows[2 * c + 1] = got[size_t(c)][1];
    counts[c] = int64_t(got[size_t(c)][2]);
  }
  *n_classes = n;
  return KSH_OK;
}
