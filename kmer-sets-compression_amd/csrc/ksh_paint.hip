// Sequences painted with colour classes (ksh_seq_class_runs): for every sequence of a 2-bit stream the
// runs of consecutive k-mer positions whose k-mers have the same class, the class being the position of the k-mer's
// row over the chosen columns in a class table as ksh_kss_color_classes returns it.
//
// The positions are numbered and cut into passes as in ksh_seq_hits (ksh_seq.h), and a pass starts like one of its
// passes: the patterns are extracted and looked up on the index's own routes, rows in scratch.  Then
//   classify : k_paint_classify, a lane a position.  A lane compares its whole W-word row with that of the lane below
//              (shuffles); the lanes where it changes, and lane 0, project their row onto the columns and find it in
//              the caller's table (cls_find: plain loads, the lanes look up side by side), every other lane takes the
//              class of the nearest such lane at or below it.  Equal rows have equal classes, so nothing is lost; a
//              wave makes as many look-ups as it has changes of row, a handful on real sequences, 64 at the worst.
//   runs     : position p starts a run if it is the first of its sequence or cls[p] != cls[p - 1] -- classes, not
//              rows: two rows that differ outside the columns project alike.  k_paint_mark writes s + 1 at the first
//              position of every sequence s that starts in the pass (into the patterns' buffer, which is free by
//              then), k_paint_count counts the flags per workgroup, a scan gives every workgroup its base, and
//              k_paint_write ranks the flags again (ballot, popcount, wave sums in LDS) and stores start, class and,
//              at a sequence's first position, the sequence's offset -- all under r < capacity.
// What a pass hands to the next lives in a PaintState on the device, in two copies that take turns: the runs so far
// and the class of the pass's last position.  A kernel reads one copy and its last thread writes the other, so no
// kernel reads a word that the same launch writes.
#include "ksh_clstable.h"
#include "ksh_seq.h"

#include <algorithm>
#include <cstring>

using namespace ksh::pc;

namespace {

constexpr uint32_t kClassNone = KSH_CLASS_NONE;
constexpr int kPaintThreads = 256;
constexpr int kTimerLookup = 6, kTimerPaint = 7;

struct PaintState {
  long long base[2];             // runs of the passes so far, copy (pass & 1) read by pass `pass`
  uint32_t carry[2];             // class of the last position of the pass before
  long long pass_runs;           // runs that start in the running pass (the scan's total)
  unsigned long long unmatched;  // positions with kClassNone
  unsigned long long noslot;     // rows that found no slot when the table was built (cannot happen)
};
static_assert(sizeof(PaintState) == 48, "read back through six words of the pinned buffer");

}  // namespace

namespace ksh {

// cls[i] of the pass's positions from their rows.  kIdentity: the columns are nodes 0 .. n_cols - 1 in order, so the
// projected row is the first two words under a mask; otherwise bit c is gathered from node s_cols[c].
template <bool kIdentity>
__global__ __launch_bounds__(kPaintThreads) void k_paint_classify(const uint64_t* __restrict__ rows, int words,
                                                                  int64_t m, ColList cols, int n_cols,
                                                                  const unsigned long long* __restrict__ g_tab,
                                                                  uint32_t g_mask, uint32_t* __restrict__ cls,
                                                                  PaintState* __restrict__ st) {
  __shared__ int32_t s_cols[kMaxCols];
  if (!kIdentity) {
    for (int c = threadIdx.x; c < n_cols; c += kPaintThreads) s_cols[c] = cols.id[c];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int64_t i = int64_t(blockIdx.x) * kPaintThreads + threadIdx.x;
  const bool valid = i < m;
  if (__ballot(valid) == 0) return;  // (uniform in the wave; positions ascend with the lane, so lane 0 is valid)
  const uint64_t* row = rows + (valid ? i : m - 1) * words;
  bool differs = false;
  for (int w = 0; w < words; w++) {
    const unsigned long long v = row[w];
    const unsigned long long below = __shfl_up(v, 1, 64);
    differs |= v != below;
  }
  const bool change = valid && (lane == 0 || differs);
  const unsigned long long changes = __ballot(change);
  uint32_t id = kClassNone;
  if (change) {
    uint64_t r0 = 0, r1 = 0;
    if (kIdentity) {
      r0 = row[0] & (n_cols >= 64 ? ~uint64_t(0) : (uint64_t(1) << n_cols) - 1);
      if (n_cols > 64) r1 = row[1] & (n_cols >= 128 ? ~uint64_t(0) : (uint64_t(1) << (n_cols - 64)) - 1);
    } else {
      for (int c = 0; c < n_cols; c++) {
        const int node = s_cols[c];
        const uint64_t bit = (row[node >> 6] >> (node & 63)) & 1;
        if (c < 64) r0 |= bit << c; else r1 |= bit << (c - 64);
      }
    }
    const unsigned long long v = cls_find<4, 1>(g_tab, g_mask, r0, r1);
    if (v) id = uint32_t(v - 1);
  }
  const unsigned long long at_or_below = changes & (~0ull >> (63 - lane));  // (bit 0 is set: never empty)
  id = __shfl(id, 63 - __clzll(at_or_below), 64);
  const unsigned long long none = __ballot(valid && id == kClassNone);
  if (lane == 0 && none) atomicAdd(&st->unmatched, static_cast<unsigned long long>(__popcll(none)));
  if (valid) cls[i] = id;
}

// mark[pstart[s] - p0] = s + 1 for every sequence s whose first position lies in the pass (mark is zero elsewhere).
// The candidates are the sequences from that of the pass's first position to that of its last: at most m + 1.
__global__ __launch_bounds__(kPaintThreads) void k_paint_mark(const int64_t* __restrict__ pstart, int64_t n_strings,
                                                              int64_t p0, int64_t m, int64_t* __restrict__ mark) {
  __shared__ int64_t s_range[2];
  if (threadIdx.x < 2) s_range[threadIdx.x] = seq_of(pstart, 0, n_strings - 1, threadIdx.x == 0 ? p0 : p0 + m - 1);
  __syncthreads();
  const int64_t s = s_range[0] + int64_t(blockIdx.x) * kPaintThreads + threadIdx.x;
  if (s > s_range[1]) return;
  const int64_t i = pstart[s] - p0;
  if (i >= 0 && i < m) mark[i] = s + 1;
}

// Does position i of the pass start a run?  (carry: the class of the position before the pass.)
__device__ __forceinline__ bool paint_flag(const uint32_t* __restrict__ cls, const int64_t* __restrict__ mark,
                                           int64_t i, uint32_t carry) {
  return mark[i] != 0 || cls[i] != (i > 0 ? cls[i - 1] : carry);
}

// The flags of a workgroup's positions counted, and a flagged thread's rank among them: *total is valid in every
// thread.  One barrier.
__device__ __forceinline__ int paint_rank(bool flag, int* total) {
  __shared__ int s_wave[kPaintThreads / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long flags = __ballot(flag);
  if (lane == 0) s_wave[wave] = __popcll(flags);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kPaintThreads / 64; w++) {
    if (w < wave) before += s_wave[w];
    all += s_wave[w];
  }
  *total = all;
  return before + __popcll(flags & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(kPaintThreads) void k_paint_count(const uint32_t* __restrict__ cls,
                                                               const int64_t* __restrict__ mark, int64_t m,
                                                               const PaintState* __restrict__ st, int turn,
                                                               int64_t* __restrict__ wg_count) {
  const int64_t i = int64_t(blockIdx.x) * kPaintThreads + threadIdx.x;
  const bool flag = i < m && paint_flag(cls, mark, i, st->carry[turn]);
  int total = 0;
  paint_rank(flag, &total);
  if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
}

// Run r = the runs of the earlier passes + those of the earlier workgroups + the rank in the workgroup.  The pass's
// last thread hands the next pass its copy of the state.
__global__ __launch_bounds__(kPaintThreads) void k_paint_write(const uint32_t* __restrict__ cls,
                                                               const int64_t* __restrict__ mark,
                                                               const int64_t* __restrict__ pstart, int64_t n_strings,
                                                               int64_t p0, int64_t m, PaintState* __restrict__ st,
                                                               int turn, const int64_t* __restrict__ wg_base,
                                                               int64_t capacity, int64_t* __restrict__ off,
                                                               uint32_t* __restrict__ run_start,
                                                               uint32_t* __restrict__ run_class) {
  const int64_t i = int64_t(blockIdx.x) * kPaintThreads + threadIdx.x;
  const bool flag = i < m && paint_flag(cls, mark, i, st->carry[turn]);
  int total = 0;
  const int rank = paint_rank(flag, &total);
  if (flag) {
    const int64_t r = st->base[turn] + wg_base[blockIdx.x] + rank;
    const int64_t first = mark[i];  // s + 1 at a sequence's first position
    if (first != 0 && off) off[first - 1] = r;
    if (r >= 0 && r < capacity) {
      const int64_t s = first != 0 ? first - 1 : seq_of(pstart, 0, n_strings - 1, p0 + i);
      run_start[r] = uint32_t(p0 + i - pstart[s]);
      run_class[r] = cls[i];
    }
  }
  if (i == m - 1) {
    st->carry[turn ^ 1] = cls[i];
    st->base[turn ^ 1] = st->base[turn] + st->pass_runs;
  }
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_seq_class_runs(const ksh_spss_view* seqs, ksh_kss_index* idx, const ksh_seq_paint* req,
                                  int64_t capacity, int64_t* d_run_offsets, uint32_t* d_run_start,
                                  uint32_t* d_run_class, int64_t* n_runs, int64_t* n_unmatched) {
  if (!seqs) return fail(KSH_INVALID_ARGUMENT, "seqs is NULL");
  if (!idx) return fail(KSH_INVALID_ARGUMENT, "idx is NULL");
  if (!req) return fail(KSH_INVALID_ARGUMENT, "req is NULL");
  if (!n_runs) return fail(KSH_INVALID_ARGUMENT, "n_runs is NULL");
  if (req->struct_size < sizeof(ksh_seq_paint))
    return fail(KSH_INVALID_ARGUMENT, "struct_size = %zu is smaller than ksh_seq_paint (%zu bytes)", req->struct_size,
                sizeof(ksh_seq_paint));
  KSH_TRY(seq_check_request(seqs, req->route, req->pass_positions));
  KSH_TRY(class_table_check_size(req->rows, req->n_classes));
  KSH_TRY(class_table_check_order(req->rows, req->n_classes));
  KSH_TRY(check_col_count(req->cols, req->n_cols, "req->cols"));
  if (capacity < 0) return fail(KSH_INVALID_ARGUMENT, "capacity = %lld is negative", (long long)capacity);
  if (capacity > 0 && !d_run_start)
    return fail(KSH_INVALID_ARGUMENT, "d_run_start is NULL with capacity = %lld", (long long)capacity);
  if (capacity > 0 && !d_run_class)
    return fail(KSH_INVALID_ARGUMENT, "d_run_class is NULL with capacity = %lld", (long long)capacity);

  const IndexShape x = index_shape(idx);
  ColList list{};
  int n_cols = 0;
  KSH_TRY(resolve_cols(req->cols, req->n_cols, x, "req->cols", &list, &n_cols));
  KSH_TRY(class_table_check_cols(req->rows, req->n_classes, n_cols));
  const int k = x.g.k;
  KSH_TRY(seq_check_k(k, ""));
  bool identity = true;
  for (int c = 0; c < n_cols; c++) identity = identity && list.id[c] == c;
  ksh_ctx* ctx = x.ctx;
  KSH_HIP(hipSetDevice(ctx->device));
  const int64_t n = seqs->n_strings;
  if (n == 0) {
    KSH_TRY(seq_check_empty(seqs, ""));
    if (d_run_offsets) {  // (the one word the call writes: there before it returns, as after every other return)
      KSH_HIP(hipMemsetAsync(d_run_offsets, 0, 8, ctx->stream));
      KSH_HIP(hipStreamSynchronize(ctx->stream));
    }
    index_set_routes(idx, 0);
    *n_runs = 0;
    if (n_unmatched) *n_unmatched = 0;
    return KSH_OK;
  }

  // 1. positions per sequence, scanned; the container's sizes are checked before anything reads its words
  PoolBuf pstart_buf(ctx), state_buf(ctx), pat_buf(ctx), rows_buf(ctx), cls_buf(ctx), wg_buf(ctx), tab(ctx), up(ctx);
  int64_t* pstart;
  KSH_TRY(pool_array(ctx, size_t(n + 1), &pstart_buf, &pstart));
  KSH_TRY(pool_alloc(ctx, 64, &state_buf.p));  // (a PaintState, and before it is one the word of seq_positions)
  auto* st = static_cast<PaintState*>(state_buf.p);
  int64_t total = 0;  // k-mer positions in all
  KSH_TRY(seq_positions(ctx, seqs, k, pstart, reinterpret_cast<unsigned long long*>(st), &total));

  // 2. the caller's table
  KSH_HIP(hipMemsetAsync(st, 0, sizeof(PaintState), ctx->stream));
  int64_t slots = 0;
  KSH_TRY(class_table_build(ctx, req->rows, req->n_classes, &tab, &up, &st->noslot, &slots));
  const auto* g_tab = static_cast<const unsigned long long*>(tab.p);

  // 3. the passes
  const int64_t pass =
      std::min(req->pass_positions > 0 ? req->pass_positions : seq_default_pass(12 + 8 * x.words), kSeqMaxPass);
  const int64_t cap = std::min(pass, total);
  const int64_t max_groups = (cap + kPaintThreads - 1) / kPaintThreads;
  uint64_t *pat, *rows;
  uint32_t* cls;
  int64_t* wg;
  KSH_TRY(pool_array(ctx, size_t(cap), &pat_buf, &pat));
  KSH_TRY(pool_array(ctx, size_t(cap) * size_t(x.words), &rows_buf, &rows));
  KSH_TRY(pool_array(ctx, size_t(cap), &cls_buf, &cls));
  KSH_TRY(pool_array(ctx, size_t(max_groups), &wg_buf, &wg));
  auto* mark = static_cast<int64_t*>(pat_buf.p);  // (the patterns are done with when the marks are written)
  KSH_HIP(hipMemsetAsync(x.d_flags, 0, 16, ctx->stream));
  uint32_t routes = total > pass ? uint32_t(KSH_QROUTE_SEQ_PASSES) : 0u;
  index_set_routes(idx, 0);
  int turn = 0;
  for (int64_t p0 = 0; p0 < total; p0 += pass, turn ^= 1) {
    const int64_t m = std::min(pass, total - p0);
    const unsigned groups = unsigned((m + kPaintThreads - 1) / kPaintThreads);
    {
      Timer timer(ctx, kTimerLookup, m);
      KSH_TRY(seq_extract(ctx, seqs, pstart, p0, m, k, req->canonicalize ? 1 : 0, pat));
      const bool join = req->route == 2 || (req->route == 0 && index_auto_joins(idx, m));
      routes |= join ? KSH_QROUTE_JOIN : KSH_QROUTE_SEARCH;
      KSH_TRY(index_lookup(idx, join, pat, m, 0, rows));  // (the patterns are canonical already, if asked)
    }
    Timer timer(ctx, kTimerPaint, m);
    if (identity)
      hipLaunchKernelGGL(k_paint_classify<true>, dim3(groups), dim3(kPaintThreads), 0, ctx->stream, rows, x.words, m,
                         list, n_cols, g_tab, uint32_t(slots - 1), cls, st);
    else
      hipLaunchKernelGGL(k_paint_classify<false>, dim3(groups), dim3(kPaintThreads), 0, ctx->stream, rows, x.words, m,
                         list, n_cols, g_tab, uint32_t(slots - 1), cls, st);
    KSH_HIP(hipGetLastError());
    KSH_HIP(hipMemsetAsync(mark, 0, size_t(m) * 8, ctx->stream));
    hipLaunchKernelGGL(k_paint_mark, dim3(unsigned((m + kPaintThreads) / kPaintThreads)), dim3(kPaintThreads), 0,
                       ctx->stream, pstart, n, p0, m, mark);
    hipLaunchKernelGGL(k_paint_count, dim3(groups), dim3(kPaintThreads), 0, ctx->stream, cls, mark, m, st, turn, wg);
    KSH_HIP(hipGetLastError());
    KSH_TRY(arena_reserve(ctx, scan_scratch_bytes(groups)));  // (the join has reset the arena: nothing of it is kept)
    arena_reset(ctx);
    KSH_TRY(scan_exclusive_i64(ctx, wg, wg, groups, reinterpret_cast<int64_t*>(&st->pass_runs)));
    hipLaunchKernelGGL(k_paint_write, dim3(groups), dim3(kPaintThreads), 0, ctx->stream, cls, mark, pstart, n, p0, m,
                       st, turn, wg, capacity, d_run_offsets, d_run_start, d_run_class);
    KSH_HIP(hipGetLastError());
  }
  index_set_routes(idx, routes);

  // 4. the totals
  if (d_run_offsets)
    KSH_HIP(hipMemcpyAsync(d_run_offsets + n, &st->base[turn], 8, hipMemcpyDeviceToDevice, ctx->stream));
  KSH_HIP(hipMemcpyAsync(ctx->h_pinned, st, sizeof(PaintState), hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  PaintState h;
  memcpy(&h, ctx->h_pinned, sizeof(PaintState));
  if (h.noslot != 0) return fail(KSH_INTERNAL, "ksh_seq_class_runs: a row found no slot in the class table");
  *n_runs = h.base[turn];
  if (n_unmatched) *n_unmatched = int64_t(h.unmatched);
  if (capacity > 0 && h.base[turn] > capacity)
    return fail(KSH_FAILED_PRECONDITION, "ksh_seq_class_runs: capacity = %lld but n_runs = %lld: d_run_start and "
                                         "d_run_class hold nothing to rely on (capacity = 0 counts the runs first)",
                (long long)capacity, (long long)h.base[turn]);
  if (!n_unmatched && h.unmatched != 0)
    return fail(KSH_FAILED_PRECONDITION, "ksh_seq_class_runs: %lld positions have a row that rows does not hold: the "
                                         "class table is that of other columns or another index "
                                         "(ksh_kss_color_classes of the same cols makes it; pass n_unmatched to allow "
                                         "a partial table)", (long long)h.unmatched);
  return KSH_OK;
}
