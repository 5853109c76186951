// The bubbles of a link graph (ksh_link_bubbles): the variant sites of the coloured graph that
// ksh_spss_links returns in canonical mode, and the sets on each arm.
// The graph: n strings, 2 n oriented strings v = 2 s + o, link_offsets[2 n + 1] and link_to[n_links], rows of at most
// four distinct targets, twin-symmetric (v -> w iff w ^ 1 -> v ^ 1).  out(v) is the row of v, outdeg(v) its length,
// indeg(v) := outdeg(v ^ 1), by twin symmetry the number of links into v.
// The walk of arm i (i = 0, 1, in row order) from a source v with outdeg(v) == 2:
//   x = out(v)[i]; arm = []
//   loop:
//     if indeg(x) != 1 or outdeg(x) != 1 or len(arm) == max_arm: the arm fails
//     arm.append(x)
//     x = out(x)[0]
//     if indeg(x) == 2: sink_i = x; stop
// (a next x with indeg 1 is met again at the top of the loop; any other indeg makes the arm fail there).  v is the
// source of a bubble (v, w, arm_0, arm_1) iff both arms succeed and sink_0 == sink_1 =: w.  Nothing else is asked: w
// may branch on (back-to-back bubbles share a node), w may be v ^ 1 (a hairpin), a ring of one-in one-out strings ends
// at max_arm.  The arms cannot merge before the sink: their first strings differ (row entries are distinct) and every
// arm string has indeg 1.  Every bubble has a twin (source w ^ 1, sink v ^ 1, arms reversed and flipped); a bubble is
// reported iff v <= w ^ 1, so once, and the output ascends by v (a source has at most one bubble).  Arm 0 is the arm
// of the lower base: row order.
// With classes the carriers of an arm are the AND of rows[string_class[x >> 1]] over its strings: the sets that hold
// every k-mer of the allele.  A set that holds only part of an arm is not a carrier.
//   check : k_bub_check, a thread an oriented string.  A row is read only after its two offsets (both inside
//           off[0 .. 2 n]) have been checked against [0, n_links], each other and 4; the twin's row likewise.  Every
//           kind of offence reports its smallest vertex or link by atomicMin, as k_cut_check does.  The same pass
//           writes, for the walks, a byte deg[v] = outdeg(v) | indeg(v) << 4 and a word first[v] = out(v)[0]
//           (scratch; of use only once the check has passed).
//   count : k_bub_walk<false>: the bubble flag and len(arm_0) + len(arm_1) of every source that is reported.  A walk
//           step reads one byte and one target.  The walks run only on a graph that passed the check, so every
//           target is a vertex and every loop ends at max_arm.
//   fill  : after the repository's scan of both, k_bub_walk<true> repeats the walk of the flagged sources and writes
//           ends, arm offsets, arm strings and the ANDed rows at the scanned positions.
// The result is a function of the graph alone: every thread writes to places that the scans give it.
#include "ksh_clstable.h"
#include "ksh_seq.h"

using ksh::pc::PoolBuf;
using ksh::pc::pool_array;

namespace {

constexpr int kBubThreads = 256;
// What k_bub_check reports, a word each: the smallest offending vertex, link or string, ~0 if none.
enum { kBadOff0 = 0, kBadOffEnd, kBadOrder, kBadLong, kBadTarget, kBadRepeat, kBadTwin, kBadClass, kBadCount = 8 };

}  // namespace

namespace ksh {

// The length of the row of v if its offsets bound a row inside link_to of at most four entries, -1 otherwise.
// Reads off[v] and off[v + 1], v in [0, 2 n).
__device__ __forceinline__ int bub_row(const int64_t* __restrict__ off, int64_t v, int64_t n_links, int64_t* lo) {
  const int64_t a = off[v], b = off[v + 1];
  *lo = a;
  if (a < 0 || b > n_links || a > b || b - a > 4) return -1;
  return int(b - a);
}

__global__ __launch_bounds__(kBubThreads) void k_bub_check(const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ to, int64_t n_oriented,
                                                           int64_t n_links, const int32_t* __restrict__ cls,
                                                           int64_t n_classes, uint8_t* __restrict__ deg,
                                                           int64_t* __restrict__ first,
                                                           unsigned long long* __restrict__ bad) {
  const int64_t v = int64_t(blockIdx.x) * kBubThreads + threadIdx.x;
  if (v >= n_oriented) return;
  const auto uv = static_cast<unsigned long long>(v);
  if (v == 0) {
    if (off[0] != 0) atomicMin(&bad[kBadOff0], 0ull);
    if (off[n_oriented] != n_links) atomicMin(&bad[kBadOffEnd], 0ull);
  }
  if (cls && !(v & 1)) {
    const int32_t c = cls[v >> 1];
    if (c < 0 || int64_t(c) >= n_classes) atomicMin(&bad[kBadClass], uv >> 1);
  }
  const int64_t a = off[v], b = off[v + 1];
  if (a > b) atomicMin(&bad[kBadOrder], uv);
  if (b - a > 4 && a <= b) atomicMin(&bad[kBadLong], uv);
  int64_t lo, twin_lo;
  const int len = bub_row(off, v, n_links, &lo);
  const int in = bub_row(off, v ^ 1, n_links, &twin_lo);
  deg[v] = uint8_t((len < 0 ? 0 : len) | (in < 0 ? 0 : in) << 4);
  first[v] = len > 0 ? to[lo] : -1;
  if (len <= 0) return;
  int64_t row[4];
#pragma unroll
  for (int j = 0; j < 4; j++) row[j] = j < len ? to[lo + j] : -1;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j >= len) break;
    const int64_t w = row[j];
    const auto link = static_cast<unsigned long long>(lo + j);
    if (w < 0 || w >= n_oriented) {
      atomicMin(&bad[kBadTarget], link);
      continue;
    }
    bool repeated = false;
#pragma unroll
    for (int i = 0; i < 4; i++) repeated |= i < j && row[i] == w;
    if (repeated) atomicMin(&bad[kBadRepeat], uv);
    int64_t wlo;  // the twin w ^ 1 -> v ^ 1 (a malformed row of w ^ 1 is reported by its own thread, and first)
    const int wlen = bub_row(off, w ^ 1, n_links, &wlo);
    if (wlen < 0) continue;
    bool found = false;
    for (int i = 0; i < wlen; i++) found |= to[wlo + i] == (v ^ 1);
    if (!found) atomicMin(&bad[kBadTwin], link);
  }
}

// One arm from its first string x: its length, or -1 if it fails; *sink where it ends.  kWrite: its strings to
// out[0 ..), and the rows of their classes ANDed into r0, r1 (cls != nullptr).
template <bool kWrite>
__device__ __forceinline__ int bub_arm(const uint8_t* __restrict__ deg, const int64_t* __restrict__ first, int64_t x,
                                       int max_arm, int64_t* sink, int64_t* __restrict__ out,
                                       const int32_t* __restrict__ cls, const uint64_t* __restrict__ rows,
                                       uint64_t* r0, uint64_t* r1) {
  int len = 0;
  for (;;) {
    if (deg[x] != 0x11 || len == max_arm) return -1;
    if (kWrite) {
      out[len] = x;
      if (cls) {
        const int64_t c = cls[x >> 1];
        *r0 &= rows[2 * c];
        *r1 &= rows[2 * c + 1];
      }
    }
    len++;
    x = first[x];
    const int in = deg[x] >> 4;
    if (in == 2) {
      *sink = x;
      return len;
    }
    if (in != 1) return -1;
  }
}

// kWrite false: flag[v] = 1 and arms[v] = len(arm_0) + len(arm_1) if v is the source of a reported bubble, 0 and 0
// otherwise.  kWrite true (flag, arms: their exclusive scans, each with its total behind): the outputs of the
// flagged sources.
template <bool kWrite>
__global__ __launch_bounds__(kBubThreads) void k_bub_walk(const int64_t* __restrict__ off,
                                                          const int64_t* __restrict__ to, int64_t n_oriented,
                                                          const uint8_t* __restrict__ deg,
                                                          const int64_t* __restrict__ first, int max_arm,
                                                          int64_t* __restrict__ flag, int64_t* __restrict__ arms,
                                                          const int32_t* __restrict__ cls,
                                                          const uint64_t* __restrict__ rows,
                                                          int64_t* __restrict__ ends, int64_t* __restrict__ arm_off,
                                                          int64_t* __restrict__ arm_strings,
                                                          uint64_t* __restrict__ arm_rows) {
  const int64_t v = int64_t(blockIdx.x) * kBubThreads + threadIdx.x;
  if (v >= n_oriented) return;
  if (kWrite) {
    const int64_t b = flag[v];
    if (flag[v + 1] == b) return;
    const int64_t at = arms[v], lo = off[v];
    int64_t w = 0;
    uint64_t r[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    const int len0 = bub_arm<true>(deg, first, to[lo], max_arm, &w, arm_strings + at, cls, rows, &r[0], &r[1]);
    bub_arm<true>(deg, first, to[lo + 1], max_arm, &w, arm_strings + at + len0, cls, rows, &r[2], &r[3]);
    ends[2 * b] = v;
    ends[2 * b + 1] = w;
    arm_off[2 * b] = at;
    arm_off[2 * b + 1] = at + len0;
    if (cls) {
#pragma unroll
      for (int i = 0; i < 4; i++) arm_rows[4 * b + i] = r[i];
    }
    return;
  }
  int64_t found = 0, total = 0;
  if ((deg[v] & 15) == 2) {
    const int64_t lo = off[v];
    int64_t w0 = 0, w1 = 0;
    const int len0 = bub_arm<false>(deg, first, to[lo], max_arm, &w0, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (len0 > 0) {
      const int len1 = bub_arm<false>(deg, first, to[lo + 1], max_arm, &w1, nullptr, nullptr, nullptr, nullptr, nullptr);
      if (len1 > 0 && w0 == w1 && v <= (w0 ^ 1)) {
        found = 1;
        total = len0 + len1;
      }
    }
  }
  flag[v] = found;
  arms[v] = total;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_link_bubbles(const ksh_link_graph* graph, ksh_ctx* ctx, int32_t max_arm, int64_t capacity,
                                int64_t arm_capacity, int64_t* d_bubble_ends, int64_t* d_arm_offsets,
                                int64_t* d_arm_strings, uint64_t* d_arm_rows, int64_t* n_bubbles,
                                int64_t* n_arm_strings) {
  if (!graph) return fail(KSH_INVALID_ARGUMENT, "graph is NULL");
  if (!ctx) return fail(KSH_INVALID_ARGUMENT, "ctx is NULL");
  if (!n_bubbles) return fail(KSH_INVALID_ARGUMENT, "n_bubbles is NULL");
  if (!n_arm_strings) return fail(KSH_INVALID_ARGUMENT, "n_arm_strings is NULL");
  if (graph->struct_size < sizeof(ksh_link_graph))
    return fail(KSH_INVALID_ARGUMENT, "graph->struct_size = %zu is smaller than ksh_link_graph (%zu)",
                graph->struct_size, sizeof(ksh_link_graph));
  const int64_t n = graph->n_strings, n_links = graph->n_links;
  if (n < 0) return fail(KSH_INVALID_ARGUMENT, "graph->n_strings = %lld is negative", (long long)n);
  if (n_links < 0) return fail(KSH_INVALID_ARGUMENT, "graph->n_links = %lld is negative", (long long)n_links);
  if (n > 0 && !graph->d_link_offsets)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_offsets is NULL with n_strings = %lld", (long long)n);
  if (n_links > 0 && !graph->d_link_to)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_to is NULL with n_links = %lld", (long long)n_links);
  if (n > (INT64_MAX >> 4) || n_links > 8 * n)
    return fail(KSH_INVALID_ARGUMENT, "graph->n_links = %lld but 2 n = %lld rows of at most four links hold no more "
                                      "than %lld", (long long)n_links, (long long)(2 * n), (long long)(8 * n));
  if (max_arm < 1 || max_arm > KSH_BUBBLE_MAX_ARM)
    return fail(KSH_INVALID_ARGUMENT, "max_arm = %d is outside [1, %d]", int(max_arm), KSH_BUBBLE_MAX_ARM);
  if (capacity < 0) return fail(KSH_INVALID_ARGUMENT, "capacity = %lld is negative", (long long)capacity);
  if (arm_capacity < 0) return fail(KSH_INVALID_ARGUMENT, "arm_capacity = %lld is negative", (long long)arm_capacity);
  const bool classes = graph->d_string_class != nullptr;
  if (classes != (graph->rows != nullptr))
    return fail(KSH_INVALID_ARGUMENT, "graph->d_string_class and graph->rows: both or neither (%s is NULL)",
                classes ? "rows" : "d_string_class");
  if (classes && (graph->n_classes < 1 || graph->n_classes > kMaxClasses))
    return fail(KSH_INVALID_ARGUMENT, "graph->n_classes = %lld is outside [1, %lld]", (long long)graph->n_classes,
                (long long)kMaxClasses);
  if (!classes && d_arm_rows) return fail(KSH_INVALID_ARGUMENT, "d_arm_rows is given but the graph has no classes");
  if (capacity > 0) {
    if (!d_bubble_ends)
      return fail(KSH_INVALID_ARGUMENT, "d_bubble_ends is NULL with capacity = %lld", (long long)capacity);
    if (!d_arm_offsets)
      return fail(KSH_INVALID_ARGUMENT, "d_arm_offsets is NULL with capacity = %lld", (long long)capacity);
    if (arm_capacity > 0 && !d_arm_strings)
      return fail(KSH_INVALID_ARGUMENT, "d_arm_strings is NULL with arm_capacity = %lld", (long long)arm_capacity);
    if (classes && !d_arm_rows)
      return fail(KSH_INVALID_ARGUMENT, "d_arm_rows is NULL with classes and capacity = %lld", (long long)capacity);
  }
  if (n == 0) {
    if (capacity > 0) {  // (the one word the call writes: there before it returns, as after every other return)
      KSH_HIP(hipSetDevice(ctx->device));
      KSH_HIP(hipMemsetAsync(d_arm_offsets, 0, 8, ctx->stream));
      KSH_HIP(hipStreamSynchronize(ctx->stream));
    }
    *n_bubbles = 0;
    *n_arm_strings = 0;
    return KSH_OK;
  }
  KSH_HIP(hipSetDevice(ctx->device));

  // 1. the graph checked, the degrees and first targets beside it: into scratch only (the first synchronisation)
  const int64_t n_oriented = 2 * n;
  PoolBuf bad_buf(ctx), deg_buf(ctx), first_buf(ctx), flag_buf(ctx), arms_buf(ctx), rows_buf(ctx);
  unsigned long long* bad;
  uint8_t* deg;
  int64_t *first, *flag, *arms;
  uint64_t* rows = nullptr;
  KSH_TRY(pool_array(ctx, 8, &bad_buf, &bad));
  KSH_TRY(pool_array(ctx, size_t(n_oriented), &deg_buf, &deg));
  KSH_TRY(pool_array(ctx, size_t(n_oriented), &first_buf, &first));
  KSH_TRY(pool_array(ctx, size_t(n_oriented + 1), &flag_buf, &flag));
  KSH_TRY(pool_array(ctx, size_t(n_oriented + 1), &arms_buf, &arms));
  if (classes) KSH_TRY(pool_array(ctx, size_t(graph->n_classes) * 2, &rows_buf, &rows));  // (two words a row)
  const int64_t* off = graph->d_link_offsets;
  const int64_t* to = graph->d_link_to;
  const dim3 grid(unsigned((n_oriented + kBubThreads - 1) / kBubThreads));
  KSH_HIP(hipMemsetAsync(bad, 0xFF, kBadCount * 8, ctx->stream));
  if (classes)
    KSH_HIP(hipMemcpyAsync(rows, graph->rows, size_t(graph->n_classes) * 16, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_bub_check, grid, dim3(kBubThreads), 0, ctx->stream, off, to, n_oriented, n_links,
                     graph->d_string_class, graph->n_classes, deg, first, bad);
  KSH_HIP(hipGetLastError());
  int64_t* h = ctx->h_pinned + 8;
  KSH_HIP(hipMemcpyAsync(h, bad, kBadCount * 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  if (h[kBadOff0] != -1) return fail(KSH_INVALID_ARGUMENT, "graph->d_link_offsets[0] is not 0");
  if (h[kBadOffEnd] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_offsets[2 n] is not n_links = %lld", (long long)n_links);
  if (h[kBadOrder] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_offsets descends behind vertex %lld", (long long)h[kBadOrder]);
  if (h[kBadLong] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_offsets: the row of vertex %lld has more than four links",
                (long long)h[kBadLong]);
  if (h[kBadTarget] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_to: the target of link %lld is outside [0, 2 n = %lld)",
                (long long)h[kBadTarget], (long long)n_oriented);
  if (h[kBadRepeat] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_to: the row of vertex %lld repeats a target",
                (long long)h[kBadRepeat]);
  if (h[kBadTwin] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_link_to: link %lld (v -> w) has no twin w ^ 1 -> v ^ 1: the call "
                                      "takes the links of canonical mode", (long long)h[kBadTwin]);
  if (h[kBadClass] != -1)
    return fail(KSH_INVALID_ARGUMENT, "graph->d_string_class: the class of string %lld is outside [0, n_classes = "
                                      "%lld)", (long long)h[kBadClass], (long long)graph->n_classes);

  // 2. every source walked and counted, both counts scanned (the second synchronisation)
  hipLaunchKernelGGL(k_bub_walk<false>, grid, dim3(kBubThreads), 0, ctx->stream, off, to, n_oriented, deg, first,
                     int(max_arm), flag, arms, static_cast<const int32_t*>(nullptr),
                     static_cast<const uint64_t*>(nullptr), static_cast<int64_t*>(nullptr),
                     static_cast<int64_t*>(nullptr), static_cast<int64_t*>(nullptr), static_cast<uint64_t*>(nullptr));
  KSH_HIP(hipGetLastError());
  KSH_TRY(arena_reserve(ctx, 2 * scan_scratch_bytes(n_oriented)));
  arena_reset(ctx);
  KSH_TRY(scan_exclusive_i64(ctx, flag, flag, n_oriented, flag + n_oriented));
  KSH_TRY(scan_exclusive_i64(ctx, arms, arms, n_oriented, arms + n_oriented));
  KSH_HIP(hipMemcpyAsync(h, flag + n_oriented, 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipMemcpyAsync(h + 1, arms + n_oriented, 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  const int64_t bubbles = h[0], arm_total = h[1];
  *n_bubbles = bubbles;
  *n_arm_strings = arm_total;
  if (capacity == 0) return KSH_OK;
  if (bubbles > capacity)
    return fail(KSH_FAILED_PRECONDITION, "ksh_link_bubbles: capacity = %lld but n_bubbles = %lld: the outputs are "
                                         "untouched (capacity = 0 counts first)", (long long)capacity,
                (long long)bubbles);
  if (arm_total > arm_capacity)
    return fail(KSH_FAILED_PRECONDITION, "ksh_link_bubbles: arm_capacity = %lld but n_arm_strings = %lld: the outputs "
                                         "are untouched (capacity = 0 counts first)", (long long)arm_capacity,
                (long long)arm_total);

  // 3. the flagged sources walked again, into the outputs (the third synchronisation)
  if (bubbles > 0) {
    hipLaunchKernelGGL(k_bub_walk<true>, grid, dim3(kBubThreads), 0, ctx->stream, off, to, n_oriented, deg, first,
                       int(max_arm), flag, arms, graph->d_string_class, static_cast<const uint64_t*>(rows),
                       d_bubble_ends, d_arm_offsets, d_arm_strings, d_arm_rows);
    KSH_HIP(hipGetLastError());
  }
  KSH_HIP(hipMemcpyAsync(d_arm_offsets + 2 * bubbles, arms + n_oriented, 8, hipMemcpyDeviceToDevice, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch goes back to the pool: nothing of the call is in flight)
  return KSH_OK;
}
