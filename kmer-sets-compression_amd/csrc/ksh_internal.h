// Internal declarations shared by the HIP translation units behind
// include/kmersets_hip.h.  gfx950 only.
#ifndef KSH_INTERNAL_H_
#define KSH_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "kmersets_hip.h"
#include "ksh_layout.h"

namespace ksh {

void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define KSH_HIP(expr)                                                                   \
  do {                                                                                  \
    hipError_t err__ = (expr);                                                          \
    if (err__ != hipSuccess)                                                            \
      return ::ksh::fail(KSH_INTERNAL, "%s failed: %s (%s:%d)", #expr,                  \
                         hipGetErrorString(err__), __FILE__, __LINE__);                 \
  } while (0)

// Device key types: the reference's KeyType (lib/core/kmer_set.h:20-31) -- uint16_t for (15, 14), uint32_t for
// (19, 10) and (23, 14), uint64_t for (31, 14) -- chosen by ksh_geom::key_bytes at run time.
#define KSH_BY_KEY(key_bytes, FN, ...)                                   \
  ((key_bytes) == 2 ? FN<uint16_t>(__VA_ARGS__)                          \
                    : (key_bytes) == 4 ? FN<uint32_t>(__VA_ARGS__) : FN<uint64_t>(__VA_ARGS__))

#define KSH_TRY(expr)              \
  do {                             \
    int rc__ = (expr);             \
    if (rc__ != KSH_OK) return rc__; \
  } while (0)

constexpr int kNumTimers = 8;

// The bits of ksh_ctx::lds_opt_in.  A kernel family takes three from its first, one per key width (u16, u32, u64):
// the encode's staged neighbour probe (ksh_encode.hip), k_bucket_sort (ksh_decode.hip), k_pair_gram
// (ksh_paircounts.hip), k_color_classes (ksh_classes.hip).
constexpr uint32_t kLdsRcProbe = 1u << 0, kLdsBucketSort = 1u << 3, kLdsPairGram = 1u << 6, kLdsClasses = 1u << 9;
template <typename KeyT>
constexpr uint32_t lds_opt_in_bit(uint32_t family) {
  return family << (sizeof(KeyT) == 2 ? 0 : sizeof(KeyT) == 4 ? 1 : 2);
}

}  // namespace ksh

// Scratch arena: one growing device buffer, carved by bump allocation and reset
// at the start of every public call that needs scratch.  The pair plan keeps its
// own buffers (they must survive until ksh_pair_write).
struct ksh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;

  char* arena = nullptr;
  size_t arena_bytes = 0;
  size_t arena_used = 0;

  // pinned host staging for small read-backs
  int64_t* h_pinned = nullptr;  // 64 int64
  int64_t* h_batch = nullptr;   // pinned, grown on demand (ksh_pair_algebra_batch totals)
  size_t h_batch_count = 0;

  // persistent device buffers that must survive between two calls
  // (decode plan -> write, encode plan -> write)
  char* slot[3] = {nullptr, nullptr, nullptr};
  size_t slot_bytes[3] = {0, 0, 0};

  // decode plan state: what ksh_spss_decode_write / ksh_kmer_count_write compare their arguments with (dec_valid
  // is cleared when a plan starts and when a write consumes it; include/kmersets_hip.h, "Plans")
  int64_t dec_words = 0, dec_groups = 0, dec_kmers = 0, dec_max_bucket = 0;
  bool dec_valid = false;
  ksh_geom dec_geom{};
  int dec_canonical = 0;
  ksh_spss_view dec_view{};
  const void* dec_offsets = nullptr;

  // encode plan state (ksh_encode.hip)
  void* enc_state = nullptr;

  // kernels of this context's device that have been granted more than 64 KB of dynamic LDS
  // (hipFuncSetAttribute acts on the current device: once per context, not once per process): a bit per kernel
  // family and key width, ksh::lds_opt_in_bit<KeyT>(family)
  uint32_t lds_opt_in = 0;

  // text -> SPSS plan state (ksh_text.hip), FASTA -> fragments plan state (ksh_fasta.hip);
  // both use slot kSlotText, so a plan of one kind invalidates a pending plan of the other
  void* text_plan = nullptr;
  void (*text_plan_free)(void*) = nullptr;
  void* fasta_plan = nullptr;
  void (*fasta_plan_free)(void*) = nullptr;
  int text_slot_owner = 0;  // 1: the text plan's arrays are in the slot, 2: the FASTA plan's
  // the pending plan of the group: 0 none (cleared when a plan of either kind starts), 1 a text plan that ran to
  // its end, 2 a FASTA plan that did; the writes ask for theirs
  int text_ready = 0;
  bool text_written = false, text_ambiguous = false;  // (as EncPlan::written / ambiguous, ksh_encode.hip)

  // pair plan (ksh_pair_plan -> ksh_pair_write)
  char* plan = nullptr;
  size_t plan_bytes = 0;
  int64_t plan_tiles = 0;
  int plan_kind = 0;  // kPlanNone, kPlanPair, kPlanUnion: cleared when a plan starts, set when it has succeeded
  ksh_geom plan_geom{};
  ksh_set_view plan_a{}, plan_b{};

  // chained scan (ksh_scan.h): the sums published by the workgroups of the running launch,
  // tagged with the launch's epoch
  unsigned long long* scan_state = nullptr;
  uint32_t scan_epoch = 0;

  // caching allocator for the loop's per-iteration buffers (ksh::pool_alloc / pool_free):
  // freed blocks are kept and reused, because hipMalloc / hipFree of 100 MB-scale blocks
  // cost milliseconds and hipFree synchronises the device.  Single stream, so reuse after
  // free is ordered.
  std::mutex pool_mu;  // (lane jobs allocate their results from their parent's pool: run_on_lanes)
  std::multimap<size_t, void*> pool_free_blocks;
  std::unordered_map<void*, size_t> pool_sizes;
  size_t pool_cached_bytes = 0;
  size_t pool_live_bytes = 0, pool_peak_bytes = 0;  // handed out and not yet given back; its maximum (ksh_ctx_mem_stats)
  // test hook (KSH_FAIL_INJECT, ksh_kss_build_owned): once inject_skip allocations of at least
  // inject_min_bytes have succeeded, every further one fails; -1: off
  long long inject_skip = -1;
  size_t inject_min_bytes = 0;
  // test hook (KSH_SCRATCH_FILL, ksh_debug_set_scratch_fill): 0..255: scratch whose contents are undefined by contract
  // is set to this byte before it is handed out (ksh::scratch_fill); -1: off.  The counters: fills
  // and bytes filled on this context since the value was last set (lane threads fill blocks of their parent's pool)
  int scratch_fill = -1;
  std::atomic<int64_t> scratch_fills{0}, scratch_fill_bytes{0};

  // Lanes: helper contexts on the same device, each with a stream, scratch slots and arena of its own, on
  // which independent jobs of one call run side by side with the context's own (ksh::run_on_lanes: the stale
  // nodes of a convergence check are independent encodes, the inputs of a build independent decodes).
  // They live as long as the context: their scratch is mapped once.
  std::vector<ksh_ctx*> lanes;
  ksh_ctx* lane_parent = nullptr;  // set in a lane: where its jobs' results are allocated
  int lanes_wanted = -1;           // ksh_ctx_set_lanes; -1: KSH_LANES or the default
  bool lanes_busy = false;

  // kernel timers: when enabled, every launch of a timed kind gets its own event
  // pair from a pool; ksh_ctx_timing_read sums them after a stream sync.
  bool timing = false;
  int timing_stride = 1;                                 // every n-th launch of a kind is timed
  int64_t timing_seen[ksh::kNumTimers] = {};    // launches of each kind since the reset
  int64_t timing_units[ksh::kNumTimers] = {};   // units (keys / k-mers) of the timed launches of each kind
  std::vector<hipEvent_t> ev_pool;                       // all events ever created
  size_t ev_next = 0;                                    // next unused event in ev_pool
  std::vector<std::pair<size_t, size_t>> ev_spans[ksh::kNumTimers];  // (start, stop) indices
};

namespace ksh {

// hipMalloc that never lets the runtime run out of memory: when the device's free memory (hipMemGetInfo) does
// not hold `bytes` plus a margin, the context's pool (and its parent's, and idle lanes' scratch) give back what
// they only cache, and if that is not enough the call FAILS here with KSH_INTERNAL.  (ROCm 7.2's own
// out-of-memory path crashes the process: hipMalloc -> KfdDriver::AllocateMemory -> GpuAgent::Trim ->
// AqlQueue::AsyncReclaimMainScratch, SIGSEGV)
int device_alloc(ksh_ctx* ctx, size_t bytes, void** out);
// The scratch fill (ksh_ctx::scratch_fill), at every point that hands out scratch with undefined contents: off, one
// branch; on, `bytes` at p set to the byte on ctx's stream and the stream drained (the block may be used on another
// stream next: a lane's results come from its parent's pool).
int scratch_fill_now(ksh_ctx* ctx, void* p, size_t bytes);
inline int scratch_fill(ksh_ctx* ctx, void* p, size_t bytes) {
  return ctx->scratch_fill < 0 ? KSH_OK : scratch_fill_now(ctx, p, bytes);
}
int arena_reserve(ksh_ctx* ctx, size_t bytes);
inline void arena_reset(ksh_ctx* ctx) { ctx->arena_used = 0; }
// Returns nullptr when the arena is too small (callers reserve first).
void* arena_alloc(ksh_ctx* ctx, size_t bytes);
// The arena's next block, laid out by `layout` (ksh_layout.h): the block is as large as the list measures.
template <typename Layout>
int arena_carve(ksh_ctx* ctx, Layout&& layout) {
  const size_t bytes = layout_bytes(layout);
  if (!layout_bind(arena_alloc(ctx, bytes), bytes, layout)) return fail(KSH_INTERNAL, "scratch arena too small");
  return KSH_OK;
}
// The usual start of a stage: the arena reserved for a layout and `extra` bytes behind it (what the stage's scans
// take: scan_scratch_bytes), emptied, and the layout bound at its start.
template <typename Layout>
int arena_layout(ksh_ctx* ctx, size_t extra, Layout&& layout) {
  KSH_TRY(arena_reserve(ctx, layout_bytes(layout) + extra));
  arena_reset(ctx);
  return arena_carve(ctx, layout);
}
int plan_reserve(ksh_ctx* ctx, size_t bytes);
enum { kSlotDecode = 0, kSlotEncode = 1, kSlotText = 2 };
// What the caller expects to find in the slot: nothing (a plan begins to use it: its contents are undefined, and the
// scratch fill poisons them), or the arrays it has written there (a plan that binds its arrays again, a lane that
// maps its scratch ahead of its jobs).  A slot that has to grow loses its contents either way.
enum SlotUse { kSlotBegin = 0, kSlotKeep = 1 };
int slot_reserve(ksh_ctx* ctx, int which, size_t bytes, SlotUse use);
// A slot reserved for what a layout measures, and the layout bound to it.
template <typename Layout>
int slot_layout(ksh_ctx* ctx, int which, SlotUse use, Layout&& layout) {
  KSH_TRY(slot_reserve(ctx, which, layout_bytes(layout), use));
  if (!layout_bind(ctx->slot[which], ctx->slot_bytes[which], layout)) return fail(KSH_INTERNAL, "scratch arena too small");
  return KSH_OK;
}
// (thread-safe; a lane's jobs allocate what outlives them from lane->lane_parent's pool)
int pool_alloc(ksh_ctx* ctx, size_t bytes, void** out);
void pool_free(ksh_ctx* ctx, void* p);
void pool_trim(ksh_ctx* ctx);

// Runs job(lane, q) for every q of `order` (most expensive first) on up to lanes_wanted helper contexts at once,
// each from a host thread of its own (the calling thread works one of them); with one lane, on the context itself.
// `prepare(lane)` reserves the scratch the largest job needs and is called for a helper lane before it is
// used (a lane that cannot get its scratch -- memory -- is left out, that is no error); `need_bytes` is what
// that reservation takes, checked against the free memory first.  The context's stream is drained before
// the jobs start and every lane's stream when they end, so callers see ordinary single-stream ordering.
// Returns the first failure (its message becomes the calling thread's last error).
int run_on_lanes(ksh_ctx* ctx, const std::vector<size_t>& order, size_t need_bytes,
                 const std::function<int(ksh_ctx*)>& prepare, const std::function<int(ksh_ctx*, size_t)>& job);
inline ksh_ctx* result_ctx(ksh_ctx* lane) { return lane->lane_parent ? lane->lane_parent : lane; }

// Scratch of an SPSS encode of n k-mers (slot + arena bytes, with the reserves' spare): what a lane reserves once, at
// its largest n (ksh_encode.hip; non-decreasing in n, so that no smaller plan on the lane maps its slot again)
size_t encode_scratch_bytes(const ksh_geom* g, int64_t n);
int encode_reserve(ksh_ctx* ctx, const ksh_geom* g, int64_t n, SlotUse use);

int check_geom(const ksh_geom* g);
int check_view(const ksh_set_view* v, const char* name);  // ksh_pair.hip
inline int64_t n_buckets(const ksh_geom* g) { return int64_t(1) << g->n_bucket_bits; }
inline int key_bits(const ksh_geom* g) { return 2 * g->k - g->n_bucket_bits; }

// Kernels of ksh_spss_cover_* (ksh_cover.hip); the plan lives beside the encode's (ksh_encode.hip), whose
// unitig-level stage it shares.  err[kCoverErr*] receives a string index that violates the precondition: the
// smallest one for the checks a string fails on its own (palindrome, same ends); for the three duplicate checks
// one of the strings that share the repeated k-mer (the smallest among those that lost the table's atomicCAS --
// which of them loses is a race).
enum { kCoverErrBases = 0, kCoverErrPalindrome, kCoverErrSameEnds, kCoverErrDupEnd, kCoverErrDupFirst,
       kCoverErrDupLast, kCoverErrCount };
void cover_launch_sizes(hipStream_t st, const uint32_t* lens, int64_t n, int k, int64_t* sizes);
void cover_launch_ends(hipStream_t st, const ksh_spss_view* in, const int64_t* in_start, const int64_t* total,
                       int k, bool directed, uint64_t* first, uint64_t* last, unsigned long long* keys,
                       uint32_t* vals, uint64_t cap, unsigned long long* err);
void cover_launch_edges(hipStream_t st, const uint64_t* first, const uint64_t* last, const uint32_t* lens, int64_t n,
                        int k, bool directed, const unsigned long long* keys, const uint32_t* vals, uint64_t cap,
                        uint32_t* u_len, uint32_t* edges, uint32_t* mate);
void cover_launch_emit(hipStream_t st, const ksh_spss_view* in, const int64_t* in_start, const uint32_t* u_len,
                       const uint32_t* u_sid, const uint32_t* u_koff, const uint8_t* u_flip, const int64_t* str_start,
                       int k, int64_t n_bases, uint8_t* bytes);

// The context and geometry a KmerSetSet was built on (ksh_kss.hip; the query index borrows both).
int kss_context(const ksh_kss* k, ksh_ctx** ctx, ksh_geom* g);

// What ksh_seq_hits (ksh_seqhits.hip) and ksh_kss_pair_counts (ksh_paircounts.hip) need of a query index (ksh_query.hip): its shape, the auto rule of
// ksh_kss_index_query for a batch of n, one look-up of n patterns on the search or the join route (rows in the
// patterns' order; it leaves the index's route bits alone), and the route bits ksh_kss_index_routes reports.
// One node's resident set, as the index's kernels read it.
struct NodeRef {
  const int64_t* off;  // int64[2^N + 1]
  const void* keys;
  int64_t n;
};
// d_flags: int[4] -- [0] the join searched an oversize slice in global memory, [1] ksh_kss_pair_counts (or
// ksh_kss_select_*, ksh_select.hip) cut a bucket by key range, [2] one of its workgroups flushed its counters before its last tile,
// [3] a workgroup of ksh_kss_color_classes (ksh_classes.hip) spilled its class table before its last tile.
struct IndexShape {
  ksh_ctx* ctx;
  ksh_geom g;
  int32_t n_nodes, words, wt;  // wt: words padded to a power of two (the look-up kernels' template width)
  int* d_flags;
  const NodeRef* d_nodes;      // n_nodes of them; what ksh_kss_pair_counts (ksh_paircounts.hip) walks
  const uint64_t* d_anc;       // n_nodes * wt words
  int64_t total_keys;          // keys of all nodes together
};
IndexShape index_shape(const ksh_kss_index* idx);
bool index_auto_joins(const ksh_kss_index* idx, int64_t n);
int index_lookup(ksh_kss_index* idx, bool join, const uint64_t* d_kmers, int64_t n, int canon, uint64_t* d_rows);
void index_set_routes(ksh_kss_index* idx, uint32_t routes);

hipEvent_t timer_event(ksh_ctx* ctx, size_t* index);
void free_plan(ksh_ctx* ctx);  // ksh_encode.hip
// The current encode / cover plan stays where it is (its memory goes when the next plan starts, as ever; stats and
// routes stay readable) but serves no write any more.
void retire_plan(ksh_ctx* ctx);  // ksh_encode.hip

// Pending plans of a context (include/kmersets_hip.h, "Plans").  A composite call that runs pair plans, decodes or
// encodes of its own on the caller's context drops the caller's pending plans of those groups when it starts, so
// that their writes are refused whatever the composite call went on to do (lanes or not, merges or none).
enum { kPlanNone = 0, kPlanPair = 1, kPlanUnion = 2 };
enum { kGroupPair = 1, kGroupDecode = 2, kGroupEncode = 4 };
inline void drop_plans(ksh_ctx* ctx, unsigned groups) {
  if (groups & kGroupPair) ctx->plan_kind = kPlanNone;
  if (groups & kGroupDecode) ctx->dec_valid = false;
  if (groups & kGroupEncode) retire_plan(ctx);
}
// (on entry AND on return: what the composite call's own last plan left behind is no plan of the caller's either)
struct BorrowedPlans {
  ksh_ctx* ctx;
  unsigned groups;
  BorrowedPlans(ksh_ctx* c, unsigned g) : ctx(c), groups(g) { drop_plans(ctx, groups); }
  ~BorrowedPlans() { drop_plans(ctx, groups); }
  BorrowedPlans(const BorrowedPlans&) = delete;
  BorrowedPlans& operator=(const BorrowedPlans&) = delete;
};
// The encode, cover, text and FASTA writes name no input.  The `_for` form states which plan the caller means:
// the sizes its buffers were allocated for and the device pointer the plan was given.  The plain form serves a
// plan only where that cannot be in doubt: once, and not when the plan replaced an unwritten plan of its own kind
// (the caller's buffers may be sized for either of the two).
struct PlanIdent {
  int64_t n_strings, n_bases;
  const void* d_input;
};
// *end_plan: the refusal ends the plan (an ambiguous one: the next plan then starts from a clean slate).
inline int claim_nameless(const char* who, const char* plan, const PlanIdent* id, bool written, bool ambiguous,
                          int64_t plan_strings, int64_t plan_bases, const void* plan_input, bool* end_plan) {
  *end_plan = !id && !written && ambiguous;
  if (!id) {
    if (written)
      return fail(KSH_FAILED_PRECONDITION, "%s without a pending %s: the current plan has been written (%s_for "
                                           "writes a plan again)", who, plan, who);
    if (ambiguous)
      return fail(KSH_FAILED_PRECONDITION, "%s: the pending %s replaced an unwritten plan of the same kind, and "
                                           "this write does not say which of the two its buffers were sized for: "
                                           "the plan ends here (plan again, or use %s_for)", who, plan, who);
    return KSH_OK;
  }
  if (id->d_input != plan_input)
    return fail(KSH_FAILED_PRECONDITION, "%s_for: the pending %s was made for another input (d_input is not the "
                                         "pointer it was given)", who, plan);
  if (id->n_strings != plan_strings || id->n_bases != plan_bases)
    return fail(KSH_FAILED_PRECONDITION, "%s_for: the buffers were sized for %lld strings and %lld bases, the "
                                         "pending %s holds %lld and %lld", who, (long long)id->n_strings,
                (long long)id->n_bases, plan, (long long)plan_strings, (long long)plan_bases);
  return KSH_OK;
}
inline bool same_geom(const ksh_geom& a, const ksh_geom& b) {
  return a.k == b.k && a.n_bucket_bits == b.n_bucket_bits && a.key_bytes == b.key_bytes;
}

struct Timer {
  ksh_ctx* ctx;
  int kind;
  size_t i0 = 0;
  bool on = false;
  // units: what the launch processes (k-mers, keys), summed over the timed launches of the kind
  Timer(ksh_ctx* c, int k, int64_t units = 0) : ctx(c), kind(k) {
    on = ctx->timing && (ctx->timing_seen[kind]++ % ctx->timing_stride) == 0;
    if (on) {
      ctx->timing_units[kind] += units;
      (void)hipEventRecord(timer_event(ctx, &i0), ctx->stream);
    }
  }
  ~Timer() {
    if (on) {
      size_t i1;
      (void)hipEventRecord(timer_event(ctx, &i1), ctx->stream);
      ctx->ev_spans[kind].emplace_back(i0, i1);
    }
  }
};

// Exclusive prefix sum of n int64 values on the context's stream; `total`
// (device, one int64, may be nullptr) receives the sum.  in may equal out.
int scan_exclusive_i64(ksh_ctx* ctx, const int64_t* d_in, int64_t* d_out, int64_t n,
                       int64_t* d_total);
// What one such scan of n values takes from the arena (its block sums, level by level, and their alignment).
inline size_t scan_scratch_bytes(int64_t n) { return (size_t(n) / 256 + 4096) * sizeof(int64_t) + (1u << 16); }

}  // namespace ksh

#endif
