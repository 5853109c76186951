/*
 * kmersets_hip.h -- C ABI of the MI355X (gfx950) k-mer-set hot path.
 *
 * The reference (kkty/kmer-sets-compression) has no FFI: its hot path is a set of
 * header-only C++17 templates (the lib/core headers).  This header is the boundary the
 * build introduces underneath them: flat extern "C" functions over
 * plain device pointers and sizes, parameterised at run time by
 * (k, n_bucket_bits, key_bytes) instead of the reference's template parameters
 * <K, N, KeyType>.  The C++17 class templates in
 * kmer-sets-compression_amd/cpp/core/ (KmerSet / KmerSetCompact / KmerSetSet, same
 * names and argument meaning as the reference) are thin wrappers over these calls;
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Device layout of a k-mer set (replaces 2^N absl::flat_hash_set<KeyType>,
 * lib/core/kmer_set.h:247-251):
 *     offsets : int64[2^N + 1]   bucket b holds keys[offsets[b] .. offsets[b+1])
 *     keys    : u16, u32 or u64  low (2K - N) bits of the k-mer, ascending inside a bucket;
 *                                key_bytes = 2 when 2K-N <= 16 (the reference's (15, 14, uint16_t)),
 *                                4 when 2K-N <= 32, else 8
 * i.e. the set is one ascending array of 2K-bit k-mers with a bucket index.
 *
 * All pointers named d_* are device pointers on the context's GPU.  Functions
 * that return host scalars synchronise the context's stream before returning;
 * the others only enqueue work.  There is no CPU fallback anywhere behind this
 * header: without a usable HIP device every call fails with KSH_INTERNAL.
 *
 * Status codes mirror the three absl codes the reference uses
 * (lib/core/io.h:26,43,63; lib/core/kmer_set_set.h:465,525,610).
 */
#ifndef KMERSETS_HIP_H_
#define KMERSETS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KSH_OK 0
#define KSH_INVALID_ARGUMENT 3
#define KSH_FAILED_PRECONDITION 9
#define KSH_INTERNAL 13

typedef struct ksh_ctx ksh_ctx;

/* <K, N, KeyType> of the reference, as run-time values. */
typedef struct ksh_geom {
  int32_t k;             /* k-mer length, 2 <= k <= 31                         */
  int32_t n_bucket_bits; /* N: top N bits of the 2K-bit k-mer pick the bucket  */
  int32_t key_bytes;     /* device key width: 2, 4 or 8 (>= ceil((2k - N) / 8)) */
  int32_t reserved;
} ksh_geom;

/* One k-mer set resident in HBM.  d_keys is 16-byte aligned and its allocation runs to a
 * multiple of 16 bytes (ksh_malloc, hipMalloc and torch all round up further): the merge
 * kernels read whole 16-byte vectors, so the last vector of a key array may reach up to 12
 * bytes past its last key (never into another allocation's bytes they would use). */
typedef struct ksh_set_view {
  const int64_t* d_offsets; /* int64[2^N + 1]                */
  const void* d_keys;       /* key_bytes * n_keys bytes      */
  int64_t n_keys;
} ksh_set_view;

/* ---- library / errors --------------------------------------------------------- */
int ksh_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* ksh_last_error(void);

/* ---- device plumbing (so that host C++ needs no HIP headers) ---------------------- */
int ksh_device_count(int* count);
int ksh_malloc(int device, size_t bytes, void** d_ptr);
int ksh_free(int device, void* d_ptr);
/* The three copies wait for the whole device first (hipDeviceSynchronize): they are ordered after
 * everything enqueued on any context's stream, blocking or not, and done when they return. */
int ksh_memcpy_h2d(int device, void* d_dst, const void* src, size_t bytes);
int ksh_memcpy_d2h(int device, void* dst, const void* d_src, size_t bytes);
int ksh_memcpy_d2d(int device, void* d_dst, const void* d_src, size_t bytes);
/* The same copies ordered after ONE context's stream only (the work of other contexts goes on): for
 * a host thread with a context of its own and buffers it produced itself or received complete --
 * the per-node writer threads of KmerSetSet::Dump (lib/core/kmer_set_set.h:497-519), the rank threads
 * of a rehearsal. */
int ksh_ctx_memcpy_h2d(ksh_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int ksh_ctx_memcpy_d2h(ksh_ctx* ctx, void* dst, const void* d_src, size_t bytes);
int ksh_ctx_memcpy_d2d(ksh_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);

/* A context = one GPU + one HIP stream + a scratch arena.  `stream` may be an
 * existing hipStream_t (e.g. torch's current stream) or NULL for a new one.
 * Contexts are not thread-safe; use one per host thread (the reference calls its
 * set operations concurrently from pool threads, lib/core/kmer_set_set.h:146-149). */
int ksh_ctx_create(int device, void* stream, ksh_ctx** out);
int ksh_ctx_destroy(ksh_ctx* ctx);
int ksh_ctx_sync(ksh_ctx* ctx);
/* Pre-sizes the scratch arena (otherwise it grows on demand). */
int ksh_ctx_reserve(ksh_ctx* ctx, size_t bytes);
/* Kernel timing for bench.py's roofline leg.  enable = n > 0: every n-th launch of a
 * timed kernel kind (the 1st, the (n+1)-th, ...) is bracketed by its own pair of HIP
 * events on the context's stream; an event pair costs the stream about 10 us of idle time,
 * so a caller that also measures throughput samples (n > 1) rather than timing every
 * launch.  ksh_ctx_timing_read synchronises the stream and returns the summed duration and
 * the number of timed launches since the last reset.
 * kinds: 0 = pair merge, write pass   1 = pair merge, count pass
 *        2 = sampled-bucket weight count pass
 *        3 = SPSS encode, neighbour probe stage (partition + LDS-staged probes: the loop's dominant stage)
 *        4 = SPSS encode, chain ranking walks (k_rank_walk / k_rank_heads, or the stamping k_ruler_walk /
 *            k_ruler_heads)   5 = SPSS encode, base emit (k_emit_rulers / k_emit_heads, or k_emit)
 *        6 = ksh_seq_class_runs, extraction and look-up of a pass   7 = ..., classification and runs of a pass
 * ksh_ctx_timing_units: the k-mers (kinds 3..5) or positions (6, 7) the timed launches of a kind covered. */
int ksh_ctx_enable_timing(ksh_ctx* ctx, int enable);
int ksh_ctx_timing_reset(ksh_ctx* ctx);
int ksh_ctx_timing_read(ksh_ctx* ctx, int kind, float* total_ms, int64_t* launches);
int ksh_ctx_timing_units(ksh_ctx* ctx, int kind, int64_t* units);
/* Lanes.  Calls that hold independent jobs -- the SPSS encodes of the stale nodes at a convergence check and at
 * the end of ksh_kss_build (lib/core/kmer_set_set.h:287,345-360), the decodes of its inputs (:138-153, which the
 * reference runs on its thread pool too) -- run them on up to n_lanes HIP streams of the context's GPU at once,
 * each from a host thread of its own with scratch of its own (one job's LDS-bound probe kernels then overlap
 * another's walks, which wait on HBM, and nobody's host round trips leave the GPU idle); results are the same,
 * node ids being fixed before the jobs start.  The lanes are helper contexts that live inside the context
 * (created on first use, mapped scratch kept, freed by ksh_ctx_destroy); every job runs on one of them and
 * allocates its result from the context's own pool, which only hands out while jobs run.  Lanes whose scratch
 * does not fit the free memory are left out; with fewer than two the jobs run on the context's stream, one
 * after the other.  n_lanes = 1: everything on the context's stream, as before; 0: the default (KSH_LANES, else 4).  The lanes run on two disjoint shares of the CUs, odd and even lanes (KSH_LANE_CUS=1: every lane on all CUs).
 * With lanes, ksh_ctx_timing_read / _units sum over the lanes (stream time: spans of different lanes overlap);
 * ksh_ctx_timing_wall is the length of the UNION of a kind's timed spans over all lanes, i.e. the wall time
 * during which at least one launch of the kind was running. */
int ksh_ctx_set_lanes(ksh_ctx* ctx, int n_lanes);
/* Device memory behind a context, bytes: stats = { pooled buffers handed out and not yet given back (the sets,
 * containers and samples of a KmerSetSet live here), the maximum of that since the context was made or the peak was
 * last reset, pooled buffers cached for reuse, the context's own scratch (encode / decode / text slots, arena, pair
 * plan), everything its helper lanes hold, number of helper lanes }.  reset_peak != 0: the peak restarts at the
 * current value.  (DESIGN.md 7.2's memory table is checked against these in tests/test_gpu_full_size.py.) */
int ksh_ctx_mem_stats(ksh_ctx* ctx, int64_t stats[6], int reset_peak);
int ksh_ctx_timing_wall(ksh_ctx* ctx, int kind, float* wall_ms);

/* ---- Plans -----------------------------------------------------------------------------------
 * Eight operations take two calls: a *_plan call sizes the output and leaves a plan inside the context, the
 * caller allocates, a *_write call consumes the plan.  The plans live in four groups, one pending plan per group
 * and context:
 *     pair   : ksh_pair_plan -> ksh_pair_write             ksh_set_union_plan -> ksh_set_union_write
 *     decode : ksh_spss_decode_plan -> ksh_spss_decode_write, or -> ksh_kmer_count_write
 *     encode : ksh_spss_encode_plan -> ksh_spss_encode_write   ksh_spss_cover_plan -> ksh_spss_cover_write
 *     text   : ksh_spss_from_text_plan -> ksh_spss_from_text_write     ksh_fasta_plan -> ksh_fasta_write
 * After a successful plan, and whatever was called in between, the write has exactly two outcomes:
 *     exact   : KSH_OK, and the outputs are the true result;
 *     refused : KSH_FAILED_PRECONDITION with a message that names the write and the plan it misses.  No output
 *               buffer is touched, nothing is launched, and the context stays usable: a fresh plan + write on it
 *               gives the true result.
 * It is never KSH_OK with anything else, and never a write sized by another plan.
 * The four writes that name no input -- ksh_spss_encode_write, ksh_spss_cover_write, ksh_spss_from_text_write,
 * ksh_fasta_write -- have two forms.  The `_for` form states the plan the caller means: the sizes its buffers were
 * allocated for (n_strings, n_bases as the plan returned them) and d_input, the device pointer the plan was given
 * (set->d_offsets, unitigs->d_words, d_text); a plan of the same kind that replaced it is told apart by these, and
 * the write is refused.  (A re-plan of the SAME input that returns the same sizes -- another mode or fast flag --
 * is not told apart: it is served.)  The plain form has nothing to compare, so it serves a plan only where there
 * can be no doubt: once, and not a plan that replaced an unwritten plan of its own kind -- the buffers may be sized
 * for either of the two: that refusal ends the plan, so that the next plan + write is served; or use `_for`.
 *
 * What ends a pending plan (its write is refused afterwards), per call issued on the SAME context:
 *     a plan call of the same group, successful, abandoned or failed     that group
 *     ksh_kss_build, ksh_kss_build_sharded, ksh_kss_build_owned           pair, decode, encode (the build plans on
 *                                                                         the context for itself; which of its jobs
 *                                                                         run there depends on lanes and memory, so
 *                                                                         it ends all three when it starts)
 *     ksh_kss_get                                                         pair (its unions)
 *     ksh_kss_index_create                                                decode (its decodes)
 *     ksh_spss_encode_release, ksh_spss_cover_release                     encode
 *     ksh_spss_decode_write, ksh_kmer_count_write                         decode (the write consumes its plan)
 * Every other call leaves every pending plan exact: hash, contains, kmers, diff, ksh_pair_weights,
 * ksh_pair_algebra, ksh_pair_algebra_batch, ksh_dsu_components, both StreamVByte calls, ksh_spss_size,
 * ksh_spss_to_text, the copies, ksh_ctx_reserve (the plans keep nothing in the arena), the timing and memory
 * calls, ksh_ctx_set_lanes, ksh_kss_index_query, ksh_seq_hits, ksh_kss_pair_counts, ksh_kss_select_count,
 * ksh_kss_select_keys, ksh_kss_select_class_ids, ksh_kss_color_classes, ksh_seq_class_runs, ksh_spss_cut, ksh_spss_links, ksh_link_bubbles and the accessors of a ksh_kss /
 * ksh_kss_index, plans and writes of another group, and anything done on a different context.  Only a plan of its own group ends a text or FASTA
 * plan: nothing else uses their slot.
 *
 * A failed plan ends the older plan of its group (it has overwritten the group's scratch) and leaves none: the
 * write after it is refused.
 * Mismatched writes are refused on the host before any launch: a geometry (k, N, key bytes), canonical flag,
 * container, set or -- for the decode -- d_offsets buffer other than the planned one; ksh_pair_write on a union
 * plan and ksh_set_union_write on a pair plan; ksh_spss_encode_write on a cover plan and the reverse; n_strings,
 * n_bases or d_input of a `_for` write other than the pending plan's; a write on a context other than the one
 * that planned.  The plan stays pending for the right write.
 * Replay: a second write on one plan is exact for the pair and union plans and for the `_for` writes of the
 * encode, cover, text and FASTA plans (the write leaves the plan as it is; outputs may be skipped or repeated),
 * and refused for the decode plan (ksh_spss_decode_write and ksh_kmer_count_write consume it) and for the plain
 * encode, cover, text and FASTA writes, the same way every time.  A write after ksh_spss_encode_release /
 * ksh_spss_cover_release is refused.
 * Identity of a planned input is by pointer and size: freeing a planned input and allocating another one at the
 * same address between the plan and the write is the caller's error and is not detected.  The inputs must stay
 * alive and unchanged until the write.  Contexts are not thread-safe (above). */

/* ---- KmerSet::Size / Hash  (lib/core/kmer_set.h:65-71, :224-244) --------------------- */
/* XOR of all k-mer bit patterns in the set. */
int ksh_set_hash(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* s, uint64_t* hash);

/* ---- KmerSet::Contains / Find  (lib/core/kmer_set.h:99-105, :116-161) ------------------------
 * contains: d_found[i] = 1 if the 2K-bit pattern d_kmers[i] is in the set, else 0 (batched: one
 * launch for n queries; enqueued on the context's stream).
 * kmers: every k-mer of the set as its full 2K-bit pattern, ascending, into d_kmers[n_keys] --
 * KmerSet::Find(n_workers); a Find with a host predicate filters this one download. */
int ksh_set_contains(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* s, const uint64_t* d_kmers, int64_t n,
                     uint8_t* d_found);
int ksh_set_kmers(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* s, uint64_t* d_kmers);

/* ---- ParallelDisjointSet  (lib/core/parallel_disjoint_set.h:15-111) ---------------------------
 * The wait-free union-find the path cover's loop detection runs on (spss.h:1541-1625), as an entry
 * of its own: n nodes, m pairs (d_x[i], d_y[i]) united concurrently (one thread per pair, 64-bit
 * compare-and-swap on rank << 32 | parent), then d_root[i] = Find(i).  WHICH node represents a
 * component depends on the interleaving, as in the reference with n_workers > 1; the partition
 * does not.  Synchronises the stream. */
int ksh_dsu_components(ksh_ctx* ctx, int64_t n, const int32_t* d_x, const int32_t* d_y, int64_t m, int32_t* d_root);

/* ---- set algebra  (lib/core/kmer_set.h:164-187, :286-305; the loop needs
 *      A&B, A\B and B\A of one pair, lib/core/kmer_set_set.h:339-343) ------------------ */
/* Pass 1.  Counts |A & B| per bucket and derives the bucket offsets of the three
 * results: d_off_i / d_off_amb / d_off_bma are int64[2^N + 1] outputs.
 * totals = { |A & B|, |A \ B|, |B \ A| } (host).  The plan stays pending for ksh_pair_write on the same
 * context with the same geometry, A and B (see "Plans" above). */
int ksh_pair_plan(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* a, const ksh_set_view* b,
                  int64_t* d_off_i, int64_t* d_off_amb, int64_t* d_off_bma, int64_t totals[3]);
/* Pass 2.  Writes the keys of the three results (buffers sized from `totals`;
 * any of them may be NULL to skip that result). */
int ksh_pair_write(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* a, const ksh_set_view* b,
                   void* d_keys_i, void* d_keys_amb, void* d_keys_bma);

/* Both passes in ONE call, enqueued back to back (one stream synchronisation, for the
 * totals, and no allocation between the passes).  The key buffers are allocated by the
 * caller before the sizes are known: d_keys_i >= min(|A|, |B|) keys, d_keys_amb >= |A|,
 * d_keys_bma >= |B|. */
int ksh_pair_algebra(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* a, const ksh_set_view* b,
                     int64_t* d_off_i, int64_t* d_off_amb, int64_t* d_off_bma, void* d_keys_i,
                     void* d_keys_amb, void* d_keys_bma, int64_t totals[3]);

/* Many independent pairs (a pairwise diff matrix, the reference's pooled loops over pairs,
 * lib/core/kmer_set_set.h:205-216): the buckets of all pairs are tiled together, so the batch is
 * one plan, one count launch and one write launch, and one stream synchronisation returns all
 * totals.  Buffers as for ksh_pair_algebra. */
typedef struct ksh_pair_job {
  ksh_set_view a, b;
  int64_t *d_off_i, *d_off_amb, *d_off_bma; /* int64[2^N + 1] each                         */
  void *d_keys_i, *d_keys_amb, *d_keys_bma; /* >= min(|A|,|B|), |A|, |B| keys               */
  int64_t totals[3];                        /* out: |A & B|, |A \ B|, |B \ A|               */
} ksh_pair_job;
int ksh_pair_algebra_batch(ksh_ctx* ctx, const ksh_geom* g, ksh_pair_job* jobs, int32_t n_jobs);

/* KmerSet::Add(other) / free Add (lib/core/kmer_set.h:164-174,286-290): A | B, same
 * two-call shape.  d_off_u is int64[2^N + 1]; d_keys_u holds `total` keys. */
int ksh_set_union_plan(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* a,
                       const ksh_set_view* b, int64_t* d_off_u, int64_t* total);
int ksh_set_union_write(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* a,
                        const ksh_set_view* b, void* d_keys_u);

/* ---- KmerSet::Diff / Equals  (lib/core/kmer_set.h:191-219) ----------------------------- */
/* |A \ B| + |B \ A|. */
int ksh_set_diff(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* a, const ksh_set_view* b,
                 int64_t* diff);

/* ---- GetEdgeWeight over sampled buckets  (lib/core/kmer_set_set.h:158-219,385-425) ----- */
/* weights[p] = sum over the listed buckets of |bucket(sets[pairs[2p]]) &
 * bucket(sets[pairs[2p+1]])|.  A "sampled set" of the reference
 * (KmerSetCompact::GetSampledKmerSet, kmer_set_compact.h:120-203) is a slice of
 * the resident sorted buckets here, so no separate structure is built.
 * sets, bucket_ids, pairs and weights are HOST arrays. */
int ksh_pair_weights(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* sets, int32_t n_sets,
                     const int32_t* bucket_ids, int32_t n_ids, const int32_t* pairs,
                     int32_t n_pairs, int64_t* weights);

/* ---- SPSS container and decode -------------------------------------------------------
 * KmerSetCompact (lib/core/kmer_set_compact.h:339-347) on device: the strings'
 * bases, 2 bits each (A=0 C=1 G=2 T=3), concatenated without separators in 64-bit
 * words -- base j of the stream at bits [63-2(j%32), 62-2(j%32)] of word j/32, i.e.
 * the reference's vector<bool> index 2j is the high bit (:236-251) -- plus
 * len - K per string (:222-223).  Nothing is promised about the bits of the last
 * word behind base n_bases - 1: they may hold anything, and the decode and the k-mer count read no k-mer
 * out of them. */
typedef struct ksh_spss_view {
  const uint64_t* d_words; /* ceil(n_bases / 32) words            */
  const uint32_t* d_lens;  /* len - K per string                  */
  int64_t n_strings;
  int64_t n_bases;         /* = KmerSetCompact::Weight() (:115)   */
} ksh_spss_view;

/* KmerSetCompact::Size (kmer_set_compact.h:90-112): sum of (len - K + 1). */
int ksh_spss_size(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* s, int64_t* n_kmers);

/* KmerSetCompact::ToKmerSet = ToStrings + GetKmerSetFromSPSS
 * (kmer_set_compact.h:52-55,290-336; lib/core/spss.h:1861-1941).
 * plan : bucket histogram -> d_offsets (int64[2^N + 1]); n_keys = k-mer positions
 *        (an upper bound on the set size: repeated k-mers collapse in write).
 * write: scatter + per-bucket sort, duplicates dropped; d_keys holds n_keys(plan)
 *        keys; d_offsets is rewritten if duplicates were dropped; n_keys = set size.
 * Any n_bucket_bits the geometry allows (<= 24, as ksh_set_view).  The counting pass keeps one 4-byte counter per
 * bucket in a workgroup's 64 KB of LDS, so above N = 14 the decode takes a wide route: it counts, scatters and
 * sorts on 2^14 coarse buckets with a composite key (the N - 14 low bucket bits, then the key; a wider scratch
 * type when 2K - 14 bits exceed the key type), then one pass derives the fine offsets and one narrows the keys.
 * There, after plan, d_offsets holds the coarse layout only (every coarse bucket's range on its last fine bucket;
 * d_offsets[2^N] = n_keys): the fine offsets are what write leaves.  The wide route costs about one extra read
 * and write of the keys.  The same holds for ksh_kmer_count_write and for everything that decodes
 * (ksh_kss_build*, ksh_kss_get, ksh_spss_from_text_*). */
int ksh_spss_decode_plan(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* s, int canonical,
                         int64_t* d_offsets, int64_t* n_keys);
int ksh_spss_decode_write(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* s, int canonical,
                          int64_t* d_offsets, void* d_keys, int64_t* n_keys);

/* ---- Text form of an SPSS: the file format of KmerSetCompact::Dump / Load ------------------
 * (lib/core/kmer_set_compact.h:62-87 over WriteLines / ReadLines, lib/core/io.h:20-126): one
 * string over ACGT per line, every line closed by '\n'; the reference spells / parses it base
 * by base on the host (ToStrings :290-336, the private constructor :206-266).
 * to_text: d_text receives exactly n_bases + n_strings bytes and needs no alignment; a view whose
 * string lengths do not sum to n_bases is KSH_INVALID_ARGUMENT, refused before anything is written.
 * from_text: d_text needs no alignment either.
 * from_text: plan counts the lines and bases of n_bytes of text in device memory (a last line
 * without '\n' counts); the caller allocates ceil(n_bases / 32) words and n_strings lengths;
 * write fills them (ksh_spss_view layout).  A byte other than A, C, G, T, '\n' or a line
 * shorter than K is KSH_INVALID_ARGUMENT (the reference asserts / underflows).  K >= 4. */
int ksh_spss_to_text(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* s, char* d_text);
int ksh_spss_from_text_plan(ksh_ctx* ctx, const ksh_geom* g, const char* d_text, int64_t n_bytes,
                            int64_t* n_strings, int64_t* n_bases);
int ksh_spss_from_text_write(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens);
int ksh_spss_from_text_write_for(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens, int64_t n_strings, int64_t n_bases,
                            const void* d_input);

/* ---- KmerCounter: FASTA -> counted k-mers -> KmerSet (the step before the loop) ---------------
 * lib/core/kmer_counter.h:136-206 FromFASTA (lines 0, 2, ... are headers starting with '>',
 * lines 1, 3, ... reads over ACGTN), :64-133 FromReads (reads split at 'N', every K-long window
 * is one k-mer, canonical or not), :209-243 ToKmerSet (k-mers seen at least `cutoff` times; the
 * second result counts the distinct k-mers seen less often).
 * ksh_fasta_plan / ksh_fasta_write turn n_bytes of FASTA text in device memory into the reads'
 * ACGT fragments of length >= K as an SPSS-shaped 2-bit stream (ksh_spss_view layout; the
 * caller allocates ceil(n_bases / 32) words and n_fragments lengths between the two calls).
 * An odd number of lines, a header that is empty or does not start with '>', or a read byte
 * outside ACGTN is KSH_FAILED_PRECONDITION with the reference's message.
 * Counting is the decode pipeline with multiplicities: ksh_spss_decode_plan on the fragments
 * (*n_keys = k-mer occurrences, the size of the key buffer), then ksh_kmer_count_write:
 * offsets + sorted keys of the k-mers whose count >= cutoff, *n_keys of them, *n_cut distinct
 * k-mers below the cutoff (cutoff in 0..255: uint8 counts saturate in the reference). */
int ksh_fasta_plan(ksh_ctx* ctx, const ksh_geom* g, const char* d_text, int64_t n_bytes,
                   int64_t* n_fragments, int64_t* n_bases);
int ksh_fasta_write(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens);
int ksh_fasta_write_for(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens, int64_t n_strings, int64_t n_bases,
                   const void* d_input);
int ksh_kmer_count_write(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* reads, int canonical,
                         int32_t cutoff, int64_t* d_offsets, void* d_keys, int64_t* n_keys,
                         int64_t* n_cut);

/* ---- StreamVByte "0124" pack of the string lengths ---------------------------------------
 * The in-memory form of KmerSetCompact::lengths_compressed_
 * (lib/core/kmer_set_compact.h:257-265 streamvbyte_encode_0124, :269-287 decode; format in
 * csrc/ksh_svb.hip).  encode: d_out holds ceil(n/4) + 4n bytes (streamvbyte_max_compressedbytes)
 * or is NULL to get the size only; *bytes = compressed size.  decode: n values out. */
int ksh_svb_encode_0124(ksh_ctx* ctx, const uint32_t* d_in, int64_t n, uint8_t* d_out, int64_t* bytes);
int ksh_svb_decode_0124(ksh_ctx* ctx, const uint8_t* d_in, int64_t n, uint32_t* d_out,
                        int64_t* bytes_read);

/* ---- SPSS encode ----------------------------------------------------------------------
 * KmerSetCompact::FromKmerSet(set, canonical, fast, n_workers)
 * (lib/core/kmer_set_compact.h:36-47) = the SPSS + the 2-bit packing constructor (:206-266).
 * canonical != 0 (the set holds canonical k-mers only):
 *   mode 0: GetSPSSCanonical(fast = true) (lib/core/spss.h:1835-1858: unitigs, greedy path
 *           cover :1358-1539, loop cut :1541-1647, stitch :1649-1829).
 *   mode 1: GetUnitigsCanonical (lib/core/spss.h:230-615), every unitig a string.
 *   mode 2: GetSPSSCanonical(fast = false) (lib/core/spss.h:1208-1356): the reference's
 *           one-thread path extension, replayed by one device thread over the edge table
 *           (sequential by definition; everything around it is the parallel pipeline).
 * canonical == 0 (k-mers as they are, edges only forward):
 *   mode 0 / 2: GetSPSS (lib/core/spss.h:697-1036; FromKmerSet ignores `fast` here).
 *   mode 1: GetUnitigs (lib/core/spss.h:73-227).
 * The strings and their order are the oracle's (the reference's n_workers == 1
 * control flow with ascending iteration).
 * KSH_INVALID_ARGUMENT for a canonical set that holds a k-mer equal to its own reverse
 * complement (even k only).
 * plan : everything up to the string layout; returns the container's sizes.
 * write: d_words = ceil(n_bases / 32) words, d_lens = n_strings values (len - K). */
int ksh_spss_encode_plan(ksh_ctx* ctx, const ksh_geom* g, const ksh_set_view* set, int canonical,
                         int mode, int64_t* n_strings, int64_t* n_bases);
int ksh_spss_encode_write(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens);
int ksh_spss_encode_write_for(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens, int64_t n_strings, int64_t n_bases,
                         const void* d_input);
/* stats = { unitigs, matching rounds, strings, bases } of the current plan. */
int ksh_spss_encode_stats(ksh_ctx* ctx, int64_t stats[4]);
/* Which variants of the encode's kernels the current plan ran (they are chosen by set size and geometry;
 * the parity tests assert the route so that a case cannot silently take another one): a mask of KSH_ROUTE_*. */
enum {
  KSH_ROUTE_PROBE_STAGED = 1 << 0,       /* neighbour probe staged in LDS (k_rc_*, k_adj_rc1 / k_adj_rc), not k_adjacency */
  KSH_ROUTE_RC_1024 = 1 << 1,            /* k_adj_rc1 / k_adj_rc with 1024 / 512 / 256 / 64 threads per group */
  KSH_ROUTE_RC_512 = 1 << 2,
  KSH_ROUTE_RC_256 = 1 << 3,
  KSH_ROUTE_RC_64 = 1 << 4,
  KSH_ROUTE_RC_BATCHED = 1 << 5,         /* some group took several batches: of its records (k_adj_rc1) or of its ranges (k_adj_rc) */
  KSH_ROUTE_SCATTER_TWO_LEVEL = 1 << 6,  /* k_rc_scatter_l1 / _l2 instead of k_rc_scatter */
  KSH_ROUTE_FWD_STAGED = 1 << 7,         /* k_adj_fwd_staged (KSH_FWD=staged) instead of k_adj_fwd */
  KSH_ROUTE_RANK_ONE_LAUNCH = 1 << 8,    /* all ruler walkers in one launch (mirror images racing) */
  KSH_ROUTE_HEADS_ONE_LAUNCH = 1 << 9,   /* the same for the chain-start walkers */
  KSH_ROUTE_JUMP_TWO_LEVEL = 1 << 10,    /* pointer jumping over the level-2 rulers (k_l2_*) */
  KSH_ROUTE_RANK_STAMPED = 1 << 11,      /* the stamping walks (sets with a non-branching loop, KSH_RANK=stamp) */
  KSH_ROUTE_EMIT_LOGS = 1 << 12,         /* strings written from the ranking walks' logs */
  KSH_ROUTE_LONG_STRETCHES = 1 << 13,    /* ... and some stretch outgrew its log (the long list) */
  KSH_ROUTE_MATCH_MORE_ROUNDS = 1 << 14, /* the matching needed more than its first batch of rounds */
  KSH_ROUTE_FWD_TARGETS = 1 << 15,       /* k_adj_fwd_targets: forward probes marked at their targets, one search per k-mer */
  KSH_ROUTE_RC1_STREAMED = 1 << 16,      /* k_adj_rc1: k_adj_rc turned round (a group's records in LDS, its ranges streamed) */
  KSH_ROUTE_RC_MARKS_GROUPS = 1 << 17,   /* ... and k_adj_rc ran for some group whose records did not fit k_adj_rc1 */
  KSH_ROUTE_TGT_PARTS = 1 << 18          /* k_tgt_split / k_tgt_subcuts cut some window of k_adj_fwd_targets into parts */
};
int ksh_spss_encode_routes(ksh_ctx* ctx, int64_t* routes);
/* Frees the current plan's device memory (also done by the next plan / ctx_destroy). */
int ksh_spss_encode_release(ksh_ctx* ctx);

/* ---- SPSS path cover from caller-supplied unitigs -------------------------------------------
 * GetSPSSCanonical(unitigs, prefixes, suffixes, fast, n_workers, n_buckets) (lib/core/spss.h:1039-1829)
 * and GetSPSS(unitigs, prefixes, n_workers, n_buckets) (:697-1014): the n strings of `unitigs`
 * (ksh_spss_view layout, e.g. what ksh_spss_encode_write with mode 1, ksh_spss_from_text_write or
 * ksh_fasta_write produce) are the nodes, in the order given; the prefix / suffix maps of the
 * reference are derived on the device.  The output strings and their order are the oracle's
 * (reference n_workers == 1): canonical != 0 with fast != 0 is the greedy path cover of
 * GetSPSSCanonical(fast = true), fast == 0 the one-thread path extension of fast = false;
 * canonical == 0 is GetSPSS (`fast` is ignored).
 * Edges come from the strings' end k-mers only, taken as they are (P = first, S = last k-mer):
 * the right side of i meets j != i where P_j == Next(S_i, c) or S_j == rc(Next(S_i, c)), the
 * left side where S_j == Prev(P_i, c) or P_j == rc(Prev(P_i, c)); non-canonical: only
 * P_j == Next(S_i, c).  Interior k-mers are not looked at (neither does the reference): a k-mer
 * that occurs in two strings is not detected.
 * Preconditions, checked on the device, each a KSH_INVALID_ARGUMENT that names it and the string:
 *   canonical: the canonical forms of the end k-mers are pairwise distinct across strings (a
 *     string given twice, or together with its reverse complement, is refused); a string whose
 *     first and last k-mers have the same canonical form must be exactly K long; no end k-mer
 *     is its own reverse complement (even k only, as the encode refuses such a set);
 *   non-canonical: the first k-mers are pairwise distinct, and so are the last k-mers;
 *   both: sum(lens + K) == n_bases.
 * Every unitig set of a k-mer set satisfies them (GetUnitigs / GetUnitigsCanonical, or the
 * unitigs of a compacted de Bruijn graph tool), in any order and orientation.
 * Limits: at most 2^30 - 1 strings (the path cover's walk records hold 31-bit state ids) and
 * fewer than 2^31 - 16 k-mers in all.  An empty input gives 0 strings and 0 bases.
 * The cover plan takes the encode plan's slot: a new plan of either kind replaces the current
 * one, ksh_spss_encode_write / _routes refuse a cover plan and ksh_spss_cover_write / _stats an
 * encode plan.  The input must stay alive and unchanged until ksh_spss_cover_write.
 * plan : edge table, path cover, string layout; returns the output's sizes.
 * write: d_words = ceil(n_bases / 32) words, d_lens = n_strings values (len - K). */
int ksh_spss_cover_plan(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* unitigs, int canonical, int fast,
                        int64_t* n_strings, int64_t* n_bases);
int ksh_spss_cover_write(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens);
int ksh_spss_cover_write_for(ksh_ctx* ctx, uint64_t* d_words, uint32_t* d_lens, int64_t n_strings, int64_t n_bases,
                        const void* d_input);
/* stats = { unitigs (input strings), matching rounds, strings, bases } of the current cover plan. */
int ksh_spss_cover_stats(ksh_ctx* ctx, int64_t stats[4]);
/* Frees the current plan (of either kind), as ksh_spss_encode_release does. */
int ksh_spss_cover_release(ksh_ctx* ctx);

/* ---- KmerSetSet: the loop kmerset-multiple-compress runs -------------------------------
 * ksh_kss_build = KmerSetSet(vector<KmerSetCompact>, canonical, n_workers)
 * (lib/core/kmer_set_set.h:109-427) on device-resident sets.  inputs are the
 * KmerSetCompact containers (device); bucket_ids replaces the unseeded
 * GetRandomInts((1 << N) / 50, ...) of :123-124 (HOST array, ascending);
 * max_iterations < 0 runs to the reference's stopping rule.  The input containers
 * must stay alive while they are nodes of the result, and the context must outlive the
 * result.  The three re-encodes of a merge (:345-360) are deferred to the points where the
 * reference reads them (Weight() at the convergence checks, :287, and the final nodes): same
 * values, fewer encodes.  Synchronises the stream before returning.
 * n_inputs == 0 (inputs, and in ksh_kss_build_owned owners, may then be NULL; so may bucket_ids when
 * n_ids == 0) is no error on any of the three entry points: KSH_OK and a structure of 0 nodes, as the
 * reference's constructor leaves one (no weights, the loop breaks at once).  Nothing is launched and, in the
 * multi-rank builds, nothing is exchanged -- n_inputs is the same on every rank.  Its accessors work:
 * ksh_kss_size 0, ksh_kss_trace 0 iterations and 0 checkpoints, ksh_kss_initial_weights 0 entries,
 * ksh_kss_stats all 0, ksh_kss_meta "0" (an empty adjacency list), ksh_kss_children none; ksh_kss_node,
 * ksh_kss_node_holder and ksh_kss_get answer KSH_INVALID_ARGUMENT for every i (there is no node i).
 * A negative n_inputs or n_ids, and a NULL array with a positive count, are KSH_INVALID_ARGUMENT. */
typedef struct ksh_kss ksh_kss;
int ksh_kss_build(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* inputs, int32_t n_inputs,
                  const int32_t* bucket_ids, int32_t n_ids, int canonical, int32_t max_iterations,
                  ksh_kss** out);
/* Multi-GPU build, one process per GPU.  Every rank calls this with the same inputs and runs the
 * same (deterministic) loop on its own resident copies of the sets; the SPSS encodes, ~85 % of
 * the loop's time, are dealt out node by node (largest set first, to the least loaded rank), and at every point
 * where the loop reads the SPSS weights (kmer_set_set.h:287 and the end) the ranks exchange
 * (n_strings, n_bases) of the freshly encoded nodes through `gather`: an all-gather of `count`
 * int64 per rank into recv[world * count], rank-major, returning 0 on success (RCCL or any other
 * transport; KB-scale, a few times per build).  Trace, checkpoints, DAG and every node's set
 * are identical on all ranks and equal to the single-GPU build; a node's SPSS is held by one
 * rank (ksh_kss_node_holder; -1 = every rank, the inputs), and ksh_kss_node answers
 * KSH_FAILED_PRECONDITION for the SPSS of a node held elsewhere. */
typedef int (*ksh_allgather_i64)(void* user, const int64_t* send, int64_t count, int64_t* recv);
int ksh_kss_build_sharded(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* inputs, int32_t n_inputs,
                          const int32_t* bucket_ids, int32_t n_ids, int canonical,
                          int32_t max_iterations, int32_t rank, int32_t world, ksh_allgather_i64 gather,
                          void* gather_user, ksh_kss** out);
int ksh_kss_node_holder(const ksh_kss* k, int32_t i, int32_t* rank);

/* ---- owner-sharded multi-GPU build --------------------------------------------------------
 * One process per GPU; no rank holds every node (config 5: 256 sets of 5 * 10^8 48-bit keys are
 * 1 TB decoded, 128 GB per GPU of an 8-GPU node).
 *   * every input set is decoded and kept by ONE rank, its owner (owners[i]); a rank passes the
 *     containers of the inputs it owns, the others' entries are ignored;
 *   * what the loop's decisions read -- the 2 % sampled buckets of every node
 *     (kmer_set_set.h:138-153) -- is all-gathered once for the inputs; after that every rank runs
 *     the same control loop on its copy of the samples (arg-max :308-316, the merged pair's new
 *     samples :349-363 = the same merge on the sampled buckets, the re-weighting :385-425) with no
 *     exchange at all: the samples of a merge's three results ARE the merge of the samples;
 *   * the full-size Intersection + Sub + Sub of iteration (j, k) (:339-343) runs on the owner of
 *     j; if k lives elsewhere its keys travel there point to point (xGMI) and k's remainder stays
 *     with j's owner, which also owns the new node;
 *   * at the points where the loop reads SPSS weights (:287 and the end) every rank encodes the
 *     stale nodes it owns and one all-gather of (n_strings, n_bases, size) per stale node puts
 *     the sum on all ranks.  A check only decides whether the loop stops, so its exchange is taken
 *     one check later: the ranks go on with the next interval meanwhile and undo it if the answer
 *     was "stop" (same result; a loaded rank no longer holds up the others at every check), and
 *     before a check's encodes run they are dealt out again: the most loaded rank hands its largest
 *     stale node to the least loaded one (the set travels under the encodes, on a second
 *     communicator), which owns it from then on.
 * Trace, checkpoints, DAG and every node's set and SPSS equal the single-GPU build's; a node's
 * set and SPSS live on its owner only (ksh_kss_node_holder; ksh_kss_node answers
 * KSH_FAILED_PRECONDITION elsewhere, ksh_kss_get when a reachable node lives elsewhere).
 *
 * Transport: RCCL, opened at run time (librccl.so), collectives enqueued on the context's stream
 * with device buffers -- rank 0 draws the id, the caller carries its 128 bytes to the other ranks
 * (MPI, torch.distributed, a file) -- or caller-supplied functions over device buffers, which
 * return when the transfer is complete (rehearsals with several ranks on one GPU, where RCCL
 * cannot run; the library drains its stream before calling them). */
#define KSH_COMM_ID_BYTES 128
typedef struct ksh_comm ksh_comm;
typedef struct ksh_comm_fns {
  /* = sizeof(ksh_comm_fns) of the header the caller was compiled against (ksh_version() >= 2): members beyond it
   * are taken as NULL, so the struct can grow without old callers being read past their end; zero-initialise
   * the struct and set the members you have */
  size_t struct_size;
  void* user;
  /* d_recv receives world * bytes, rank-major */
  int (*allgather)(void* user, const void* d_send, void* d_recv, size_t bytes);
  int (*send)(void* user, const void* d_buf, size_t bytes, int32_t peer);
  int (*recv)(void* user, void* d_buf, size_t bytes, int32_t peer);
  /* optional (may be NULL): called once when this rank gives the build up at a point where it cannot
   * follow the exchange protocol any longer; it should make the peers' pending calls fail */
  void (*abort)(void* user);
} ksh_comm_fns;
int ksh_comm_unique_id(unsigned char id[KSH_COMM_ID_BYTES]);
int ksh_comm_create_rccl(ksh_ctx* ctx, int32_t rank, int32_t world, const unsigned char id[KSH_COMM_ID_BYTES],
                         ksh_comm** out);
int ksh_comm_create_custom(ksh_ctx* ctx, int32_t rank, int32_t world, const ksh_comm_fns* fns, ksh_comm** out);
int ksh_comm_destroy(ksh_comm* comm);
/* Collective: every rank's id through the transport's all-gather (device buffers); *n_ranks = distinct
 * ids received: the ranks that actually took part (bench.py quotes it as multi_gpu.ranks_seen). */
int ksh_comm_ranks_seen(ksh_comm* comm, int32_t* n_ranks);
/* owners[i] in [0, world): the rank that holds input i.  inputs[i] is read on that rank only. */
int ksh_kss_build_owned(ksh_ctx* ctx, ksh_comm* comm, const ksh_geom* g, const ksh_spss_view* inputs,
                        int32_t n_inputs, const int32_t* owners, const int32_t* bucket_ids, int32_t n_ids,
                        int canonical, int32_t max_iterations, ksh_kss** out);
/* stats = { bytes this rank sent point to point, bytes it received, sets it sent (merged pairs whose
 * members lived on different ranks), bytes it contributed to all-gathers, convergence checks whose
 * exchange was deferred by one check (the ranks go on with the next interval instead of waiting for the
 * slowest encoder; KSH_OWNED_LOOKAHEAD=0 turns that off), intervals undone because a deferred check
 * said "stop", sets this rank handed to a less loaded rank for encoding at a check (they live there
 * afterwards; KSH_OWNED_MIGRATE=0 turns that off), all-gathers of per-pair int64 weights (one per iteration
 * with KSH_OWNED_WEIGHTS=sharded: the weight tables dealt out by pair list, lib/core/kmer_set_set.h:205-218,
 * 385-425; 0 by default: every rank weighs its replica of the samples and nothing is exchanged) }. */
int ksh_kss_comm_stats(const ksh_kss* k, int64_t stats[8]);
/* SPSS encodes this process ran for the build, and the k-mers they covered (the sharded build's
 * balance; in a single-GPU build: how many encodes the deferral left). */
int ksh_kss_encode_counts(const ksh_kss* k, int64_t* n_encodes, int64_t* n_encoded_kmers);
/* Of those encodes, the ones that only computed Weight() (the encode's plan without the write): with
 * KSH_KSS_LOOP=ahead ksh_kss_build runs the control loop on the samples two intervals ahead of the sets
 * (every decision of the loop reads sampled buckets only) and only weighs the stale nodes it will merge
 * again.  Off by default: on loops of a few checks the strings owed when the last check stops the loop
 * cost what the skipped writes saved. */
int ksh_kss_weighed_counts(const ksh_kss* k, int64_t* n_weighed, int64_t* n_weighed_kmers);
/* Wall seconds the build spent in: [0] decode of the inputs, [1] weight computations,
 * [2] merges (pair plan + write), [3] SPSS encodes (with, in a sharded build, the exchanges). */
int ksh_kss_phase_seconds(const ksh_kss* k, double seconds[4]);
int ksh_kss_destroy(ksh_kss* k);
/* KmerSetSet::Size (:430): number of nodes. */
int ksh_kss_size(const ksh_kss* k, int32_t* n_nodes);
/* Node i: its SPSS container, its resident set and its k-mer count (any may be NULL). */
int ksh_kss_node(const ksh_kss* k, int32_t i, ksh_spss_view* compact, ksh_set_view* set,
                 int64_t* size);
/* children_[i] (:365-366); the pointer stays valid until ksh_kss_destroy. */
int ksh_kss_children(const ksh_kss* k, int32_t i, const int32_t** children, int32_t* n_children);
/* Line 0 of meta.<ext> (SerializeAdjacencyList, :45-56), keys ascending. */
const char* ksh_kss_meta(const ksh_kss* k);
/* Per-iteration rows {j, k, weight, |S_j| + |S_k|, size_diff} (the values the reference
 * logs at :324,:380) and per-checkpoint rows {iteration, previous, updated, stopped}
 * with the float improvement of :289-295. */
int ksh_kss_trace(const ksh_kss* k, int64_t* n_iterations, const int64_t** rows,
                  int64_t* n_checkpoints, const int64_t** checkpoint_rows,
                  const float** improvements);
int ksh_kss_initial_weights(const ksh_kss* k, const int64_t** weights, int64_t* n);
/* stats = { initial total_size, final total_size, initial total_spss_weight, N_proc
 * (SURVEY.md 8d), final total_spss_weight, sum over nodes of ceil(2 Weight / 8) bytes, sum
 * over nodes of the StreamVByte-0124 size of the lengths, nodes }: bytes/k-mer after SPSS =
 * (stats[5] + stats[6]) / sum of the input set sizes (metric 2). */
int ksh_kss_stats(const ksh_kss* k, int64_t stats[8]);
/* KmerSetSet::Get(i) (:433-454): union over the nodes reachable from i.  Returns new
 * device buffers (release with ksh_free). */
int ksh_kss_get(const ksh_kss* k, int32_t i, int64_t** d_offsets, void** d_keys, int64_t* n_keys);

/* ---- Membership queries over a KmerSetSet: which nodes' Get(i) hold each k-mer ----------------
 * Column i of a row is Get(i).Contains(q) (kmer_set_set.h:433-454) for EVERY node i of the structure,
 * not only the inputs (they are columns 0 .. n_inputs - 1).  q is in Get(i) iff some node j whose own
 * set holds q is reachable from i (i itself included); the index keeps the ancestor closure of the
 * DAG, so a row is the OR of anc[j] over the nodes j that hold q.
 * Rows: W = ceil(n_nodes / 64) uint64 words per query, row-major in the caller's query order; bit
 * i % 64 of word i / 64 is column i.  Rows are held in registers / LDS: at most 16 words, i.e.
 * structures of more than 1024 nodes are refused (KSH_INVALID_ARGUMENT, by name).
 * Queries are 2K-bit patterns as in ksh_set_contains.  canonicalize != 0 looks up min(q, rc(q)) (the
 * call for a structure built with canonical = 1).  A pattern with bits at or above 2K is in no set:
 * its row is all zeros (checked before canonicalising). */
typedef struct ksh_kss_index ksh_kss_index;
/* From a built structure: borrows its resident node sets (no decode, no copy) and its context.  The
 * index must be destroyed before the ksh_kss.  KSH_FAILED_PRECONDITION for an owner-sharded build in
 * which some node lives on another rank. */
int ksh_kss_index_from_kss(const ksh_kss* k, ksh_kss_index** out);
/* From node containers and the DAG (what KmerSetSet::Load has): decodes every node (the ordinary
 * decode, any N up to 24) into index-owned sets allocated from ctx's pool.  children as CSR on the
 * HOST: node i's children are child_ids[child_offsets[i] .. child_offsets[i + 1]).  KSH_INVALID_ARGUMENT
 * for a child id out of range, a self edge, a cycle, a malformed geometry or container view, and
 * n_nodes outside [1, 1024]; the DAG is checked before any device work.  The containers are only read
 * during the call; ctx must outlive the index. */
int ksh_kss_index_create(ksh_ctx* ctx, const ksh_geom* g, const ksh_spss_view* nodes, int32_t n_nodes,
                         const int64_t* child_offsets, const int32_t* child_ids, int canonical,
                         ksh_kss_index** out);
/* d_rows[n * W] for the n patterns d_kmers[n] (device), enqueued on the context's stream (the join
 * route synchronises it once per pass of 2^24 queries, for the pass's tile count).
 * route: 0 auto, 1 per-query search, 2 bucket join.  Scratch: the context's arena. */
int ksh_kss_index_query(ksh_kss_index* idx, const uint64_t* d_kmers, int64_t n, int canonicalize,
                        int route, uint64_t* d_rows);
/* n_nodes, W, and the bytes of the resident sets the index reads (offsets included). */
int ksh_kss_index_info(const ksh_kss_index* idx, int32_t* n_nodes, int32_t* words_per_row,
                       int64_t* resident_bytes);
/* The routes the last query (ksh_kss_index_query, ksh_seq_hits, ksh_kss_pair_counts, ksh_kss_select_count,
 * ksh_kss_select_keys, ksh_kss_select_class_ids, ksh_kss_color_classes or ksh_seq_class_runs) took, a mask of
 * KSH_QROUTE_* (synchronises the stream). */
enum {
  KSH_QROUTE_SEARCH = 1 << 0,    /* per-query search                                            */
  KSH_QROUTE_JOIN = 1 << 1,      /* bucket join                                                  */
  KSH_QROUTE_OVERSIZE = 1 << 2,  /* ... some node's slice outgrew the LDS stage: searched in HBM */
  KSH_QROUTE_CHUNKED = 1 << 3,   /* ... the batch took more than one pass of 2^24 queries        */
  KSH_QROUTE_SEQ_PASSES = 1 << 4, /* ksh_seq_hits, ksh_seq_class_runs: more than one pass of positions */
  KSH_QROUTE_PAIR_SPLIT = 1 << 5, /* ksh_kss_pair_counts, ksh_kss_select_count, ksh_kss_select_keys: some bucket's
                                     k-mers did not fit one tile and were cut by key range (ksh_kss_color_classes
                                     reports it with the same meaning, and so does
                                     ksh_kss_select_class_ids)                                    */
  KSH_QROUTE_PAIR_FLUSH = 1 << 6, /* ... some workgroup flushed its counters before its last tile */
  KSH_QROUTE_CLASS_SPILL = 1 << 7 /* ksh_kss_color_classes: some workgroup emptied its on-chip class table into
                                     the global one before its last tile                          */
};
int ksh_kss_index_routes(const ksh_kss_index* idx, uint32_t* bits);
int ksh_kss_index_destroy(ksh_kss_index* idx);

/* ---- Sequence queries: k-mer hits per sequence and node ------------------------------------------
 * d_hits[s * n_nodes + i] = number of k-mer positions p of sequence s (0 <= p <= lens[s]) whose k-mer is in
 * Get(i), for every node i of the index.  Sequences: ksh_spss_view layout, as ksh_fasta_write,
 * ksh_spss_from_text_write and ksh_spss_encode_write produce it.  Positions are counted, not distinct k-mers:
 * a k-mer that occurs twice in a sequence counts twice.  Windows never cross from one string into the next.
 * canonicalize and route: as in ksh_kss_index_query (the auto rule is applied to every pass).
 * pass_positions: k-mer positions handled per pass; the k-mers and bit rows of a pass stay in scratch from the
 * context's pool, 8 + 8 W bytes per position.  0: the default, which keeps that scratch within 256 MiB and a pass
 * within the join's 2^24 queries (2^24 positions at W = 1, about 1.9 * 10^6 at W = 16).  Any value >= 1 is taken
 * as it is (values above 2^28 as 2^28); a sequence longer than a pass is split across passes and its counts add
 * up.  ksh_kss_index_routes reports the routes of all passes, and KSH_QROUTE_SEQ_PASSES when there were several.
 * d_hits (n_strings * n_nodes values, device) is written in full, zeros included; n_strings == 0 is KSH_OK with
 * nothing written.  Enqueued on the index's context stream; the stream is synchronised once for the size check
 * and, on the join route, once per pass.
 * KSH_INVALID_ARGUMENT, before anything is counted: a NULL argument, a negative size or pass_positions, a route
 * outside 0..2, an index whose geometry has K < 4 (all before any device work); lens[s] == UINT32_MAX, or
 * sum(lens + K) != n_bases (as the cover: checked on the device before the words are read).
 * The index must be usable as for ksh_kss_index_query: one made by ksh_kss_index_from_kss borrows the node sets
 * of its ksh_kss and must not be used after ksh_kss_destroy. */
int ksh_seq_hits(const ksh_spss_view* seqs, ksh_kss_index* idx, int canonicalize, int route,
                 int64_t pass_positions, uint32_t* d_hits);

/* ---- Pairwise intersection counts of the sets of a KmerSetSet ---------------------------------------
 * d_counts[a * n_cols + b] = |Get(cols[a]) & Get(cols[b])| (kmer_set_set.h:433-454), exact, from one pass over the
 * index's resident node sets: nothing is decompressed and no Get(i) is formed.  The matrix is symmetric and its
 * diagonal is |Get(cols[a])|; the exact Jaccard similarity of two sets is c_ab / (c_aa + c_bb - c_ab).
 * cols: HOST array of n_cols distinct node ids in any order, 1 <= n_cols <= 128 (the inputs are ids
 * 0 .. n_inputs - 1; internal nodes are allowed).  It is only read during the call.  NULL: all nodes in order
 * (n_cols is ignored), refused on an index of more than 128 nodes.  A larger collection is covered by several
 * calls: cut the ids into blocks of at most 64, and call once per pair of blocks with cols = the two blocks one
 * after the other (and once per block alone, or with any partner, for its diagonal block); the off-diagonal
 * quadrant of each result is the block pair's part of the table.
 * d_counts: device int64[n_cols * n_cols], written in full, zeros included.
 * n_distinct (host, may be NULL): the number of distinct k-mers held by any node of the index -- all nodes, not only
 * cols.  When it is non-NULL the call synchronises the stream once; otherwise the work is only enqueued on the
 * index's context stream.
 * flush_rows: the rows (distinct k-mers with their column bits) a workgroup accumulates in its 32-bit on-chip
 * counters between flushes to d_counts.  0: the default, 2^31 - 2048 -- a counter grows by at most one per row and
 * a workgroup checks after every tile of at most 1024 rows, so no counter can reach 2^31.  Any value >= 1 is taken
 * as it is (values above the default as the default); small values only make the pass slower.
 * ksh_kss_index_routes reports KSH_QROUTE_PAIR_SPLIT and KSH_QROUTE_PAIR_FLUSH for the last call.
 * The pass reads every node's offsets of every bucket: at large N (2^20 buckets and more) that, not the keys, is
 * most of what it reads -- correct, and slow.
 * KSH_INVALID_ARGUMENT, each with a message and before any device work: NULL idx or d_counts, n_cols outside
 * [1, 128] with non-NULL cols, an id outside [0, n_nodes), a repeated id, a negative flush_rows, NULL cols on an
 * index of more than 128 nodes.
 * Scratch comes from the context's pool and is given back before the call returns; the call keeps nothing and
 * ends no pending plan.  (As in ksh_seq_hits, the index is not the first parameter: the columns asked for are.)  The index must be usable as for ksh_kss_index_query. */
int ksh_kss_pair_counts(const int32_t* cols, int32_t n_cols, ksh_kss_index* idx, int64_t flush_rows,
                        int64_t* d_counts, int64_t* n_distinct);

/* ---- Selections: the k-mers that chosen sets of a KmerSetSet share, or do not -------------------------------
 * For a k-mer q held by any node of the index, c(q) = the number of a with q in Get(cols[a]).  q is selected iff
 *     min_count <= c(q) <= max_count,   q in Get(r) for every r of require,   q not in Get(x) for every x of exclude.
 * min_count >= 1, so a selected k-mer always lies in the union of the columns.  Some selections over n columns:
 * the union 1..n; the core n..n; private to s: require = {s}, max_count = 1; accessory 2..n-1; A & B \ C:
 * cols = {A, B, C}, require = {A, B}, exclude = {C}.
 * Both calls are stateless: each is one pass over the index's resident node sets (the pass of ksh_kss_pair_counts
 * with another consumer: nothing is decompressed and no Get(i) is formed), they keep no plan in the context, join no
 * plan group and end no pending plan -- which is why the second is not named *_write: that ending belongs to the
 * two-call pairs of "Plans".  As in ksh_seq_hits and ksh_kss_pair_counts the request comes first, the index second.
 * Everything a ksh_kss_selection points to is HOST memory and only read during the call. */
typedef struct ksh_kss_selection {
  size_t struct_size;            /* sizeof(ksh_kss_selection) of the caller's header, as ksh_comm_fns::struct_size */
  const int32_t* cols;           /* n_cols distinct node ids, any order, 1..128; NULL: all nodes in order (n_cols is
                                    ignored; refused on an index of more than 128 nodes) */
  int32_t n_cols;
  int32_t min_count, max_count;  /* 1 <= min_count <= max_count <= n_cols; max_count == 0 means n_cols */
  const int32_t* require;        /* node ids, each one of cols: q must be in Get(id) */
  int32_t n_require;
  const int32_t* exclude;        /* node ids, each one of cols: q must not be in Get(id) */
  int32_t n_exclude;
} ksh_kss_selection;
/* The size of a selection, its bucket offsets and the multiplicity spectrum; any of the three outputs may be NULL,
 * not all of them.
 * d_offsets (device, int64[2^N + 1]): the bucket offsets of the selection, as a ksh_set_view has them.
 * n_keys (host): the selection's size.
 * spectrum (HOST, int64[n_cols + 1]): spectrum[m] = the number of distinct k-mers of the whole structure with
 * c(q) == m, whatever the thresholds, require and exclude say; spectrum[0] counts the k-mers that only nodes outside
 * cols hold.  So sum(spectrum) is the n_distinct of ksh_kss_pair_counts and sum(m * spectrum[m]) the trace of its
 * table.  All counts are exact at any structure size: they are kept in 64-bit counters throughout.
 * The call synchronises the index's context stream once.  Scratch: the context's pool (given back before the call
 * returns) and, for the scan of more than 2^18 buckets, its arena. */
int ksh_kss_select_count(const ksh_kss_selection* sel, ksh_kss_index* idx, int64_t* d_offsets, int64_t* n_keys,
                         int64_t* spectrum);
/* The selected keys: the same pass again, with d_offsets as ksh_kss_select_count of the same request and index made
 * them.  Bucket b goes to d_keys[d_offsets[b] .. d_offsets[b + 1]) in the index's key width, ascending, so that
 * (d_offsets, d_keys, n_keys) is an ordinary ksh_set_view that every other call accepts (as for every set, a key
 * buffer should be at least 16 bytes: the merge kernels read, never write, up to 16 bytes past a short set).
 * n_keys is the capacity of d_keys in keys: nothing is written at or beyond it, nor outside a bucket's own range, nor
 * beyond a bucket's last key.  The pass counts again as it goes: if some bucket's selection is not exactly
 * d_offsets[b + 1] - d_offsets[b] keys inside [0, n_keys) -- offsets of another selection or index -- the call
 * returns KSH_FAILED_PRECONDITION with a message, after its one synchronisation; d_keys is then unspecified within
 * [0, n_keys).  n_keys == 0 with all-zero offsets is KSH_OK: nothing is written and d_keys may be NULL.
 * KSH_INVALID_ARGUMENT for both calls, each with a message that names the field.  Before the index is dereferenced:
 * NULL sel or idx; struct_size smaller than the struct up to n_exclude; n_cols outside [1, 128] with non-NULL cols;
 * min_count < 1, max_count < 0, or a non-zero max_count < min_count; a negative n_require or n_exclude, or a NULL
 * list with a positive count; all three outputs NULL (count); NULL d_offsets, a negative n_keys, NULL d_keys with
 * n_keys > 0 (keys).  After reading only the index's host fields: an id outside [0, n_nodes); a repeated id in cols;
 * a require or exclude id that is not in cols; an id in both require and exclude; max_count or min_count above
 * n_cols; NULL cols on an index of more than 128 nodes.  The index still serves after a refusal.
 * ksh_kss_index_routes reports KSH_QROUTE_PAIR_SPLIT for the last call with the meaning it has for
 * ksh_kss_pair_counts: some bucket was cut by key range.  The index must be usable as for ksh_kss_index_query. */
int ksh_kss_select_keys(const ksh_kss_selection* sel, ksh_kss_index* idx, const int64_t* d_offsets, int64_t n_keys,
                        void* d_keys);

/* ---- Colour classes: the k-mers of a KmerSetSet per exact membership pattern --------------------------------
 * For a k-mer q held by any node of the index, its row over the chosen columns has bit a set iff q is in
 * Get(cols[a]).  A colour class is a distinct row; the call returns every class with the number of distinct k-mers
 * of the structure that have exactly that row: the data of an UpSet plot, the private k-mers of every set at once
 * (the classes with one bit), the split support of a phylogeny, the colour-class table of a coloured de Bruijn
 * graph.  The multiplicity spectrum of ksh_kss_select_count is its sum by popcount, the table of ksh_kss_pair_counts
 * its sum over the classes that hold two given bits.  One pass over the index's resident node sets (the pass of
 * ksh_kss_pair_counts with another consumer): nothing is decompressed and no Get(i) is formed.
 * cols, n_cols: as in ksh_kss_pair_counts -- a HOST array of 1..128 distinct node ids in any order (internal nodes
 * are allowed), only read during the call; NULL: all nodes in order (n_cols is ignored), refused on an index of more
 * than 128 nodes.
 * capacity: the classes the caller has room for, 1 <= capacity <= 2^24.  rows: HOST uint64[2 * capacity]; counts:
 * HOST int64[capacity]; n_classes: host.
 * On KSH_OK *n_classes <= capacity classes are written and nothing beyond them: class c has rows[2 c] = the bits of
 * columns 0..63, rows[2 c + 1] = the bits of columns 64..127, and counts[c] >= 1.  Classes are ascending by
 * (rows[2 c + 1], rows[2 c]) read as one 128-bit integer.  Row zero is a class like any other: the k-mers that only
 * nodes outside cols hold (what spectrum[0] counts), so sum(counts) is the n_distinct of ksh_kss_pair_counts.  An
 * index without k-mers gives *n_classes = 0.  All counts are exact at any structure size: 64-bit counters throughout.
 * More classes than capacity: KSH_FAILED_PRECONDITION with a message that names capacity, *n_classes = capacity + 1,
 * rows and counts unspecified within their first capacity entries and untouched beyond them; the index still serves.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  Before the index is dereferenced: NULL idx, rows,
 * counts or n_classes; capacity outside [1, 2^24]; n_cols outside [1, 128] with non-NULL cols.  After reading only
 * the index's host fields: an id outside [0, n_nodes); a repeated id; NULL cols on an index of more than 128 nodes.
 * The call is stateless: scratch comes from the context's pool (16 bytes per node, 32 bytes per slot of a table of
 * the next power of two >= 2 * capacity slots, 24 bytes per class of capacity) and is given back before the call
 * returns; it keeps no plan, joins no plan group and ends no pending plan.  As in ksh_kss_pair_counts the request
 * comes first and the index third.  It synchronises the index's context stream once; a table of more than 4096
 * classes takes a second copy and synchronisation for the classes beyond them.
 * ksh_kss_index_routes reports KSH_QROUTE_PAIR_SPLIT (as for ksh_kss_pair_counts) and KSH_QROUTE_CLASS_SPILL for the
 * last call.  The index must be usable as for ksh_kss_index_query. */
int ksh_kss_color_classes(const int32_t* cols, int32_t n_cols, ksh_kss_index* idx, int64_t capacity, uint64_t* rows,
                          int64_t* counts, int64_t* n_classes);

/* ---- The colour class of every selected k-mer: a coloured-graph export ---------------------------------------
 * ksh_kss_select_keys with, beside every key, the position of the k-mer's row in a class table: the union selection
 * with the whole table of ksh_kss_color_classes over the same cols is what a coloured de Bruijn graph stores, the
 * k-mers and one small integer per k-mer that indexes the table.
 * sel, idx, d_offsets, n_keys, d_keys: as in ksh_kss_select_keys -- the offsets are those ksh_kss_select_count made
 * for the same request and index, bucket b goes to d_keys[d_offsets[b] .. d_offsets[b + 1]) ascending in the index's
 * key width, nothing is written at or beyond n_keys nor outside a bucket's own range, and a bucket that does not
 * match its offsets gives KSH_FAILED_PRECONDITION after the call's one synchronisation.  d_keys may be NULL: only the
 * ids are written.
 * rows: a HOST class table of n_classes rows, uint64[2 * n_classes], 1 <= n_classes <= 2^24, in the format and order
 * ksh_kss_color_classes returns for the same cols: rows[2 c] = the bits of columns 0..63, rows[2 c + 1] = the bits of
 * columns 64..127, strictly ascending by (rows[2 c + 1], rows[2 c]).  It is only read during the call.  It may be the
 * whole table or any strictly ascending subset of it -- only the one-bit classes, say, to label private k-mers by
 * sample.
 * d_class_ids (device, uint32[n_keys]): d_class_ids[p] is the class of the key written (or, with d_keys NULL, that
 * would be written) at d_keys[p]: the c with rows[2 c], rows[2 c + 1] equal to that k-mer's row over sel->cols, or
 * KSH_CLASS_NONE if the table does not hold the row.
 * n_unmatched (host) says what a row that the table does not hold means.  NULL: any selected k-mer with such a row
 * makes the call KSH_FAILED_PRECONDITION with a message that names rows and gives the number of such k-mers -- the
 * table belongs to another request or index; the outputs are then unspecified within [0, n_keys).  Non-NULL: it
 * receives that number and the call is KSH_OK.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  Before the index is dereferenced: what
 * ksh_kss_select_keys refuses there (but for a NULL d_keys); NULL rows; n_classes outside [1, 2^24]; NULL d_class_ids
 * with n_keys > 0; rows that are not strictly ascending (the message gives the first offending index).  After reading
 * only the index's host fields: what ksh_kss_select_keys refuses there; a row with a bit at or above n_cols.  The
 * index still serves after any refusal.
 * The call is stateless like its siblings: scratch comes from the context's pool (16 bytes per node, 16 bytes per
 * class, 32 bytes per slot of a table of the next power of two >= 2 * n_classes slots) and is given back before the
 * call returns; it synchronises the index's context stream once; it keeps no plan, joins no plan group and ends no
 * pending plan.  ksh_kss_index_routes reports KSH_QROUTE_PAIR_SPLIT for the last call with the meaning it has for
 * ksh_kss_pair_counts.  The index must be usable as for ksh_kss_index_query. */
#define KSH_CLASS_NONE 0xFFFFFFFFu
int ksh_kss_select_class_ids(const ksh_kss_selection* sel, ksh_kss_index* idx, const uint64_t* rows,
                             int64_t n_classes, const int64_t* d_offsets, int64_t n_keys, void* d_keys,
                             uint32_t* d_class_ids, int64_t* n_unmatched);

/* ---- Painting sequences with colour classes: runs of equal class per sequence ----------------------------------
 * Which stretch of a contig, a read or a reference genome is held by which exact subset of the chosen sets.  Sequences
 * and positions are those of ksh_seq_hits: sequence s has positions 0 .. lens[s], no window crosses from one string
 * into the next.  The row of a position has bit a set iff its k-mer (canonicalised if asked) is in Get(cols[a]); a
 * k-mer that no node holds has the zero row, and so has one that only nodes outside cols hold.  The class of a
 * position is the c whose rows[2 c], rows[2 c + 1] equal its row, or KSH_CLASS_NONE if the table does not hold the
 * row.  A run is a maximal stretch of consecutive positions of one sequence with the same class: adjacent runs of a
 * sequence differ in class, a run never continues from one sequence into the next (even when the classes agree), and
 * every sequence has at least one run, so n_runs >= n_strings.  Painting the strings of ksh_spss_encode of the union
 * selection with the whole table of ksh_kss_color_classes gives the compact colouring of a coloured de Bruijn graph:
 * one class per run of positions, not one per k-mer (DESIGN.md 3.8g has the measured ratio).
 * Everything a ksh_seq_paint points to is HOST memory and only read during the call. */
typedef struct ksh_seq_paint {
  size_t struct_size;          /* sizeof(ksh_seq_paint) of the caller's header */
  const int32_t* cols;         /* as ksh_kss_color_classes: 1..128 distinct node ids, any order, internal nodes
                                  allowed; NULL = all nodes in order (n_cols ignored), refused above 128 nodes */
  int32_t n_cols;
  int32_t canonicalize;        /* as ksh_seq_hits */
  const uint64_t* rows;        /* class table, as ksh_kss_select_class_ids: uint64[2 * n_classes], strictly */
  int64_t n_classes;           /* ascending by (rows[2c+1], rows[2c]), 1..2^24, whole table or any subset of it */
  int32_t route;               /* as ksh_seq_hits: 0 auto, 1 search, 2 join */
  int64_t pass_positions;      /* as ksh_seq_hits: 0 = default */
} ksh_seq_paint;
/* *n_runs (host, required): the number of runs of all sequences -- always the true number, also on the capacity
 * refusal below.
 * d_run_offsets (device int64[n_strings + 1], may be NULL): the runs of sequence s are runs off[s] .. off[s + 1);
 * off[n_strings] == n_runs.
 * d_run_start, d_run_class (device uint32[capacity]): run r of sequence s begins at position d_run_start[r] of s (the
 * first run of a sequence at 0), has class d_run_class[r], and ends before the next run of s begins, or at
 * lens[s] + 1.  capacity == 0: count only, the two arrays may be NULL and are not touched.  capacity > 0: both are
 * required.  n_runs > capacity > 0: KSH_FAILED_PRECONDITION with a message that names capacity and gives n_runs; the
 * first capacity entries are then unspecified.  Nothing is ever written at or beyond capacity, whatever the inputs.
 * n_unmatched (host) counts the POSITIONS with KSH_CLASS_NONE, and is as in ksh_kss_select_class_ids.  NULL: any such
 * position makes the call KSH_FAILED_PRECONDITION with a message that names rows and gives their number.  Non-NULL: it
 * receives the number and the call is KSH_OK.
 * n_strings == 0: KSH_OK, *n_runs = 0, d_run_offsets[0] = 0 if given, *n_unmatched = 0 if given.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  Before the index is dereferenced: NULL seqs, idx,
 * req or n_runs; struct_size smaller than the struct; what ksh_seq_hits refuses about sizes, route and
 * pass_positions; what ksh_kss_select_class_ids refuses about rows and n_classes (NULL, out of range, not strictly
 * ascending, with the first offending index); n_cols outside [1, 128] with non-NULL cols; a negative capacity; a NULL
 * d_run_start or d_run_class with capacity > 0.  After reading only the index's host fields: an id outside
 * [0, n_nodes); a repeated id; NULL cols on an index of more than 128 nodes; a row with a bit at or above n_cols;
 * K < 4.  On the device, before the words are read: lens[s] == UINT32_MAX, sum(lens + K) != n_bases.  The index still
 * serves after any refusal.
 * pass_positions: as in ksh_seq_hits, with 12 + 8 W bytes of scratch per position (the k-mer, the class, the row); the
 * default keeps that within 256 MiB and a pass within the join's 2^24 queries.  The result does not depend on it.
 * The call is stateless like its siblings: scratch comes from the context's pool (that of a pass, 8 bytes per
 * sequence, 16 bytes per class and 32 bytes per slot of a table of the next power of two >= 2 * n_classes slots) and
 * is given back before the call returns; it keeps no plan, joins no plan group and ends no pending plan.  It
 * synchronises the index's context stream once for the size check, once per pass on the join route, and once at the
 * end.  ksh_kss_index_routes reports SEARCH / JOIN / OVERSIZE / CHUNKED / SEQ_PASSES as for ksh_seq_hits.  As there,
 * the sequences come first and the index second.  The index must be usable as for ksh_kss_index_query.
 * Timing kinds (ksh_ctx_enable_timing): 6 = the extraction and look-up of a pass, 7 = its classification and runs. */
int ksh_seq_class_runs(const ksh_spss_view* seqs, ksh_kss_index* idx, const ksh_seq_paint* req,
                       int64_t capacity, int64_t* d_run_offsets, uint32_t* d_run_start, uint32_t* d_run_class,
                       int64_t* n_runs, int64_t* n_unmatched);

/* ---- Cutting the strings of a container at runs: coloured unitigs ------------------------------------------------
 * The strings of an SPSS container cut at given k-mer positions, the K - 1 bases behind every cut repeated: the
 * k-mers of the output strings in order are the k-mers of the input strings in order, so the k-mer set is unchanged.
 * Cut at the runs that ksh_seq_class_runs gives for the strings of ksh_spss_encode of the union selection, every output
 * string is monochromatic -- all its k-mers have one colour class, d_run_class[r] is the class of string r -- which is
 * the form coloured-graph tools exchange (coloured unitigs and the class table beside them).  Any run list can drive
 * the call, not only a painting.
 * Input string s has P_s = lens[s] + 1 positions; pstart is the exclusive scan of P_s, and string s begins at base
 * pstart[s] + s (K - 1) of the stream.  The run list is d_run_offsets (device int64[n_strings + 1]) and d_run_start
 * (device uint32[n_runs]) exactly as ksh_seq_class_runs writes them: run r belongs to string s when off[s] <= r <
 * off[s + 1], and covers positions a = start[r] up to e, e = start[r + 1] if r + 1 < off[s + 1], otherwise P_s.
 * Output: a container of n_runs strings.  String r is bases [a, e + K - 1) of input string s, and d_lens[r] =
 * e - a - 1.  Every cut repeats K - 1 bases: n_bases_out = n_bases + (n_runs - n_strings)(K - 1), which the caller
 * computes to size d_words (ceil(n_bases_out / 32) words) -- there is no plan call; d_lens holds n_runs entries.
 * Nothing is written outside these two ranges, whatever the inputs.  With q_r = pstart[s] + a, output string r begins
 * at output base q_r + r (K - 1), and its bases are the input bases at the same index minus (r - s)(K - 1).  The bits
 * behind base n_bases_out - 1 of the last word are unspecified, as in every container.  *n_bases (host, may be NULL)
 * receives n_bases_out.
 * n_strings == 0 requires n_runs == 0: KSH_OK, *n_bases = 0, nothing is read or written on the device.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  On the host: NULL seqs, ctx, g or (with strings)
 * arrays; negative sizes; n_runs < n_strings; a geometry no call accepts; K < 4.  On the device, by one check kernel
 * and one synchronisation before any output word or length is written, naming the first offending string or run:
 * off[0] != 0; off[n_strings] != n_runs; off[s] >= off[s + 1]; start[off[s]] != 0; starts not strictly ascending
 * within a string; a start >= P_s; and what ksh_seq_hits refuses of the container, lens[s] == UINT32_MAX and
 * sum(lens + K) != n_bases.  The context still serves after any refusal.
 * The call is stateless like the sequence queries: scratch comes from the context's pool (8 bytes per string, 8 bytes
 * per run) and is given back before the call returns; it keeps no plan, joins no plan group and ends no pending plan.
 * It synchronises the context's stream twice: for the checks and at the end.  As with ksh_seq_hits the sequences come
 * first and the context second. */
int ksh_spss_cut(const ksh_spss_view* seqs, ksh_ctx* ctx, const ksh_geom* g, const int64_t* d_run_offsets,
                 const uint32_t* d_run_start, int64_t n_runs, uint64_t* d_words, uint32_t* d_lens, int64_t* n_bases);

/* ---- The links between the strings of a container: the edges of the graph -----------------------------------------
 * The strings of an SPSS container as the nodes of a graph, and its edges (GFA: S lines, and L lines with a (K-1)M
 * overlap).  The container has n strings over ACGT whose k-mers are all distinct.
 * The oriented string v = 2 s + o is string s as written (o = 0) or its reverse complement (o = 1); first(v) and
 * last(v) are its first and last k-mer, first(2 s + 1) = rc(last(2 s)).
 * canonical != 0: for each base b of ACGT in this order let y = last(v)[1:] + b.  If canon(y) == canon(last(v)) the
 * base is skipped; otherwise v -> w is a link iff first(w) == y.  canonical == 0: only the vertices with o = 0 exist,
 * a base is skipped when y == last(v), and the rows 2 s + 1 are empty.
 * Skipped, then, is a k-mer followed by itself: the one-k-mer loop AAAAA -> AAAAA and the hairpin x -> rc(x) of a K - 1
 * overlap that is its own reverse complement (the unitig walk of ksh_spss_encode ignores both as well).  A circular
 * string of two or more k-mers does link to itself (v -> v).
 * Output, in CSR form: d_link_offsets (device int64[2 n + 1], may be NULL; written whenever given) and d_link_to
 * (device int64[capacity]): the links of v are entries off[v] .. off[v + 1) of d_link_to, ascending by b.  A base
 * reaches at most one w, so a row has at most 4 entries and n_links <= 8 n.  In canonical mode v -> w iff
 * w ^ 1 -> v ^ 1: both twins are listed.
 * ONLY STRING ENDS ARE LOOKED AT: an extension that lands inside a string is no link.  When the strings are the
 * unitigs of their k-mer set (ksh_spss_encode, mode 1) or any cut of them (ksh_spss_cut), the k-mer pairs
 * (last(v), first(w)) of the links together with the consecutive k-mer pairs inside the oriented strings are exactly
 * the edges x -> y with canon(x) != canon(y) of the set's node-centric de Bruijn graph, and the two parts are
 * disjoint.  For other containers -- a mode-0 path cover, say -- the links are the edges between string ends only.
 * *n_links (host, required) is always the true number.  capacity == 0 counts only: d_link_to may be NULL and is not
 * touched.  n_links > capacity > 0: KSH_FAILED_PRECONDITION with a message that names capacity and gives n_links;
 * d_link_to is then untouched (the offsets, if given, are whole).  Nothing is ever written at or beyond capacity, or
 * beyond 2 n + 1 offsets.
 * n_strings == 0: KSH_OK, *n_links = 0, d_link_offsets[0] = 0 if given; nothing else touches the device.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  On the host: NULL seqs, ctx, g or n_links;
 * negative sizes, NULL words or lens with strings; a geometry no call accepts; K < 4; a negative capacity; a NULL
 * d_link_to with capacity > 0.  On the device, before any output element is written, naming the smallest offending
 * string: what ksh_seq_hits refuses of the container, lens[s] == UINT32_MAX and sum(lens + K) != n_bases (before the
 * words are read); two string ends with the same end k-mer (after canonicalisation in canonical mode) -- the two ends
 * of a one-k-mer string are one end and are fine, a longer string whose first and last k-mer coincide is refused; in
 * canonical mode an end k-mer that is its own reverse complement (even K only; ksh_spss_encode refuses such sets
 * too).  The context still serves after any refusal.
 * The call is stateless like ksh_spss_cut: scratch comes from the context's pool (40 bytes per string, and 16 bytes
 * per slot of an end table of the next power of two >= 4 n slots) and is given back before the call returns; it keeps
 * no plan, joins no plan group and ends no pending plan.  It synchronises the context's stream three times: for the
 * container's sizes, for the end check and the count, and at the end.  A row is a function of the container alone.
 * As with ksh_spss_cut the sequences come first and the context second. */
int ksh_spss_links(const ksh_spss_view* seqs, ksh_ctx* ctx, const ksh_geom* g, int canonical, int64_t capacity,
                   int64_t* d_link_offsets, int64_t* d_link_to, int64_t* n_links);

/* ---- The bubbles of a link graph: variant sites and the sets on each arm -------------------------------------------
 * The input is the link graph as ksh_spss_links writes it in CANONICAL mode: n strings, 2 n oriented strings
 * v = 2 s + o, d_link_offsets[2 n + 1], d_link_to[n_links], rows of at most four distinct targets, twin-symmetric
 * (v -> w iff w ^ 1 -> v ^ 1).  out(v) is the row of v and outdeg(v) its length; indeg(v) := outdeg(v ^ 1), by twin
 * symmetry the number of links into v.
 * The walk of arm i (i = 0, 1, in row order) from a source v with outdeg(v) == 2:
 *     x = out(v)[i]; arm = []
 *     loop:
 *       if indeg(x) != 1 or outdeg(x) != 1 or len(arm) == max_arm: the arm fails
 *       arm.append(x)
 *       x = out(x)[0]
 *       if indeg(x) == 2: sink_i = x; stop
 * A next x with indeg 1 is met again at the top of the loop; any other indeg makes the arm fail there.
 * v is the source of a bubble (v, w, arm_0, arm_1) iff both arms succeed and sink_0 == sink_1 =: w.  The definition
 * imposes nothing else: w may branch on (outdeg(w) is free; bubbles back to back share a node), w may be v ^ 1 (a
 * hairpin bubble), and a ring of one-in one-out strings ends at max_arm.  The two arms cannot merge before the sink:
 * their first strings differ, because row entries are distinct, and every arm string has indeg 1.
 * Every bubble has a twin: source w ^ 1, sink v ^ 1, arms reversed and flipped.  A bubble is reported iff
 * v <= w ^ 1, so once.  The output ascends by v; a source has at most one bubble, so that is a total order.  Arm 0 is
 * the arm of the lower base, which is row order.
 * With classes (d_string_class[n] the class of each string, rows the class table, 128 bits a class) the carriers of
 * an arm are the AND of rows[d_string_class[x >> 1]] over its strings: the sets that hold every k-mer of the allele.
 * A SET THAT HOLDS ONLY PART OF AN ARM IS NOT A CARRIER.
 * The arms are chains because ksh_spss_cut cuts unitigs wherever the class changes: an arm that a partly covering set
 * enters or leaves is several strings, each with one link in and one out.  Nested and multi-allelic sites (a source
 * of outdeg 3, a bubble inside an arm of another) are no bubbles of this definition.
 * The result is a function of the graph alone.
 * Outputs: bubble b has source d_bubble_ends[2 b] and sink d_bubble_ends[2 b + 1]; its arm i is entries
 * d_arm_offsets[2 b + i] .. d_arm_offsets[2 b + i + 1] of d_arm_strings, oriented strings in walk order; the
 * carriers of that arm are the two words d_arm_rows[2 (2 b + i)], [.. + 1].
 * *n_bubbles and *n_arm_strings (host, required) are always the true numbers.  capacity == 0 counts only: the output
 * pointers may be NULL and nothing is written.  capacity > 0 with n_bubbles > capacity or n_arm_strings >
 * arm_capacity: KSH_FAILED_PRECONDITION with a message that names the capacity and gives the number; all four
 * outputs stay untouched.  Nothing is ever written at or beyond a capacity (2 capacity ends, 2 capacity + 1 offsets,
 * arm_capacity strings, 4 capacity row words).  No bubbles with capacity > 0: d_arm_offsets[0] = 0.
 * n_strings == 0: KSH_OK, both counts 0, d_arm_offsets[0] = 0 with capacity > 0; nothing else touches the device.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  On the host: NULL graph, ctx, n_bubbles or
 * n_arm_strings; a struct_size smaller than the struct; negative sizes; NULL offsets with strings; NULL d_link_to
 * with n_links > 0; n_links > 8 n; max_arm outside [1, KSH_BUBBLE_MAX_ARM]; a negative capacity; with capacity > 0 a
 * NULL d_bubble_ends or d_arm_offsets, a NULL d_arm_strings with arm_capacity > 0; exactly one of d_string_class /
 * rows; with classes n_classes outside [1, 2^24]; d_arm_rows given without classes, or missing with classes when
 * capacity > 0.  On the device, before any walk and before any output element is written, each kind with its smallest
 * offending vertex or link, the offsets first: off[0] != 0; off[2 n] != n_links; off[v] > off[v + 1]; a row longer
 * than 4; a target outside [0, 2 n); a repeated target in a row; a link v -> w whose twin w ^ 1 -> v ^ 1 is missing
 * (so the links of ksh_spss_links in non-canonical mode are refused as soon as there is one: canonical links are what
 * the call takes); a class outside [0, n_classes).  The arrays are the caller's: no kernel reads outside them
 * whatever they contain, and a malformed graph ends in a refusal.  The context still serves after any refusal.
 * Stateless like ksh_spss_links: scratch comes from the context's pool (50 bytes per string, 16 bytes per class) and
 * goes back before the call returns; it keeps no plan, joins no plan group and ends no pending plan.  At most three
 * synchronisations: the check, the counts, the end.  The graph comes first and the context second. */
#define KSH_BUBBLE_MAX_ARM 64

typedef struct ksh_link_graph {
  size_t struct_size;
  int64_t n_strings;             /* n; the CSR has 2 n rows */
  const int64_t* d_link_offsets; /* device int64[2 n + 1] */
  const int64_t* d_link_to;      /* device int64[n_links] */
  int64_t n_links;
  const int32_t* d_string_class; /* device int32[n], or NULL */
  const uint64_t* rows;          /* HOST uint64[2 * n_classes] as ksh_seq_paint, or NULL; both or neither */
  int64_t n_classes;
} ksh_link_graph;

int ksh_link_bubbles(const ksh_link_graph* graph, ksh_ctx* ctx, int32_t max_arm, int64_t capacity,
                     int64_t arm_capacity, int64_t* d_bubble_ends, int64_t* d_arm_offsets, int64_t* d_arm_strings,
                     uint64_t* d_arm_rows, int64_t* n_bubbles, int64_t* n_arm_strings);

/* ---- Where the string ends of one container occur in another: the graph placed on a reference ----------------------
 * Two containers: n strings, whose 2 n ends are located, and a reference of m sequences, whose k-mers may repeat.
 * End e = 2 s is the first k-mer of string s as written, e = 2 s + 1 its last; for a one-k-mer string both ends are
 * the same k-mer.  Ends need not be distinct, within a string or between strings: unitigs, cut unitigs and reads are
 * all taken.
 * The reference's k-mer positions are numbered in one line, as for ksh_seq_hits: sequence r owns the global positions
 * pstart[r] .. pstart[r + 1), pstart being the exclusive scan of lens + 1, and a window never crosses from one
 * sequence into the next.  A position with k-mer x matches an end k-mer y when x == y (strand 0) or, with
 * canonical != 0 only, x == rc(y) (strand 1).  A k-mer that is its own reverse complement (even K) reads strand 0.
 * d_count[e] is the number of matching positions; d_where[e] is (g << 1) | strand of the matching position with the
 * smallest global index g, -1 when there is none.  The host turns g into (sequence, position) with pstart.
 * *n_located (host, may be NULL) is the number of ends with d_count[e] >= 1.
 * The result is a function of the two containers alone.  Nothing is written outside [0, 2 n) of either output.
 * n_strings == 0 of `strings`: KSH_OK, *n_located = 0, nothing is written and the device is not touched.  A reference
 * of no sequences: -1 and 0 everywhere.  A reference of 2^32 k-mer positions or more is refused, so d_count is exact.
 * KSH_INVALID_ARGUMENT, each with a message that names the field.  On the host: NULL req, ctx, g or strings; a
 * struct_size smaller than the struct; negative sizes of either view; a geometry no call accepts; K < 4; with strings
 * a NULL reference, NULL words or lens of a container that has sequences, a NULL d_where or d_count.  On the device,
 * before any output element is written, naming the container and the first offending string: what ksh_seq_hits
 * refuses, lens[s] == UINT32_MAX and sum(lens + K) != n_bases, of the strings first and of the reference second (each
 * before that container's words are read).  The context still serves after any refusal.
 * The call is stateless like ksh_spss_links: scratch comes from the context's pool (24 bytes per string, 8 bytes per
 * reference sequence, and 20 bytes per slot of an end table of the next power of two >= 4 n slots) and is given back
 * before the call returns; it keeps no plan, joins no plan group and ends no pending plan.  It synchronises the
 * context's stream three times: for the sizes of the strings, for those of the reference, and at the end (twice when
 * the reference has no sequences).
 * The request is the only parameter: the context is a field of it. */
typedef struct ksh_seq_locate_req {
  size_t struct_size;
  ksh_ctx* ctx;
  const ksh_geom* g;
  const ksh_spss_view* strings;   /* n strings: their 2 n ends are located   */
  const ksh_spss_view* reference; /* m sequences; k-mers may repeat          */
  int32_t canonical;
  int64_t* d_where;               /* device int64[2 n]                       */
  uint32_t* d_count;              /* device uint32[2 n]                      */
  int64_t* n_located;             /* host, may be NULL: ends with count >= 1 */
} ksh_seq_locate_req;

int ksh_seq_locate(const ksh_seq_locate_req* req);

#ifdef __cplusplus
}
#endif

#endif /* KMERSETS_HIP_H_ */
