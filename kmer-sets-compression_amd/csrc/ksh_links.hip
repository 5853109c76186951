// The links between the strings of an SPSS container (ksh_spss_links): the edges of the graph whose
// nodes the strings are, in CSR form over the 2 n oriented strings.  The oriented string v = 2 s + o is string s as
// written (o = 0) or its reverse complement (o = 1); v -> w is a link when the last k-mer of v, moved on by one base,
// is the first k-mer of w.  A k-mer followed by itself (the move gives the k-mer again, in canonical mode also its
// reverse complement) is no link.  Only string ends are looked at: a move that lands inside a string is no link.
//   ends   : k_link_ends, a thread a string: its first and last k-mer as written (seq_ends), into ends[2 s],
//            ends[2 s + 1], and both into the end table under their key (the k-mer, in canonical mode its canonical
//            form).  A one-k-mer string has one end and one entry.
//   table  : open addressing, the next power of two >= 4 n slots of a key word and an owner word, each set once by
//            atomicCAS from 0.  An owner that finds another owner under its key is a duplicate end, reported by
//            atomicMin as k_cut_check does.  Nobody waits for a value; the table is read by later kernels only.
//   count  : k_link_rows<false>, a thread an oriented string: its four candidates looked up, the hits counted.
//   fill   : after the repository's scan of the counts, k_link_rows<true> looks them up again and writes the targets.
// An entry's owner word is ((s + 1) << 3) | single << 2 | last << 1 | flipped, flipped saying that the key is the
// reverse complement of the k-mer as written.  A candidate y with key c and flip f (y != c) meets the entry of c:
//   a first end : y is that k-mer as written iff f == flipped: the link goes to 2 s.  Otherwise y is the reverse
//                 complement of a first k-mer, which begins no oriented string of two or more k-mers.
//   a last end  : y is the reverse complement of the last k-mer iff f != flipped: the link goes to 2 s + 1.
//   single      : both, told apart the same way: 2 s + (f != flipped).
// Every end has a key of its own (anything else is refused), so the entry a look-up finds is a function of the
// container alone, whatever the order of insertion, the table's size or the grid.
#include "ksh_clstable.h"
#include "ksh_seq.h"

using ksh::pc::PoolBuf;
using ksh::pc::pool_array;

namespace {

constexpr int kLinkThreads = 256;
// What k_link_ends reports, a word each: the smallest offending string, ~0 if none.
enum { kBadDup = 0, kBadPalin, kBadNoSlot, kBadCount, kBadLens = 4 };
enum : unsigned long long { kOwnFlip = 1, kOwnLast = 2, kOwnSingle = 4 };

}  // namespace

namespace ksh {

__device__ __forceinline__ uint64_t link_slot(uint64_t key, uint64_t mask) { return pc::pc_mix(key) & mask; }

// The end `x` (as written) of string s into the table: its key claimed or found, its owner word set if nobody's is.
__device__ __forceinline__ void link_insert(unsigned long long* __restrict__ tab, uint64_t mask, uint64_t x, int k,
                                            int canon, int64_t s, unsigned long long kind,
                                            unsigned long long* __restrict__ bad) {
  uint64_t key = x;
  unsigned long long own = (static_cast<unsigned long long>(s + 1) << 3) | kind;
  if (canon) {
    const uint64_t r = revcomp(x, k);
    if (r == x) atomicMin(&bad[kBadPalin], static_cast<unsigned long long>(s));
    if (r < x) {
      key = r;
      own |= kOwnFlip;
    }
  }
  const unsigned long long kw = key | kValid;
  uint64_t h = link_slot(key, mask);
  for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    unsigned long long* slot = tab + 2 * h;
    const unsigned long long prev = atomicCAS(slot, 0ull, kw);
    if (prev != 0 && prev != kw) continue;
    const unsigned long long other = atomicCAS(slot + 1, 0ull, own);
    if (other != 0) {  // another end under this key (that of this very string too: it is inserted once)
      const unsigned long long t = (other >> 3) - 1;
      atomicMin(&bad[kBadDup], min(t, static_cast<unsigned long long>(s)));
    }
    return;
  }
  atomicMin(&bad[kBadNoSlot], static_cast<unsigned long long>(s));  // (cannot happen: at most half load)
}

__global__ __launch_bounds__(kLinkThreads) void k_link_ends(const uint64_t* __restrict__ words,
                                                            const uint32_t* __restrict__ lens,
                                                            const int64_t* __restrict__ pstart, int64_t n_strings,
                                                            int k, int canon, uint64_t* __restrict__ ends,
                                                            unsigned long long* __restrict__ tab, uint64_t mask,
                                                            unsigned long long* __restrict__ bad) {
  const int64_t s = int64_t(blockIdx.x) * kLinkThreads + threadIdx.x;
  if (s >= n_strings) return;
  uint64_t first, last;
  const bool single = seq_ends(words, lens, pstart, s, k, &first, &last);
  ends[2 * s] = first;
  ends[2 * s + 1] = last;
  if (single) {
    link_insert(tab, mask, first, k, canon, s, kOwnSingle, bad);
  } else {
    link_insert(tab, mask, first, k, canon, s, 0, bad);
    link_insert(tab, mask, last, k, canon, s, kOwnLast, bad);
  }
}

// The owner word under `key` in the finished table, 0 if the key has no slot.  Plain loads, the probe order of
// link_insert: a key's slot lies between its hash and the first empty slot behind it.  The owner word is loaded
// inside the loop, by the lane that has just matched: as "find the slot, then load its owner word" the load came to
// stand behind the loop, where a lane waits for the wave's last lane to end its probe, and k_link_rows took 152.6
// instead of 123.5 us to count and 169.5 instead of 140.7 us to fill (782 939 strings, 2^22 slots, MI355X).
__device__ __forceinline__ unsigned long long link_find(const unsigned long long* __restrict__ tab, uint64_t mask,
                                                        uint64_t key) {
  const unsigned long long kw = key | kValid;
  uint64_t h = link_slot(key, mask);
  for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    const unsigned long long got = tab[2 * h];
    if (got == 0) return 0;
    if (got == kw) return tab[2 * h + 1];
  }
  return 0;
}

// The links of oriented string v, ascending by the appended base: counted (kWrite false: cnt[v]) or written from
// off[v] on (kWrite true).  In non-canonical mode the rows 2 s + 1 are empty.
template <bool kWrite>
__global__ __launch_bounds__(kLinkThreads) void k_link_rows(const uint64_t* __restrict__ ends, int64_t n_oriented,
                                                            int k, int canon,
                                                            const unsigned long long* __restrict__ tab, uint64_t mask,
                                                            int64_t* __restrict__ cnt,
                                                            const int64_t* __restrict__ off,
                                                            int64_t* __restrict__ link_to) {
  const int64_t v = int64_t(blockIdx.x) * kLinkThreads + threadIdx.x;
  if (v >= n_oriented) return;
  int found = 0;
  if (canon || !(v & 1)) {
    const uint64_t x = (v & 1) ? revcomp(ends[v - 1], k) : ends[v + 1];  // last(v)
    const uint64_t xc = canon ? canonical(x, k) : x;
    int64_t at = kWrite ? off[v] : 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint64_t y = kmer_next(x, k, c);
      uint64_t key = y;
      unsigned long long flip = 0;
      if (canon) {
        const uint64_t r = revcomp(y, k);
        if (r < y) {
          key = r;
          flip = kOwnFlip;
        }
      }
      if (key == xc) continue;  // a k-mer followed by itself
      const unsigned long long own = link_find(tab, mask, key);
      if (own == 0) continue;
      const bool as_written = ((own ^ flip) & kOwnFlip) == 0;  // y is the entry's k-mer as written
      int64_t w;
      if (own & kOwnSingle) {
        w = as_written ? 0 : 1;
      } else if (own & kOwnLast) {
        if (as_written) continue;  // y is a last k-mer as written: it begins no oriented string
        w = 1;
      } else {
        if (!as_written) continue;
        w = 0;
      }
      if (kWrite) link_to[at++] = 2 * int64_t((own >> 3) - 1) + w;
      found++;
    }
  }
  if (!kWrite) cnt[v] = found;
}

}  // namespace ksh

using namespace ksh;

extern "C" int ksh_spss_links(const ksh_spss_view* seqs, ksh_ctx* ctx, const ksh_geom* g, int canonical,
                              int64_t capacity, int64_t* d_link_offsets, int64_t* d_link_to, int64_t* n_links) {
  if (!seqs) return fail(KSH_INVALID_ARGUMENT, "seqs is NULL");
  if (!ctx) return fail(KSH_INVALID_ARGUMENT, "ctx is NULL");
  if (!g) return fail(KSH_INVALID_ARGUMENT, "g is NULL");
  if (!n_links) return fail(KSH_INVALID_ARGUMENT, "n_links is NULL");
  KSH_TRY(check_geom(g));
  KSH_TRY(seq_check_request(seqs, 0, 0));
  const int k = g->k;
  KSH_TRY(seq_check_k(k, ""));
  if (capacity < 0) return fail(KSH_INVALID_ARGUMENT, "capacity = %lld is negative", (long long)capacity);
  if (capacity > 0 && !d_link_to)
    return fail(KSH_INVALID_ARGUMENT, "d_link_to is NULL with capacity = %lld", (long long)capacity);
  const int64_t n = seqs->n_strings;
  if (n == 0) {
    KSH_TRY(seq_check_empty(seqs, ""));
    if (d_link_offsets) {  // (the one word the call writes: there before it returns, as after every other return)
      KSH_HIP(hipSetDevice(ctx->device));
      KSH_HIP(hipMemsetAsync(d_link_offsets, 0, 8, ctx->stream));
      KSH_HIP(hipStreamSynchronize(ctx->stream));
    }
    *n_links = 0;
    return KSH_OK;
  }
  KSH_HIP(hipSetDevice(ctx->device));
  const int canon = canonical ? 1 : 0;

  // 1. the container's own sizes, before anything reads its words (the first synchronisation)
  uint64_t slots = 1;
  while (slots < 4 * uint64_t(n)) slots <<= 1;
  PoolBuf pstart_buf(ctx), bad_buf(ctx), ends_buf(ctx), tab_buf(ctx), off_buf(ctx);
  int64_t *pstart, *off;
  unsigned long long *bad, *tab;
  uint64_t* ends;
  KSH_TRY(pool_array(ctx, size_t(n + 1), &pstart_buf, &pstart));
  KSH_TRY(pool_array(ctx, 8, &bad_buf, &bad));
  KSH_TRY(pool_array(ctx, size_t(2 * n), &ends_buf, &ends));
  KSH_TRY(pool_array(ctx, size_t(slots) * 2, &tab_buf, &tab));  // (a key word and an owner word per slot)
  KSH_TRY(pool_array(ctx, size_t(2 * n + 1), &off_buf, &off));
  int64_t total = 0;  // k-mer positions in all
  KSH_TRY(seq_positions(ctx, seqs, k, pstart, bad + kBadLens, &total));

  // 2. the ends into the table, the links counted and scanned: into scratch only (the second synchronisation)
  const int64_t n_oriented = 2 * n;
  const dim3 grid_strings(unsigned((n + kLinkThreads - 1) / kLinkThreads));
  const dim3 grid_oriented(unsigned((n_oriented + kLinkThreads - 1) / kLinkThreads));
  KSH_HIP(hipMemsetAsync(bad, 0xFF, kBadCount * 8, ctx->stream));
  KSH_HIP(hipMemsetAsync(tab, 0, size_t(slots) * 16, ctx->stream));
  hipLaunchKernelGGL(k_link_ends, grid_strings, dim3(kLinkThreads), 0, ctx->stream, seqs->d_words, seqs->d_lens, pstart,
                     n, k, canon, ends, tab, slots - 1, bad);
  hipLaunchKernelGGL(k_link_rows<false>, grid_oriented, dim3(kLinkThreads), 0, ctx->stream, ends, n_oriented, k, canon,
                     tab, slots - 1, off, static_cast<const int64_t*>(nullptr), static_cast<int64_t*>(nullptr));
  KSH_HIP(hipGetLastError());
  KSH_TRY(arena_reserve(ctx, scan_scratch_bytes(n_oriented)));
  arena_reset(ctx);
  KSH_TRY(scan_exclusive_i64(ctx, off, off, n_oriented, off + n_oriented));
  int64_t* h = ctx->h_pinned + 8;
  KSH_HIP(hipMemcpyAsync(h, bad, kBadCount * 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipMemcpyAsync(h + kBadCount, off + n_oriented, 8, hipMemcpyDeviceToHost, ctx->stream));
  KSH_HIP(hipStreamSynchronize(ctx->stream));
  if (h[kBadNoSlot] != -1) return fail(KSH_INTERNAL, "ksh_spss_links: an end found no slot in the end table");
  if (h[kBadPalin] != -1)
    return fail(KSH_INVALID_ARGUMENT, "seqs: an end k-mer of string %lld is its own reverse complement (canonical "
                                      "mode, even K)", (long long)h[kBadPalin]);
  if (h[kBadDup] != -1)
    return fail(KSH_INVALID_ARGUMENT, "seqs: an end k-mer of string %lld is the end k-mer of another end%s: the "
                                      "k-mers of a container are distinct", (long long)h[kBadDup],
                canon ? " (after canonicalisation)" : "");
  const int64_t links = h[kBadCount];  // (the word behind the reports)
  *n_links = links;

  // 3. the offsets, and the targets if they fit (the third synchronisation)
  if (d_link_offsets)
    KSH_HIP(hipMemcpyAsync(d_link_offsets, off, size_t(n_oriented + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
  const bool fits = capacity > 0 && links <= capacity;
  if (fits && links > 0) {
    hipLaunchKernelGGL(k_link_rows<true>, grid_oriented, dim3(kLinkThreads), 0, ctx->stream, ends, n_oriented, k, canon,
                       tab, slots - 1, static_cast<int64_t*>(nullptr), off, d_link_to);
    KSH_HIP(hipGetLastError());
  }
  KSH_HIP(hipStreamSynchronize(ctx->stream));  // (the scratch goes back to the pool: nothing of the call is in flight)
  if (capacity > 0 && !fits)
    return fail(KSH_FAILED_PRECONDITION, "ksh_spss_links: capacity = %lld but n_links = %lld: d_link_to is untouched "
                                         "(capacity = 0 counts the links first)", (long long)capacity,
                (long long)links);
  return KSH_OK;
}
