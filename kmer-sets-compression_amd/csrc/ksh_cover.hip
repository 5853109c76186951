// Path cover from caller-supplied unitigs: ksh_spss_cover_plan / ksh_spss_cover_write.
//
// GetSPSSCanonical(unitigs, prefixes, suffixes, fast, ...) and GetSPSS(unitigs, prefixes, ...)
// (lib/core/spss.h:697-1014, :1039-1829): the strings of a ksh_spss_view are the nodes, in the order
// given.  The encode finds its unitigs in a k-mer set and builds their edge table from the set
// (k_edges); here the edge table comes from the strings' end k-mers alone, then the encode's
// unitig-level stage runs unchanged (cover_stage in ksh_encode.hip: matching, loop cut, walks,
// stitch order), and the output is spelled from the caller's packed bases.
//
//   k_cover_sizes  bases per string (lens + K), for the scan of the strings' base offsets
//   k_cover_ends   first and last k-mer of every string; an open-addressing table of the ends, filled by
//                  64-bit atomicCAS (a CAS that meets the same key from another string is a duplicate end);
//                  the preconditions: a violation a string commits alone is recorded with the smallest such index,
//                  a duplicate end with one of the strings that share the k-mer (whichever lost the CAS)
//   k_cover_edges  <= 4 neighbours per side by looking up the candidates of the end (spss.h:1039-1206):
//                  the edge table in exactly the layout k_edges writes
//   k_cover_emit   every input base, reverse-complemented when its unitig is traversed flipped, to its place in
//                  its string, one byte per base, balanced over the input stream (the encode's k_pack makes the words)
#include "ksh_internal.h"
#include "ksh_kmer.h"

namespace ksh {

namespace {

constexpr uint32_t kNoString = 0xFFFFFFFFu;
constexpr unsigned long long kEmptyKey = ~0ull;  // no k-mer (K <= 31) has all 64 bits set

__device__ __forceinline__ uint64_t hash_key(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// The K bases at base position p of a 2-bit stream (ksh_spss_view layout: base j at the bits
// [63 - 2 (j % 32), 62 - 2 (j % 32)] of word j / 32).  The caller guarantees p + K <= n_bases.
__device__ __forceinline__ uint64_t kmer_at(const uint64_t* __restrict__ words, int64_t p, int k, int64_t n_words) {
  const int64_t w = p >> 5;
  const int off = int(p & 31);
  uint64_t x = words[w] << (2 * off);
  if (off + k > 32 && w + 1 < n_words) x |= words[w + 1] >> (64 - 2 * off);
  return x >> (64 - 2 * k);
}

__device__ __forceinline__ void table_insert(unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                             uint64_t cap_mask, uint64_t key, uint32_t i,
                                             unsigned long long* __restrict__ dup) {
  uint64_t h = hash_key(key) & cap_mask;
  for (uint64_t probe = 0; probe <= cap_mask; probe++) {
    const unsigned long long prev = atomicCAS(&keys[h], kEmptyKey, (unsigned long long)key);
    if (prev == kEmptyKey) {
      vals[h] = i;
      return;
    }
    if (prev == key) {
      atomicMin(dup, (unsigned long long)i);
      return;
    }
    h = (h + 1) & cap_mask;
  }
}

// (called in a later kernel than every insert: the values are all written)
__device__ __forceinline__ uint32_t table_find(const unsigned long long* __restrict__ keys,
                                               const uint32_t* __restrict__ vals, uint64_t cap_mask, uint64_t key) {
  uint64_t h = hash_key(key) & cap_mask;
  for (uint64_t probe = 0; probe <= cap_mask; probe++) {
    const unsigned long long at = keys[h];
    if (at == key) return vals[h];
    if (at == kEmptyKey) return kNoString;
    h = (h + 1) & cap_mask;
  }
  return kNoString;
}

__global__ __launch_bounds__(256) void k_cover_sizes(const uint32_t* __restrict__ lens, int64_t n, int k,
                                                     int64_t* __restrict__ sizes) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) sizes[i] = int64_t(lens[i]) + k;
}

// err[kCoverErr*]: a string index that violates the precondition (~0: none) -- the smallest one for the palindrome
// and same-ends checks; for the duplicates the smallest among the strings whose insert met the key already there,
// and which of the strings that share a k-mer gets there first is a race.  The strings' base offsets
// must add up to the view's n_bases before anything is read (a view whose lens say otherwise reads nothing).
__global__ __launch_bounds__(256) void k_cover_ends(const uint64_t* __restrict__ words, int64_t n_words,
                                                    const uint32_t* __restrict__ lens,
                                                    const int64_t* __restrict__ in_start, const int64_t* __restrict__ total,
                                                    int64_t n, int64_t n_bases, int k, bool directed,
                                                    uint64_t* __restrict__ first, uint64_t* __restrict__ last,
                                                    unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                    uint64_t cap_mask, unsigned long long* __restrict__ err) {
  const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (*total != n_bases) {
    if (i == 0) atomicMin(&err[kCoverErrBases], 0ull);
    return;
  }
  const uint64_t p = kmer_at(words, in_start[i], k, n_words);
  const uint64_t s = kmer_at(words, in_start[i] + lens[i], k, n_words);
  first[i] = p;
  last[i] = s;
  if (directed) {  // two tables: first k-mers, then last k-mers
    table_insert(keys, vals, cap_mask, p, uint32_t(i), &err[kCoverErrDupFirst]);
    table_insert(keys + cap_mask + 1, vals + cap_mask + 1, cap_mask, s, uint32_t(i), &err[kCoverErrDupLast]);
    return;
  }
  const uint64_t rp = revcomp(p, k), rs = revcomp(s, k);
  if (p == rp || s == rs) {  // (even K only)
    atomicMin(&err[kCoverErrPalindrome], (unsigned long long)i);
    return;
  }
  const uint64_t cp = p < rp ? p : rp, cs = s < rs ? s : rs;
  if (cp == cs) {
    if (lens[i] != 0) {
      atomicMin(&err[kCoverErrSameEnds], (unsigned long long)i);
      return;
    }
    table_insert(keys, vals, cap_mask, cp, uint32_t(i), &err[kCoverErrDupEnd]);  // a K-long string: one end k-mer
    return;
  }
  table_insert(keys, vals, cap_mask, cp, uint32_t(i), &err[kCoverErrDupEnd]);
  table_insert(keys, vals, cap_mask, cs, uint32_t(i), &err[kCoverErrDupEnd]);
}

// vertex v = 2u + side (0 = left end, 1 = right end); edges[4v + c] = other vertex or kNoString (k_edges' layout).
// canonical (ko_spss.h edges_right / edges_left, spss.h:1039-1206): the right side of u meets j where
// P_j == Next(S_u, c) (j's left side) or S_j == rc(Next(S_u, c)) (j's right side); the left side where
// S_j == Prev(P_u, c) (right side) or P_j == rc(Prev(P_u, c)) (left side); j != u.  Under the preconditions a
// candidate's canonical form is the end of at most one string and at most one of the two tests holds.
// directed (spss.h:706-726): the right side meets the first k-mers Next(S_u, c), the left side the last k-mers
// Prev(P_u, c).
__global__ __launch_bounds__(256) void k_cover_edges(const uint64_t* __restrict__ first, const uint64_t* __restrict__ last,
                                                     const uint32_t* __restrict__ lens, int64_t n_vertices, int k,
                                                     bool directed, const unsigned long long* __restrict__ keys,
                                                     const uint32_t* __restrict__ vals, uint64_t cap_mask,
                                                     uint32_t* __restrict__ u_len, uint32_t* __restrict__ edges,
                                                     uint32_t* __restrict__ mate) {
  const int64_t v = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n_vertices) return;
  const uint32_t u = uint32_t(v >> 1), side = uint32_t(v & 1);
  mate[v] = kNoString;
  if (!side) u_len[u] = lens[u] + 1;
  uint32_t out[4] = {kNoString, kNoString, kNoString, kNoString};
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const uint64_t y = side ? kmer_next(last[u], k, c) : kmer_prev(first[u], k, c);
    if (directed) {
      const uint32_t j = side ? table_find(keys, vals, cap_mask, y)
                              : table_find(keys + cap_mask + 1, vals + cap_mask + 1, cap_mask, y);
      if (j != kNoString && j != u) out[c] = 2 * j + (side ? 0u : 1u);
      continue;
    }
    const uint64_t r = revcomp(y, k);
    const uint32_t j = table_find(keys, vals, cap_mask, y < r ? y : r);
    if (j == kNoString || j == u) continue;
    // right side: y as is is j's first k-mer (left side), its rc j's last (right side); left side: mirrored
    if (side) {
      if (first[j] == y) out[c] = 2 * j;
      else if (last[j] == r) out[c] = 2 * j + 1;
    } else {
      if (last[j] == y) out[c] = 2 * j + 1;
      else if (first[j] == r) out[c] = 2 * j;
    }
  }
  *reinterpret_cast<uint4*>(edges + 4 * v) = make_uint4(out[0], out[1], out[2], out[3]);
}

// One thread per kCoverEmitRun consecutive bases of the INPUT stream (unitigs of any length, balanced): the thread
// finds its unitig by a binary search over the input offsets, then every base at source offset s of unitig u goes
// to traversal position t = s (or len + K - 2 - s when u is flipped, complemented) of its place in the output,
// str_start[sid] + koff + t; a unitig after the first of its string leaves out t < K - 1 (they are the last K - 1
// bases of the one before it, ko_spss.h string_from_path), so every byte is written exactly once.
constexpr int kCoverEmitRun = 4;
__global__ __launch_bounds__(256) void k_cover_emit(const uint64_t* __restrict__ words, int64_t n_in_bases,
                                                    const int64_t* __restrict__ in_start,
                                                    const uint32_t* __restrict__ u_len, const uint32_t* __restrict__ u_sid,
                                                    const uint32_t* __restrict__ u_koff, const uint8_t* __restrict__ u_flip,
                                                    const int64_t* __restrict__ str_start, int64_t n_u, int k,
                                                    int64_t n_bases, uint8_t* __restrict__ bytes) {
  const int64_t q0 = (int64_t(blockIdx.x) * blockDim.x + threadIdx.x) * kCoverEmitRun;
  if (q0 >= n_in_bases) return;
  int64_t lo = 0, hi = n_u - 1;  // the last unitig u with in_start[u] <= q0
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (in_start[mid] <= q0) lo = mid; else hi = mid - 1;
  }
  int64_t u = lo;
  int64_t u0 = in_start[u], u1 = u + 1 < n_u ? in_start[u + 1] : n_in_bases;
  for (int j = 0; j < kCoverEmitRun; j++) {
    const int64_t q = q0 + j;
    if (q >= n_in_bases) return;
    while (q >= u1) {
      u++;
      u0 = u1;
      u1 = u + 1 < n_u ? in_start[u + 1] : n_in_bases;
    }
    const int64_t nb = int64_t(u_len[u]) + k - 1;
    const bool flip = u_flip[u] != 0;
    const int64_t t = flip ? nb - 1 - (q - u0) : q - u0;
    if (u_koff[u] && t < k - 1) continue;
    uint32_t b = uint32_t(words[q >> 5] >> (62 - 2 * (q & 31))) & 3u;
    if (flip) b = 3u - b;
    const int64_t at = str_start[u_sid[u]] + u_koff[u] + t;
    if (at < n_bases) bytes[at] = uint8_t(b);
  }
}

}  // namespace

void cover_launch_sizes(hipStream_t st, const uint32_t* lens, int64_t n, int k, int64_t* sizes) {
  hipLaunchKernelGGL(k_cover_sizes, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, lens, n, k, sizes);
}

void cover_launch_ends(hipStream_t st, const ksh_spss_view* in, const int64_t* in_start, const int64_t* total,
                       int k, bool directed, uint64_t* first, uint64_t* last, unsigned long long* keys,
                       uint32_t* vals, uint64_t cap, unsigned long long* err) {
  const int64_t n = in->n_strings;
  hipLaunchKernelGGL(k_cover_ends, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, in->d_words,
                     (in->n_bases + 31) / 32, in->d_lens, in_start, total, n, in->n_bases, k, directed, first, last,
                     keys, vals, cap - 1, err);
}

void cover_launch_edges(hipStream_t st, const uint64_t* first, const uint64_t* last, const uint32_t* lens, int64_t n,
                        int k, bool directed, const unsigned long long* keys, const uint32_t* vals, uint64_t cap,
                        uint32_t* u_len, uint32_t* edges, uint32_t* mate) {
  hipLaunchKernelGGL(k_cover_edges, dim3(unsigned((2 * n + 255) / 256)), dim3(256), 0, st, first, last, lens, 2 * n,
                     k, directed, keys, vals, cap - 1, u_len, edges, mate);
}

void cover_launch_emit(hipStream_t st, const ksh_spss_view* in, const int64_t* in_start, const uint32_t* u_len,
                       const uint32_t* u_sid, const uint32_t* u_koff, const uint8_t* u_flip, const int64_t* str_start,
                       int k, int64_t n_bases, uint8_t* bytes) {
  const int64_t threads = (in->n_bases + kCoverEmitRun - 1) / kCoverEmitRun;
  hipLaunchKernelGGL(k_cover_emit, dim3(unsigned((threads + 255) / 256)), dim3(256), 0, st, in->d_words, in->n_bases,
                     in_start, u_len, u_sid, u_koff, u_flip, str_start, in->n_strings, k, n_bases, bytes);
}

}  // namespace ksh
