// The open-addressing table of 128-bit rows that ksh_kss_color_classes (ksh_classes.hip) counts classes in and
// ksh_kss_select_class_ids (ksh_classids.hip) looks class ids up in.  gfx950 only.
//
// A slot is three set-once key words and a 64-bit word.  Word i of slot s is base[s * kStride + i * kPlane]:
// i = 0, 1, 2 the key, i = 3 the count (for the class ids: the id + 1 of a row that is inserted once).
#ifndef KSH_CLSTABLE_H_
#define KSH_CLSTABLE_H_

#include "ksh_rowtile.h"

namespace ksh {

constexpr unsigned long long kValid = 1ull << 63;  // set in every written key word: 0 is "not yet written"

__device__ __forceinline__ uint32_t cls_hash(uint64_t r0, uint64_t r1) {
  return uint32_t(pc::pc_mix(r0 ^ pc::pc_mix(r1 + 0x9E3779B97F4A7C15ull)));
}

// Adds cnt to the slot of row (r0, r1), taking an empty slot if the row has none.  At 128 columns every 128-bit
// value is a row, so no row word has a value to spare for "empty" and there is no 128-bit compare-and-swap: the key
// is three words that carry 63 bits of r0, 63 bits of r1 and the two top bits, each with kValid set, each written
// once, by atomicCAS from 0.  A thread claims word 0; if it was 0 or is its own it claims word 1 the same way, then
// word 2; on any other value it goes to the next slot.
//   - Whoever writes word i of a slot goes on to word i + 1 of it, and had matched the words before i: so every
//     slot whose word 0 is written ends with all three written, and they are the key of the thread that wrote (or
//     first matched) word 2 -- the key of a row that was inserted, which then adds its count: no slot stays half
//     written or with a zero count once the inserting threads are done.
//   - A thread leaves a slot only on a word that holds another value, and words never change once written: two
//     threads with the same row decide alike at every slot and settle on the same one.  A row has one slot.
//   - Nobody waits for a value: a wave's lanes may insert side by side, in lockstep.
// The loop visits every slot at most once.  Returns false when each held another row.  *claims grows by the
// slots whose word 0 this call wrote: each is some row's new slot (not necessarily this row's).
template <int kStride, int kPlane>
__device__ __forceinline__ bool cls_insert(unsigned long long* base, uint32_t mask, uint64_t r0, uint64_t r1,
                                           unsigned long long cnt, int* claims) {
  const unsigned long long w0 = (r0 & ~kValid) | kValid, w1 = (r1 & ~kValid) | kValid;
  const unsigned long long w2 = (r0 >> 63) | ((r1 >> 63) << 1) | kValid;
  uint32_t h = cls_hash(r0, r1) & mask;
  for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    unsigned long long* s = base + size_t(h) * kStride;
    unsigned long long prev = atomicCAS(s, 0ull, w0);
    if (prev != 0 && prev != w0) continue;
    if (prev == 0) *claims += 1;
    prev = atomicCAS(s + kPlane, 0ull, w1);
    if (prev != 0 && prev != w1) continue;
    prev = atomicCAS(s + 2 * kPlane, 0ull, w2);
    if (prev != 0 && prev != w2) continue;
    atomicAdd(s + 3 * kPlane, cnt);
    return true;
  }
  return false;
}

// The count word of the slot of row (r0, r1) in a table that nobody inserts into any more (the kernel that filled
// it has ended), 0 if the row has no slot.  Plain loads only, the probe order of cls_insert: a row's slot lies
// between its hash and the first empty slot behind it, since cls_insert passes over a slot only when another row
// holds it, and a finished table has no half-written slot.  The loop visits every slot at most once; no lane waits
// for another.
template <int kStride, int kPlane>
__device__ __forceinline__ unsigned long long cls_find(const unsigned long long* __restrict__ base, uint32_t mask,
                                                       uint64_t r0, uint64_t r1) {
  const unsigned long long w0 = (r0 & ~kValid) | kValid, w1 = (r1 & ~kValid) | kValid;
  const unsigned long long w2 = (r0 >> 63) | ((r1 >> 63) << 1) | kValid;
  uint32_t h = cls_hash(r0, r1) & mask;
  for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
    const unsigned long long* s = base + size_t(h) * kStride;
    const unsigned long long k0 = s[0];
    if (k0 == 0) return 0;
    if (k0 == w0 && s[kPlane] == w1 && s[2 * kPlane] == w2) return s[3 * kPlane];
  }
  return 0;
}

__device__ __forceinline__ unsigned long long cls_peek(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The class table of a caller (ksh_kss_select_class_ids, ksh_seq_class_runs): rows as ksh_kss_color_classes returns
// them, looked up on the device by cls_find<4, 1>, whose word is the row's position + 1.  ksh_classids.hip.
constexpr int64_t kMaxClasses = int64_t(1) << 24;
// Host checks that need no index: rows not NULL and n_classes in [1, kMaxClasses]; the rows strictly ascending by
// (rows[2 c + 1], rows[2 c]), with the first offending index in the message.
int class_table_check_size(const uint64_t* rows, int64_t n_classes);
int class_table_check_order(const uint64_t* rows, int64_t n_classes);
// ... and one that needs the number of columns: no row has a bit at or above n_cols.
int class_table_check_cols(const uint64_t* rows, int64_t n_classes, int n_cols);
// Uploads the rows (up: 16 bytes per class) and inserts row c with the word c + 1 into a zeroed table of *slots =
// the next power of two >= 2 * n_classes slots of 32 bytes (tab), all from the context's pool and on its stream.
// *d_noslot (device, zeroed by the caller) counts the rows that found no slot (cannot happen: at most half load).
int class_table_build(ksh_ctx* ctx, const uint64_t* rows, int64_t n_classes, pc::PoolBuf* tab, pc::PoolBuf* up,
                      unsigned long long* d_noslot, int64_t* slots);

}  // namespace ksh

#endif
