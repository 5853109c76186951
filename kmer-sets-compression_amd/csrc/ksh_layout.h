// How a block of device scratch is laid out: one list of arrays per block, run twice.  A stage writes a function
// that takes a Carver and fills its pointer struct; run on a measuring Carver it gives the bytes to reserve, run on
// the reserved block it gives the pointers -- by the same calls, so the two cannot disagree.  Host only, no HIP.
#ifndef KSH_LAYOUT_H_
#define KSH_LAYOUT_H_

#include <cstddef>

namespace ksh {

// every array of a block starts on a multiple of this (the blocks themselves come from hipMalloc or arena_alloc)
inline size_t round256(size_t x) { return (x + 255) & ~size_t(255); }

class Carver {
 public:
  Carver() = default;                                              // measures: every take() returns nullptr
  explicit Carver(void* base) : base_(static_cast<char*>(base)) {}  // hands out pointers into the block at `base`

  // `count` elements of T, 256-aligned.  *capacity (optional): the bytes the array owns, its rounding included --
  // what a stage that borrows the array for something else may use.
  template <typename T>
  T* take(size_t count, size_t* capacity = nullptr) {
    at_ = round256(at_);
    T* p = base_ ? reinterpret_cast<T*>(base_ + at_) : nullptr;
    const size_t bytes = round256(count * sizeof(T));
    at_ += bytes;
    if (capacity) *capacity = bytes;
    return p;
  }
  // An array that only some plans use: its room is counted either way (the block's size must not depend on the
  // condition), the pointer is null when it is not used.
  template <typename T>
  T* take_if(bool used, size_t count) {
    T* p = take<T>(count);
    return used ? p : nullptr;
  }
  // Room that no array owns: allowances that the hand-written sums carried and that a kernel may lean on.
  void pad(size_t bytes) { at_ += bytes; }
  size_t bytes() const { return at_; }

 private:
  char* base_ = nullptr;
  size_t at_ = 0;
};

// The bytes of a layout: `layout(Carver&)` run on a measuring carver.
template <typename Layout>
size_t layout_bytes(Layout&& layout) {
  Carver c;
  layout(c);
  return c.bytes();
}

// Binds a layout to its block; false when the block is missing or the list takes more than `reserved`.
template <typename Layout>
bool layout_bind(void* base, size_t reserved, Layout&& layout) {
  if (!base) return false;
  Carver c(base);
  layout(c);
  return c.bytes() <= reserved;
}

}  // namespace ksh

#endif
