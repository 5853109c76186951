// Stand-alone check of csrc/ksh_layout.h (tests/test_layout_cpu.py compiles it with the address and undefined-
// behaviour sanitizers and reads what it prints): a handful of mixed layouts, each run on a measuring carver and
// on a real block.  One line per run ("layout <name> <mode> <extent> <block bytes>") and one per array
// ("take <name> <mode> <offset or -1 for null> <bytes the array needs>").  Every array handed out is filled, so
// that an array past its block's end stops the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "ksh_layout.h"

using ksh::Carver;

struct Wide {  // a 16-byte element
  uint64_t a, b;
};

struct Run {
  const char* name;
  const char* mode;
  char* base;
  template <typename T>
  void note(T* p, size_t count) {
    const long long off = p ? (long long)(reinterpret_cast<char*>(p) - base) : -1;
    std::printf("take %s %s %lld %zu\n", name, mode, off, count * sizeof(T));
    if (p) std::memset(p, 0xA5, count * sizeof(T));
  }
};

template <typename T>
void take(Carver& c, Run& r, size_t count) {
  r.note(c.take<T>(count), count);
}
template <typename T>
void take_if(Carver& c, Run& r, bool used, size_t count) {
  r.note(c.take_if<T>(used, count), count);
}

using Layout = std::function<void(Carver&, Run&)>;

static void run(const char* name, const Layout& layout) {
  Run measuring{name, "measure", nullptr};
  const size_t bytes = ksh::layout_bytes([&](Carver& c) { layout(c, measuring); });
  std::printf("layout %s measure %zu %zu\n", name, bytes, bytes);
  char* block = static_cast<char*>(std::aligned_alloc(256, ksh::round256(bytes ? bytes : 1)));
  Run binding{name, "bind", block};
  Carver c(block);
  layout(c, binding);
  std::printf("layout %s bind %zu %zu\n", name, c.bytes(), bytes);
  const bool fits = ksh::layout_bind(block, bytes, [&](Carver& k) { Run quiet{name, "rebind", block}; layout(k, quiet); });
  const bool tight = bytes == 0 || !ksh::layout_bind(block, bytes - 1, [&](Carver& k) { Run quiet{name, "rebind", block}; layout(k, quiet); });
  const bool null_refused = !ksh::layout_bind(nullptr, bytes, [&](Carver&) {});
  std::printf("bind %s %d %d %d\n", name, int(fits), int(tight), int(null_refused));
  std::free(block);
}

int main() {
  std::printf("round %zu %zu %zu %zu %zu\n", ksh::round256(0), ksh::round256(1), ksh::round256(255), ksh::round256(256),
              ksh::round256(257));
  run("every-width", [](Carver& c, Run& r) {
    take<uint8_t>(c, r, 1);
    take<uint16_t>(c, r, 3);
    take<uint32_t>(c, r, 0);
    take<uint64_t>(c, r, 1);
    take<Wide>(c, r, 5);
  });
  for (const bool used : {false, true})
    run(used ? "sometimes-used" : "sometimes-unused", [used](Carver& c, Run& r) {
      take<uint32_t>(c, r, 1000);
      c.pad(4096);
      take<uint64_t>(c, r, 77);
      take_if<uint32_t>(c, r, used, 10);
      take<uint16_t>(c, r, 1);
    });
  run("all-empty", [](Carver& c, Run& r) {
    take<uint8_t>(c, r, 0);
    take<uint64_t>(c, r, 0);
  });
  run("odd-pad", [](Carver& c, Run& r) {
    take<Wide>(c, r, 1);
    take<uint8_t>(c, r, 257);
    c.pad(24);  // (not a multiple of the alignment: the next array still starts on one)
    take<uint16_t>(c, r, 129);
    take<uint64_t>(c, r, 33);
    c.pad(4096);
  });
  return 0;
}
