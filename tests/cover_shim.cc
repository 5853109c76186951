// Test-side entry points into the oracle's path cover from unitigs (oracle/ko_spss.h) that its C API does not
// export: GetSPSSCanonical(unitigs, ..., fast = false) and GetSPSS(unitigs, ...) on strings in any order.
// Compiled with g++ into a temporary directory by tests/test_spss_cover_cpu.py and tests/test_gpu_spss_cover.py.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ko_spss.h"

static thread_local std::vector<std::string> g_out;

// variant 0: canonical, fast; 1: canonical, fast = false; 2: non-canonical.  Returns the number of strings.
extern "C" int64_t cover_shim_run(const char* chars, const int64_t* lens, int64_t n, int k, int variant) {
  std::vector<std::string> u;
  u.reserve(static_cast<std::size_t>(n));
  int64_t at = 0;
  for (int64_t i = 0; i < n; i++) {
    u.emplace_back(chars + at, static_cast<std::size_t>(lens[i]));
    at += lens[i];
  }
  if (variant == 2)
    g_out = ko::spss_directed_from_unitigs(u, ko::prefixes_from_unitigs(u, k), k);
  else
    g_out = ko::spss_canonical_from_unitigs(u, ko::prefixes_from_unitigs(u, k), ko::suffixes_from_unitigs(u, k), k,
                                            variant == 0);
  return static_cast<int64_t>(g_out.size());
}

extern "C" int64_t cover_shim_total() {
  int64_t t = 0;
  for (const auto& s : g_out) t += static_cast<int64_t>(s.size());
  return t;
}

extern "C" void cover_shim_get(char* chars, int64_t* lens) {
  int64_t at = 0;
  for (std::size_t i = 0; i < g_out.size(); i++) {
    std::memcpy(chars + at, g_out[i].data(), g_out[i].size());
    lens[i] = static_cast<int64_t>(g_out[i].size());
    at += lens[i];
  }
}
