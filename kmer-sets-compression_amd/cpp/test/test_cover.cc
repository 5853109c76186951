// Host-side tests of the mirror's path cover from caller-supplied unitigs: GetPrefixesFromUnitigs,
// GetSuffixesFromUnitigs and the unitig overloads of GetSPSS / GetSPSSCanonical (lib/core/spss.h:619-1829), on
// reference-style random sets (test/spss.cc:99-153).  Needs a GPU: the covers run through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "core/kmer.h"
#include "core/kmer_set.h"
#include "core/random.h"
#include "core/spss.h"

static int g_failed = 0, g_checks = 0;
#define EXPECT_TRUE(x)                                                        \
  do {                                                                        \
    g_checks++;                                                               \
    if (!(x)) {                                                               \
      g_failed++;                                                             \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);     \
    }                                                                         \
  } while (0)
#define EXPECT_EQ(a, b) EXPECT_TRUE((a) == (b))

static std::uint64_t g_ctr = 0;
static std::uint64_t Rand() { return ksc::Mix64(0xC0FE0000 + g_ctr++); }

// reads of random k-mers, half of them doubled (a loop), as in the reference's GetRandomKmerSet
template <int K>
std::string RandomRead() {
  std::string s;
  const int n = 1 + int(Rand() % 100);
  for (int j = 0; j < n; j++) s += Kmer<K>(Rand() & (~std::uint64_t(0) >> (64 - 2 * K))).String();
  if (Rand() % 2 == 0) s += s;
  return s;
}

template <int K, int N, typename KeyType>
KmerSet<K, N, KeyType> RandomKmerSet(int n, bool canonical) {
  std::set<std::uint64_t> kmers;
  while (static_cast<int>(kmers.size()) < n) {
    const std::string s = RandomRead<K>();
    for (int j = 0; j + K <= static_cast<int>(s.size()) && static_cast<int>(kmers.size()) < n; j++) {
      Kmer<K> kmer(s.substr(j, K));
      if (canonical) kmer = kmer.Canonical();
      kmers.insert(kmer.Bits());
    }
  }
  return KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end()));
}

// The maps hold, for every unitig i in ascending order, its first (last) k-mer -> i, and nothing else.
template <int K>
static void CheckEndMap(const std::unordered_map<Kmer<K>, std::vector<std::int64_t>>& m,
                        const std::vector<std::string>& unitigs, bool last) {
  std::size_t entries = 0;
  bool ok = true;
  for (const auto& kv : m) {
    entries += kv.second.size();
    for (std::size_t j = 0; j < kv.second.size(); j++) {
      const std::int64_t i = kv.second[j];
      if (i < 0 || i >= static_cast<std::int64_t>(unitigs.size())) {
        ok = false;
        continue;
      }
      const std::string& u = unitigs[static_cast<std::size_t>(i)];
      if (!(Kmer<K>(last ? u.substr(u.length() - K, K) : u.substr(0, K)) == kv.first)) ok = false;
      if (j > 0 && kv.second[j - 1] >= i) ok = false;
    }
  }
  EXPECT_TRUE(ok);
  EXPECT_EQ(entries, unitigs.size());
}

template <int K, int N, typename KeyType>
static void TestCover(int size) {
  auto s = RandomKmerSet<K, N, KeyType>(size, true);
  const std::vector<std::string> unitigs = GetUnitigsCanonical(s, 1);
  const auto prefixes = GetPrefixesFromUnitigs<K>(unitigs, 1);
  const auto suffixes = GetSuffixesFromUnitigs<K>(unitigs, 1);
  CheckEndMap<K>(prefixes, unitigs, false);
  CheckEndMap<K>(suffixes, unitigs, true);
  EXPECT_EQ(prefixes.size(), unitigs.size());  // every k-mer once: the ends are distinct
  for (bool fast : {true, false}) {
    const auto from_unitigs = GetSPSSCanonical<K, N, KeyType>(unitigs, prefixes, suffixes, fast, 1);
    EXPECT_TRUE(from_unitigs == GetSPSSCanonical(s, fast, 1));
  }
  auto f = RandomKmerSet<K, N, KeyType>(size, false);
  const std::vector<std::string> fu = GetUnitigs(f, 1);
  const auto fp = GetPrefixesFromUnitigs<K>(fu, 1);
  CheckEndMap<K>(fp, fu, false);
  EXPECT_TRUE((GetSPSS<K, N, KeyType>(fu, fp, 1) == GetSPSS(f, 1)));
}

int main() {
  try {
    {  // the maps of hand-made unitigs: a shared first k-mer lists both unitigs, in order
      const std::vector<std::string> u = {"ACGTAC", "ACGTTT", "GGACG"};
      const auto p = GetPrefixesFromUnitigs<4>(u, 1);
      const auto q = GetSuffixesFromUnitigs<4>(u, 1);
      EXPECT_EQ(p.size(), 2u);
      EXPECT_TRUE((p.at(Kmer<4>(std::string("ACGT"))) == std::vector<std::int64_t>{0, 1}));
      EXPECT_TRUE((p.at(Kmer<4>(std::string("GGAC"))) == std::vector<std::int64_t>{2}));
      EXPECT_EQ(q.size(), 3u);
      EXPECT_TRUE((q.at(Kmer<4>(std::string("GTTT"))) == std::vector<std::int64_t>{1}));
      EXPECT_EQ(std::hash<Kmer<4>>()(Kmer<4>(std::string("ACGT"))), Kmer<4>(std::string("ACGT")).Hash());
    }
    for (int size : {1, 300, 20000, 65536}) TestCover<9, 10, std::uint8_t>(size);
    TestCover<15, 14, std::uint16_t>(30000);
    TestCover<31, 14, std::uint64_t>(30000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
