// Host-side tests of the mirror at 2^16 .. 2^22 buckets: KmerSetCompact::ToKmerSet, KmerCounter, the KmerSetSet
// constructor, Dump / Load and KmerSetSetReader::Get all decode, and above N = 14 the decode takes its wide route
// (ksh_decode.hip).  Needs a GPU: everything runs through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <filesystem>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "core/kmer.h"
#include "core/kmer_counter.h"
#include "core/kmer_set.h"
#include "core/kmer_set_compact.h"
#include "core/kmer_set_set.h"
#include "core/random.h"

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
static std::uint64_t Rand() { return ksc::Mix64(0x3D1E0000 + g_ctr++); }

static std::string RandomGenome(int length) {
  std::string g;
  for (int i = 0; i < length; i++) g += "ACGT"[Rand() % 4];
  return g;
}

template <int K>
static std::set<std::uint64_t> CanonicalKmers(const std::string& s) {
  std::set<std::uint64_t> out;
  for (int j = 0; j + K <= static_cast<int>(s.size()); j++) out.insert(Kmer<K>(s.substr(j, K)).Canonical().Bits());
  return out;
}

// A correlated family: one random genome, point substitutions per member.
template <int K, int N, typename KeyType>
static std::vector<KmerSet<K, N, KeyType>> Family(int n_sets, int length) {
  const std::string genome = RandomGenome(length);
  std::vector<KmerSet<K, N, KeyType>> out;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    const auto kmers = CanonicalKmers<K>(g);
    out.push_back(KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end())));
  }
  return out;
}

template <int K, int N, typename KeyType>
static void TestCompactRoundTrip(const KmerSet<K, N, KeyType>& s) {
  using Compact = KmerSetCompact<K, N, KeyType>;
  const Compact c = Compact::FromKmerSet(s, true, true, 4);
  const auto back = c.ToKmerSet(true, 4);
  EXPECT_EQ(back.Size(), s.Size());
  EXPECT_EQ(back.Hash(4), s.Hash(4));
  EXPECT_TRUE(back.Equals(s, 4));
  // a hand-written SPSS with repeated k-mers decodes to the same set
  std::vector<std::string> strings = c.ToStrings(4);
  strings.push_back(strings[0]);
  strings.push_back(strings[0].substr(0, K + 2));
  EXPECT_TRUE(Compact::FromStrings(strings).ToKmerSet(true, 4).Equals(s, 4));
  const std::string file = (std::filesystem::temp_directory_path() / "ksc_test_wide.txt").string();
  EXPECT_TRUE(c.Dump(file, "", 4).ok());
  auto loaded = Compact::Load(file, "");
  EXPECT_TRUE(loaded.ok());
  if (loaded.ok()) EXPECT_TRUE(loaded.value().ToKmerSet(true, 4).Equals(s, 4));
  std::filesystem::remove(file);
}

template <int K, int N, typename KeyType>
static void TestCounter() {
  using Counter = KmerCounter<K, N, KeyType, std::uint8_t>;
  const std::string genome = RandomGenome(3000);
  std::vector<std::string> reads;
  for (int r = 0; r < 150; r++) reads.push_back(genome.substr(Rand() % (genome.size() - 100), 100));
  std::map<std::uint64_t, int> count;
  for (const std::string& read : reads)
    for (int j = 0; j + K <= static_cast<int>(read.size()); j++) count[Kmer<K>(read.substr(j, K)).Canonical().Bits()]++;
  const Counter c = Counter::FromReads(reads, true, 4);
  EXPECT_EQ(c.Size(), static_cast<std::int64_t>(count.size()));
  for (int cutoff : {1, 3}) {
    std::vector<std::uint64_t> want;
    std::int64_t below = 0;
    for (const auto& kv : count) {
      if (kv.second >= cutoff) want.push_back(kv.first);
      else below++;
    }
    auto r = c.ToKmerSet(cutoff, 4);
    EXPECT_EQ(r.second, below);
    EXPECT_TRUE(r.first.Equals(KmerSet<K, N, KeyType>::FromSortedBits(want), 4));
  }
}

template <int K, int N, typename KeyType>
static void TestSetSet(int n_sets, int length) {
  auto sets = Family<K, N, KeyType>(n_sets, length);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  EXPECT_TRUE(kss.Size() >= n_sets);
  for (int i = 0; i < n_sets; i++) EXPECT_TRUE(kss.Get(i, true, 4).Equals(sets[i], 4));
  const std::string dir = (std::filesystem::temp_directory_path() / "ksc_test_wide_kss").string();
  std::filesystem::remove_all(dir);
  EXPECT_TRUE(kss.Dump(dir, "", "txt", 4).ok());
  auto loaded = KmerSetSet<K, N, KeyType>::Load(dir, "", "txt", 4);
  EXPECT_TRUE(loaded.ok());
  if (loaded.ok()) {
    EXPECT_EQ(loaded.value().Size(), kss.Size());
    for (int i = 0; i < n_sets; i++) EXPECT_TRUE(loaded.value().Get(i, true, 4).Equals(sets[i], 4));
  }
  auto reader = KmerSetSetReader<K, N, KeyType>::FromDirectory(dir, "txt", "", true);
  EXPECT_TRUE(reader.ok());
  if (reader.ok())
    for (int i = 0; i < n_sets; i++) {
      auto got = reader.value().Get(i, 4);
      EXPECT_TRUE(got.ok());
      if (got.ok()) EXPECT_TRUE(got.value().Equals(sets[i], 4));
    }
  std::filesystem::remove_all(dir);
  std::printf("  KmerSetSet<%d,%d>: %d -> %d nodes\n", K, N, n_sets, kss.Size());
}

template <int K, int N, typename KeyType>
static void TestGeometry(int n_sets, int length) {
  const auto sets = Family<K, N, KeyType>(1, 30000);
  TestCompactRoundTrip(sets[0]);
  TestCounter<K, N, KeyType>();
  TestSetSet<K, N, KeyType>(n_sets, length);
}

int main() {
  try {
    TestGeometry<23, 16, std::uint32_t>(6, 20000);
    TestGeometry<31, 20, std::uint64_t>(4, 20000);
    TestGeometry<19, 22, std::uint16_t>(4, 8000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
