// Host-side tests of the mirror's KmerSetSetIndex: on a constructed and on a Dumped-then-Loaded KmerSetSet, bit i
// of every query's row equals Get(i).Contains(kmer) for every node i.  Needs a GPU: everything runs through
// libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <filesystem>
#include <set>
#include <string>
#include <vector>

#include "core/kmer.h"
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
static std::uint64_t Rand() { return ksc::Mix64(0x1DE40000 + g_ctr++); }

static std::string RandomGenome(int length) {
  std::string g;
  for (int i = 0; i < length; i++) g += "ACGT"[Rand() % 4];
  return g;
}

// A correlated family: one random genome, point substitutions per member; also returns the genomes.
template <int K, int N, typename KeyType>
static std::vector<KmerSet<K, N, KeyType>> Family(int n_sets, int length, std::vector<std::string>* genomes) {
  const std::string genome = RandomGenome(length);
  std::vector<KmerSet<K, N, KeyType>> out;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    std::set<std::uint64_t> kmers;
    for (int j = 0; j + K <= length; j++) kmers.insert(Kmer<K>(g.substr(j, K)).Canonical().Bits());
    out.push_back(KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end())));
    genomes->push_back(g);
  }
  return out;
}

template <int K, int N, typename KeyType>
static void CheckIndex(const KmerSetSet<K, N, KeyType>& kss, const std::vector<Kmer<K>>& queries) {
  const KmerSetSetIndex<K, N, KeyType> index(kss);
  EXPECT_EQ(index.Words(), (kss.Size() + 63) / 64);
  const std::vector<std::uint64_t> rows = index.Query(queries, true);
  EXPECT_EQ(rows.size(), queries.size() * std::size_t(index.Words()));
  if (rows.size() != queries.size() * std::size_t(index.Words())) return;
  int mismatches = 0;
  for (int i = 0; i < kss.Size(); i++) {
    const KmerSet<K, N, KeyType> got = kss.Get(i, true, 4);
    for (std::size_t q = 0; q < queries.size(); q++) {
      const bool bit = (rows[q * index.Words() + std::size_t(i) / 64] >> (i % 64)) & 1;
      if (bit != got.Contains(queries[q].Canonical())) mismatches++;
    }
  }
  EXPECT_EQ(mismatches, 0);
  EXPECT_TRUE(index.Query({}, true).empty());
}

template <int K, int N, typename KeyType>
static void TestIndex(int n_sets, int length) {
  std::vector<std::string> genomes;
  const auto sets = Family<K, N, KeyType>(n_sets, length, &genomes);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  std::vector<Kmer<K>> queries;
  for (const std::string& g : genomes)  // members, as they are (not canonical) ...
    for (int j = 0; j < 200; j++) queries.push_back(Kmer<K>(g.substr(Rand() % (g.size() - K + 1), K)));
  for (int j = 0; j < 500; j++)  // ... and random k-mers
    queries.push_back(Kmer<K>(Rand() & (~std::uint64_t(0) >> (64 - 2 * K))));
  CheckIndex(kss, queries);
  const std::string dir = (std::filesystem::temp_directory_path() / "ksc_test_kss_index").string();
  std::filesystem::remove_all(dir);
  EXPECT_TRUE(kss.Dump(dir, "", "txt", 4).ok());
  auto loaded = KmerSetSet<K, N, KeyType>::Load(dir, "", "txt", 4);
  EXPECT_TRUE(loaded.ok());
  if (loaded.ok()) CheckIndex(loaded.value(), queries);
  std::filesystem::remove_all(dir);
  std::printf("  KmerSetSetIndex<%d,%d>: %d sets -> %d nodes\n", K, N, n_sets, kss.Size());
}

int main() {
  try {
    TestIndex<23, 14, std::uint32_t>(6, 20000);
    TestIndex<31, 16, std::uint64_t>(4, 10000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
