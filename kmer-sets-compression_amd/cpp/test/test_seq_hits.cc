// Host-side tests of the mirror's KmerSetSetIndex::CountHits: on a constructed and on a Dumped-then-Loaded
// KmerSetSet, the hits of every string and node equal the sum of Get(i).Contains over the string's k-mers, for
// the node strings themselves (every k-mer a member of its node) and for random strings.  Needs a GPU: everything
// runs through libkmersets_hip.so.
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
static std::uint64_t Rand() { return ksc::Mix64(0x5E9B0000 + g_ctr++); }

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
static void CheckHits(const KmerSetSet<K, N, KeyType>& kss, const std::vector<std::string>& sequences) {
  const KmerSetSetIndex<K, N, KeyType> index(kss);
  EXPECT_EQ(index.Nodes(), kss.Size());
  const std::vector<std::uint32_t> hits = index.CountHits(sequences, true);
  EXPECT_EQ(hits.size(), sequences.size() * std::size_t(kss.Size()));
  if (hits.size() != sequences.size() * std::size_t(kss.Size())) return;
  // the container overload gives the same table
  EXPECT_TRUE(index.CountHits(KmerSetCompact<K, N, KeyType>::FromStrings(sequences), true) == hits);
  int mismatches = 0, nonzero = 0, partial = 0;
  for (int i = 0; i < kss.Size(); i++) {
    const KmerSet<K, N, KeyType> got = kss.Get(i, true, 4);
    for (std::size_t s = 0; s < sequences.size(); s++) {
      std::uint32_t want = 0;
      const std::size_t positions = sequences[s].size() - K + 1;
      for (std::size_t j = 0; j < positions; j++)
        if (got.Contains(Kmer<K>(sequences[s].substr(j, K)).Canonical())) want++;
      if (hits[s * std::size_t(kss.Size()) + std::size_t(i)] != want) mismatches++;
      if (want) nonzero++;
      if (want && want < positions) partial++;
    }
  }
  EXPECT_EQ(mismatches, 0);
  EXPECT_TRUE(nonzero > 0 && partial > 0);
  EXPECT_TRUE(index.CountHits(std::vector<std::string>{}, true).empty());
}

template <int K, int N, typename KeyType>
static void TestHits(int n_sets, int length) {
  std::vector<std::string> genomes;
  const auto sets = Family<K, N, KeyType>(n_sets, length, &genomes);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  std::vector<std::string> sequences;
  for (int i = 0; i < kss.Size(); i++)  // the node strings: every k-mer of them is in its node ...
    for (const std::string& s : kss.Node(i).ToStrings(1)) sequences.push_back(s);
  for (const std::string& g : genomes)  // ... reads cut from the genomes, as they are ...
    for (int j = 0; j < 20; j++) sequences.push_back(g.substr(Rand() % (g.size() - 150), 150));
  for (int j = 0; j < 50; j++)  // ... and random strings of K .. 199 bases
    sequences.push_back(RandomGenome(K + int(Rand() % (200 - K))));
  CheckHits(kss, sequences);
  const std::string dir = (std::filesystem::temp_directory_path() / "ksc_test_seq_hits").string();
  std::filesystem::remove_all(dir);
  EXPECT_TRUE(kss.Dump(dir, "", "txt", 4).ok());
  auto loaded = KmerSetSet<K, N, KeyType>::Load(dir, "", "txt", 4);
  EXPECT_TRUE(loaded.ok());
  if (loaded.ok()) CheckHits(loaded.value(), sequences);
  std::filesystem::remove_all(dir);
  std::printf("  CountHits<%d,%d>: %d sets -> %d nodes, %zu sequences\n", K, N, n_sets, kss.Size(), sequences.size());
}

int main() {
  try {
    TestHits<23, 14, std::uint32_t>(6, 20000);
    TestHits<31, 16, std::uint64_t>(4, 10000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
