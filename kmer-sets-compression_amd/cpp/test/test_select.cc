// Host-side test of the mirror's KmerSetSetIndex::Select and Spectrum: on one small family, the core, the union and
// the k-mers private to one input equal what the mirror's own Get / Intersection / Add / Sub give, a selection with
// require and exclude equals (Get(0) & Get(1)) \ Get(2), and the spectrum sums to the size of the union of all
// nodes.  Needs a GPU: everything runs through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
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
static std::uint64_t Rand() { return ksc::Mix64(0x5E1EC700 + g_ctr++); }

// A correlated family: one random genome, point substitutions per member.
template <int K, int N, typename KeyType>
static std::vector<KmerSet<K, N, KeyType>> Family(int n_sets, int length) {
  std::string genome;
  for (int i = 0; i < length; i++) genome += "ACGT"[Rand() % 4];
  std::vector<KmerSet<K, N, KeyType>> out;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    std::set<std::uint64_t> kmers;
    for (int j = 0; j + K <= length; j++) kmers.insert(Kmer<K>(g.substr(j, K)).Canonical().Bits());
    out.push_back(KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end())));
  }
  return out;
}

template <int K, int N, typename KeyType>
static void TestSelect(int n_sets, int length) {
  using Set = KmerSet<K, N, KeyType>;
  const auto sets = Family<K, N, KeyType>(n_sets, length);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const KmerSetSetIndex<K, N, KeyType> index(kss);
  const int n = kss.Size();
  std::vector<Set> gets;
  for (int i = 0; i < n; i++) gets.push_back(kss.Get(i, true, 4));
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);

  Set core = gets[0], all = gets[0], others = gets[1];
  for (int i = 1; i < n_sets; i++) {
    core = Intersection(core, gets[i], 4);
    all.Add(gets[i], 4);
    if (i > 1) others.Add(gets[i], 4);
  }
  const Set got_core = index.Select(inputs, n_sets, 0);
  EXPECT_TRUE(core.Size() > 0 && core.Size() < all.Size());
  EXPECT_EQ(got_core.Size(), core.Size());
  EXPECT_TRUE(got_core.Equals(core, 4));
  EXPECT_EQ(got_core.Hash(4), core.Hash(4));
  const Set got_all = index.Select(inputs);
  EXPECT_EQ(got_all.Size(), all.Size());
  EXPECT_TRUE(got_all.Equals(all, 4));
  const Set priv = Sub(gets[0], others, 4);
  const Set got_priv = index.Select(inputs, 1, 1, {0});
  EXPECT_TRUE(priv.Size() > 0);
  EXPECT_EQ(got_priv.Size(), priv.Size());
  EXPECT_TRUE(got_priv.Equals(priv, 4));
  const Set ab_not_c = Sub(Intersection(gets[0], gets[1], 4), gets[2], 4);
  const Set got_abc = index.Select({2, 0, 1}, 1, 0, {0, 1}, {2});
  EXPECT_EQ(got_abc.Size(), ab_not_c.Size());
  EXPECT_TRUE(got_abc.Equals(ab_not_c, 4));
  // the result is a set like any other: k-mers ascending, and an operand of the pair algebra
  const std::vector<Kmer<K>> kmers = got_core.Find(4);
  bool ascending = true;
  for (std::size_t i = 1; i < kmers.size(); i++) ascending = ascending && kmers[i - 1].Bits() < kmers[i].Bits();
  EXPECT_TRUE(ascending);
  EXPECT_EQ(Intersection(got_all, got_core, 4).Size(), core.Size());

  // the spectrum of the inputs: every k-mer of the structure is in some input's Get, its classes add up to the
  // union, its core class is the core; over all nodes it sums to the same union
  const std::vector<std::int64_t> spectrum = index.Spectrum(inputs);
  EXPECT_EQ(spectrum.size(), std::size_t(n_sets) + 1);
  std::int64_t sum = 0, weighted = 0, sizes = 0;
  for (std::size_t m = 0; m < spectrum.size(); m++) {
    sum += spectrum[m];
    weighted += std::int64_t(m) * spectrum[m];
  }
  for (int i = 0; i < n_sets; i++) sizes += gets[i].Size();
  EXPECT_EQ(spectrum[0], 0);
  EXPECT_EQ(sum, all.Size());
  EXPECT_EQ(weighted, sizes);
  EXPECT_EQ(spectrum[n_sets], core.Size());
  EXPECT_EQ(spectrum[1], index.Select(inputs, 1, 1).Size());
  const std::vector<std::int64_t> every = index.Spectrum();
  EXPECT_EQ(every.size(), std::size_t(n) + 1);
  std::int64_t sum_every = 0;
  for (std::int64_t v : every) sum_every += v;
  EXPECT_EQ(sum_every, all.Size());
  std::printf("  Select<%d,%d>: %d sets -> %d nodes, core %lld of %lld\n", K, N, n_sets, n,
              static_cast<long long>(core.Size()), static_cast<long long>(all.Size()));
}

int main() {
  try {
    TestSelect<23, 14, std::uint32_t>(6, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
