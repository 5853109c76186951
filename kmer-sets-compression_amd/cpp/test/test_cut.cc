// Host-side test of the mirror's KmerSetCompact::Cut and KmerSetSetIndex::ColoredUnitigs: on one small family, the
// k-mers of the coloured unitigs with the class of their string are the k-mers of SelectClasses with their classes --
// every k-mer once -- every string is one class and there are more strings than the uncut encode has; a cut of
// hand-made strings gives the slices with K - 1 bases repeated, and a malformed run list is refused with the context
// serving afterwards.  Needs a GPU: everything runs through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <map>
#include <set>
#include <string>
#include <utility>
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
static std::uint64_t Rand() { return ksc::Mix64(0xC07ED + g_ctr++); }

template <int K, int N, typename KeyType>
static void TestCutByHand() {
  using Compact = KmerSetCompact<K, N, KeyType>;
  std::vector<std::string> seqs;
  for (int len : {K + 40, K, K + 7}) {
    std::string s;
    for (int i = 0; i < len; i++) s += "ACGT"[Rand() % 4];
    seqs.push_back(s);
  }
  const Compact in = Compact::FromStrings(seqs);
  const std::vector<std::int64_t> offsets{0, 3, 4, 6};
  const std::vector<std::uint32_t> start{0, 1, 33, 0, 0, 7};
  const Compact out = in.Cut(offsets, start);
  const std::vector<std::string> want{seqs[0].substr(0, K),      seqs[0].substr(1, 32 + K - 1), seqs[0].substr(33),
                                      seqs[1],                   seqs[2].substr(0, 7 + K - 1),  seqs[2].substr(7)};
  EXPECT_TRUE(out.ToStrings(1) == want);
  EXPECT_EQ(out.StringCount(), 6);
  EXPECT_EQ(out.Weight(), in.Weight() + 3 * (K - 1));
  EXPECT_TRUE(in.Cut({0, 1, 2, 3}, {0, 0, 0}).ToStrings(1) == seqs);  // no cut
  bool refused = false;
  try {
    in.Cut(offsets, {0, 1, 1, 0, 0, 7});  // not ascending
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("d_run_start[2]") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  EXPECT_TRUE(in.Cut(offsets, start).ToStrings(1) == want);  // the context still serves
}

template <int K, int N, typename KeyType>
static void TestColoredUnitigs(int n_sets, int length) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
  // a correlated family: one random genome, point substitutions per member
  std::string genome;
  for (int i = 0; i < length; i++) genome += "ACGT"[Rand() % 4];
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    std::set<std::uint64_t> kmers;
    for (int j = 0; j + K <= length; j++) kmers.insert(Kmer<K>(g.substr(j, K)).Canonical().Bits());
    const auto set = KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end()));
    compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(set, true, true, 4));
  }
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const Index index(kss);
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);

  // expected: the class of every k-mer of the union
  const auto classes = index.ColorClasses(inputs);
  const auto all = index.SelectClasses(inputs, classes);
  const std::vector<Kmer<K>> kmers = all.first.Find(4);
  std::map<std::uint64_t, std::uint32_t> class_of;
  for (std::size_t i = 0; i < kmers.size(); i++) class_of[kmers[i].Bits()] = all.second[i];
  EXPECT_TRUE(class_of.size() == kmers.size() && classes.size() > 3);

  const auto colored = index.ColoredUnitigs(inputs);
  const std::vector<std::string> strings = colored.strings.ToStrings(1);
  EXPECT_EQ(strings.size(), colored.cls.size());
  EXPECT_EQ(colored.classes.size(), classes.size());
  std::map<std::uint64_t, std::uint32_t> got;
  std::size_t positions = 0, longer = 0;
  bool ok = true;
  for (std::size_t r = 0; r < strings.size() && ok; r++) {
    ok = strings[r].size() >= std::size_t(K) && colored.cls[r] < classes.size();
    longer += strings[r].size() > std::size_t(K);
    for (std::size_t p = 0; p + K <= strings[r].size(); p++, positions++)
      got[Kmer<K>(strings[r].substr(p, K)).Canonical().Bits()] = colored.cls[r];
  }
  EXPECT_TRUE(ok);
  EXPECT_EQ(positions, kmers.size());  // every k-mer once
  EXPECT_TRUE(got == class_of);
  const auto uncut = KmerSetCompact<K, N, KeyType>::FromKmerSet(all.first, true, true, 1);
  EXPECT_TRUE(std::int64_t(strings.size()) > uncut.StringCount() && longer > 0);
  EXPECT_EQ(colored.strings.Weight(), uncut.Weight() + (std::int64_t(strings.size()) - uncut.StringCount()) * (K - 1));
  EXPECT_TRUE(colored.strings.ToKmerSet(true, 1).Equals(all.first, 1));
  std::printf("  ColoredUnitigs<%d,%d>: %d sets -> %d nodes, %zu classes, %zu k-mers in %zu strings (%lld uncut)\n", K, N,
              n_sets, kss.Size(), classes.size(), kmers.size(), strings.size(), (long long)uncut.StringCount());
}

int main() {
  try {
    TestCutByHand<23, 14, std::uint32_t>();
    TestCutByHand<4, 4, std::uint16_t>();
    TestColoredUnitigs<23, 14, std::uint32_t>(6, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
