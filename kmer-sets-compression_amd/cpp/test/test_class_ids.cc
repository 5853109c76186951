// Host-side test of the mirror's KmerSetSetIndex::SelectClasses: on one small family, the class id of every k-mer
// of the union of the inputs equals the one computed on the host from the mirror's own Get(i) k-mers, the ids counted
// per class are the counts of ColorClasses, a selection and a part of the table give the same classes, and a table of
// other columns is refused with the index serving afterwards.  Needs a GPU: everything runs through
// libkmersets_hip.so.
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
static std::uint64_t Rand() { return ksc::Mix64(0xC1A551D5 + g_ctr++); }

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
static void TestClassIds(int n_sets, int length) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
  using Class = typename Index::ColorClass;
  const auto sets = Family<K, N, KeyType>(n_sets, length);
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (const auto& s : sets) compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(s, true, true, 4));
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const Index index(kss);
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);

  // expected on the host: the row of every k-mer of the inputs' Get (every node is reachable from an input), the
  // distinct rows in ascending order, and a k-mer's id = the position of its row among them
  std::map<std::uint64_t, std::uint64_t> row_of;
  for (int i = 0; i < n_sets; i++)
    for (const Kmer<K>& kmer : kss.Get(i, true, 4).Find(4)) row_of[kmer.Bits()] |= std::uint64_t(1) << i;
  std::map<std::uint64_t, std::uint32_t> id_of;
  for (const auto& kv : row_of) id_of[kv.second] = 0;
  std::uint32_t next = 0;
  for (auto& kv : id_of) kv.second = next++;

  const std::vector<Class> classes = index.ColorClasses(inputs);
  EXPECT_TRUE(id_of.size() > std::size_t(n_sets));
  EXPECT_EQ(classes.size(), id_of.size());

  // the union: every k-mer with its class, in the ascending order of the set
  const auto all = index.SelectClasses(inputs, classes);
  const std::vector<Kmer<K>> kmers = all.first.Find(4);
  EXPECT_EQ(kmers.size(), row_of.size());
  EXPECT_EQ(all.second.size(), kmers.size());
  bool equal = kmers.size() == row_of.size() && all.second.size() == kmers.size(), ascending = true;
  std::vector<std::int64_t> histogram(classes.size(), 0);
  for (std::size_t i = 0; i < kmers.size() && equal; i++) {
    if (i > 0) ascending = ascending && kmers[i - 1].Bits() < kmers[i].Bits();
    const auto it = row_of.find(kmers[i].Bits());
    equal = it != row_of.end() && all.second[i] == id_of[it->second] && all.second[i] < classes.size();
    if (equal) histogram[all.second[i]]++;
  }
  EXPECT_TRUE(equal);
  EXPECT_TRUE(ascending);
  bool counted = equal;
  for (std::size_t c = 0; c < classes.size() && counted; c++) counted = histogram[c] == classes[c].count;
  EXPECT_TRUE(counted);

  // the k-mers of inputs 0 and 1 that input 2 lacks, against the whole table
  const auto some = index.SelectClasses(inputs, classes, 1, 0, {0, 1}, {2});
  const std::vector<Kmer<K>> some_kmers = some.first.Find(4);
  std::size_t want_some = 0;
  for (const auto& kv : row_of) want_some += (kv.second & 7) == 3;
  EXPECT_TRUE(want_some > 0);
  EXPECT_EQ(some_kmers.size(), want_some);
  bool some_equal = some_kmers.size() == want_some && some.second.size() == want_some;
  for (std::size_t i = 0; i < some_kmers.size() && some_equal; i++) {
    const std::uint64_t row = row_of[some_kmers[i].Bits()];
    some_equal = (row & 7) == 3 && some.second[i] == id_of[row];
  }
  EXPECT_TRUE(some_equal);

  // the private k-mers by sample: the one-bit classes alone are table enough, and the id is the sample
  std::vector<Class> one_bit;
  for (const Class& c : classes)
    if (__builtin_popcountll(c.row[0]) == 1 && c.row[1] == 0) one_bit.push_back(c);
  EXPECT_EQ(one_bit.size(), std::size_t(n_sets));
  const auto priv = index.SelectClasses(inputs, one_bit, 1, 1);
  const std::vector<Kmer<K>> priv_kmers = priv.first.Find(4);
  bool priv_equal = priv.second.size() == priv_kmers.size() && !priv_kmers.empty();
  for (std::size_t i = 0; i < priv_kmers.size() && priv_equal; i++)
    priv_equal = row_of[priv_kmers[i].Bits()] == std::uint64_t(1) << priv.second[i];
  EXPECT_TRUE(priv_equal);

  // a foreign table: that of fewer columns has no row for most k-mers of the union; one of more columns has bits
  // the request has no column for
  bool refused = false;
  try {
    index.SelectClasses(inputs, one_bit);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("rows") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  refused = false;
  try {
    index.SelectClasses({0, 1}, classes);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("n_cols") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  EXPECT_TRUE(index.SelectClasses(inputs, classes).second == all.second);  // the index still serves
  std::printf("  SelectClasses<%d,%d>: %d sets -> %d nodes, %zu classes of %zu k-mers, %zu private\n", K, N, n_sets,
              kss.Size(), classes.size(), kmers.size(), priv_kmers.size());
}

int main() {
  try {
    TestClassIds<23, 14, std::uint32_t>(6, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
