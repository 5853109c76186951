// Host-side test of the mirror's KmerSetCompact::Links and KmerSetSetIndex::ColoredGraph: links worked by hand in both
// modes, a duplicate end refused with the context serving afterwards, and on one small family the links of the coloured
// graph checked textually (K - 1 bases of overlap), twin by twin, and -- with the k-mer pairs inside the strings --
// against the de Bruijn edges of the union found by brute force.  Needs a GPU: everything runs through
// libkmersets_hip.so.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <exception>
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
static std::uint64_t Rand() { return ksc::Mix64(0x11A85 + g_ctr++); }

static std::string Rc(const std::string& s) {
  std::string r(s.rbegin(), s.rend());
  for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
  return r;
}
static std::string Canon(const std::string& s) { return std::min(s, Rc(s)); }
static std::string Oriented(const std::vector<std::string>& strings, std::int64_t v) {
  return (v & 1) ? Rc(strings[std::size_t(v >> 1)]) : strings[std::size_t(v >> 1)];
}

static void TestByHand() {
  using Compact = KmerSetCompact<4, 4, std::uint16_t>;
  // AACCG ends in ACCG; CCGTA begins with CCGT: 0 -> 2, and the twin 3 -> 1
  const Compact c = Compact::FromStrings({"AACCG", "CCGTA"});
  const auto both = c.Links(true);
  EXPECT_TRUE((both.offsets == std::vector<std::int64_t>{0, 1, 1, 1, 2}));
  EXPECT_TRUE((both.to == std::vector<std::int64_t>{2, 1}));
  const auto directed = c.Links(false);
  EXPECT_TRUE((directed.offsets == std::vector<std::int64_t>{0, 1, 1, 1, 1}));
  EXPECT_TRUE((directed.to == std::vector<std::int64_t>{2}));
  const auto none = Compact().Links(true);
  EXPECT_TRUE(none.offsets == std::vector<std::int64_t>{0} && none.to.empty());
  bool refused = false;
  try {
    Compact::FromStrings({"AACCG", "GGTTA"}).Links(true);  // GGTT is the reverse complement of AACC
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("string 0") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  EXPECT_TRUE(c.Links(true).to == both.to);  // the context still serves
}

template <int K, int N, typename KeyType>
static void TestColoredGraph(int n_sets, int length) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
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

  const auto graph = index.ColoredGraph(inputs);
  const std::vector<std::string> strings = graph.strings.ToStrings(1);
  const std::size_t n = strings.size();
  EXPECT_EQ(graph.cls.size(), n);
  EXPECT_EQ(graph.links.offsets.size(), 2 * n + 1);
  EXPECT_TRUE(graph.links.offsets.back() == std::int64_t(graph.links.to.size()) && !graph.links.to.empty());

  // the nodes: every k-mer of the union once, in pieces of unitigs
  const auto all = index.SelectClasses(inputs, graph.classes);
  EXPECT_TRUE(graph.strings.ToKmerSet(true, 1).Equals(all.first, 1));
  const auto unitigs = KmerSetCompact<K, N, KeyType>::UnitigsOf(all.first, true);
  // (members that differ by substitutions change class only where the union's graph branches: the painting may
  // cut no unitig at all, and then the strings are the unitigs)
  EXPECT_TRUE(std::int64_t(n) >= unitigs.StringCount());
  EXPECT_EQ(graph.strings.Weight(), unitigs.Weight() + (std::int64_t(n) - unitigs.StringCount()) * (K - 1));

  // the edges, textually; both twins; some between classes
  std::set<std::pair<std::int64_t, std::int64_t>> pairs;
  std::set<std::pair<std::string, std::string>> got;
  bool overlap = true, rows = true;
  std::size_t mixed = 0;
  for (std::size_t v = 0; v < 2 * n; v++) {
    rows = rows && graph.links.offsets[v + 1] - graph.links.offsets[v] <= 4;
    const std::string from = Oriented(strings, std::int64_t(v));
    for (std::int64_t i = graph.links.offsets[v]; i < graph.links.offsets[v + 1]; i++) {
      const std::int64_t w = graph.links.to[std::size_t(i)];
      const std::string to = Oriented(strings, w);
      overlap = overlap && from.substr(from.size() - (K - 1)) == to.substr(0, K - 1);
      pairs.insert({std::int64_t(v), w});
      got.insert({from.substr(from.size() - K), to.substr(0, K)});
      mixed += graph.cls[v >> 1] != graph.cls[std::size_t(w >> 1)];
    }
  }
  EXPECT_TRUE(overlap && rows && mixed > 0);
  EXPECT_EQ(pairs.size(), graph.links.to.size());
  bool twins = true;
  for (const auto& p : pairs) twins = twins && pairs.count({p.second ^ 1, p.first ^ 1}) == 1;
  EXPECT_TRUE(twins);
  const std::size_t between = got.size();
  EXPECT_EQ(between, graph.links.to.size());
  for (std::size_t v = 0; v < 2 * n; v++) {
    const std::string t = Oriented(strings, std::int64_t(v));
    for (std::size_t i = 0; i + K < t.size(); i++) got.insert({t.substr(i, K), t.substr(i + 1, K)});
  }
  // brute force: the edges x -> y, canon(x) != canon(y), of the union's k-mers in either orientation
  std::set<std::string> nodes;
  for (const std::string& s : strings)
    for (std::size_t i = 0; i + K <= s.size(); i++) {
      nodes.insert(s.substr(i, K));
      nodes.insert(Rc(s.substr(i, K)));
    }
  EXPECT_EQ(nodes.size(), 2 * std::size_t(all.first.Size()));
  std::set<std::pair<std::string, std::string>> want;
  for (const std::string& x : nodes)
    for (char b : std::string("ACGT")) {
      const std::string y = x.substr(1) + b;
      if (nodes.count(y) && Canon(x) != Canon(y)) want.insert({x, y});
    }
  EXPECT_TRUE(got == want);
  std::printf("  ColoredGraph<%d,%d>: %d sets, %zu classes, %zu strings (%lld unitigs), %zu links, %zu between classes\n",
              K, N, n_sets, graph.classes.size(), n, (long long)unitigs.StringCount(), graph.links.to.size(), mixed);
}

int main() {
  try {
    TestByHand();
    TestColoredGraph<23, 14, std::uint32_t>(6, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
