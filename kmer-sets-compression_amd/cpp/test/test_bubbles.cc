// Host-side test of the mirror's KmerSetCompact::LinkBubbles and KmerSetSetIndex::ColoredBubbles: bubbles worked by
// hand on link vectors (a plain bubble with classes, a hairpin), a link without its twin refused with the context
// serving afterwards, and on one small family the bubbles of the coloured graph compared with the definition walked on
// the host, their alleles checked textually against source and sink and their carriers against the AND of the classes'
// rows.  Needs a GPU: everything runs through libkmersets_hip.so.
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

using I64 = std::vector<std::int64_t>;
using U64 = std::vector<std::uint64_t>;

static std::uint64_t g_ctr = 0;
static std::uint64_t Rand() { return ksc::Mix64(0xB0BB1E + g_ctr++); }

static std::string Rc(const std::string& s) {
  std::string r(s.rbegin(), s.rend());
  for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
  return r;
}
static std::string Oriented(const std::vector<std::string>& strings, std::int64_t v) {
  return (v & 1) ? Rc(strings[std::size_t(v >> 1)]) : strings[std::size_t(v >> 1)];
}

static void TestByHand() {
  using Compact = KmerSetCompact<4, 4, std::uint16_t>;
  // 0 -> 4 -> 2 and 0 -> 6 -> 2, with the twins 3 -> 5 -> 1 and 3 -> 7 -> 1
  const I64 off{0, 2, 2, 2, 4, 5, 6, 7, 8}, to{4, 6, 5, 7, 2, 1, 2, 1};
  const auto plain = Compact::LinkBubbles(off, to);
  EXPECT_TRUE((plain.ends == I64{0, 2}) && (plain.arm_offsets == I64{0, 1, 2}) && (plain.arm_strings == I64{4, 6}));
  EXPECT_TRUE(plain.arm_rows.empty() && plain.Size() == 1);
  const auto colored = Compact::LinkBubbles(off, to, 1, {0, 1, 1, 2}, U64{7, 0, 3, 0, 5, 1});
  EXPECT_TRUE((colored.ends == plain.ends) && (colored.arm_strings == plain.arm_strings));
  EXPECT_TRUE((colored.arm_rows == U64{3, 0, 5, 1}));
  // the hairpin 0 -> 2 -> 1 and its twin 0 -> 3 -> 1: one string in both orientations
  const auto hairpin = Compact::LinkBubbles({0, 2, 2, 3, 4}, {2, 3, 1, 1});
  EXPECT_TRUE((hairpin.ends == I64{0, 1}) && (hairpin.arm_strings == I64{2, 3}));
  const auto none = Compact::LinkBubbles({0}, {});
  EXPECT_TRUE(none.ends.empty() && (none.arm_offsets == I64{0}) && none.arm_strings.empty());
  bool no_twin = false, no_arm = false;
  try {
    Compact::LinkBubbles({0, 1, 1, 1, 1}, {2});  // what Links(false) gives: 0 -> 2 alone
  } catch (const std::exception& e) {
    no_twin = std::string(e.what()).find("twin") != std::string::npos;
  }
  try {
    Compact::LinkBubbles(off, to, 0);
  } catch (const std::exception& e) {
    no_arm = std::string(e.what()).find("max_arm") != std::string::npos;
  }
  EXPECT_TRUE(no_twin && no_arm);
  EXPECT_TRUE(Compact::LinkBubbles(off, to).ends == plain.ends);  // the context still serves
}

// The definition of include/kmersets_hip.h walked on the host: (v, w, arm_0, arm_1) of every reported bubble.
struct HostBubble {
  std::int64_t v, w;
  I64 arm[2];
};
static std::vector<HostBubble> HostBubbles(const I64& off, const I64& to, int max_arm) {
  const std::int64_t m = std::int64_t(off.size()) - 1;
  const auto outdeg = [&](std::int64_t v) { return off[std::size_t(v + 1)] - off[std::size_t(v)]; };
  std::vector<HostBubble> out;
  for (std::int64_t v = 0; v < m; v++) {
    if (outdeg(v) != 2) continue;
    HostBubble b{v, -1, {}};
    std::int64_t sink[2] = {-1, -2};
    bool ok = true;
    for (int i = 0; i < 2 && ok; i++) {
      std::int64_t x = to[std::size_t(off[std::size_t(v)] + i)];
      for (;;) {
        if (outdeg(x ^ 1) != 1 || outdeg(x) != 1 || int(b.arm[i].size()) == max_arm) {
          ok = false;
          break;
        }
        b.arm[i].push_back(x);
        x = to[std::size_t(off[std::size_t(x)])];
        if (outdeg(x ^ 1) == 2) {
          sink[i] = x;
          break;
        }
        if (outdeg(x ^ 1) != 1) {
          ok = false;
          break;
        }
      }
    }
    if (!ok || sink[0] != sink[1] || v > (sink[0] ^ 1)) continue;
    b.w = sink[0];
    out.push_back(b);
  }
  return out;
}

template <int K, int N, typename KeyType>
static void TestColoredBubbles(int n_sets, int length, int max_arm) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
  std::string genome;
  for (int i = 0; i < length; i++) genome += "ACGT"[Rand() % 4];
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    // (the last two members are striped: one holds the k-mers that start in the even hundreds of the genome, the other
    // those in the odd hundreds.  They enter and leave the others' unitigs -- and, where a stripe ends inside one, an
    // arm -- mid-way)
    const int stripe = s >= n_sets - 2 ? s - (n_sets - 2) : -1;
    std::set<std::uint64_t> kmers;
    for (int j = 0; j + K <= length; j++)
      if (stripe < 0 || (j / 100) % 2 == stripe) kmers.insert(Kmer<K>(g.substr(j, K)).Canonical().Bits());
    const auto set = KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end()));
    compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(set, true, true, 4));
  }
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const Index index(kss);
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);

  const auto result = index.ColoredBubbles(inputs, max_arm);
  const auto& graph = result.graph;
  const auto& bub = result.bubbles;
  const auto again = index.ColoredGraph(inputs);
  const std::vector<std::string> strings = graph.strings.ToStrings(1);
  EXPECT_TRUE(strings == again.strings.ToStrings(1) && graph.cls == again.cls);
  EXPECT_TRUE(graph.links.offsets == again.links.offsets && graph.links.to == again.links.to);

  const std::vector<HostBubble> want = HostBubbles(graph.links.offsets, graph.links.to, max_arm);
  const std::size_t nb = bub.Size();
  EXPECT_TRUE(nb > 0 && nb == want.size());
  EXPECT_EQ(bub.arm_offsets.size(), 2 * nb + 1);
  EXPECT_EQ(bub.arm_rows.size(), 4 * nb);
  EXPECT_TRUE(bub.arm_offsets.front() == 0 && bub.arm_offsets.back() == std::int64_t(bub.arm_strings.size()));
  bool same = true, text = true, carriers = true, lower_base = true;
  std::size_t long_arms = 0;
  for (std::size_t b = 0; b < nb && b < want.size(); b++) {
    const std::int64_t v = bub.ends[2 * b], w = bub.ends[2 * b + 1];
    same = same && v == want[b].v && w == want[b].w;
    const std::string source = Oriented(strings, v), sink = Oriented(strings, w);
    std::string allele[2];
    for (int i = 0; i < 2; i++) {
      const I64 arm(bub.arm_strings.begin() + bub.arm_offsets[2 * b + std::size_t(i)],
                    bub.arm_strings.begin() + bub.arm_offsets[2 * b + std::size_t(i) + 1]);
      same = same && arm == want[b].arm[i];
      long_arms += arm.size() > 1;
      std::uint64_t r0 = ~0ull, r1 = ~0ull;
      for (const std::int64_t x : arm) {
        const std::string t = Oriented(strings, x);
        text = text && (allele[i].empty() || allele[i].substr(allele[i].size() - (K - 1)) == t.substr(0, K - 1));
        allele[i] += allele[i].empty() ? t : t.substr(K - 1);
        r0 &= graph.classes[graph.cls[std::size_t(x >> 1)]].row[0];
        r1 &= graph.classes[graph.cls[std::size_t(x >> 1)]].row[1];
      }
      carriers = carriers && bub.arm_rows[4 * b + 2 * std::size_t(i)] == r0 &&
                 bub.arm_rows[4 * b + 2 * std::size_t(i) + 1] == r1;
      text = text && allele[i].substr(0, K - 1) == source.substr(source.size() - (K - 1)) &&
             allele[i].substr(allele[i].size() - (K - 1)) == sink.substr(0, K - 1);
    }
    lower_base = lower_base && allele[0][K - 1] < allele[1][K - 1];
  }
  EXPECT_TRUE(same);
  EXPECT_TRUE(text);
  EXPECT_TRUE(carriers);
  EXPECT_TRUE(lower_base);
  EXPECT_TRUE(long_arms > 0);  // (the stripes: arms that are chains of strings)
  std::printf("  ColoredBubbles<%d,%d>: %d sets, %zu strings, %zu links, %zu bubbles, %zu arms of several strings\n", K, N,
              n_sets, strings.size(), graph.links.to.size(), nb, long_arms);
}

int main() {
  try {
    TestByHand();
    TestColoredBubbles<23, 14, std::uint32_t>(6, 20000, 8);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
