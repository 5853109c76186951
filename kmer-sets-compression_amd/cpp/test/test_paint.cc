// Host-side test of the mirror's KmerSetSetIndex::Paint: on one small family, the runs of every sequence expanded
// to one class per k-mer position equal the pattern a host loop over Get(i).Contains gives that position, adjacent
// runs of a sequence differ, a partial table leaves the other positions without a class and counts them (or is
// refused), and too small a capacity is refused with the index serving afterwards.  Needs a GPU: everything runs
// through libkmersets_hip.so.
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
static std::uint64_t Rand() { return ksc::Mix64(0x9A1E7 + g_ctr++); }

template <int K, int N, typename KeyType>
static void TestPaint(int n_sets, int length) {
  using Index = KmerSetSetIndex<K, N, KeyType>;
  using Class = typename Index::ColorClass;
  using Runs = typename Index::ClassRuns;
  // a correlated family: one random genome, point substitutions per member
  std::string genome;
  for (int i = 0; i < length; i++) genome += "ACGT"[Rand() % 4];
  std::vector<std::string> members;
  std::vector<KmerSetCompact<K, N, KeyType>> compacts;
  for (int s = 0; s < n_sets; s++) {
    std::string g = genome;
    for (int i = 0; i < length; i++)
      if (Rand() % 300 == 0) g[i] = "ACGT"[Rand() % 4];
    std::set<std::uint64_t> kmers;
    for (int j = 0; j + K <= length; j++) kmers.insert(Kmer<K>(g.substr(j, K)).Canonical().Bits());
    const auto set = KmerSet<K, N, KeyType>::FromSortedBits(std::vector<std::uint64_t>(kmers.begin(), kmers.end()));
    compacts.push_back(KmerSetCompact<K, N, KeyType>::FromKmerSet(set, true, true, 4));
    members.push_back(g);
  }
  const KmerSetSet<K, N, KeyType> kss(compacts, true, 4);
  const Index index(kss);
  std::vector<int> inputs;
  for (int i = 0; i < n_sets; i++) inputs.push_back(i);
  std::vector<KmerSet<K, N, KeyType>> gets;
  for (int i = 0; i < n_sets; i++) gets.push_back(kss.Get(i, true, 4));

  // the sequences: pieces of two members, a piece of the unmutated genome, one string of exactly K bases, and a
  // random string that no set knows
  std::vector<std::string> seqs{members[0].substr(0, 3000), members[1].substr(1000, 2500), genome.substr(500, 1500),
                                members[2].substr(77, K)};
  std::string noise;
  for (int i = 0; i < 200; i++) noise += "ACGT"[Rand() % 4];
  seqs.push_back(noise);

  // expected on the host: the pattern of every position
  std::vector<std::vector<std::uint64_t>> want(seqs.size());
  std::set<std::uint64_t> patterns;
  for (std::size_t s = 0; s < seqs.size(); s++)
    for (std::size_t p = 0; p + K <= seqs[s].size(); p++) {
      const Kmer<K> kmer = Kmer<K>(seqs[s].substr(p, K)).Canonical();
      std::uint64_t row = 0;
      for (int i = 0; i < n_sets; i++)
        if (gets[std::size_t(i)].Contains(kmer)) row |= std::uint64_t(1) << i;
      want[s].push_back(row);
      patterns.insert(row);
    }
  EXPECT_TRUE(patterns.size() > 3 && patterns.count(0) == 1);

  // the table: the classes of the structure, and the zero pattern (the noise) if the structure has no such k-mer
  std::vector<Class> classes = index.ColorClasses(inputs);
  if (classes.empty() || classes[0].row[0] != 0 || classes[0].row[1] != 0)
    classes.insert(classes.begin(), Class{{0, 0}, 0});

  const auto check = [&](const Runs& runs, const std::vector<Class>& table, std::int64_t* unmatched) {
    bool ok = runs.offsets.size() == seqs.size() + 1 && runs.offsets[0] == 0 &&
              runs.offsets.back() == std::int64_t(runs.start.size()) && runs.start.size() == runs.cls.size();
    *unmatched = 0;
    for (std::size_t s = 0; s < seqs.size() && ok; s++) {
      const std::int64_t a = runs.offsets[s], b = runs.offsets[s + 1];
      ok = b > a && runs.start[std::size_t(a)] == 0;
      for (std::int64_t r = a; r < b && ok; r++) {
        const std::size_t from = runs.start[std::size_t(r)];
        const std::size_t to = r + 1 < b ? runs.start[std::size_t(r + 1)] : want[s].size();
        const std::uint32_t c = runs.cls[std::size_t(r)];
        ok = from < to && to <= want[s].size() && (r == a || c != runs.cls[std::size_t(r - 1)]);
        for (std::size_t p = from; p < to && ok; p++) {
          if (c == Index::kNoClass) {
            *unmatched += 1;
            for (const Class& t : table) ok = ok && t.row[0] != want[s][p];  // the table does not hold it
          } else {
            ok = c < table.size() && table[c].row[0] == want[s][p] && table[c].row[1] == 0;
          }
        }
      }
    }
    return ok;
  };

  std::int64_t unmatched = 0;
  const Runs all = index.Paint(seqs, inputs, classes, true, false);
  EXPECT_TRUE(check(all, classes, &unmatched));
  EXPECT_EQ(unmatched, 0);
  EXPECT_TRUE(all.start.size() > seqs.size() + 5);
  EXPECT_EQ(all.offsets[4] - all.offsets[3], 1);  // the string of K bases is one run

  // the one-bit classes alone: every other position is without a class, and counted
  std::vector<Class> one_bit;
  for (const Class& c : classes)
    if (__builtin_popcountll(c.row[0]) == 1 && c.row[1] == 0) one_bit.push_back(c);
  EXPECT_EQ(one_bit.size(), std::size_t(n_sets));
  const Runs part = index.Paint(seqs, inputs, one_bit);
  EXPECT_TRUE(check(part, one_bit, &unmatched));
  EXPECT_TRUE(unmatched > 0 && unmatched == part.n_unmatched);
  bool refused = false;
  try {
    index.Paint(seqs, inputs, one_bit, true, false);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("rows") != std::string::npos &&
              std::string(e.what()).find(std::to_string(unmatched)) != std::string::npos;
  }
  EXPECT_TRUE(refused);

  // the capacity: exact is enough, one less is refused with the number of runs
  const std::int64_t n_runs = std::int64_t(all.start.size());
  const Runs exact = index.Paint(seqs, inputs, classes, true, false, n_runs);
  EXPECT_TRUE(exact.offsets == all.offsets && exact.start == all.start && exact.cls == all.cls);
  refused = false;
  try {
    index.Paint(seqs, inputs, classes, true, false, n_runs - 1);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("capacity") != std::string::npos &&
              std::string(e.what()).find(std::to_string(n_runs)) != std::string::npos;
  }
  EXPECT_TRUE(refused);
  // a table of more columns than the request
  refused = false;
  try {
    index.Paint(seqs, {0, 1}, classes);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("n_cols") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  const Runs again = index.Paint(KmerSetCompact<K, N, KeyType>::FromStrings(seqs), inputs, classes);
  EXPECT_TRUE(again.start == all.start && again.cls == all.cls && again.n_unmatched == 0);  // the index still serves
  std::printf("  Paint<%d,%d>: %d sets -> %d nodes, %zu classes, %zu sequences in %zu runs, %lld positions "
              "outside the one-bit classes\n", K, N, n_sets, kss.Size(), classes.size(), seqs.size(),
              all.start.size(), (long long)unmatched);
}

int main() {
  try {
    TestPaint<23, 14, std::uint32_t>(6, 20000);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
