// Host-side test of the mirror's KmerSetCompact::Locate: ends located by hand in both modes (a hit on either strand,
// a repeated k-mer, an end that spans two reference sequences, no strings, no reference), a malformed reference
// refused with the context serving afterwards, and reads cut from a random reference against a brute-force search.
// Needs a GPU: everything runs through libkmersets_hip.so.
#include <cstdint>
#include <cstdio>
#include <exception>
#include <string>
#include <vector>

#include "core/kmer.h"
#include "core/kmer_set.h"
#include "core/kmer_set_compact.h"
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
static std::uint64_t Rand() { return ksc::Mix64(0x10CA7E + g_ctr++); }

static std::string Rc(const std::string& s) {
  std::string r(s.rbegin(), s.rend());
  for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
  return r;
}
static std::string Random(int n) {
  std::string s;
  for (int i = 0; i < n; i++) s += "ACGT"[Rand() % 4];
  return s;
}

static void TestByHand() {
  using Compact = KmerSetCompact<5, 4, std::uint16_t>;
  using I64 = std::vector<std::int64_t>;
  using U32 = std::vector<std::uint32_t>;
  // the reference: ACGTTGCA has positions 0 .. 3, GGACGTT positions 4 .. 6
  const Compact ref = Compact::FromStrings({"ACGTTGCA", "GGACGTT"});
  // ACGTT lies at 0 and at 6; TGCAA's first k-mer is rc(TTGCA), which lies at 3; GCAGG spans both sequences
  const Compact strings = Compact::FromStrings({"ACGTT", "TGCAACC", "GCAGG"});
  const auto both = strings.Locate(ref, true);
  EXPECT_TRUE((both.where == I64{0, 0, 3 << 1 | 1, -1, -1, -1}));
  EXPECT_TRUE((both.count == U32{2, 2, 1, 0, 0, 0}));
  EXPECT_EQ(both.n_located, 3);
  const auto directed = strings.Locate(ref, false);
  EXPECT_TRUE((directed.where == I64{0, 0, -1, -1, -1, -1}));
  EXPECT_TRUE((directed.count == U32{2, 2, 0, 0, 0, 0}));
  EXPECT_EQ(directed.n_located, 2);
  const auto none = Compact().Locate(ref, true);
  EXPECT_TRUE(none.where.empty() && none.count.empty() && none.n_located == 0);
  const auto nowhere = strings.Locate(Compact(), true);
  EXPECT_TRUE((nowhere.where == I64(6, -1)) && (nowhere.count == U32(6, 0)) && nowhere.n_located == 0);
  // a reference that declares a base more than its strings hold (the words are there)
  bool refused = false;
  try {
    const Compact whole = Compact::FromStrings({"ACGTTGCA", "GGACGTTA"});
    const ksh_spss_view v = whole.View();
    const Compact bad = Compact::FromDevice(ksc::DeviceBuffer::FromHost(std::vector<std::uint64_t>(1, 0)),
                                            ksc::DeviceBuffer::FromHost(U32{3, 2}), 2, v.n_bases);
    strings.Locate(bad, true);
  } catch (const std::exception& e) {
    refused = std::string(e.what()).find("req->reference: sum(lens + K)") != std::string::npos;
  }
  EXPECT_TRUE(refused);
  EXPECT_TRUE(strings.Locate(ref, true).where == both.where);  // the context still serves
}

template <int K, int N, typename KeyType>
static void TestReads(int n_seqs, int n_reads) {
  using Compact = KmerSetCompact<K, N, KeyType>;
  std::vector<std::string> reference, reads;
  for (int i = 0; i < n_seqs; i++) reference.push_back(Random(K + int(Rand() % 700)));
  for (int i = 0; i < n_reads; i++) {
    const std::string& t = reference[Rand() % reference.size()];
    const std::size_t a = Rand() % (t.size() - K + 1), len = K + Rand() % (t.size() - a - K + 1);
    reads.push_back(i % 3 == 0 ? Rc(t.substr(a, len)) : t.substr(a, len));
  }
  for (int i = 0; i < 10; i++) reads.push_back(Random(K + 3));
  const Compact ref = Compact::FromStrings(reference), strings = Compact::FromStrings(reads);
  for (const bool canonical : {true, false}) {
    const auto got = strings.Locate(ref, canonical);
    bool same = got.where.size() == 2 * reads.size();
    std::int64_t located = 0, flipped = 0;
    for (std::size_t e = 0; same && e < 2 * reads.size(); e++) {
      const std::string& r = reads[e / 2];
      const std::string y = e % 2 ? r.substr(r.size() - K) : r.substr(0, K), back = Rc(y);
      std::int64_t where = -1, g = 0;
      std::uint32_t count = 0;
      for (const std::string& t : reference)
        for (std::size_t p = 0; p + K <= t.size(); p++, g++) {
          const bool fwd = t.compare(p, K, y) == 0, rev = canonical && !fwd && t.compare(p, K, back) == 0;
          if (!fwd && !rev) continue;
          if (count++ == 0) where = g << 1 | (rev ? 1 : 0);
        }
      same = where == got.where[e] && count == got.count[e];
      located += count > 0;
      flipped += where >= 0 && (where & 1);
    }
    EXPECT_TRUE(same);
    EXPECT_EQ(located, got.n_located);
    EXPECT_TRUE(located >= std::int64_t(reads.size()) / 2 && (flipped > 0) == canonical);
    std::printf("  Locate<%d,%d> %s: %zu reads in %zu sequences, %lld of %zu ends located, %lld on strand 1\n", K, N,
                canonical ? "canonical" : "directed", reads.size(), reference.size(), (long long)located,
                2 * reads.size(), (long long)flipped);
  }
}

int main() {
  try {
    TestByHand();
    TestReads<23, 14, std::uint32_t>(30, 200);
    TestReads<31, 14, std::uint64_t>(12, 80);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 2;
  }
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
