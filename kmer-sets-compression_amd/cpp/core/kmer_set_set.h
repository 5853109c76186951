// KmerSetSet<K, N, KeyType> and KmerSetSetReader: the reference's set-of-sets compressor
// (lib/core/kmer_set_set.h:102-775) over the device loop ksh_kss_build.
//   ctor(vector<KmerSetCompact>, canonical, n_workers)  -> ksh_kss_build (the hot path)
//   Size / Get / Dump / DumpGraph / Load                 -> same meaning and file format:
//       meta.<ext> line 0 = "<#keys> {<key> <#children> <child>...}", line 1 = node count;
//       <i>.<ext> = one SPSS string per line; DOT graph "digraph G {" / "v%d -> v%d" / "}".
// bucket_ids come from ksc::SampleBucketIds (seeded) or from the caller.
#ifndef KSC_CORE_KMER_SET_SET_H_
#define KSC_CORE_KMER_SET_SET_H_

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdint>
#include <filesystem>
#include <map>
#include <queue>
#include <sstream>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "core/device.h"
#include "core/io.h"
#include "core/kmer_set.h"
#include "core/kmer_set_compact.h"
#include "core/random.h"
#include "core/status.h"

namespace internal {

// The reference's map is an absl::flat_hash_map (iteration order unspecified); ordered here.
using AdjacencyList = std::map<int, std::vector<int>>;

inline std::string SerializeAdjacencyList(const AdjacencyList& adjacency_list) {
  std::stringstream ss;
  ss << adjacency_list.size();
  for (const auto& p : adjacency_list) {
    ss << ' ' << p.first << ' ' << p.second.size();
    for (int i : p.second) ss << ' ' << i;
  }
  return ss.str();
}

inline AdjacencyList DeserializeAdjacencyList(const std::string& s) {
  std::stringstream ss(s);
  AdjacencyList adjacency_list;
  std::size_t size;
  ss >> size;
  for (std::size_t i = 0; i < size; i++) {
    int key;
    std::size_t value_size;
    ss >> key >> value_size;
    std::vector<int> value(value_size);
    for (std::size_t j = 0; j < value_size; j++) ss >> value[j];
    adjacency_list[key] = std::move(value);
  }
  return adjacency_list;
}

}  // namespace internal

template <int K, int N, typename KeyType>
class KmerSetSet {
 public:
  using Compact = KmerSetCompact<K, N, KeyType>;
  using Set = KmerSet<K, N, KeyType>;

  struct Iteration {
    std::int64_t j, k, weight, original_size, size_diff;
  };

  KmerSetSet() = default;

  KmerSetSet(std::vector<Compact> kmer_sets_compact, bool canonical, int n_workers)
      : KmerSetSet(std::move(kmer_sets_compact), canonical, n_workers,
                   ksc::SampleBucketIds(N, ksc::BucketSeedFromEnv())) {}

  // One process per GPU: every rank constructs the same KmerSetSet with its own rank, and the
  // SPSS encodes are dealt out (ksh_kss_build_sharded).  `gather` is the all-gather the build
  // needs a few times (ksh_allgather_i64: RCCL ncclAllGather on a staging buffer, MPI, ...).
  // Nodes held by another rank stay empty here (Holder(i) says which); Dump writes the files
  // of the nodes this rank holds, so the ranks together write the directory.
  struct Shard {
    int rank = 0, world = 1;
    ksh_allgather_i64 gather = nullptr;
    void* user = nullptr;
    // The owner-sharded build (ksh_kss_build_owned) when `comm` is set: a node's set and SPSS live on
    // one rank; `owners[i]` holds input i, whose container only that rank needs to pass (the others'
    // entries are ignored); comm comes from ksh_comm_create_rccl (or _custom) with this rank / world.
    ksh_comm* comm = nullptr;
    std::vector<std::int32_t> owners;
  };

  KmerSetSet(std::vector<Compact> kmer_sets_compact, bool canonical, int /*n_workers*/,
             const std::vector<int>& bucket_ids, int max_iterations = -1, Shard shard = Shard()) {
    const ksh_geom g = Set::Geom();
    std::vector<ksh_spss_view> views;
    for (const Compact& c : kmer_sets_compact) views.push_back(c.View());
    std::vector<std::int32_t> ids(bucket_ids.begin(), bucket_ids.end());
    ksh_kss* kss = nullptr;
    if (shard.comm) {
      std::vector<std::int32_t> owners = shard.owners;
      if (owners.empty())  // contiguous blocks
        for (std::size_t i = 0; i < views.size(); i++)
          owners.push_back(static_cast<std::int32_t>(i * std::size_t(shard.world) / views.size()));
      ksc::Check(ksh_kss_build_owned(ksc::Ctx(), shard.comm, &g, views.data(), static_cast<std::int32_t>(views.size()),
                                     owners.data(), ids.data(), static_cast<std::int32_t>(ids.size()),
                                     canonical ? 1 : 0, max_iterations, &kss));
    } else if (shard.world > 1)
      ksc::Check(ksh_kss_build_sharded(ksc::Ctx(), &g, views.data(), static_cast<std::int32_t>(views.size()),
                                       ids.data(), static_cast<std::int32_t>(ids.size()), canonical ? 1 : 0,
                                       max_iterations, shard.rank, shard.world, shard.gather, shard.user, &kss));
    else
      ksc::Check(ksh_kss_build(ksc::Ctx(), &g, views.data(), static_cast<std::int32_t>(views.size()),
                               ids.data(), static_cast<std::int32_t>(ids.size()), canonical ? 1 : 0,
                               max_iterations, &kss));
    std::int32_t n_nodes = 0;
    ksc::Check(ksh_kss_size(kss, &n_nodes));
    for (std::int32_t i = 0; i < n_nodes; i++) {
      ksh_spss_view v{nullptr, nullptr, 0, 0};
      std::int32_t holder = -1;
      ksc::Check(ksh_kss_node_holder(kss, i, &holder));
      holders_.push_back(holder);
      my_rank_ = shard.rank;
      if (holder < 0 || holder == shard.rank) ksc::Check(ksh_kss_node(kss, i, &v, nullptr, nullptr));
      ksc::DeviceBuffer words(std::size_t((v.n_bases + 31) / 32) * 8), lens(std::size_t(v.n_strings) * 4);
      if (v.n_bases) ksc::Check(ksh_ctx_memcpy_d2d(ksc::Ctx(), words.get(), v.d_words, std::size_t((v.n_bases + 31) / 32) * 8));
      if (v.n_strings) ksc::Check(ksh_ctx_memcpy_d2d(ksc::Ctx(), lens.get(), v.d_lens, std::size_t(v.n_strings) * 4));
      kmer_sets_compact_.push_back(Compact::FromDevice(std::move(words), std::move(lens), v.n_strings, v.n_bases));
      const std::int32_t* ch = nullptr;
      std::int32_t n_ch = 0;
      ksc::Check(ksh_kss_children(kss, i, &ch, &n_ch));
      if (n_ch) children_[i] = std::vector<int>(ch, ch + n_ch);
    }
    std::int64_t n_it = 0;
    const std::int64_t* rows = nullptr;
    ksc::Check(ksh_kss_trace(kss, &n_it, &rows, nullptr, nullptr, nullptr));
    for (std::int64_t i = 0; i < n_it; i++)
      iterations_.push_back({rows[5 * i], rows[5 * i + 1], rows[5 * i + 2], rows[5 * i + 3], rows[5 * i + 4]});
    ksc::Check(ksh_kss_stats(kss, stats_));
    ksc::Check(ksh_kss_destroy(kss));
  }

  int Size() const { return static_cast<int>(kmer_sets_compact_.size()); }

  // Rank holding node i's SPSS after a sharded construction; -1: every rank (and always after
  // a single-process construction or Load).
  int Holder(int i) const { return i < static_cast<int>(holders_.size()) ? holders_[i] : -1; }

  // Reconstructs the ith k-mer set: union over the nodes reachable from i.
  Set Get(int i, bool canonical, int n_workers) const {
    Set kmer_set;
    std::queue<int> queue;
    queue.push(i);
    while (!queue.empty()) {
      const int current = queue.front();
      queue.pop();
      kmer_set.Add(kmer_sets_compact_[current].ToKmerSet(canonical, n_workers), n_workers);
      auto it = children_.find(current);
      if (it != children_.end())
        for (int child : it->second) queue.push(child);
    }
    return kmer_set;
  }

  ksc::Status Dump(const std::string& directory_name, const std::string& compressor,
                   const std::string& extension, int n_workers) {
    try {
      std::filesystem::create_directories(directory_name);
    } catch (...) {
      return ksc::InternalError("failed to create a directory");
    }
    const std::filesystem::path dir(directory_name);
    if (my_rank_ == 0) {
      std::vector<std::string> v;
      v.push_back(internal::SerializeAdjacencyList(children_));
      v.push_back(std::to_string(kmer_sets_compact_.size()));
      ksc::Status status = ksc::WriteLines((dir / ("meta." + extension)).string(), compressor, v);
      if (!status.ok()) return status;
    }
    // One writer per worker, a node's file per task (kmer_set_set.h:497-519): each writer thread has
    // its own device context (ksc::Ctx() is per thread), spells its node's lines on the GPU and feeds
    // its own file or compressor pipe, so the (de)compressor processes of different nodes overlap.
    // After a sharded construction a node's file is written by the rank that holds it (the inputs,
    // held everywhere, by rank 0).
    std::vector<std::size_t> mine;
    for (std::size_t i = 0; i < kmer_sets_compact_.size(); i++) {
      const int holder = Holder(static_cast<int>(i));
      if (holder >= 0 ? holder == my_rank_ : my_rank_ == 0) mine.push_back(i);
    }
    std::atomic<std::size_t> next{0};
    std::atomic<int> fail_count{0};
    const auto writer = [&] {
      for (std::size_t q = next++; q < mine.size(); q = next++) {
        const std::size_t i = mine[q];
        ksc::Status status = ksc::InternalError("exception");
        try {
          status = kmer_sets_compact_[i].Dump((dir / (std::to_string(i) + "." + extension)).string(), compressor, 1);
        } catch (...) {
        }
        if (!status.ok()) fail_count += 1;
      }
    };
    const int n_threads = std::max(1, std::min<int>(n_workers, static_cast<int>(mine.size())));
    if (n_threads == 1) {
      writer();
    } else {
      std::vector<std::thread> pool;
      for (int w = 0; w < n_threads; w++) pool.emplace_back(writer);
      for (std::thread& t : pool) t.join();
    }
    if (fail_count > 0) return ksc::InternalError("failed to write " + std::to_string(fail_count) + " files");
    return ksc::OkStatus();
  }

  ksc::Status DumpGraph(const std::string& file_name) const {
    std::vector<std::string> lines;
    lines.emplace_back("digraph G {");
    for (const auto& p : children_)
      for (int i : p.second) lines.push_back("v" + std::to_string(p.first) + " -> v" + std::to_string(i));
    lines.emplace_back("}");
    return ksc::WriteLines(file_name, "", lines);
  }

  static ksc::StatusOr<KmerSetSet> Load(const std::string& directory_name, const std::string& decompressor,
                                        const std::string& extension, int /*n_workers*/) {
    const std::filesystem::path dir(directory_name);
    ksc::StatusOr<std::vector<std::string>> meta =
        ksc::ReadLines((dir / ("meta." + extension)).string(), decompressor);
    if (!meta.ok()) return meta.status();
    if (meta.value().size() < 2) return ksc::InternalError("malformed meta file");
    KmerSetSet out;
    out.children_ = internal::DeserializeAdjacencyList(meta.value()[0]);
    const int n = std::stoi(meta.value()[1]);
    int n_fail = 0;
    for (int i = 0; i < n; i++) {
      ksc::StatusOr<Compact> c = Compact::Load((dir / (std::to_string(i) + "." + extension)).string(), decompressor);
      if (!c.ok()) {
        n_fail += 1;
        continue;
      }
      out.kmer_sets_compact_.push_back(std::move(c).value());
    }
    if (n_fail > 0) return ksc::InternalError("failed to dump " + std::to_string(n_fail) + " files");
    return out;
  }

  // What the reference logs per iteration (kmer_set_set.h:324,380) and the totals.
  const std::vector<Iteration>& Iterations() const { return iterations_; }
  const std::map<int, std::vector<int>>& Children() const { return children_; }
  const Compact& Node(int i) const { return kmer_sets_compact_[i]; }
  std::int64_t ProcessedKmers() const { return stats_[3]; }        // N_proc of SURVEY.md 8(d)
  std::int64_t TotalSpssWeight() const { return stats_[4]; }

 private:
  internal::AdjacencyList children_;
  std::vector<Compact> kmer_sets_compact_;
  std::vector<int> holders_;  // sharded construction: the rank holding each node's SPSS (-1: all)
  int my_rank_ = 0;
  std::vector<Iteration> iterations_;
  std::int64_t stats_[8] = {};
};

// Which nodes' Get(i) hold each k-mer, for every node i (no counterpart in the reference): the index
// decodes the nodes of a KmerSetSet, constructed or Load()ed, once (ksh_kss_index_create), and answers
// batches of queries on the device.  Query returns Words() uint64 per query, row-major; bit i % 64 of
// word i / 64 is Get(i).Contains(kmer).  canonical = look up Canonical() of each k-mer (the call for a
// structure built with canonical = true).  Lives on the calling thread's context (ksc::Ctx()).
template <int K, int N, typename KeyType>
class KmerSetSetIndex {
 public:
  explicit KmerSetSetIndex(const KmerSetSet<K, N, KeyType>& kss, bool canonical = true) {
    const ksh_geom g = KmerSet<K, N, KeyType>::Geom();
    std::vector<ksh_spss_view> views;
    std::vector<std::int64_t> offsets{0};
    std::vector<std::int32_t> ids;
    for (int i = 0; i < kss.Size(); i++) {
      views.push_back(kss.Node(i).View());
      auto it = kss.Children().find(i);
      if (it != kss.Children().end()) ids.insert(ids.end(), it->second.begin(), it->second.end());
      offsets.push_back(static_cast<std::int64_t>(ids.size()));
    }
    ksc::Check(ksh_kss_index_create(ksc::Ctx(), &g, views.data(), static_cast<std::int32_t>(views.size()),
                                    offsets.data(), ids.data(), canonical ? 1 : 0, &index_));
    ksc::Check(ksh_kss_index_info(index_, &nodes_, &words_, nullptr));
  }
  KmerSetSetIndex(const KmerSetSetIndex&) = delete;
  KmerSetSetIndex& operator=(const KmerSetSetIndex&) = delete;
  ~KmerSetSetIndex() {
    if (index_) ksh_kss_index_destroy(index_);
  }

  int Words() const { return words_; }

  std::vector<std::uint64_t> Query(const std::vector<Kmer<K>>& kmers, bool canonical) const {
    std::vector<std::uint64_t> bits;
    bits.reserve(kmers.size());
    for (const Kmer<K>& kmer : kmers) bits.push_back(kmer.Bits());
    if (bits.empty()) return {};
    const ksc::DeviceBuffer d_kmers = ksc::DeviceBuffer::FromHost(bits);
    ksc::DeviceBuffer d_rows(bits.size() * std::size_t(words_) * 8);
    ksc::Check(ksh_kss_index_query(index_, static_cast<const std::uint64_t*>(d_kmers.get()),
                                   static_cast<std::int64_t>(bits.size()), canonical ? 1 : 0, 0,
                                   static_cast<std::uint64_t*>(d_rows.get())));
    return d_rows.ToHost<std::uint64_t>(bits.size() * std::size_t(words_));
  }

  int Nodes() const { return nodes_; }

  // Hits per sequence and node (ksh_seq_hits): element s * Nodes() + i is the number of k-mer positions of
  // string s of `sequences` whose k-mer -- its Canonical() with canonical = true -- is in Get(i).  A k-mer
  // that occurs twice in a string counts twice.
  std::vector<std::uint32_t> CountHits(const KmerSetCompact<K, N, KeyType>& sequences, bool canonical) const {
    const std::size_t cells = std::size_t(sequences.StringCount()) * std::size_t(nodes_);
    if (cells == 0) return {};
    const ksh_spss_view v = sequences.View();
    ksc::DeviceBuffer d_hits(cells * 4);
    ksc::Check(ksh_seq_hits(&v, index_, canonical ? 1 : 0, 0, 0, static_cast<std::uint32_t*>(d_hits.get())));
    return d_hits.ToHost<std::uint32_t>(cells);
  }
  // The same for strings over ACGT, each at least K long.
  std::vector<std::uint32_t> CountHits(const std::vector<std::string>& sequences, bool canonical) const {
    return CountHits(KmerSetCompact<K, N, KeyType>::FromStrings(sequences), canonical);
  }

  // Exact pairwise intersection counts (ksh_kss_pair_counts): element a * n + b is |Get(cols[a]) & Get(cols[b])|,
  // n = cols.size(); at most 128 distinct node ids in any order.  Empty `cols`: all nodes in order (n = Nodes(),
  // refused above 128 nodes).
  std::vector<std::int64_t> PairCounts(const std::vector<int>& cols = {}) const {
    const std::vector<std::int32_t> ids(cols.begin(), cols.end());
    const std::size_t n = ids.empty() ? std::size_t(nodes_) : ids.size();
    const std::size_t side = n < 128 ? n : 128;  // (what the call refuses is never written)
    ksc::DeviceBuffer d_counts(side * side * 8);
    ksc::Check(ksh_kss_pair_counts(ids.empty() ? nullptr : ids.data(), static_cast<std::int32_t>(ids.size()), index_,
                                   0, static_cast<std::int64_t*>(d_counts.get()), nullptr));
    return d_counts.ToHost<std::int64_t>(n * n);
  }

  // The k-mers q with min_count <= c(q) <= max_count, c(q) = the number of a with q in Get(cols[a]), that are in
  // Get(r) for every r of `require` and in no Get(x) of `exclude` (ksh_kss_select_count + ksh_kss_select_keys): one
  // pass over the node sets each, no Get(i) is formed.  At most 128 distinct node ids in `cols`, any order; empty
  // `cols`: all nodes (refused above 128 nodes); max_count == 0: the number of columns.  The core of cols is
  // Select(cols, cols.size(), 0), the k-mers private to s are Select(cols, 1, 1, {s}).
  KmerSet<K, N, KeyType> Select(const std::vector<int>& cols, int min_count = 1, int max_count = 0,
                                const std::vector<int>& require = {}, const std::vector<int>& exclude = {}) const {
    using Set = KmerSet<K, N, KeyType>;
    const std::vector<std::int32_t> ids(cols.begin(), cols.end()), req(require.begin(), require.end()),
        exc(exclude.begin(), exclude.end());
    const ksh_kss_selection sel = Selection(ids, min_count, max_count, req, exc);
    ksc::DeviceBuffer off(std::size_t(Set::kBucketsNum + 1) * 8);
    std::int64_t n = 0;
    ksc::Check(ksh_kss_select_count(&sel, index_, static_cast<std::int64_t*>(off.get()), &n, nullptr));
    ksc::DeviceBuffer keys(std::max<std::size_t>(std::size_t(n) * Set::kDeviceKeyBytes, 16));
    ksc::Check(ksh_kss_select_keys(&sel, index_, static_cast<const std::int64_t*>(off.get()), n, keys.get()));
    return Set::FromDevice(std::move(off), std::move(keys), n);
  }

  // Element m: the number of distinct k-mers of the whole structure that exactly m of the sets Get(cols[a]) hold
  // (element 0: those that only nodes outside cols hold); cols.size() + 1 elements.  Empty `cols`: all nodes.
  std::vector<std::int64_t> Spectrum(const std::vector<int>& cols = {}) const {
    const std::vector<std::int32_t> ids(cols.begin(), cols.end());
    const ksh_kss_selection sel = Selection(ids, 1, 0, {}, {});
    const std::size_t n = ids.empty() ? std::size_t(nodes_) : ids.size();
    std::vector<std::int64_t> spectrum((n < 128 ? n : 128) + 1, 0);  // (what the call refuses is never written)
    ksc::Check(ksh_kss_select_count(&sel, index_, nullptr, nullptr, spectrum.data()));
    return spectrum;
  }

  // A colour class: a distinct membership pattern over the chosen columns (bit a % 64 of row[a / 64]: the class's
  // k-mers are in Get(cols[a])) and the number of distinct k-mers of the structure with exactly that pattern.
  struct ColorClass {
    std::array<std::uint64_t, 2> row;
    std::int64_t count;
  };
  // Every colour class of `cols` (ksh_kss_color_classes), ascending by (row[1], row[0]); the zero row counts the
  // k-mers that only nodes outside cols hold.  At most 128 distinct node ids in any order; empty `cols`: all nodes
  // (refused above 128 nodes).  capacity: the classes there is room for; 0: min(2^n, 2^16), times 4 for as long as
  // the call answers that there are more, up to min(2^n, 2^24), where the refusal is thrown.  A given capacity is
  // tried once.
  std::vector<ColorClass> ColorClasses(const std::vector<int>& cols = {}, std::int64_t capacity = 0) const {
    const std::vector<std::int32_t> ids(cols.begin(), cols.end());
    const std::size_t n = ids.empty() ? std::size_t(nodes_) : ids.size();
    const std::int64_t top = std::int64_t(1) << std::min<std::size_t>(n, 24);
    std::int64_t cap = capacity > 0 ? capacity : std::min<std::int64_t>(top, std::int64_t(1) << 16);
    for (;;) {
      const std::size_t room = std::size_t(std::min<std::int64_t>(cap, std::int64_t(1) << 24));
      std::vector<std::uint64_t> rows(2 * room);  // (what the call refuses is never written)
      std::vector<std::int64_t> counts(room);
      std::int64_t got = 0;
      const int rc = ksh_kss_color_classes(ids.empty() ? nullptr : ids.data(), static_cast<std::int32_t>(ids.size()),
                                           index_, cap, rows.data(), counts.data(), &got);
      if (rc == KSH_FAILED_PRECONDITION && got == cap + 1 && capacity <= 0 && cap < top) {
        cap = std::min<std::int64_t>(4 * cap, top);
        continue;
      }
      ksc::Check(rc);
      std::vector<ColorClass> out(static_cast<std::size_t>(got));
      for (std::size_t c = 0; c < out.size(); c++) out[c] = ColorClass{{rows[2 * c], rows[2 * c + 1]}, counts[c]};
      return out;
    }
  }

  // The selection of Select with the colour class of every k-mer (ksh_kss_select_class_ids): the set, and for the
  // i-th k-mer of the set in ascending order -- the order of Find() -- the position in `classes` of its membership
  // pattern over cols.  `classes` is what ColorClasses(cols) returned, or any part of it in the same order that
  // holds the pattern of every selected k-mer; a table that misses one (that of other columns or another
  // structure) is refused.  The union selection with the whole table is a coloured de Bruijn graph.
  std::pair<KmerSet<K, N, KeyType>, std::vector<std::uint32_t>> SelectClasses(
      const std::vector<int>& cols, const std::vector<ColorClass>& classes, int min_count = 1, int max_count = 0,
      const std::vector<int>& require = {}, const std::vector<int>& exclude = {}) const {
    using Set = KmerSet<K, N, KeyType>;
    const std::vector<std::int32_t> ids(cols.begin(), cols.end()), req(require.begin(), require.end()),
        exc(exclude.begin(), exclude.end());
    const ksh_kss_selection sel = Selection(ids, min_count, max_count, req, exc);
    std::vector<std::uint64_t> rows;
    rows.reserve(2 * classes.size());
    for (const ColorClass& c : classes) rows.insert(rows.end(), {c.row[0], c.row[1]});
    ksc::DeviceBuffer off(std::size_t(Set::kBucketsNum + 1) * 8);
    std::int64_t n = 0;
    ksc::Check(ksh_kss_select_count(&sel, index_, static_cast<std::int64_t*>(off.get()), &n, nullptr));
    ksc::DeviceBuffer keys(std::max<std::size_t>(std::size_t(n) * Set::kDeviceKeyBytes, 16));
    ksc::DeviceBuffer d_ids(std::max<std::size_t>(std::size_t(n) * 4, 16));
    if (n > 0 || !rows.empty())  // (an index without k-mers has no class, and the call takes no empty table)
      ksc::Check(ksh_kss_select_class_ids(&sel, index_, rows.data(), static_cast<std::int64_t>(classes.size()),
                                          static_cast<const std::int64_t*>(off.get()), n, keys.get(),
                                          static_cast<std::uint32_t*>(d_ids.get()), nullptr));
    std::vector<std::uint32_t> out;
    if (n > 0) out = d_ids.ToHost<std::uint32_t>(std::size_t(n));
    return {Set::FromDevice(std::move(off), std::move(keys), n), std::move(out)};
  }

  // Sequences painted with colour classes (ksh_seq_class_runs): the runs of string s are runs offsets[s] ..
  // offsets[s + 1); run r begins at k-mer position start[r] of its string (the first run of a string at 0), ends
  // before the next run of the string begins or with the string, and every k-mer position of it has the membership
  // pattern classes[cls[r]] over cols -- or, with cls[r] == kNoClass, a pattern that `classes` does not hold.
  // n_unmatched is the number of such positions.
  struct ClassRuns {
    std::vector<std::int64_t> offsets;
    std::vector<std::uint32_t> start, cls;
    std::int64_t n_unmatched = 0;
  };
  static constexpr std::uint32_t kNoClass = KSH_CLASS_NONE;
  // `classes`: what ColorClasses(cols) returned, or any part of it in the same order.  A k-mer that no node holds,
  // or only nodes outside cols, has the zero pattern.  allow_unmatched = false: a position whose pattern `classes`
  // does not hold is refused.  capacity: the runs there is room for; 0: one call counts them and a second one
  // writes them; a given capacity that is too small is refused with the number of runs in the message.
  ClassRuns Paint(const KmerSetCompact<K, N, KeyType>& sequences, const std::vector<int>& cols,
                  const std::vector<ColorClass>& classes, bool canonical = true, bool allow_unmatched = true,
                  std::int64_t capacity = 0) const {
    const std::vector<std::int32_t> ids(cols.begin(), cols.end());
    std::vector<std::uint64_t> rows;
    rows.reserve(2 * classes.size());
    for (const ColorClass& c : classes) rows.insert(rows.end(), {c.row[0], c.row[1]});
    ksh_seq_paint req{};
    req.struct_size = sizeof(req);
    req.cols = ids.empty() ? nullptr : ids.data();
    req.n_cols = static_cast<std::int32_t>(ids.size());
    req.canonicalize = canonical ? 1 : 0;
    req.rows = rows.data();
    req.n_classes = static_cast<std::int64_t>(classes.size());
    const ksh_spss_view v = sequences.View();
    const std::size_t n = std::size_t(sequences.StringCount());
    ClassRuns out;
    std::int64_t n_runs = 0;
    std::int64_t* missing = allow_unmatched ? &out.n_unmatched : nullptr;
    ksc::DeviceBuffer off((n + 1) * 8);
    if (capacity <= 0) {
      ksc::Check(ksh_seq_class_runs(&v, index_, &req, 0, nullptr, nullptr, nullptr, &n_runs, missing));
      capacity = n_runs;
    }
    const std::size_t room = std::max<std::size_t>(std::size_t(capacity) * 4, 16);
    ksc::DeviceBuffer start(room), cls(room);
    ksc::Check(ksh_seq_class_runs(&v, index_, &req, capacity, static_cast<std::int64_t*>(off.get()),
                                  capacity > 0 ? static_cast<std::uint32_t*>(start.get()) : nullptr,
                                  capacity > 0 ? static_cast<std::uint32_t*>(cls.get()) : nullptr, &n_runs, missing));
    out.offsets = off.ToHost<std::int64_t>(n + 1);
    if (n_runs > 0) {
      out.start = start.ToHost<std::uint32_t>(std::size_t(n_runs));
      out.cls = cls.ToHost<std::uint32_t>(std::size_t(n_runs));
    }
    return out;
  }
  // The same for strings over ACGT, each at least K long.
  ClassRuns Paint(const std::vector<std::string>& sequences, const std::vector<int>& cols,
                  const std::vector<ColorClass>& classes, bool canonical = true, bool allow_unmatched = true,
                  std::int64_t capacity = 0) const {
    return Paint(KmerSetCompact<K, N, KeyType>::FromStrings(sequences), cols, classes, canonical, allow_unmatched,
                 capacity);
  }

  // The coloured de Bruijn graph of `cols` as monochromatic strings (coloured unitigs): `strings` holds every k-mer
  // that a column holds exactly once, all k-mers of string r have the membership pattern classes[cls[r]] over cols,
  // and `classes` is ColorClasses(cols).  The union selection is encoded (KmerSetCompact::FromKmerSet), painted
  // (Paint) and cut at the runs (KmerSetCompact::Cut, ksh_spss_cut).  canonical: as the structure was built.
  struct ColoredStrings {
    KmerSetCompact<K, N, KeyType> strings;
    std::vector<std::uint32_t> cls;
    std::vector<ColorClass> classes;
  };
  ColoredStrings ColoredUnitigs(const std::vector<int>& cols, bool canonical = true) const {
    ColoredStrings out;
    out.classes = ColorClasses(cols);
    const KmerSet<K, N, KeyType> all = SelectClasses(cols, out.classes).first;
    if (all.Size() == 0) return out;
    const auto uncut = KmerSetCompact<K, N, KeyType>::FromKmerSet(all, canonical, true, 1);
    ClassRuns runs = Paint(uncut, cols, out.classes, canonical, false);
    out.strings = uncut.Cut(runs.offsets, runs.start);
    out.cls = std::move(runs.cls);
    return out;
  }

  // The coloured compacted de Bruijn graph of `cols`, nodes and edges: as ColoredUnitigs, but the union selection is
  // encoded as unitigs (KmerSetCompact::UnitigsOf), so that the strings are pieces of unitigs and `links`
  // (KmerSetCompact::Links of them, ksh_spss_links) holds every edge of the graph.
  struct ColoredGraphResult {
    KmerSetCompact<K, N, KeyType> strings;
    std::vector<std::uint32_t> cls;
    std::vector<ColorClass> classes;
    typename KmerSetCompact<K, N, KeyType>::LinkList links;
  };
  ColoredGraphResult ColoredGraph(const std::vector<int>& cols, bool canonical = true) const {
    ColoredGraphResult out;
    out.classes = ColorClasses(cols);
    out.links.offsets.assign(1, 0);
    const KmerSet<K, N, KeyType> all = SelectClasses(cols, out.classes).first;
    if (all.Size() == 0) return out;
    const auto uncut = KmerSetCompact<K, N, KeyType>::UnitigsOf(all, canonical);
    ClassRuns runs = Paint(uncut, cols, out.classes, canonical, false);
    out.strings = uncut.Cut(runs.offsets, runs.start);
    out.cls = std::move(runs.cls);
    out.links = out.strings.Links(canonical);
    return out;
  }

  // The bubbles of that graph (KmerSetCompact::LinkBubbles of its links, ksh_link_bubbles) with the graph's classes
  // passed in: `graph` is ColoredGraph(cols), `bubbles` its variant sites with arms of at most max_arm strings, and
  // bit a of an arm's two words in bubbles.arm_rows is column cols[a].  The graph is built canonical: the call takes
  // no other links.
  struct ColoredBubblesResult {
    ColoredGraphResult graph;
    typename KmerSetCompact<K, N, KeyType>::BubbleList bubbles;
  };
  ColoredBubblesResult ColoredBubbles(const std::vector<int>& cols, int max_arm = 8) const {
    ColoredBubblesResult out;
    out.graph = ColoredGraph(cols, true);
    std::vector<std::uint64_t> rows;
    rows.reserve(2 * out.graph.classes.size());
    for (const ColorClass& c : out.graph.classes) rows.insert(rows.end(), {c.row[0], c.row[1]});
    if (out.graph.cls.empty()) rows.clear();  // (no string, no class to name: the call takes no empty table)
    out.bubbles = KmerSetCompact<K, N, KeyType>::LinkBubbles(out.graph.links.offsets, out.graph.links.to, max_arm,
                                                            out.graph.cls, rows);
    return out;
  }

 private:
  static ksh_kss_selection Selection(const std::vector<std::int32_t>& ids, int min_count, int max_count,
                                     const std::vector<std::int32_t>& req, const std::vector<std::int32_t>& exc) {
    ksh_kss_selection sel{};
    sel.struct_size = sizeof(sel);
    sel.cols = ids.empty() ? nullptr : ids.data();
    sel.n_cols = static_cast<std::int32_t>(ids.size());
    sel.min_count = min_count;
    sel.max_count = max_count;
    sel.require = req.data();
    sel.n_require = static_cast<std::int32_t>(req.size());
    sel.exclude = exc.data();
    sel.n_exclude = static_cast<std::int32_t>(exc.size());
    return sel;
  }

  ksh_kss_index* index_ = nullptr;
  std::int32_t words_ = 0, nodes_ = 0;
};

// Reconstructs sets from a dumped directory without loading every node
// (lib/core/kmer_set_set.h:629-775).
template <int K, int N, typename KeyType>
class KmerSetSetReader {
 public:
  using Compact = KmerSetCompact<K, N, KeyType>;
  using Set = KmerSet<K, N, KeyType>;

  KmerSetSetReader() = default;

  static ksc::StatusOr<KmerSetSetReader> FromDirectory(std::string directory_name, std::string extension,
                                                       std::string decompressor, bool canonical) {
    const std::filesystem::path dir(directory_name);
    ksc::StatusOr<std::vector<std::string>> meta =
        ksc::ReadLines((dir / ("meta." + extension)).string(), decompressor);
    if (!meta.ok()) return meta.status();
    if (meta.value().size() < 2) return ksc::InternalError("malformed meta file");
    KmerSetSetReader r;
    r.directory_name_ = std::move(directory_name);
    r.extension_ = std::move(extension);
    r.decompressor_ = std::move(decompressor);
    r.canonical_ = canonical;
    r.children_ = internal::DeserializeAdjacencyList(meta.value()[0]);
    r.size_ = std::stoi(meta.value()[1]);
    return r;
  }

  int Size() const { return size_; }

  ksc::StatusOr<Set> Get(int i, int n_workers) const {
    std::vector<int> ids;
    std::queue<int> queue;
    queue.push(i);
    while (!queue.empty()) {
      const int current = queue.front();
      queue.pop();
      ids.push_back(current);
      auto it = children_.find(current);
      if (it == children_.end()) continue;
      for (int child : it->second) queue.push(child);
    }
    Set to_return;
    int n_fail = 0;
    const std::filesystem::path dir(directory_name_);
    for (int id : ids) {
      ksc::StatusOr<Compact> c = Compact::Load((dir / (std::to_string(id) + "." + extension_)).string(), decompressor_);
      if (!c.ok()) {
        n_fail += 1;
        continue;
      }
      to_return.Add(c.value().ToKmerSet(canonical_, 1), n_workers);
    }
    if (n_fail > 0) return ksc::InternalError("failed to load data from " + std::to_string(n_fail) + " files");
    return to_return;
  }

 private:
  std::string directory_name_, extension_, decompressor_;
  bool canonical_ = true;
  internal::AdjacencyList children_;
  int size_ = 0;
};

#endif
