// KmerSetCompact<K, N, KeyType>: the reference's SPSS container
// (lib/core/kmer_set_compact.h:29-348) with its bases resident in HBM: 2 bits per base
// in 64-bit words + (len - K) per string (layout in include/kmersets_hip.h).
//   FromKmerSet  -> ksh_spss_encode_plan/write  (GetSPSSCanonical fast / slow, or GetSPSS for
//                   canonical == false)
//   ToKmerSet    -> ksh_spss_decode_plan/write  (ToStrings + GetKmerSetFromSPSS)
//   Size, Weight -> ksh_spss_size, n_bases
//   GetSampledKmerSet -> decode, then the listed buckets (already sorted)
//   Dump / Load  -> the reference's text format (one string per line)
#ifndef KSC_CORE_KMER_SET_COMPACT_H_
#define KSC_CORE_KMER_SET_COMPACT_H_

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "core/device.h"
#include "core/io.h"
#include "core/kmer.h"
#include "core/kmer_set.h"
#include "core/status.h"

template <int K, int N, typename KeyType>
class KmerSetCompact {
 public:
  using Set = KmerSet<K, N, KeyType>;

  KmerSetCompact() = default;

  // lib/core/kmer_set_compact.h:36-47: canonical ? GetSPSSCanonical(set, fast) : GetSPSS(set).
  static KmerSetCompact FromKmerSet(const Set& kmer_set, bool canonical, bool fast, int /*n_workers*/) {
    const ksh_geom g = Set::Geom();
    const ksh_set_view v = kmer_set.View();
    KmerSetCompact c;
    ksc::Check(ksh_spss_encode_plan(ksc::Ctx(), &g, &v, canonical ? 1 : 0, fast ? 0 : 2, &c.n_,
                                    &c.n_bases_));
    c.words_ = ksc::DeviceBuffer(std::size_t((c.n_bases_ + 31) / 32) * 8);
    c.lens_ = ksc::DeviceBuffer(std::size_t(c.n_) * 4);
    ksc::Check(ksh_spss_encode_write_for(ksc::Ctx(), static_cast<std::uint64_t*>(c.words_.get()),
                                         static_cast<std::uint32_t*>(c.lens_.get()), c.n_, c.n_bases_,
                                         v.d_offsets));
    ksc::Check(ksh_ctx_sync(ksc::Ctx()));
    ksc::Check(ksh_spss_encode_release(ksc::Ctx()));
    return c;
  }

  // The unitigs of the set as a container (GetUnitigsCanonical / GetUnitigs kept on the device: ksh_spss_encode,
  // mode 1).  Links() of it, or of any Cut of it, is the whole de Bruijn graph of the set.
  static KmerSetCompact UnitigsOf(const Set& kmer_set, bool canonical) {
    const ksh_geom g = Set::Geom();
    const ksh_set_view v = kmer_set.View();
    KmerSetCompact c;
    ksc::Check(ksh_spss_encode_plan(ksc::Ctx(), &g, &v, canonical ? 1 : 0, 1, &c.n_, &c.n_bases_));
    c.words_ = ksc::DeviceBuffer(std::size_t((c.n_bases_ + 31) / 32) * 8);
    c.lens_ = ksc::DeviceBuffer(std::size_t(c.n_) * 4);
    ksc::Check(ksh_spss_encode_write_for(ksc::Ctx(), static_cast<std::uint64_t*>(c.words_.get()),
                                         static_cast<std::uint32_t*>(c.lens_.get()), c.n_, c.n_bases_,
                                         v.d_offsets));
    ksc::Check(ksh_ctx_sync(ksc::Ctx()));
    ksc::Check(ksh_spss_encode_release(ksc::Ctx()));
    return c;
  }

  // From SPSS strings over ACGT (the reference's private constructor, :206-266).
  static KmerSetCompact FromStrings(const std::vector<std::string>& spss) {
    KmerSetCompact c;
    c.n_ = static_cast<std::int64_t>(spss.size());
    std::vector<std::uint32_t> lens(spss.size());
    std::int64_t total = 0;
    for (std::size_t i = 0; i < spss.size(); i++) {
      lens[i] = static_cast<std::uint32_t>(spss[i].length()) - static_cast<std::uint32_t>(K);
      total += static_cast<std::int64_t>(spss[i].length());
    }
    c.n_bases_ = total;
    std::vector<std::uint64_t> words(static_cast<std::size_t>((total + 31) / 32), 0);
    std::int64_t at = 0;
    for (const std::string& s : spss) {
      for (char ch : s) {
        std::uint64_t code = 0;
        switch (ch) {
          case 'C': code = 1; break;
          case 'G': code = 2; break;
          case 'T': code = 3; break;
          default: break;
        }
        words[at / 32] |= code << (62 - 2 * (at % 32));
        at++;
      }
    }
    c.words_ = ksc::DeviceBuffer::FromHost(words);
    c.lens_ = ksc::DeviceBuffer::FromHost(lens);
    return c;
  }

  // Takes ownership of device buffers in the C-ABI layout.
  static KmerSetCompact FromDevice(ksc::DeviceBuffer words, ksc::DeviceBuffer lens, std::int64_t n_strings,
                                   std::int64_t n_bases) {
    KmerSetCompact c;
    c.words_ = std::move(words);
    c.lens_ = std::move(lens);
    c.n_ = n_strings;
    c.n_bases_ = n_bases;
    return c;
  }

  Set ToKmerSet(bool canonical, int /*n_workers*/) const {
    const ksh_geom g = Set::Geom();
    const ksh_spss_view v = View();
    ksc::DeviceBuffer off(std::size_t(Set::kBucketsNum + 1) * 8);
    std::int64_t n = 0;
    ksc::Check(ksh_spss_decode_plan(ksc::Ctx(), &g, &v, canonical ? 1 : 0,
                                    static_cast<std::int64_t*>(off.get()), &n));
    ksc::DeviceBuffer keys(std::size_t(n) * Set::kDeviceKeyBytes);
    ksc::Check(ksh_spss_decode_write(ksc::Ctx(), &g, &v, canonical ? 1 : 0,
                                     static_cast<std::int64_t*>(off.get()), keys.get(), &n));
    return Set::FromDevice(std::move(off), std::move(keys), n);
  }

  // The lines are spelled on the device (ksh_spss_to_text); the host writes one buffer.
  ksc::Status Dump(const std::string& file_name, const std::string& compressor, int /*n_workers*/) const {
    const std::string text = ToText();
    return ksc::WriteBytes(file_name, compressor, text.data(), text.size());
  }

  // The file's bytes go to the device as they are and are parsed there
  // (ksh_spss_from_text_plan / _write).
  static ksc::StatusOr<KmerSetCompact> Load(const std::string& file_name, const std::string& decompressor) {
    ksc::StatusOr<std::string> bytes = ksc::ReadBytes(file_name, decompressor);
    if (!bytes.ok()) return bytes.status();
    return FromText(bytes.value());
  }

  // "line\nline\n...": the text Dump writes.
  std::string ToText() const {
    std::string text(static_cast<std::size_t>(n_bases_ + n_), '\0');
    if (text.empty()) return text;
    const ksh_geom g = Set::Geom();
    const ksh_spss_view v = View();
    ksc::DeviceBuffer d_text(text.size());
    ksc::Check(ksh_spss_to_text(ksc::Ctx(), &g, &v, static_cast<char*>(d_text.get())));
    ksc::Check(ksh_ctx_sync(ksc::Ctx()));
    ksc::Check(ksh_ctx_memcpy_d2h(ksc::Ctx(), &text[0], d_text.get(), text.size()));
    return text;
  }

  static KmerSetCompact FromText(const std::string& text) {
    KmerSetCompact c;
    if (text.empty()) return c;
    const ksh_geom g = Set::Geom();
    ksc::DeviceBuffer d_text(text.size());
    ksc::Check(ksh_ctx_memcpy_h2d(ksc::Ctx(), d_text.get(), text.data(), text.size()));
    ksc::Check(ksh_spss_from_text_plan(ksc::Ctx(), &g, static_cast<const char*>(d_text.get()),
                                       static_cast<std::int64_t>(text.size()), &c.n_, &c.n_bases_));
    c.words_ = ksc::DeviceBuffer(std::size_t((c.n_bases_ + 31) / 32) * 8);
    c.lens_ = ksc::DeviceBuffer(std::size_t(c.n_) * 4);
    ksc::Check(ksh_spss_from_text_write_for(ksc::Ctx(), static_cast<std::uint64_t*>(c.words_.get()),
                                            static_cast<std::uint32_t*>(c.lens_.get()), c.n_, c.n_bases_,
                                            d_text.get()));
    return c;
  }

  std::int64_t Size(int /*n_workers*/) const {
    const ksh_geom g = Set::Geom();
    const ksh_spss_view v = View();
    std::int64_t n = 0;
    ksc::Check(ksh_spss_size(ksc::Ctx(), &g, &v, &n));
    return n;
  }

  std::int64_t Weight() const { return n_bases_; }

  // The strings cut at k-mer positions (ksh_spss_cut): the runs of string s are runs offsets[s] .. offsets[s + 1),
  // run r begins at position start[r] of its string (the first run of a string at 0) -- the run list that
  // KmerSetSetIndex::Paint returns.  Every run becomes a string of its own, the K - 1 bases behind a cut repeated:
  // the same k-mers in the same order, in offsets.back() strings.
  KmerSetCompact Cut(const std::vector<std::int64_t>& offsets, const std::vector<std::uint32_t>& start) const {
    const ksh_geom g = Set::Geom();
    const ksh_spss_view v = View();
    KmerSetCompact c;
    c.n_ = static_cast<std::int64_t>(start.size());
    if (offsets.size() != std::size_t(n_) + 1) throw std::invalid_argument("Cut: offsets holds n_strings + 1 values");
    c.n_bases_ = n_bases_ + (c.n_ - n_) * (K - 1);  // (the closed form: the call needs no plan)
    if (c.n_ < n_) throw std::invalid_argument("Cut: fewer runs than strings");
    c.words_ = ksc::DeviceBuffer(std::size_t((c.n_bases_ + 31) / 32) * 8);
    c.lens_ = ksc::DeviceBuffer(start.size() * 4);
    const ksc::DeviceBuffer d_off = ksc::DeviceBuffer::FromHost(offsets);
    const ksc::DeviceBuffer d_start = ksc::DeviceBuffer::FromHost(start);
    ksc::Check(ksh_spss_cut(&v, ksc::Ctx(), &g, static_cast<const std::int64_t*>(d_off.get()),
                            static_cast<const std::uint32_t*>(d_start.get()), c.n_,
                            static_cast<std::uint64_t*>(c.words_.get()), static_cast<std::uint32_t*>(c.lens_.get()),
                            &c.n_bases_));
    return c;
  }

  // The links between the strings (ksh_spss_links), the edges of the graph whose nodes they are.  The oriented
  // string v = 2 s + o is string s as written (o = 0) or reverse-complemented (o = 1); v -> w is a link when the last
  // k-mer of v moved on by one base is the first k-mer of w, a k-mer followed by itself (canonical: or by its reverse
  // complement) excepted.  The links of v are to[offsets[v]] .. to[offsets[v + 1]), ascending by the appended base;
  // canonical == false: only the rows 2 s have any.  Only string ends are looked at.
  struct LinkList {
    std::vector<std::int64_t> offsets, to;
  };
  LinkList Links(bool canonical = true) const {
    const ksh_geom g = Set::Geom();
    const ksh_spss_view v = View();
    LinkList out;
    std::int64_t n_links = 0;
    ksc::DeviceBuffer off(std::size_t(2 * n_ + 1) * 8);
    ksc::Check(ksh_spss_links(&v, ksc::Ctx(), &g, canonical ? 1 : 0, 0, static_cast<std::int64_t*>(off.get()), nullptr,
                              &n_links));
    out.offsets = off.ToHost<std::int64_t>(std::size_t(2 * n_ + 1));
    if (n_links > 0) {
      ksc::DeviceBuffer to(std::size_t(n_links) * 8);
      ksc::Check(ksh_spss_links(&v, ksc::Ctx(), &g, canonical ? 1 : 0, n_links, nullptr,
                                static_cast<std::int64_t*>(to.get()), &n_links));
      out.to = to.ToHost<std::int64_t>(std::size_t(n_links));
    }
    return out;
  }

  // The bubbles of a link graph (ksh_link_bubbles) over the vectors Links(true) returns: a source v with two links,
  // two arms of at most max_arm strings each -- every arm string has one link in and one out -- and the sink w where
  // both arms end.  Each bubble is listed once, as the twin with v <= w ^ 1, ascending by v: bubble b has source
  // ends[2 b] and sink ends[2 b + 1], and its arm i (arm 0: the lower base) is arm_strings[arm_offsets[2 b + i]] ..
  // [arm_offsets[2 b + i + 1]), oriented strings in walk order.  With `classes` (the class of every string) and
  // `rows` (the class table, two words a class) arm_rows holds two words an arm: the AND of the rows of its strings'
  // classes, the columns that hold every k-mer of the allele (a column that holds only part of an arm is not a
  // carrier); without both it stays empty.  Only canonical links are taken: a link without its twin is refused.
  struct BubbleList {
    std::vector<std::int64_t> ends, arm_offsets, arm_strings;
    std::vector<std::uint64_t> arm_rows;
    std::size_t Size() const { return ends.size() / 2; }
  };
  static BubbleList LinkBubbles(const std::vector<std::int64_t>& offsets, const std::vector<std::int64_t>& to,
                                int max_arm = 8, const std::vector<std::uint32_t>& classes = {},
                                const std::vector<std::uint64_t>& rows = {}) {
    const bool colored = !classes.empty() || !rows.empty();
    const ksc::DeviceBuffer d_off = ksc::DeviceBuffer::FromHost(offsets), d_to = ksc::DeviceBuffer::FromHost(to);
    const ksc::DeviceBuffer d_cls = ksc::DeviceBuffer::FromHost(classes);
    ksh_link_graph graph{};
    graph.struct_size = sizeof(graph);
    graph.n_strings = offsets.empty() ? 0 : std::int64_t(offsets.size() - 1) / 2;
    graph.d_link_offsets = static_cast<const std::int64_t*>(d_off.get());
    graph.d_link_to = static_cast<const std::int64_t*>(d_to.get());
    graph.n_links = std::int64_t(to.size());
    graph.d_string_class = classes.empty() ? nullptr : static_cast<const std::int32_t*>(d_cls.get());
    graph.rows = rows.empty() ? nullptr : rows.data();
    graph.n_classes = std::int64_t(rows.size() / 2);
    BubbleList out;
    std::int64_t n_bubbles = 0, n_arm = 0;
    ksc::Check(ksh_link_bubbles(&graph, ksc::Ctx(), max_arm, 0, 0, nullptr, nullptr, nullptr, nullptr, &n_bubbles,
                                &n_arm));
    out.arm_offsets.assign(1, 0);
    if (n_bubbles == 0) return out;
    const std::size_t nb = std::size_t(n_bubbles), na = std::size_t(n_arm);
    ksc::DeviceBuffer ends(2 * nb * 8), arm_off((2 * nb + 1) * 8), arm(na * 8), arm_rows(colored ? 4 * nb * 8 : 0);
    ksc::Check(ksh_link_bubbles(&graph, ksc::Ctx(), max_arm, n_bubbles, n_arm, static_cast<std::int64_t*>(ends.get()),
                                static_cast<std::int64_t*>(arm_off.get()), static_cast<std::int64_t*>(arm.get()),
                                colored ? static_cast<std::uint64_t*>(arm_rows.get()) : nullptr, &n_bubbles, &n_arm));
    out.ends = ends.ToHost<std::int64_t>(2 * nb);
    out.arm_offsets = arm_off.ToHost<std::int64_t>(2 * nb + 1);
    out.arm_strings = arm.ToHost<std::int64_t>(na);
    if (colored) out.arm_rows = arm_rows.ToHost<std::uint64_t>(4 * nb);
    return out;
  }

  // Where the ends of the strings occur in `reference` (ksh_seq_locate).  End 2 s is the first k-mer of string s as
  // written, end 2 s + 1 its last.  count[e] is the number of k-mer positions of the reference that hold the end's
  // k-mer (canonical: or its reverse complement); where[e] is (g << 1) | strand of the one with the smallest global
  // position g, strand 1 meaning that the reference reads the reverse complement, or -1.  Global positions number
  // the k-mer positions of all reference sequences in one line: sequence r owns length(r) - K + 1 of them.
  struct LocateList {
    std::vector<std::int64_t> where;
    std::vector<std::uint32_t> count;
    std::int64_t n_located = 0;
  };
  LocateList Locate(const KmerSetCompact& reference, bool canonical = true) const {
    const ksh_geom g = Set::Geom();
    const ksh_spss_view strings = View(), ref = reference.View();
    LocateList out;
    if (n_ == 0) return out;
    ksc::DeviceBuffer where(std::size_t(2 * n_) * 8), count(std::size_t(2 * n_) * 4);
    ksh_seq_locate_req req{};
    req.struct_size = sizeof(req);
    req.ctx = ksc::Ctx();
    req.g = &g;
    req.strings = &strings;
    req.reference = &ref;
    req.canonical = canonical ? 1 : 0;
    req.d_where = static_cast<std::int64_t*>(where.get());
    req.d_count = static_cast<std::uint32_t*>(count.get());
    req.n_located = &out.n_located;
    ksc::Check(ksh_seq_locate(&req));
    out.where = where.ToHost<std::int64_t>(std::size_t(2 * n_));
    out.count = count.ToHost<std::uint32_t>(std::size_t(2 * n_));
    return out;
  }

  // bucket_ids[i] = j  <->  result[i] holds the sorted keys of bucket j.
  std::vector<std::vector<KeyType>> GetSampledKmerSet(const std::vector<int>& bucket_ids, bool canonical,
                                                      int n_workers) const {
    const Set s = ToKmerSet(canonical, n_workers);
    const std::vector<std::uint64_t>& bits = s.HostBits();
    std::vector<std::vector<KeyType>> out(bucket_ids.size());
    for (std::size_t i = 0; i < bucket_ids.size(); i++) {
      const std::uint64_t lo = std::uint64_t(bucket_ids[i]) << Set::kKeyBits;
      const std::uint64_t hi = std::uint64_t(bucket_ids[i] + 1) << Set::kKeyBits;
      auto b = std::lower_bound(bits.begin(), bits.end(), lo);
      auto e = std::lower_bound(bits.begin(), bits.end(), hi);
      for (auto it = b; it != e; ++it) out[i].push_back(static_cast<KeyType>(*it - lo));
    }
    return out;
  }

  // The stored strings (downloaded).
  std::vector<std::string> ToStrings(int /*n_workers*/) const {
    const std::vector<std::uint64_t> words = words_.ToHost<std::uint64_t>(std::size_t((n_bases_ + 31) / 32));
    const std::vector<std::uint32_t> lens = lens_.ToHost<std::uint32_t>(std::size_t(n_));
    std::vector<std::string> strings(static_cast<std::size_t>(n_));
    std::int64_t at = 0;
    for (std::int64_t i = 0; i < n_; i++) {
      const std::uint32_t len = lens[i] + K;
      strings[i].resize(len);
      for (std::uint32_t j = 0; j < len; j++, at++)
        strings[i][j] = "ACGT"[(words[at / 32] >> (62 - 2 * (at % 32))) & 3];
    }
    return strings;
  }

  ksh_spss_view View() const {
    return ksh_spss_view{static_cast<const std::uint64_t*>(words_.get()),
                         static_cast<const std::uint32_t*>(lens_.get()), n_, n_bases_};
  }

  std::int64_t StringCount() const { return n_; }

 private:
  std::int64_t n_ = 0;        // number of stored strings (value-initialised, unlike :339)
  std::int64_t n_bases_ = 0;  // = Weight()
  ksc::DeviceBuffer words_, lens_;
};

#endif
