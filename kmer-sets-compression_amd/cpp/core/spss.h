// Free functions of lib/core/spss.h on the device path: GetUnitigs (:73-227), GetUnitigsCanonical
// (:230-615), GetPrefixesFromUnitigs / GetSuffixesFromUnitigs (:619-695), GetSPSS (:697-1036, from
// unitigs or from a set), GetSPSSCanonical (:1039-1858, from unitigs or from a set, fast or not) and
// GetKmerSetFromSPSS (:1861-1941).  Strings come back
// as std::vector<std::string>, as in the reference; their order is the oracle's
// (n_workers == 1 control flow, ascending iteration).
#ifndef KSC_CORE_SPSS_H_
#define KSC_CORE_SPSS_H_

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "core/kmer_set.h"
#include "core/kmer_set_compact.h"

namespace internal {
// "ACGTT" -> "AACGT" (lib/core/spss.h:45-68).
inline std::string Complement(std::string s) {
  std::string out(s.rbegin(), s.rend());
  for (char& c : out) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
  return out;
}
}  // namespace internal

namespace ksc_detail {
template <int K, int N, typename KeyType>
std::vector<std::string> Encode(const KmerSet<K, N, KeyType>& kmer_set, bool canonical, int mode) {
  const ksh_geom g = KmerSet<K, N, KeyType>::Geom();
  const ksh_set_view v = kmer_set.View();
  std::int64_t n = 0, n_bases = 0;
  ksc::Check(ksh_spss_encode_plan(ksc::Ctx(), &g, &v, canonical ? 1 : 0, mode, &n, &n_bases));
  ksc::DeviceBuffer words(std::size_t((n_bases + 31) / 32) * 8), lens(std::size_t(n) * 4);
  ksc::Check(ksh_spss_encode_write_for(ksc::Ctx(), static_cast<std::uint64_t*>(words.get()),
                                       static_cast<std::uint32_t*>(lens.get()), n, n_bases, v.d_offsets));
  ksc::Check(ksh_ctx_sync(ksc::Ctx()));
  ksc::Check(ksh_spss_encode_release(ksc::Ctx()));
  return KmerSetCompact<K, N, KeyType>::FromDevice(std::move(words), std::move(lens), n, n_bases)
      .ToStrings(1);
}

// The path cover of caller-supplied unitigs (ksh_spss_cover_plan / _write): the strings are packed, the device
// derives their ends, and the output comes back as strings.
template <int K, int N, typename KeyType>
std::vector<std::string> Cover(const std::vector<std::string>& unitigs, bool canonical, bool fast) {
  const ksh_geom g = KmerSet<K, N, KeyType>::Geom();
  const KmerSetCompact<K, N, KeyType> in = KmerSetCompact<K, N, KeyType>::FromStrings(unitigs);
  const ksh_spss_view v = in.View();
  std::int64_t n = 0, n_bases = 0;
  ksc::Check(ksh_spss_cover_plan(ksc::Ctx(), &g, &v, canonical ? 1 : 0, fast ? 1 : 0, &n, &n_bases));
  ksc::DeviceBuffer words(std::size_t((n_bases + 31) / 32) * 8), lens(std::size_t(n) * 4);
  ksc::Check(ksh_spss_cover_write_for(ksc::Ctx(), static_cast<std::uint64_t*>(words.get()),
                                      static_cast<std::uint32_t*>(lens.get()), n, n_bases, v.d_words));
  ksc::Check(ksh_ctx_sync(ksc::Ctx()));
  ksc::Check(ksh_spss_cover_release(ksc::Ctx()));
  return KmerSetCompact<K, N, KeyType>::FromDevice(std::move(words), std::move(lens), n, n_bases).ToStrings(1);
}

// GetPrefixesFromUnitigs / GetSuffixesFromUnitigs: first (last) k-mer of every unitig -> the unitigs' indices, in
// ascending order.
template <int K>
std::unordered_map<Kmer<K>, std::vector<std::int64_t>> EndMap(const std::vector<std::string>& unitigs, bool last) {
  std::unordered_map<Kmer<K>, std::vector<std::int64_t>> m;
  for (std::size_t i = 0; i < unitigs.size(); i++) {
    const std::string& u = unitigs[i];
    m[Kmer<K>(last ? u.substr(u.length() - K, K) : u.substr(0, K))].push_back(static_cast<std::int64_t>(i));
  }
  return m;
}
}  // namespace ksc_detail

template <int K>
std::unordered_map<Kmer<K>, std::vector<std::int64_t>> GetPrefixesFromUnitigs(const std::vector<std::string>& unitigs,
                                                                               int /*n_workers*/) {
  return ksc_detail::EndMap<K>(unitigs, false);
}

template <int K>
std::unordered_map<Kmer<K>, std::vector<std::int64_t>> GetSuffixesFromUnitigs(const std::vector<std::string>& unitigs,
                                                                               int /*n_workers*/) {
  return ksc_detail::EndMap<K>(unitigs, true);
}

// The path covers from unitigs take the prefix / suffix maps for the reference's signature but do not read them:
// every caller of the reference passes the maps of the same unitigs, and the device derives the ends itself.  The
// unitigs must meet the preconditions of ksh_spss_cover_plan (include/kmersets_hip.h), else ksc::Check throws.
template <int K, int N, typename KeyType>
std::vector<std::string> GetSPSS(const std::vector<std::string>& unitigs,
                                 const std::unordered_map<Kmer<K>, std::vector<std::int64_t>>& /*prefixes*/,
                                 int /*n_workers*/, int /*n_buckets*/ = 64) {
  return ksc_detail::Cover<K, N, KeyType>(unitigs, false, true);
}

template <int K, int N, typename KeyType>
std::vector<std::string> GetSPSSCanonical(const std::vector<std::string>& unitigs,
                                          const std::unordered_map<Kmer<K>, std::vector<std::int64_t>>& /*prefixes*/,
                                          const std::unordered_map<Kmer<K>, std::vector<std::int64_t>>& /*suffixes*/,
                                          bool fast, int /*n_workers*/, int /*n_buckets*/ = 512) {
  return ksc_detail::Cover<K, N, KeyType>(unitigs, true, fast);
}

template <int K, int N, typename KeyType>
std::vector<std::string> GetUnitigsCanonical(const KmerSet<K, N, KeyType>& kmer_set, int /*n_workers*/) {
  return ksc_detail::Encode(kmer_set, true, 1);
}

// The non-canonical variant (k-mers as they are, edges only forward).
template <int K, int N, typename KeyType>
std::vector<std::string> GetUnitigs(const KmerSet<K, N, KeyType>& kmer_set, int /*n_workers*/) {
  return ksc_detail::Encode(kmer_set, false, 1);
}

template <int K, int N, typename KeyType>
std::vector<std::string> GetSPSS(const KmerSet<K, N, KeyType>& kmer_set, int /*n_workers*/,
                                 int /*n_buckets*/ = 64) {
  return ksc_detail::Encode(kmer_set, false, 0);
}

template <int K, int N, typename KeyType>
std::vector<std::string> GetSPSSCanonical(const KmerSet<K, N, KeyType>& kmer_set, bool fast,
                                          int /*n_workers*/, int /*n_buckets*/ = 512) {
  return ksc_detail::Encode(kmer_set, true, fast ? 0 : 2);
}

template <int K, int N, typename KeyType>
KmerSet<K, N, KeyType> GetKmerSetFromSPSS(const std::vector<std::string>& spss, bool canonical,
                                          int n_workers) {
  return KmerSetCompact<K, N, KeyType>::FromStrings(spss).ToKmerSet(canonical, n_workers);
}

#endif
