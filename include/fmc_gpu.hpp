// fmc_gpu.hpp — C++ host mirror of the reference's template API for the backward-search path, on top of the C-ABI
// (include/fmgpu.h, libfmgpu.so).  Header-only, C++17.  Same names, argument meaning and error behaviour as
// SGSSGene/fmindex-collection for: FMIndex / BiFMIndex (fmindex/FMIndex.h:14-134, fmindex/BiFMIndex.h:17-216), their cursors
// (fmindex/FMIndexCursor.h, fmindex/BiFMIndexCursor.h: lb, lbRev, len, steps, count(), empty(), begin/end, extendLeft / extendRight with and
// without a symbol, symbolLeft / symbolRight), single_locate_step, fmc::Search{...}(),
// search_no_errors::search (search/SearchNoErrors.h), search_backtracking::search (search/Backtracking.h),
// search_ng26::search (search/SearchNg26.h:426-444), search_hamming_sm::{ScoringMatrix, search} (search/SearchHammingSM.h), fmc::search<Edit> (search/search.h:26-35), LocateLinear (locate.h:14-57),
// search_scheme::{Search, Scheme, generator::{h2, pigeon_opt, pigeon_trivial, backtracking}, createUniformPartition, expand,
// limitToHamming, isValid, isComplete} (search_scheme/).
//
// Differences that follow from batching on a GPU: searches run over the whole `queries` range in one call and the delegates
// are invoked on the host afterwards — in ascending qidx and, inside a query, in the reference's callback order.  Both Hamming
// (Edit = false) and edit distance (Edit = true, the reference's default) run on the GPU.
#pragma once

#include "fmgpu.h"

#include <algorithm>
#include <cmath>
#include <array>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <numeric>
#include <optional>
#if __has_include(<span>) && __cplusplus >= 202002L
#include <span>
#endif
#include <stdexcept>
#include <iterator>
#include <string>
#include <string_view>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

namespace fmc {

namespace detail {
inline void check(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("fmindex-collection (gpu): ") + fmgpu_last_error());
}
template <typename Seqs>
inline void flatten(Seqs const& seqs, std::vector<uint8_t>& buf, std::vector<uint64_t>& off) {
    off.assign(1, 0);
    for (auto const& s : seqs) {
        for (auto c : s) buf.push_back(static_cast<uint8_t>(c));
        off.push_back(buf.size());
    }
    if (buf.empty()) buf.push_back(0);
}
}  // namespace detail

// ------------------------------------------------------------------------------------------------ occurrence-table tags
namespace string {
#define FMC_GPU_STRING_TAG(NAME, ID) \
    template <size_t TSigma> struct NAME { static constexpr size_t Sigma = TSigma; static constexpr int layout = ID; };
FMC_GPU_STRING_TAG(InterleavedBitvector8, FMGPU_IB8)
FMC_GPU_STRING_TAG(InterleavedBitvector16, FMGPU_IB16)
FMC_GPU_STRING_TAG(InterleavedBitvector32, FMGPU_IB32)
FMC_GPU_STRING_TAG(InterleavedBitvector16Aligned, FMGPU_IB16A)
FMC_GPU_STRING_TAG(InterleavedBitvectorPrefix16, FMGPU_IBP16)
FMC_GPU_STRING_TAG(InterleavedEPR8, FMGPU_EPR8)
FMC_GPU_STRING_TAG(InterleavedEPR16, FMGPU_EPR16)
FMC_GPU_STRING_TAG(InterleavedEPR32, FMGPU_EPR32)
FMC_GPU_STRING_TAG(InterleavedEPRV2_8, FMGPU_EPRV2_8)
FMC_GPU_STRING_TAG(InterleavedEPRV2_16, FMGPU_EPRV2_16)
FMC_GPU_STRING_TAG(InterleavedEPRV2_32, FMGPU_EPRV2_32)
FMC_GPU_STRING_TAG(Wavelet, FMGPU_WAVELET)
FMC_GPU_STRING_TAG(EPRV3_8, FMGPU_EPRV3_8)
FMC_GPU_STRING_TAG(EPRV3_16, FMGPU_EPRV3_16)
FMC_GPU_STRING_TAG(EPRV3_32, FMGPU_EPRV3_32)
FMC_GPU_STRING_TAG(EPRV4, FMGPU_EPRV4)
FMC_GPU_STRING_TAG(EPRV5, FMGPU_EPRV5)
FMC_GPU_STRING_TAG(InterleavedEPRV7, FMGPU_IEPRV7)
FMC_GPU_STRING_TAG(FlattenedBitvectors_64_64k, FMGPU_FBV_64_64K)
FMC_GPU_STRING_TAG(FlattenedBitvectors_512_64k, FMGPU_FBV_512_64K)
FMC_GPU_STRING_TAG(FlattenedBitvectors_2048_64k, FMGPU_FBV_2048_64K)
#undef FMC_GPU_STRING_TAG
}  // namespace string

// ------------------------------------------------------------------------------------------------ indices
template <size_t TSigma, template <size_t> class String, bool Bidirectional>
struct GpuIndexBase {
    static constexpr size_t Sigma = TSigma;
    static constexpr size_t FirstSymb = 1;
    static constexpr bool IsBidirectional = Bidirectional;
    using LEntry = std::tuple<uint32_t, uint32_t, size_t>;   // (seqId, pos, steps): decltype(tuple_cat(ADEntry{}, tuple<size_t>{}))

    fmgpu_index_t handle{};
    uint64_t n{};

    GpuIndexBase() = default;
    GpuIndexBase(GpuIndexBase const&) = delete;
    GpuIndexBase(GpuIndexBase&& o) noexcept : handle{o.handle}, n{o.n} { o.handle = nullptr; }
    auto operator=(GpuIndexBase&& o) noexcept -> GpuIndexBase& { std::swap(handle, o.handle); std::swap(n, o.n); return *this; }
    ~GpuIndexBase() { if (handle) fmgpu_index_destroy(handle); }

    // FMIndex(Sequences, samplingRate, threadNbr) / BiFMIndex(Sequences, samplingRate, threadNbr): built on the GPU
    template <typename Seqs>
    GpuIndexBase(Seqs const& input, size_t samplingRate, size_t /*threadNbr*/) {
        std::vector<uint8_t> buf; std::vector<uint64_t> off;
        detail::flatten(input, buf, off);
        detail::check(fmgpu_build_index(buf.data(), off.data(), off.size() - 1, static_cast<int32_t>(Sigma), String<Sigma>::layout, samplingRate,
                                        Bidirectional ? 1 : 0, 0, &handle, nullptr));
        detail::check(fmgpu_index_info(handle, &n, nullptr, nullptr, nullptr, nullptr));
    }

    size_t size() const { return n; }

    auto locate(size_t idx) const -> LEntry {
        uint64_t row = idx, seq{}, pos{}, steps{};
        detail::check(fmgpu_locate(handle, &row, 1, &seq, &pos, &steps, nullptr, nullptr));
        return {static_cast<uint32_t>(seq), static_cast<uint32_t>(pos), static_cast<size_t>(steps)};
    }
    // single_locate_step(idx) (fmindex/FMIndex.h:126-128): the sampled entry of row idx, if that row is sampled
    auto single_locate_step(size_t idx) const -> std::optional<std::tuple<uint32_t, uint32_t>> {
        auto [seq, pos, steps] = locate(idx);
        if (steps != 0) return std::nullopt;
        return std::tuple<uint32_t, uint32_t>{seq, pos};
    }
    auto locate(std::vector<uint64_t> const& rows) const -> std::vector<LEntry> {
        std::vector<uint64_t> seq(rows.size()), pos(rows.size()), steps(rows.size());
        detail::check(fmgpu_locate(handle, rows.data(), rows.size(), seq.data(), pos.data(), steps.data(), nullptr, nullptr));
        std::vector<LEntry> out(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) out[i] = {static_cast<uint32_t>(seq[i]), static_cast<uint32_t>(pos[i]), static_cast<size_t>(steps[i])};
        return out;
    }
    // every row of every hit record located in one call (fmgpu_locate_hits): one fmgpu_position per row, hits in the given order, inside a hit the rows
    // lb .. lb + len - 1 — what a LocateLinear per cursor gives, with pos = sampled pos + offset
    auto locateHits(std::vector<fmgpu_hit> const& hits) const -> std::vector<fmgpu_position> {
        uint64_t total = 0;
        for (auto const& h : hits) total += h.len;
        std::vector<fmgpu_position> out(std::max<uint64_t>(total, 1));
        uint64_t count = 0;
        detail::check(fmgpu_locate_hits(handle, hits.data(), hits.size(), out.data(), total, &count, nullptr, nullptr));
        out.resize(count);
        return out;
    }
    // fmgpu_index_accelerate_extract: the text map and sample table that extract() reads (not saved, not cloned)
    void accelerateExtract(bool enable = true) { detail::check(fmgpu_index_accelerate_extract(handle, enable ? 1 : 0)); }
    // the symbols of every range, concatenated in the given order (fmgpu_extract); needs accelerateExtract()
    auto extract(std::vector<fmgpu_text_range> const& ranges) const -> std::vector<uint8_t> {
        uint64_t total = 0;
        for (auto const& r : ranges) total += r.len;
        std::vector<uint8_t> out(std::max<uint64_t>(total, 1));
        uint64_t count = 0;
        detail::check(fmgpu_extract(handle, ranges.data(), ranges.size(), out.data(), total, &count, nullptr, nullptr));
        out.resize(count);
        return out;
    }
};

template <size_t TSigma, template <size_t> class String = string::FlattenedBitvectors_512_64k>   // fmindex/FMIndex.h:14
struct FMIndex : GpuIndexBase<TSigma, String, false> {
    using GpuIndexBase<TSigma, String, false>::GpuIndexBase;
};
template <size_t TSigma, template <size_t> class String = string::FlattenedBitvectors_512_64k>   // fmindex/BiFMIndex.h:17
struct BiFMIndex : GpuIndexBase<TSigma, String, true> {
    using GpuIndexBase<TSigma, String, true>::GpuIndexBase;
};

// saveIndex / loadIndex (fmindex/diskStorage.h:12-27) on this library's own index file (include/fmgpu.h: fmgpu_index_save / fmgpu_index_load — a
// flat file of the device arrays, NOT the reference's cereal archive).  withTables: also the optional tables the handle holds right now.
template <typename Index>
void saveIndex(Index const& index, std::string const& fileName, bool withTables = true) {
    detail::check(fmgpu_index_save(index.handle, fileName.c_str(), withTables ? 1 : 0));
}
template <typename Index>
auto loadIndex(std::string const& fileName) -> Index {
    Index index{};
    detail::check(fmgpu_index_load(fileName.c_str(), &index.handle));
    int32_t sigma{}, bidir{};
    detail::check(fmgpu_index_info(index.handle, &index.n, &sigma, nullptr, &bidir, nullptr));
    if (static_cast<size_t>(sigma) != Index::Sigma || (bidir != 0) != Index::IsBidirectional)
        throw std::runtime_error("loadIndex: " + fileName + " holds an index of Sigma " + std::to_string(sigma) + (bidir ? " (BiFMIndex)" : " (FMIndex)"));
    return index;
}

// reconstructText(index, seqNbr) / reconstructText(index) (utils.h:672-703): the sentinel rows (rank(size(), 0) of them) are located, each one's text runs from
// the previous delimiter of its seqId (or pos 0) up to its own, and the symbols come from ONE fmgpu_extract call.  The extract table is built for the call
// if the index lacks it, and dropped again.
namespace detail {
inline auto sentinelRanges(fmgpu_index_t h, uint64_t n) -> std::vector<fmgpu_text_range> {
    uint64_t idx = n, nsent = 0;
    uint8_t symb = 0, what = 0;
    check(fmgpu_string_query(h, 0, &idx, &symb, &what, 1, &nsent, nullptr));
    std::vector<uint64_t> rows(nsent), seq(nsent), pos(nsent), steps(nsent);
    for (uint64_t i = 0; i < nsent; ++i) rows[i] = i;
    if (nsent) check(fmgpu_locate(h, rows.data(), nsent, seq.data(), pos.data(), steps.data(), nullptr, nullptr));
    for (uint64_t i = 0; i < nsent; ++i) pos[i] += steps[i];
    std::vector<uint64_t> order(rows);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return std::tie(seq[a], pos[a]) < std::tie(seq[b], pos[b]); });
    std::vector<fmgpu_text_range> out(nsent);
    for (uint64_t k = 0; k < nsent; ++k) {
        const uint64_t i = order[k];
        const uint64_t from = k > 0 && seq[order[k - 1]] == seq[i] ? pos[order[k - 1]] + 1 : 0;
        out[i] = fmgpu_text_range{seq[i], from, pos[i] - from};
    }
    return out;
}
template <typename Index>
auto extractWithTable(Index const& index, std::vector<fmgpu_text_range> const& ranges) -> std::vector<uint8_t> {
    uint32_t mask = 0;
    check(fmgpu_index_formats(index.handle, &mask));
    const bool build = !(mask & FMGPU_FMT_EXTRACT);
    if (build) check(fmgpu_index_accelerate_extract(index.handle, 1));
    std::vector<uint8_t> out;
    try { out = index.extract(ranges); } catch (...) { if (build) fmgpu_index_accelerate_extract(index.handle, 0); throw; }
    if (build) check(fmgpu_index_accelerate_extract(index.handle, 0));
    return out;
}
}  // namespace detail

template <typename Index>
auto reconstructText(Index const& index, size_t seqNbr) -> std::vector<uint8_t> {
    auto const ranges = detail::sentinelRanges(index.handle, index.n);
    if (seqNbr >= ranges.size()) throw std::out_of_range("reconstructText: seqNbr " + std::to_string(seqNbr) + " is not a sentinel row");
    return detail::extractWithTable(index, {ranges[seqNbr]});
}
template <typename Index>
auto reconstructText(Index const& index) -> std::vector<std::vector<uint8_t>> {
    auto const ranges = detail::sentinelRanges(index.handle, index.n);
    std::vector<size_t> order(ranges.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return std::tie(ranges[a].seq_id, a) < std::tie(ranges[b].seq_id, b); });   // (seqId, i)
    std::vector<fmgpu_text_range> sorted;
    for (size_t i : order) sorted.push_back(ranges[i]);
    auto const sym = detail::extractWithTable(index, sorted);
    std::vector<std::vector<uint8_t>> res;
    size_t at = 0;
    for (auto const& r : sorted) { res.emplace_back(sym.begin() + at, sym.begin() + at + r.len); at += r.len; }
    return res;
}

// ------------------------------------------------------------------------------------------------ cursors
struct IntIterator {   // utils.h:656-669
    size_t i;
    auto operator*() const -> size_t { return i; }
    auto operator++() -> IntIterator& { ++i; return *this; }
    bool operator!=(IntIterator const& o) const { return i != o.i; }
};
namespace detail {
// one cursor step on the device (fmgpu_cursor_extend): symb < 0 = every symbol
inline void extend(fmgpu_index_t h, int direction, uint64_t lb, uint64_t lbRev, uint64_t len, int symb, bool bidir, uint64_t* olb, uint64_t* orev, uint64_t* olen) {
    uint8_t c = static_cast<uint8_t>(symb < 0 ? 0 : symb);
    check(fmgpu_cursor_extend(h, direction, 1, &lb, bidir ? &lbRev : nullptr, &len, symb < 0 ? nullptr : &c, olb, bidir ? orev : nullptr, olen, nullptr));
}
inline size_t symbol_at(fmgpu_index_t h, int which, uint64_t row) {
    uint8_t what = 2; uint64_t out{};
    check(fmgpu_string_query(h, which, &row, nullptr, &what, 1, &out, nullptr));
    return static_cast<size_t>(out);
}
}  // namespace detail

// Single cursor steps go through the batched device call one cursor at a time: they are here so that code written against the reference's cursor
// API runs unchanged (tests, small tools); a search loop belongs into the batched search calls below.
template <typename Index>
struct FMIndexCursor {   // fmindex/FMIndexCursor.h:12-63
    static constexpr size_t Sigma = Index::Sigma;
    Index const* index{};
    size_t lb{}, len{};
    FMIndexCursor() = default;
    explicit FMIndexCursor(Index const& idx) : index{&idx}, lb{0}, len{idx.size()} {}
    FMIndexCursor(Index const& idx, size_t lb_, size_t len_) : index{&idx}, lb{lb_}, len{len_} {}
    bool empty() const { return len == 0; }
    size_t count() const { return len; }
    auto extendLeft(size_t symb) const -> FMIndexCursor {                            // :33-37
        uint64_t nlb{}, nlen{};
        detail::extend(index->handle, 0, lb, 0, len, static_cast<int>(symb), false, &nlb, nullptr, &nlen);
        return FMIndexCursor{*index, static_cast<size_t>(nlb), static_cast<size_t>(nlen)};
    }
    auto extendLeft() const -> std::array<FMIndexCursor, Sigma> {                    // :38-53
        std::array<uint64_t, Sigma> nlb{}, nlen{};
        detail::extend(index->handle, 0, lb, 0, len, -1, false, nlb.data(), nullptr, nlen.data());
        std::array<FMIndexCursor, Sigma> out;
        for (size_t c = 0; c < Sigma; ++c) out[c] = FMIndexCursor{*index, static_cast<size_t>(nlb[c]), static_cast<size_t>(nlen[c])};
        return out;
    }
};
template <typename Index>
struct BiFMIndexCursor {   // fmindex/BiFMIndexCursor.h:13-191
    static constexpr size_t Sigma = Index::Sigma;
    Index const* index{};
    size_t lb{}, lbRev{}, len{}, steps{};
    BiFMIndexCursor() = default;
    explicit BiFMIndexCursor(Index const& idx) : index{&idx}, lb{0}, lbRev{0}, len{idx.size()}, steps{0} {}
    BiFMIndexCursor(Index const& idx, size_t lb_, size_t lbRev_, size_t len_, size_t steps_) : index{&idx}, lb{lb_}, lbRev{lbRev_}, len{len_}, steps{steps_} {}
    bool empty() const { return len == 0; }
    size_t count() const { return len; }
    bool operator==(BiFMIndexCursor const& o) const noexcept { return lb == o.lb && len == o.len; }
    auto extendLeft(size_t symb) const -> BiFMIndexCursor { return step(0, symb); }   // :113-120
    auto extendRight(size_t symb) const -> BiFMIndexCursor { return step(1, symb); }  // :121-128
    auto extendLeft() const -> std::array<BiFMIndexCursor, Sigma> { return fan(0); }  // :58-69
    auto extendRight() const -> std::array<BiFMIndexCursor, Sigma> { return fan(1); } // :71-82
    auto symbolLeft() const -> size_t { return detail::symbol_at(index->handle, 0, lb); }      // :180-184
    auto symbolRight() const -> size_t { return detail::symbol_at(index->handle, 1, lbRev); }  // :186-190
private:
    auto step(int direction, size_t symb) const -> BiFMIndexCursor {
        uint64_t nlb{}, nrev{}, nlen{};
        detail::extend(index->handle, direction, lb, lbRev, len, static_cast<int>(symb), true, &nlb, &nrev, &nlen);
        return BiFMIndexCursor{*index, static_cast<size_t>(nlb), static_cast<size_t>(nrev), static_cast<size_t>(nlen), steps + 1};
    }
    auto fan(int direction) const -> std::array<BiFMIndexCursor, Sigma> {
        std::array<uint64_t, Sigma> nlb{}, nrev{}, nlen{};
        detail::extend(index->handle, direction, lb, lbRev, len, -1, true, nlb.data(), nrev.data(), nlen.data());
        std::array<BiFMIndexCursor, Sigma> out;
        for (size_t c = 0; c < Sigma; ++c) out[c] = BiFMIndexCursor{*index, static_cast<size_t>(nlb[c]), static_cast<size_t>(nrev[c]), static_cast<size_t>(nlen[c]), steps + 1};
        return out;
    }
};
template <typename C> auto begin(C const& c) -> decltype(IntIterator{c.lb}) { return IntIterator{c.lb}; }
template <typename C> auto end(C const& c) -> decltype(IntIterator{c.lb + c.len}) { return IntIterator{c.lb + c.len}; }

template <typename Index> struct select_cursor { using type = FMIndexCursor<Index>; };
template <size_t S, template <size_t> class Str> struct select_cursor<BiFMIndex<S, Str>> { using type = BiFMIndexCursor<BiFMIndex<S, Str>>; };
template <typename Index> using select_cursor_t = typename select_cursor<Index>::type;

// ------------------------------------------------------------------------------------------------ search schemes
namespace search_scheme {
struct Search {
    std::vector<size_t> pi, l, u;
    bool operator==(Search const& o) const { return std::tie(pi, l, u) == std::tie(o.pi, o.l, o.u); }
};
using Scheme = std::vector<Search>;

inline auto isValid(Search const& s) -> bool {   // isValid.h:55-93
    if (s.pi.empty() || s.pi.size() != s.l.size() || s.pi.size() != s.u.size()) return false;
    size_t lo = s.pi[0], hi = s.pi[0];
    for (size_t i = 1; i < s.pi.size(); ++i) {
        if (s.pi[i] == hi + 1) hi = s.pi[i];
        else if (s.pi[i] + 1 == lo) lo = s.pi[i];
        else return false;
    }
    if (lo != 0) return false;
    for (size_t i = 0; i < s.pi.size(); ++i) {
        if (i && (s.l[i - 1] > s.l[i] || s.u[i - 1] > s.u[i])) return false;
        if (s.l[i] > s.u[i]) return false;
    }
    return true;
}
inline auto isValid(Scheme const& ss) -> bool {
    return std::all_of(ss.begin(), ss.end(), [&](Search const& s) { return isValid(s) && s.pi.size() == ss.front().pi.size(); });
}

inline auto createUniformPartition(size_t parts, size_t totalSum) -> std::vector<size_t> {   // expand.h:324-335
    if (parts == 0 || totalSum < parts) throw std::invalid_argument("createUniformPartition: need 0 < parts <= totalSum");
    auto counts = std::vector<size_t>(parts, totalSum / parts);
    for (size_t i = 0; i < totalSum % parts; ++i) counts[i] += 1;
    return counts;
}
inline auto createUniformPartition(Scheme const& ss, size_t totalSum) -> std::vector<size_t> {
    if (ss.empty()) throw std::invalid_argument("createUniformPartition: empty scheme");
    return createUniformPartition(ss[0].pi.size(), totalSum);
}

// part p of the search becomes counts[p] parts (expand.h:167-177)
inline auto expand(Search const& s, std::vector<size_t> const& counts) -> std::optional<Search> {
    size_t P = s.pi.size(), newLen = 0;
    if (counts.size() != P) throw std::invalid_argument("expand: one count per part");
    std::vector<size_t> starts(P, 0);
    for (size_t i = 1; i < P; ++i) starts[i] = starts[i - 1] + counts[i - 1];
    for (size_t c : counts) newLen += c;
    Search r;
    for (size_t i = 0; i < P; ++i) {
        bool forward = i == 0 ? (P == 1 || s.pi[1] > s.pi[0]) : s.pi[i] > s.pi[i - 1];
        size_t lo = starts[s.pi[i]], cnt = counts[s.pi[i]];
        for (size_t j = 0; j < cnt; ++j) r.pi.push_back(forward ? lo + j : lo + cnt - 1 - j);
        if (cnt >= 1) { for (size_t j = 1; j < cnt; ++j) r.l.push_back(i ? s.l[i - 1] : 0); r.l.push_back(s.l[i]); }
        else if (!r.l.empty()) r.l.back() = s.l[i];
        for (size_t j = 0; j < cnt; ++j) r.u.push_back(s.u[i]);
    }
    if (r.pi.size() != newLen || !isValid(r)) return std::nullopt;
    return r;
}
inline auto expand(Search const& s, size_t newLen) -> std::optional<Search> {   // expand.h:146-155: uniformly
    size_t P = s.pi.size();
    std::vector<size_t> counts(P, newLen / P);
    for (size_t i = 0; i < newLen % P; ++i) counts[i] += 1;
    return expand(s, counts);
}
inline auto expand(Scheme const& ss, size_t newLen) -> Scheme {
    Scheme r;
    for (auto const& s : ss) if (auto o = expand(s, newLen)) r.push_back(*o);
    return r;
}
inline auto expand(Scheme const& ss, std::vector<size_t> const& counts) -> Scheme {   // expand.h:179-189
    Scheme r;
    for (auto const& s : ss) if (auto o = expand(s, counts)) r.push_back(*o);
    return r;
}
// nodes a search visits when a node of depth n survives with probability min(1, N / sigma^n) (weightedNodeCount.h:21-69; the weight in double, the sums in
// long double as there, so that expandByWNC takes the reference's decisions)
template <bool Edit>
inline long double weightedNodeCount(Search const& s, size_t sigma, size_t N) {
    size_t e = *std::max_element(s.u.begin(), s.u.end());
    std::vector<long double> last(e + 1, 0), cur(e + 1, 0);
    last[0] = 1;
    long double acc = 0;
    for (size_t n = 1; n <= s.pi.size(); ++n) {
        double f = static_cast<double>(N) / std::pow(static_cast<double>(sigma), static_cast<double>(n));
        if (f > 1) f = 1.;
        for (size_t i = 0; i <= e; ++i) {
            if (s.l[n - 1] <= i && i <= s.u[n - 1]) {
                cur[i] = last[i];
                if (i > 0) cur[i] += Edit ? (sigma - 1) * last[i - 1] + sigma * last[i - 1] + last[i - 1] : (sigma - 1) * last[i - 1];
                cur[i] *= f;
                acc += cur[i];
            } else cur[i] = 0;
        }
        std::swap(cur, last);
    }
    return acc;
}
template <bool Edit>
inline long double weightedNodeCount(Scheme const& ss, size_t sigma, size_t N) {
    long double v = 0;
    for (auto const& s : ss) v = v + weightedNodeCount<Edit>(s, sigma, N);
    return v;
}
// expand.h:218-247: the parts grow one position at a time, each time where the weighted node count of the expanded scheme is smallest
template <bool Edit = false>
inline auto optimizeByWNC(Scheme const& ss, size_t newLen, size_t sigma, size_t N) -> std::vector<size_t> {
    if (ss.empty()) return {};
    size_t P = ss[0].pi.size();
    if (newLen < P) throw std::invalid_argument("optimizeByWNC: the new length is shorter than the scheme");
    std::vector<size_t> counts(P, 1);
    for (size_t i = 0; i < newLen - P; ++i) {
        double best = std::numeric_limits<double>::max();      // (a double, like the reference's running best)
        size_t bestPos = 0;
        for (size_t j = 0; j < P; ++j) {
            counts[j] += 1;
            long double f = weightedNodeCount<Edit>(expand(ss, counts), sigma, N);
            counts[j] -= 1;
            if (f < best) { best = static_cast<double>(f); bestPos = j; }
        }
        counts[bestPos] += 1;
    }
    return counts;
}
template <bool Edit = false>
inline auto expandByWNC(Scheme const& ss, size_t newLen, size_t sigma, size_t N) -> Scheme {
    return expand(ss, optimizeByWNC<Edit>(ss, newLen, sigma, N));
}
inline auto limitToHamming(Scheme ss) -> Scheme {   // expand.h:301-319
    for (auto& s : ss) {
        for (size_t i = s.pi.size() - 1; i > 0; --i) { if (s.l[i] == 0) break; s.l[i - 1] = std::max(s.l[i - 1], s.l[i] - 1); }
        for (size_t i = 1; i < s.pi.size(); ++i) s.u[i] = std::min(s.u[i], s.u[i - 1] + 1);
    }
    return ss;
}
inline auto isComplete(Scheme const& ss, size_t minK, size_t maxK) -> bool {   // isComplete.h:69-84
    if (ss.empty()) return false;
    size_t P = ss[0].pi.size();
    std::vector<size_t> cfg(P, 0);
    auto covered = [&]() {
        for (auto const& s : ss) {
            size_t a = 0; bool ok = true;
            for (size_t i = 0; i < P && ok; ++i) { a += cfg[s.pi[i]]; ok = s.l[i] <= a && a <= s.u[i]; }
            if (ok) return true;
        }
        return false;
    };
    bool complete = minK > 0 || covered();
    auto rec = [&](auto&& self, size_t k, size_t start) -> void {
        if (k >= maxK || !complete) return;
        for (size_t i = start; i < P && complete; ++i) {
            cfg[i] += 1;
            if (k + 1 >= minK && !covered()) complete = false;
            self(self, k + 1, i);
            cfg[i] -= 1;
        }
    };
    rec(rec, 0, 0);
    return complete;
}

namespace generator {
inline auto backtracking(size_t N, size_t minK, size_t K) -> Scheme {   // generator/backtracking.h:14-21
    Search s{std::vector<size_t>(N), std::vector<size_t>(N, 0), std::vector<size_t>(N, K)};
    std::iota(s.pi.begin(), s.pi.end(), size_t{0});
    s.l.back() = minK;
    return {s};
}
inline auto pigeon(size_t minK, size_t K, bool opt) -> Scheme {   // generator/pigeon.h:14-102
    size_t N = K + 1;
    Scheme res;
    for (size_t i = 0; i < N; ++i) {
        Search s;
        s.pi.push_back(i); s.l.push_back(0); s.u.push_back(0);
        for (size_t j = i; j > 0; --j) { s.pi.push_back(j - 1); s.l.push_back(opt ? i - j + 1 : 0); s.u.push_back(opt ? K - j + 1 : K); }
        for (size_t j = i + 1; j < N; ++j) { s.pi.push_back(j); s.l.push_back(opt ? i : 0); s.u.push_back(K); }
        s.l.back() = std::max(s.l.back(), minK);
        res.push_back(s);
    }
    return res;
}
inline auto pigeon_opt(size_t minK, size_t K) -> Scheme { return pigeon(minK, K, true); }
inline auto pigeon_trivial(size_t minK, size_t K) -> Scheme { return pigeon(minK, K, false); }

inline auto h2(size_t N, size_t minK, size_t K) -> Scheme {   // generator/h2.h:128-153
    if (N <= K || minK > K) throw std::invalid_argument("h2(N, minK, K) needs N > K >= minK");
    size_t R = K + 1;
    auto at = [&](std::vector<size_t>& m, size_t r, size_t c) -> size_t& { return m[r * N + c]; };
    std::vector<size_t> pi(R * N), l(R * N, 0), u(R * N, 0), d(R * N, 0);
    for (size_t r = 0; r < R; ++r) for (size_t c = 0; c < N; ++c) {
        size_t skip = K - r;
        at(pi, r, c) = c < N - skip ? c + skip : N - c - 1;
        if (c >= N - (K - r + 1)) at(l, r, c) = r;
        at(d, r, c) = c >= K ? K - r : (r < K ? (r + K - c) % K : K);
    }
    auto fits = [&](size_t row, size_t col, size_t v) {
        if (row == col) return false;
        if (row > col) { for (size_t i = 0; i < col; ++i) if (at(d, row, i) < v) return false; }
        else for (size_t i = row + 1; i < col; ++i) if (at(d, row, i) > v) return false;
        return true;
    };
    for (size_t c = 0; c < N; ++c) for (size_t r = 0; r < R; ++r) {
        if (c == r || at(d, r, c) == 0 || fits(r, c, at(d, r, c))) continue;
        for (size_t o = r + 1; o < R; ++o)
            if (fits(r, c, at(d, o, c)) && fits(o, c, at(d, r, c))) { std::swap(at(d, r, c), at(d, o, c)); break; }
    }
    for (size_t c = 1; c < N; ++c) for (size_t r = R; r-- > 0;)
        at(u, r, c) = std::max(at(u, r, c - 1), at(l, r, c - 1) + at(d, K - r, at(pi, r, c)));
    Scheme ss;
    for (size_t r = 0; r < R; ++r) {
        Search s;
        s.pi.assign(pi.begin() + r * N, pi.begin() + (r + 1) * N);
        s.l.assign(l.begin() + r * N, l.begin() + (r + 1) * N);
        s.u.assign(u.begin() + r * N, u.begin() + (r + 1) * N);
        s.l.back() = std::max(s.l.back(), minK);
        ss.push_back(s);
    }
    return ss;
}
}  // namespace generator
}  // namespace search_scheme

// ------------------------------------------------------------------------------------------------ searches
namespace detail {
template <typename Index, typename Delegate>
void report(Index const& index, std::vector<fmgpu_hit>& hits, Delegate&& delegate) {
    check(fmgpu_hits_sort(hits.data(), hits.size(), nullptr));    // (qidx, seq): the reference's callback order, sorted on the device
    using cursor_t = select_cursor_t<Index>;
    for (auto const& h : hits) {
        cursor_t cur{};
        cur.index = &index; cur.lb = h.lb; cur.len = h.len;
        if constexpr (std::is_same_v<cursor_t, BiFMIndexCursor<Index>>) cur.lbRev = h.lb_rev;
        delegate(static_cast<size_t>(h.qidx), cur, static_cast<size_t>(h.errors));
    }
}
// lowerBound: the count a call reports with FMGPU_ERR_CAPACITY is a lower bound of the total (the best-stratum calls: the records up to the stratum that
// overflowed) — growing to max(count, 2 x capacity) ends within as many rounds as the ladder has schemes
template <typename Call>
std::vector<fmgpu_hit> run_hits(size_t nq, Call&& call, bool lowerBound = false) {
    std::vector<fmgpu_hit> hits(std::max<size_t>(1024, 4 * nq));
    for (;;) {
        uint64_t count = 0;
        int rc = call(hits.data(), hits.size(), &count);
        if (rc == FMGPU_ERR_CAPACITY) { hits.resize(lowerBound ? std::max<size_t>(count, 2 * hits.size()) : count); continue; }
        check(rc);
        hits.resize(count);
        return hits;
    }
}
}  // namespace detail

// A batch in the 4-bit packed query form (include/fmgpu.h): symbol i of the batch = nibble i & 1 of byte i >> 1, the even index in the low nibble; qoff as in the
// byte form.  pack() is the host packer (the same bytes as fmgpu_queries_pack4): a symbol >= sigma becomes 15; with a complement table (sigma entries) every read is
// followed by its reverse complement.  The search entry points below take it in place of a Sequences object and call the `_q4` entry points.
struct PackedQueries {
    std::vector<uint8_t> packed;
    std::vector<uint64_t> qoff{0};
    auto size() const -> size_t { return qoff.size() - 1; }
    auto unpack() const -> std::vector<std::vector<uint8_t>> {       // the byte form: nibble 15 comes back as 255
        std::vector<std::vector<uint8_t>> out(size());
        for (size_t q = 0; q < size(); ++q)
            for (uint64_t i = qoff[q]; i < qoff[q + 1]; ++i) {
                uint8_t c = (packed[i >> 1] >> (4 * (i & 1))) & 15;
                out[q].push_back(c == 15 ? 255 : c);
            }
        return out;
    }
    template <typename Seqs>
    static auto pack(Seqs const& seqs, size_t sigma, std::vector<uint8_t> const& complement = {}) -> PackedQueries {
        if (sigma < 2 || sigma > 15) throw std::runtime_error("fmindex-collection (gpu): 4-bit packed queries need 2 <= sigma <= 15");
        if (!complement.empty() && complement.size() < sigma) throw std::runtime_error("fmindex-collection (gpu): the complement table needs sigma entries");
        PackedQueries out;
        uint64_t at = 0;
        auto put = [&](size_t c) {
            if ((at & 1) == 0) out.packed.push_back(static_cast<uint8_t>(c)); else out.packed.back() |= static_cast<uint8_t>(c << 4);
            ++at;
        };
        for (auto const& q : seqs) {
            for (auto c : q) put(static_cast<size_t>(c) < sigma ? static_cast<size_t>(c) : 15);
            out.qoff.push_back(at);
            if (complement.empty()) continue;
            for (auto it = q.rbegin(); it != q.rend(); ++it) {
                size_t c = static_cast<size_t>(*it) < sigma ? complement[static_cast<size_t>(*it)] : 15;
                put(c < sigma ? c : 15);
            }
            out.qoff.push_back(at);
        }
        return out;
    }
    // the same batch made by fmgpu_queries_pack4: the reads go to the device as bytes once, the packing and the second strand happen there
    template <typename Seqs>
    static auto packOnDevice(Seqs const& seqs, size_t sigma, std::vector<uint8_t> const& complement = {}) -> PackedQueries {
        if (!complement.empty() && complement.size() < sigma) throw std::runtime_error("fmindex-collection (gpu): the complement table needs sigma entries");
        std::vector<uint8_t> buf; std::vector<uint64_t> off;
        detail::flatten(seqs, buf, off);
        size_t const nq = off.size() - 1, strands = complement.empty() ? 1 : 2;
        PackedQueries out;
        out.qoff.assign(strands * nq + 1, 0);
        out.packed.assign((strands * off.back() + 1) / 2, 0);
        detail::check(fmgpu_queries_pack4(buf.data(), off.data(), nq, static_cast<int32_t>(sigma), complement.empty() ? nullptr : complement.data(),
                                          out.packed.data(), out.qoff.data(), nullptr));
        return out;
    }
};

// ---- query text (include/fmgpu.h: fmgpu_queries_parse) ------------------------------------------------------------------------------------------
// The bytes of a read file — one read per line, FASTA or FASTQ — parsed on the device: `auto reads = fmc::parseQueries(text, fmc::TextFormat::Fastq,
// fmc::SymbolTable::dna5());`.  A SymbolTable says what every byte of a sequence line becomes: a rank, nothing (Drop), or 255 counted as foreign (Foreign).
enum class TextFormat : int32_t { Lines = FMGPU_TEXT_LINES, Fasta = FMGPU_TEXT_FASTA, Fastq = FMGPU_TEXT_FASTQ };
struct SymbolTable {
    static constexpr uint8_t Drop = FMGPU_SYM_DROP, Foreign = FMGPU_SYM_FOREIGN;
    std::array<uint8_t, 256> map;
    // letters[i] -> firstRank + i (both cases unless caseInsensitive is false), the bytes of `drop` -> Drop, every other byte -> other
    explicit SymbolTable(std::string_view letters = "ACGT", uint8_t firstRank = 1, bool caseInsensitive = true, uint8_t other = Foreign, std::string_view drop = {}) {
        map.fill(other);
        for (size_t i = 0; i < letters.size(); ++i) {
            auto const c = static_cast<unsigned char>(letters[i]);
            auto const rank = static_cast<uint8_t>(firstRank + i);
            map[c] = rank;
            if (caseInsensitive && c >= 'A' && c <= 'Z') map[c - 'A' + 'a'] = rank;
            if (caseInsensitive && c >= 'a' && c <= 'z') map[c - 'a' + 'A'] = rank;
        }
        for (char c : drop) map[static_cast<unsigned char>(c)] = Drop;
    }
    auto set(char byte, uint8_t value) -> SymbolTable& { map[static_cast<unsigned char>(byte)] = value; return *this; }
    // $ A C G T = 0 .. 4, the ranks of the example and the datasets; any other byte is Foreign, or rank 1 (the example's --convertUnknownChar)
    static auto dna5(bool unknownToA = false) -> SymbolTable { return SymbolTable{"ACGT", 1, true, unknownToA ? uint8_t{1} : Foreign}.set('$', 0); }
    // $ A C G T N = 0 .. 5; any other byte is Foreign, or rank 5
    static auto dna6(bool unknownToN = false) -> SymbolTable { return SymbolTable{"ACGTN", 1, true, unknownToN ? uint8_t{5} : Foreign}.set('$', 0); }
    // the amino-acid letters in alphabetical order = ranks 1 .. 20, $ = 0
    static auto protein(std::string_view letters = "ACDEFGHIKLMNPQRSTVWY") -> SymbolTable { return SymbolTable{letters}.set('$', 0); }
};

// What parseQueries returns: the batch in the byte form plus where each read's name and quality line lie in the text.  It is a range of reads (contiguous one-byte
// symbols), so every search call, PackedQueries::pack / packOnDevice, fmc::map and a Feed take it wherever they take a Sequences object.  Like
// PackedQueries::packOnDevice the work happens on the device and the batch comes back to host vectors, which is what the calls of this mirror are handed.
struct ParsedQueries {
    struct Read {
        uint8_t const* first; size_t count;
        auto data() const -> uint8_t const* { return first; }
        auto size() const -> size_t { return count; }
        auto empty() const -> bool { return count == 0; }
        auto begin() const -> uint8_t const* { return first; }
        auto end() const -> uint8_t const* { return first + count; }
        auto rbegin() const { return std::reverse_iterator<uint8_t const*>{end()}; }
        auto rend() const { return std::reverse_iterator<uint8_t const*>{begin()}; }
        auto operator[](size_t i) const -> uint8_t { return first[i]; }
    };
    struct iterator {
        ParsedQueries const* batch; size_t q;
        auto operator*() const -> Read { return (*batch)[q]; }
        auto operator++() -> iterator& { ++q; return *this; }
        bool operator!=(iterator const& o) const { return q != o.q; }
        bool operator==(iterator const& o) const { return q == o.q; }
    };
    std::vector<uint8_t> qbuf;
    std::vector<uint64_t> qoff{0};
    std::vector<fmgpu_text_span> names, quals;
    uint64_t consumed{0}, foreign{0};                                 // where the next chunk of the text starts; symbols written as 255

    auto size() const -> size_t { return qoff.size() - 1; }
    auto operator[](size_t q) const -> Read { return {qbuf.data() + qoff[q], static_cast<size_t>(qoff[q + 1] - qoff[q])}; }
    auto begin() const -> iterator { return {this, 0}; }
    auto end() const -> iterator { return {this, size()}; }
    // the name (the header line without its first byte) and the quality line of read q, as views into the text that was parsed
    auto name(std::string_view text, size_t q) const -> std::string_view { return text.substr(names[q].offset, names[q].len); }
    auto quality(std::string_view text, size_t q) const -> std::string_view { return text.substr(quals[q].offset, quals[q].len); }
};

// final = false: `text` is a chunk of a longer input; only the records it proves complete are parsed and the next chunk starts at `.consumed`.
// A text error throws std::runtime_error naming the line.
inline auto parseQueries(std::string_view text, TextFormat format, SymbolTable const& table, bool final = true) -> ParsedQueries {
    struct DeviceText {                                               // the text goes to the device once for the counting call and the call that writes
        void* p{nullptr};
        ~DeviceText() { if (p) fmgpu_free(p); }
    } staged;
    auto const* bytes = reinterpret_cast<uint8_t const*>(text.data());
    if (!text.empty()) {
        detail::check(fmgpu_malloc(&staged.p, text.size()));
        detail::check(fmgpu_memcpy_h2d(staged.p, bytes, text.size()));
        bytes = static_cast<uint8_t const*>(staged.p);
    }
    fmgpu_parse_result res{};
    auto const fmt = static_cast<int32_t>(format);
    detail::check(fmgpu_queries_parse(bytes, text.size(), fmt, final ? 1 : 0, table.map.data(), nullptr, 0, nullptr, 0, nullptr, nullptr, &res, nullptr));
    ParsedQueries out;
    out.qbuf.assign(std::max<size_t>(res.symbols, 1), 0);
    out.qoff.assign(res.reads + 1, 0);
    out.names.assign(res.reads, fmgpu_text_span{0, 0});
    out.quals.assign(res.reads, fmgpu_text_span{0, 0});
    detail::check(fmgpu_queries_parse(bytes, text.size(), fmt, final ? 1 : 0, table.map.data(), out.qbuf.data(), res.symbols, out.qoff.data(), res.reads,
                                      out.names.data(), out.quals.data(), &res, nullptr));
    out.consumed = res.consumed; out.foreign = res.foreign;
    return out;
}

namespace search_no_errors {
template <typename Index, typename Delegate>
void search(Index const& index, PackedQueries const& queries, Delegate&& delegate) {
    size_t nq = queries.size();
    std::vector<uint64_t> lb(nq), len(nq);
    detail::check(fmgpu_search_exact_q4(index.handle, queries.packed.data(), queries.qoff.data(), nq, lb.data(), len.data(), nullptr, nullptr));
    using cursor_t = select_cursor_t<Index>;
    for (size_t q = 0; q < nq; ++q) {
        if (len[q] == 0) continue;
        cursor_t cur{};
        cur.index = &index; cur.lb = lb[q]; cur.len = len[q];
        delegate(q, cur);
    }
}
// search(index, queries, delegate(qidx, cursor)) — search/SearchNoErrors.h:28-86; only non-empty cursors are reported
template <typename Index, typename Queries, typename Delegate>
void search(Index const& index, Queries const& queries, Delegate&& delegate, size_t /*BatchSize*/ = 32) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    size_t nq = off.size() - 1;
    std::vector<uint64_t> lb(nq), len(nq);
    detail::check(fmgpu_search_exact(index.handle, buf.data(), off.data(), nq, lb.data(), len.data(), nullptr, nullptr));
    using cursor_t = select_cursor_t<Index>;
    for (size_t q = 0; q < nq; ++q) {
        if (len[q] == 0) continue;
        cursor_t cur{};
        cur.index = &index; cur.lb = lb[q]; cur.len = len[q];
        delegate(q, cur);
    }
}
}  // namespace search_no_errors

namespace search_backtracking {
// search(index, queries, maxError, delegate(qidx, cursor, errors)) — search/Backtracking.h:85-89
template <typename Index, typename Queries, typename Delegate>
void search(Index const& index, Queries const& queries, size_t maxError, Delegate&& delegate) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    size_t nq = off.size() - 1;
    auto hits = detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
        return fmgpu_search_backtracking(index.handle, buf.data(), off.data(), nq, maxError, out, cap, count, nullptr, nullptr);
    });
    detail::report(index, hits, delegate);
}
}  // namespace search_backtracking

namespace search_ng26 {
namespace detail2 {
// one scheme over one batch; qmap (optional) renames the batch's query numbers; q4: buf is the 4-bit packed form
template <bool Edit, typename Index>
std::vector<fmgpu_hit> run(Index const& index, std::vector<uint8_t> const& buf, std::vector<uint64_t> const& off, search_scheme::Scheme const& scheme,
                           std::vector<size_t> const& partition, size_t n, std::vector<uint64_t> const* qmap, bool q4 = false) {
    size_t nq = off.size() - 1;
    if (scheme.empty() || nq == 0 || n == 0) return {};
    size_t P = scheme[0].pi.size();
    std::vector<uint64_t> pi, l, u, part(partition.begin(), partition.end());
    for (auto const& s : scheme) {
        if (s.pi.size() != P) throw std::runtime_error("fmindex-collection (gpu): searches of a scheme must have the same number of parts");
        pi.insert(pi.end(), s.pi.begin(), s.pi.end()); l.insert(l.end(), s.l.begin(), s.l.end()); u.insert(u.end(), s.u.begin(), s.u.end());
    }
    fmgpu_scheme sc{static_cast<int32_t>(scheme.size()), static_cast<int32_t>(P), pi.data(), l.data(), u.data(), part.empty() ? nullptr : part.data(),
                    Edit ? 1 : 0, 0};
    auto hits = detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
        return (q4 ? fmgpu_search_scheme_q4 : fmgpu_search_scheme)(index.handle, buf.data(), off.data(), nq, &sc, n, out, cap, count, nullptr, nullptr);
    });
    if (qmap) for (auto& h : hits) h.qidx = (*qmap)[h.qidx];
    return hits;
}
}  // namespace detail2

// search<Edit>(index, queries, scheme, partition, delegate(qidx, cursor, errors), n) — search/SearchNg26.h:426-433.
// Edit = true (the reference's default) adds insertions and deletions (:146-218, :286-362); Edit = false is Hamming distance.
template <bool Edit = true, typename Index, typename Queries, typename Delegate>
void search(Index const& index, Queries const& queries, search_scheme::Scheme const& scheme, std::vector<size_t> const& partition,
            Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    auto hits = detail2::run<Edit>(index, buf, off, scheme, partition, n, nullptr);
    detail::report(index, hits, delegate);
}
template <bool Edit = true, typename Index, typename Delegate>
void search(Index const& index, PackedQueries const& queries, search_scheme::Scheme const& scheme, std::vector<size_t> const& partition,
            Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    auto hits = detail2::run<Edit>(index, queries.packed, queries.qoff, scheme, partition, n, nullptr, true);
    detail::report(index, hits, delegate);
}
// search<Edit>(index, queries, maxErrors, delegate, n) — search/SearchNg26.h:436-444: per query length the cached scheme
// h2(maxErrors + (length == 2 ? 1 : 2), 0, maxErrors) (CachedSearchScheme.h:16-36) with a uniform partition.  For Edit = false the
// reference additionally applies limitToHamming to the un-expanded scheme, which loses hits — not reproduced here.
template <bool Edit = true, typename Index, typename Queries, typename Delegate>
void search(Index const& index, Queries const& queries, size_t maxErrors, Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    std::vector<fmgpu_hit> all;
    for (int shortLen = 0; shortLen < 2; ++shortLen) {
        std::vector<uint8_t> buf; std::vector<uint64_t> off{0}, qmap;
        size_t qidx = 0;
        for (auto const& q : queries) {
            if ((q.size() == 2) == (shortLen == 1)) { buf.insert(buf.end(), q.begin(), q.end()); off.push_back(buf.size()); qmap.push_back(qidx); }
            ++qidx;
        }
        if (qmap.empty()) continue;
        auto hits = detail2::run<Edit>(index, buf, off, search_scheme::generator::h2(maxErrors + (shortLen ? 1 : 2), 0, maxErrors), {}, n, &qmap);
        all.insert(all.end(), hits.begin(), hits.end());
    }
    detail::report(index, all, delegate);
}
// the same for a packed batch: a batch of one length class (no read of length 2, or only such reads) goes down as it is, a mixed one is split in the byte form
template <bool Edit = true, typename Index, typename Delegate>
void search(Index const& index, PackedQueries const& queries, size_t maxErrors, Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    size_t shortReads = 0;
    for (size_t q = 0; q < queries.size(); ++q) shortReads += queries.qoff[q + 1] - queries.qoff[q] == 2;
    if (shortReads != 0 && shortReads != queries.size()) { search<Edit>(index, queries.unpack(), maxErrors, std::forward<Delegate>(delegate), n); return; }
    if (queries.size() == 0) return;
    auto hits = detail2::run<Edit>(index, queries.packed, queries.qoff, search_scheme::generator::h2(maxErrors + (shortReads ? 1 : 2), 0, maxErrors), {}, n, nullptr, true);
    detail::report(index, hits, delegate);
}
// search_best<Edit>(index, queries, {(scheme, partition), ...}, delegate, n) — search/SearchNg26.h:447-473: per query the first scheme
// that reports anything wins.  One fmgpu_search_best call: the ladder is cut per batch on the device (a scheme without a search finds nothing and is left out).
namespace detail2 {
template <bool Edit, typename Index>
std::vector<fmgpu_hit> run_best(Index const& index, std::vector<uint8_t> const& buf, std::vector<uint64_t> const& off,
                                std::vector<std::tuple<search_scheme::Scheme, std::vector<size_t>>> const& schemes, size_t n, bool q4 = false,
                                bool pairs = false) {
    size_t nq = off.size() - 1;
    if (nq == 0 || n == 0) return {};
    struct Flat { std::vector<uint64_t> pi, l, u, part; };
    std::vector<Flat> flat;
    flat.reserve(schemes.size());
    std::vector<fmgpu_scheme> ladder;
    for (auto const& [scheme, partition] : schemes) {
        if (scheme.empty()) continue;
        size_t P = scheme[0].pi.size();
        flat.emplace_back();
        auto& f = flat.back();
        f.part.assign(partition.begin(), partition.end());
        for (auto const& s : scheme) {
            if (s.pi.size() != P) throw std::runtime_error("fmindex-collection (gpu): searches of a scheme must have the same number of parts");
            f.pi.insert(f.pi.end(), s.pi.begin(), s.pi.end()); f.l.insert(f.l.end(), s.l.begin(), s.l.end()); f.u.insert(f.u.end(), s.u.begin(), s.u.end());
        }
        ladder.push_back(fmgpu_scheme{static_cast<int32_t>(scheme.size()), static_cast<int32_t>(P), f.pi.data(), f.l.data(), f.u.data(),
                                      f.part.empty() ? nullptr : f.part.data(), Edit ? 1 : 0, 0});
    }
    if (ladder.empty()) return {};
    return detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
        return (pairs ? fmgpu_search_best_pairs : q4 ? fmgpu_search_best_q4 : fmgpu_search_best)(index.handle, buf.data(), off.data(), nq, ladder.data(), static_cast<int32_t>(ladder.size()), n, out, cap, count,
                                                               nullptr, nullptr, nullptr);
    }, true);
}
}  // namespace detail2
template <bool Edit = true, typename Index, typename Queries, typename Delegate>
void search_best(Index const& index, Queries const& queries, std::vector<std::tuple<search_scheme::Scheme, std::vector<size_t>>> const& schemes,
                 Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    auto hits = detail2::run_best<Edit>(index, buf, off, schemes, n);
    detail::report(index, hits, delegate);
}
template <bool Edit = true, typename Index, typename Delegate>
void search_best(Index const& index, PackedQueries const& queries, std::vector<std::tuple<search_scheme::Scheme, std::vector<size_t>>> const& schemes,
                 Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    auto hits = detail2::run_best<Edit>(index, queries.packed, queries.qoff, schemes, n, true);
    detail::report(index, hits, delegate);
}
// search_best_pairs<Edit>: search_best over a batch whose reads 2j and 2j + 1 are the two strands of one read (fmc::bothStrands): one fmgpu_search_best_pairs call —
// once either strand of a read is found, neither goes on.  The delegate sees qidx of the doubled batch.
template <bool Edit = true, typename Index, typename Queries, typename Delegate>
void search_best_pairs(Index const& index, Queries const& queries, std::vector<std::tuple<search_scheme::Scheme, std::vector<size_t>>> const& schemes,
                       Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    auto hits = detail2::run_best<Edit>(index, buf, off, schemes, n, false, true);
    detail::report(index, hits, delegate);
}
// search_best<Edit>(index, queries, maxErrors, delegate, n) — search/SearchNg26.h:476-487: the whole batch with 0, 1, ... maxErrors - 1
// errors (the reference's loop ends before maxErrors), stopping at the first error count for which any query reports a hit
template <bool Edit = true, typename Index, typename Queries, typename Delegate>
void search_best(Index const& index, Queries const& queries, size_t maxErrors, Delegate&& delegate, size_t n = std::numeric_limits<size_t>::max()) {
    bool found = false;
    for (size_t i = 0; i < maxErrors && !found; ++i)
        search<Edit>(index, queries, i, [&](size_t qidx, auto cursor, size_t e) { if (cursor.count() == 0) return; found = true; delegate(qidx, cursor, e); }, n);
}
}  // namespace search_ng26

// search/SearchHammingSM.h: the search-scheme Hamming walk with a scoring matrix (fmgpu_search_hamming_sm).  Every (query rank, text rank) pair is a free match,
// a mismatch that costs one error, or not pairable; the query alphabet may be larger than the index's.
namespace search_hamming_sm {
// ScoringMatrix<QuerySigma, RefSigma> (:16-45) as the two mask arrays of fmgpu_scoring_matrix.  Default-constructed like the reference's: identity free, every other
// pair of ranks 1.. at cost 1.  The search walks the members of a mask in ascending rank, which is the reference's list order when setCost is called in ascending
// refRank per query rank (its default constructor and its test do so).
template <size_t QuerySigma, size_t RefSigma = QuerySigma>
struct ScoringMatrix {
    static_assert(QuerySigma >= 1 && QuerySigma <= 256 && RefSigma >= 1 && RefSigma <= 32, "query ranks 0 .. 255 have a row; the masks are one word");
    std::array<uint32_t, QuerySigma> freeMask{}, costMask{};

    ScoringMatrix() {
        for (size_t y{1}; y < RefSigma; ++y)
            for (size_t x{1}; x < QuerySigma; ++x) setCost(x, y, x == y ? 0 : 1);
    }
    void setCost(size_t queryRank, size_t refRank, size_t cost) {   // cost 0 or 1
        if (queryRank >= QuerySigma || refRank >= RefSigma || cost > 1) throw std::runtime_error("fmindex-collection (gpu): ScoringMatrix::setCost out of range");
        setUnpairable(queryRank, refRank);
        (cost ? costMask : freeMask)[queryRank] |= uint32_t{1} << refRank;
    }
    void setUnpairable(size_t queryRank, size_t refRank) {
        freeMask.at(queryRank) &= ~(uint32_t{1} << refRank);
        costMask.at(queryRank) &= ~(uint32_t{1} << refRank);
    }
    auto raw() const -> fmgpu_scoring_matrix { return {static_cast<int32_t>(QuerySigma), 0, freeMask.data(), costMask.data()}; }
};
// query ranks 1..4 = A C G T, 5..15 = R Y S W K M B D H V N on a sigma = 5 index: every code is free for its bases and costs one error for the others
inline auto iupacDna() -> ScoringMatrix<16, 5> {
    ScoringMatrix<16, 5> sm;
    char const* bases[11] = {"AG", "CT", "CG", "AT", "GT", "AC", "CGT", "AGT", "ACT", "ACG", "ACGT"};
    for (size_t k = 0; k < 11; ++k)
        for (size_t r = 1; r <= 4; ++r) sm.setCost(5 + k, r, std::string(bases[k]).find("ACGT"[r - 1]) != std::string::npos ? 0 : 1);
    return sm;
}

// search(index, queries, scheme, sm, delegate(qidx, cursor, errors)[, n]) — :199-212, with the `n` of search_ng26 (n results per query at most).  The parts are
// createUniformPartition(scheme parts, query length); a query shorter than the scheme has parts reports nothing.
template <typename Index, typename Queries, typename SM, typename Delegate>
void search(Index const& index, Queries const& queries, search_scheme::Scheme const& scheme, SM const& sm, Delegate&& delegate,
            size_t n = std::numeric_limits<size_t>::max()) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    size_t nq = off.size() - 1;
    if (scheme.empty() || nq == 0 || n == 0) return;
    size_t P = scheme[0].pi.size();
    std::vector<uint64_t> pi, l, u;
    for (auto const& s : scheme) {
        if (s.pi.size() != P) throw std::runtime_error("fmindex-collection (gpu): searches of a scheme must have the same number of parts");
        pi.insert(pi.end(), s.pi.begin(), s.pi.end()); l.insert(l.end(), s.l.begin(), s.l.end()); u.insert(u.end(), s.u.begin(), s.u.end());
    }
    fmgpu_scheme sc{static_cast<int32_t>(scheme.size()), static_cast<int32_t>(P), pi.data(), l.data(), u.data(), nullptr, 0, 0};
    fmgpu_scoring_matrix m = sm.raw();
    auto hits = detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
        return fmgpu_search_hamming_sm(index.handle, buf.data(), off.data(), nq, &sc, &m, n, out, cap, count, nullptr, nullptr);
    });
    detail::report(index, hits, delegate);
}
}  // namespace search_hamming_sm

// search/SearchNg21.h: edit-distance search over an EXPANDED scheme (search_scheme::expand(scheme, query length): one {pi, l, u} entry per
// query symbol), so the queries of a call have that length; shorter ones — which the reference would read out of bounds — report nothing.
namespace search_ng21 {
namespace detail2 {
template <typename Index>
std::vector<fmgpu_hit> run(Index const& index, std::vector<uint8_t> const& buf, std::vector<uint64_t> const& off, search_scheme::Scheme const& scheme,
                           size_t n, std::vector<uint64_t> const* qmap, bool q4 = false) {
    size_t nq = off.size() - 1;
    if (scheme.empty() || nq == 0) return {};                                         // :205
    size_t M = scheme[0].pi.size();
    std::vector<uint64_t> pi, l, u;
    for (auto const& s : scheme) {
        if (s.pi.size() != M || s.l.size() != M || s.u.size() != M) throw std::runtime_error("fmindex-collection (gpu): searches of an expanded scheme must have the same length");
        pi.insert(pi.end(), s.pi.begin(), s.pi.end()); l.insert(l.end(), s.l.begin(), s.l.end()); u.insert(u.end(), s.u.begin(), s.u.end());
    }
    fmgpu_expanded_scheme sc{static_cast<int32_t>(scheme.size()), 0, M, pi.data(), l.data(), u.data()};
    auto hits = detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
        return (q4 ? fmgpu_search_ng21_q4 : fmgpu_search_ng21)(index.handle, buf.data(), off.data(), nq, &sc, n, out, cap, count, nullptr, nullptr);
    });
    if (qmap) for (auto& h : hits) h.qidx = (*qmap)[h.qidx];
    return hits;
}
// search_best / search_best_n: one fmgpu_search_best_ng21 call, the ladder is cut per batch on the device (`if (ct > 0) break;` :261, :290 is its "found"; a scheme
// without a search finds nothing and is left out)
template <typename Index, typename Delegate>
void best(Index const& index, std::vector<uint8_t> const& buf, std::vector<uint64_t> const& off, std::vector<search_scheme::Scheme> const& schemes, size_t n,
          Delegate&& delegate, bool q4 = false, bool pairs = false) {
    size_t nq = off.size() - 1;
    struct Flat { std::vector<uint64_t> pi, l, u; };
    std::vector<Flat> flat;
    flat.reserve(schemes.size());
    std::vector<fmgpu_expanded_scheme> ladder;
    for (auto const& scheme : schemes) {
        if (scheme.empty()) continue;
        size_t M = scheme[0].pi.size();
        flat.emplace_back();
        auto& f = flat.back();
        for (auto const& s : scheme) {
            if (s.pi.size() != M || s.l.size() != M || s.u.size() != M) throw std::runtime_error("fmindex-collection (gpu): searches of an expanded scheme must have the same length");
            f.pi.insert(f.pi.end(), s.pi.begin(), s.pi.end()); f.l.insert(f.l.end(), s.l.begin(), s.l.end()); f.u.insert(f.u.end(), s.u.begin(), s.u.end());
        }
        ladder.push_back(fmgpu_expanded_scheme{static_cast<int32_t>(scheme.size()), 0, M, f.pi.data(), f.l.data(), f.u.data()});
    }
    std::vector<fmgpu_hit> hits;
    if (nq != 0 && !ladder.empty())
        hits = detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
            return (pairs ? fmgpu_search_best_ng21_pairs : q4 ? fmgpu_search_best_ng21_q4 : fmgpu_search_best_ng21)(index.handle, buf.data(), off.data(), nq, ladder.data(), static_cast<int32_t>(ladder.size()), n, out,
                                                                             cap, count, nullptr, nullptr, nullptr);
        }, true);
    detail::report(index, hits, delegate);
}
}  // namespace detail2

// search(index, queries, search_scheme, delegate(qidx, cursor, errors)) — :205-217
template <typename Index, typename Queries, typename Delegate>
void search(Index const& index, Queries const& queries, search_scheme::Scheme const& scheme, Delegate&& delegate) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    auto hits = detail2::run(index, buf, off, scheme, std::numeric_limits<size_t>::max(), nullptr);
    detail::report(index, hits, delegate);
}
// search_n(index, queries, search_scheme, n, delegate) — :220-240: at most n rows per query, the last cursor clipped
template <typename Index, typename Queries, typename Delegate>
void search_n(Index const& index, Queries const& queries, search_scheme::Scheme const& scheme, size_t n, Delegate&& delegate) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    auto hits = detail2::run(index, buf, off, scheme, n, nullptr);
    detail::report(index, hits, delegate);
}
template <typename Index, typename Delegate>
void search(Index const& index, PackedQueries const& queries, search_scheme::Scheme const& scheme, Delegate&& delegate) {
    auto hits = detail2::run(index, queries.packed, queries.qoff, scheme, std::numeric_limits<size_t>::max(), nullptr, true);
    detail::report(index, hits, delegate);
}
template <typename Index, typename Delegate>
void search_n(Index const& index, PackedQueries const& queries, search_scheme::Scheme const& scheme, size_t n, Delegate&& delegate) {
    auto hits = detail2::run(index, queries.packed, queries.qoff, scheme, n, nullptr, true);
    detail::report(index, hits, delegate);
}
// search_best(index, queries, search_schemes, delegate) — :242-264: per query the first scheme of the list that reports any row
template <typename Index, typename Queries, typename Delegate>
void search_best(Index const& index, Queries const& queries, std::vector<search_scheme::Scheme> const& schemes, Delegate&& delegate) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    detail2::best(index, buf, off, schemes, std::numeric_limits<size_t>::max(), std::forward<Delegate>(delegate));
}
template <typename Index, typename Delegate>
void search_best(Index const& index, PackedQueries const& queries, std::vector<search_scheme::Scheme> const& schemes, Delegate&& delegate) {
    detail2::best(index, queries.packed, queries.qoff, schemes, std::numeric_limits<size_t>::max(), std::forward<Delegate>(delegate), true);
}
// search_best_pairs: search_best_n over a batch whose reads 2j and 2j + 1 are the two strands of one read (one fmgpu_search_best_ng21_pairs call)
template <typename Index, typename Queries, typename Delegate>
void search_best_pairs(Index const& index, Queries const& queries, std::vector<search_scheme::Scheme> const& schemes, Delegate&& delegate,
                       size_t n = std::numeric_limits<size_t>::max()) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    detail2::best(index, buf, off, schemes, n, std::forward<Delegate>(delegate), false, true);
}
// search_best_n(index, queries, search_schemes, n, delegate) — :267-293
template <typename Index, typename Queries, typename Delegate>
void search_best_n(Index const& index, Queries const& queries, std::vector<search_scheme::Scheme> const& schemes, size_t n, Delegate&& delegate) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    detail2::best(index, buf, off, schemes, n, std::forward<Delegate>(delegate));
}
template <typename Index, typename Delegate>
void search_best_n(Index const& index, PackedQueries const& queries, std::vector<search_scheme::Scheme> const& schemes, size_t n, Delegate&& delegate) {
    detail2::best(index, queries.packed, queries.qoff, schemes, n, std::forward<Delegate>(delegate), true);
}
}  // namespace search_ng21

// fmc::search<EditDistance>(index, queries, errors, delegate(qidx, cursor, errors)) — search/search.h:26-35
template <bool EditDistance, typename Index, typename Queries, typename Delegate>
void search(Index const& index, Queries const& queries, size_t errors, Delegate&& delegate) {
    if (errors == 0) search_no_errors::search(index, queries, [&](size_t qidx, auto const& cursor) { delegate(qidx, cursor, size_t{0}); });
    else search_ng26::search<EditDistance>(index, queries, errors, std::forward<Delegate>(delegate));
}
// fmc::search_n<EditDistance>(index, queries, errors, n, delegate) — search/search.h:43-46
template <bool EditDistance, typename Index, typename Queries, typename Delegate>
void search_n(Index const& index, Queries const& queries, size_t errors, size_t n, Delegate&& delegate) {
    search_ng26::search<EditDistance>(index, queries, errors, std::forward<Delegate>(delegate), n);
}

// fmc::search_smems(index, queries, minLen, maxRows, delegate(qidx, cursor, qbeg, qlen)) — no counterpart in the reference: the super-maximal exact matches of
// every read (fmgpu_search_smems), reported in ascending (qidx, qbeg).  cursor holds the rows of queries[qidx][qbeg .. qbeg + qlen); it has been extended leftwards
// only (lbRev = 0 on a BiFMIndex).  A seed is kept if qlen >= minLen and (maxRows == 0 or) it has at most maxRows rows.
namespace detail {
template <typename Index, typename Call, typename Delegate>
void report_smems(Index const& index, size_t nq, Call&& call, Delegate&& delegate) {
    std::vector<fmgpu_hit> hits(std::max<size_t>(1024, 4 * nq));
    std::vector<fmgpu_seed_span> spans(hits.size());
    uint64_t count = 0;
    int rc = call(hits.data(), spans.data(), hits.size(), &count);
    if (rc == FMGPU_ERR_CAPACITY) {                               // once more with the size the call reported
        hits.resize(count); spans.resize(count);
        rc = call(hits.data(), spans.data(), hits.size(), &count);
    }
    check(rc);
    using cursor_t = select_cursor_t<Index>;
    for (size_t k = 0; k < count; ++k) {
        cursor_t cur{};
        cur.index = &index; cur.lb = hits[k].lb; cur.len = hits[k].len;
        delegate(static_cast<size_t>(hits[k].qidx), cur, static_cast<size_t>(spans[k].qbeg), static_cast<size_t>(spans[k].qlen));
    }
}
}  // namespace detail
template <typename Index, typename Queries, typename Delegate>
void search_smems(Index const& index, Queries const& queries, size_t minLen, size_t maxRows, Delegate&& delegate) {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    size_t nq = off.size() - 1;
    detail::report_smems(index, nq, [&](fmgpu_hit* out, fmgpu_seed_span* span, uint64_t cap, uint64_t* count) {
        return fmgpu_search_smems(index.handle, buf.data(), off.data(), nq, static_cast<uint32_t>(minLen), maxRows, out, span, cap, count, nullptr, nullptr, nullptr);
    }, std::forward<Delegate>(delegate));
}
template <typename Index, typename Delegate>
void search_smems(Index const& index, PackedQueries const& queries, size_t minLen, size_t maxRows, Delegate&& delegate) {
    detail::report_smems(index, queries.size(), [&](fmgpu_hit* out, fmgpu_seed_span* span, uint64_t cap, uint64_t* count) {
        return fmgpu_search_smems_q4(index.handle, queries.packed.data(), queries.qoff.data(), queries.size(), static_cast<uint32_t>(minLen), maxRows, out, span, cap, count,
                                     nullptr, nullptr, nullptr);
    }, std::forward<Delegate>(delegate));
}

// LocateLinear{index, cursor}: for (auto [seqId, pos, offset] : LocateLinear{index, cursor}) — locate.h:14-57 (one batched call)
template <typename Index, typename Cursor>
struct LocateLinear {
    std::vector<typename Index::LEntry> entries;
    LocateLinear(Index const& index, Cursor const& cursor) {
        std::vector<uint64_t> rows(cursor.len);
        std::iota(rows.begin(), rows.end(), uint64_t{cursor.lb});
        entries = index.locate(rows);
    }
    auto begin() const { return entries.begin(); }
    auto end() const { return entries.end(); }
};
template <typename Index, typename Cursor> LocateLinear(Index const&, Cursor const&) -> LocateLinear<Index, Cursor>;

// fmc::Search{index, queries, editDistance, errors, maxResults, reportFunc}() — search/search.h:48-75: searches, locates every row of every
// reported cursor and calls reportFunc(qidx, seqId, pos + offset, errors).  The cursors of the batch are collected in callback order and located
// by ONE fmgpu_locate_hits call; the reports come in the order of the reference's per-cursor LocateLinear loop.
template <typename index_t, typename queries_t, typename delegate_t>
struct Search {
    index_t const&        index;
    queries_t const&      queries;
    bool                  editDistance{true};
    size_t                errors{0};
    std::optional<size_t> maxResults{};
    delegate_t const&     reportFunc;
    void operator()() {
        std::vector<fmgpu_hit> hits;
        auto report = [&](size_t qidx, auto const& cursor, size_t e) {
            fmgpu_hit h{};
            h.qidx = qidx; h.lb = cursor.lb; h.len = cursor.len; h.errors = static_cast<uint32_t>(e);
            hits.push_back(h);
        };
        if (maxResults) {
            if (editDistance) search_n<true>(index, queries, errors, *maxResults, report);
            else search_n<false>(index, queries, errors, *maxResults, report);
        } else {
            if (editDistance) search<true>(index, queries, errors, report);
            else search<false>(index, queries, errors, report);
        }
        for (auto const& p : index.locateHits(hits))     // (seqId as LocateLinear's entry holds it: 32 bits)
            reportFunc(static_cast<size_t>(p.qidx), static_cast<uint32_t>(p.seq_id), static_cast<size_t>(p.pos), static_cast<size_t>(p.errors));
    }
};
template <typename I, typename Q, typename D> Search(I const&, Q const&, bool, size_t, std::optional<size_t>, D const&) -> Search<I, Q, D>;

// fmc::map(index, queries, MapQuery) — include/fmgpu.h: fmgpu_map: the whole path of fmc::Search behind one call.  The search (exact, a best-hit ladder of schemes or of
// expanded schemes), the callback order and the locate of every row run on the device; the hit records never visit the host in between.  MapResult::positions is in
// fmc::Search's report order (position.hit indexes MapResult::hits); stratum[q] = the ladder's scheme that found read q (exact search: 0), 255 if none did.
// MapQuery::search(errors, edit) is the query fmc::Search{index, queries, edit, errors, maxResults} runs: search_no_errors for 0 errors without maxResults, else the single
// scheme h2(errors + 2, 0, errors) with uniform partitions (`parts` = another number of parts: a batch of 2-symbol reads, which the reference searches with
// h2(errors + 1, 0, errors), takes parts = errors + 1; a scheme skips the reads that are shorter than its parts);
// MapQuery::ladder(maxErrors, edit) is h2(k + 2, 0, k) for k = 0 .. maxErrors, the best-stratum mode of a read mapper.
struct MapQuery {
    enum class Kind { Exact, Schemes, Ng21 };
    Kind kind{Kind::Exact};
    std::vector<std::tuple<search_scheme::Scheme, std::vector<size_t>>> schemes;     // Kind::Schemes: (scheme, partition; empty = uniform per read)
    std::vector<search_scheme::Scheme> expanded;                                      // Kind::Ng21: expanded schemes (search_scheme::expand)
    bool   editDistance{true};
    size_t maxResults{std::numeric_limits<size_t>::max()};
    bool   locate{true};
    size_t firstRecords{0};

    static auto search(size_t errors, bool edit = true, std::optional<size_t> maxResults = {}, size_t parts = 0) -> MapQuery {
        MapQuery q;
        q.editDistance = edit;
        if (maxResults) q.maxResults = *maxResults;
        if (errors == 0 && !maxResults) return q;
        q.kind = Kind::Schemes;
        q.schemes.emplace_back(search_scheme::generator::h2(parts ? parts : errors + 2, 0, errors), std::vector<size_t>{});
        return q;
    }
    static auto ladder(size_t maxErrors, bool edit = true) -> MapQuery {
        MapQuery q;
        q.kind = Kind::Schemes; q.editDistance = edit;
        for (size_t k = 0; k <= maxErrors; ++k) q.schemes.emplace_back(search_scheme::generator::h2(k + 2, 0, k), std::vector<size_t>{});
        return q;
    }
};
struct MapResult {
    std::vector<fmgpu_position> positions;
    std::vector<fmgpu_hit>      hits;
    std::vector<uint8_t>        stratum;
};
namespace detail {
// a MapQuery flattened into the C struct (the arrays live as long as this object)
struct FlatMapQuery {
    struct Flat { std::vector<uint64_t> pi, l, u, part; };
    std::vector<Flat> flat;
    std::vector<fmgpu_scheme> ladder;
    std::vector<fmgpu_expanded_scheme> expanded;
    fmgpu_map_query what{};
    FlatMapQuery(FlatMapQuery const&) = delete;
    FlatMapQuery& operator=(FlatMapQuery const&) = delete;
    explicit FlatMapQuery(MapQuery const& q) {
        auto append = [](Flat& f, search_scheme::Scheme const& scheme, size_t width) {
            for (auto const& s : scheme) {
                if (s.pi.size() != width) throw std::runtime_error("fmindex-collection (gpu): searches of a scheme must have the same number of parts");
                f.pi.insert(f.pi.end(), s.pi.begin(), s.pi.end()); f.l.insert(f.l.end(), s.l.begin(), s.l.end()); f.u.insert(f.u.end(), s.u.begin(), s.u.end());
            }
        };
        flat.reserve(q.schemes.size() + q.expanded.size());
        if (q.kind == MapQuery::Kind::Schemes) {
            for (auto const& [scheme, partition] : q.schemes) {
                size_t P = scheme.empty() ? 0 : scheme[0].pi.size();
                auto& f = flat.emplace_back();
                f.part.assign(partition.begin(), partition.end());
                append(f, scheme, P);
                ladder.push_back(fmgpu_scheme{static_cast<int32_t>(scheme.size()), static_cast<int32_t>(P), f.pi.data(), f.l.data(), f.u.data(),
                                              f.part.empty() ? nullptr : f.part.data(), q.editDistance ? 1 : 0, 0});
            }
            what.kind = FMGPU_MAP_SCHEME; what.n_schemes = static_cast<int32_t>(ladder.size()); what.schemes = ladder.data();
        } else if (q.kind == MapQuery::Kind::Ng21) {
            for (auto const& scheme : q.expanded) {
                size_t len = scheme.empty() ? 0 : scheme[0].pi.size();
                auto& f = flat.emplace_back();
                append(f, scheme, len);
                expanded.push_back(fmgpu_expanded_scheme{static_cast<int32_t>(scheme.size()), 0, len, f.pi.data(), f.l.data(), f.u.data()});
            }
            what.kind = FMGPU_MAP_NG21; what.n_schemes = static_cast<int32_t>(expanded.size()); what.schemes = expanded.data();
        }
        what.max_hits_per_query = q.maxResults == std::numeric_limits<size_t>::max() ? UINT64_MAX : q.maxResults;
        what.locate = q.locate ? 1 : 0;
        what.first_records = q.firstRecords;
    }
};
// the call into vectors: the counts are exact also on FMGPU_ERR_CAPACITY, so a second call with them fits
template <typename Call>
auto run_map(size_t nq, bool locate, Call&& call) -> MapResult {
    MapResult r;
    r.stratum.assign(nq, 255);
    uint64_t cap = locate ? std::max<uint64_t>(1024, 4 * nq) : 0, hcap = std::max<uint64_t>(1024, 4 * nq), count = 0, hcount = 0;
    for (int round = 0; round < 2; ++round) {
        r.positions.resize(cap); r.hits.resize(hcap);
        int rc = call(r.positions.data(), cap, &count, r.hits.data(), hcap, &hcount, r.stratum.data());
        if (rc == FMGPU_ERR_CAPACITY && round == 0) { cap = std::max(cap, count); hcap = std::max(hcap, hcount); continue; }
        check(rc);
        break;
    }
    r.positions.resize(count); r.hits.resize(hcount);
    return r;
}
}  // namespace detail
template <typename Index, typename Queries>
auto map(Index const& index, Queries const& queries, MapQuery const& query) -> MapResult {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    size_t nq = off.size() - 1;
    detail::FlatMapQuery flat{query};
    return detail::run_map(nq, query.locate, [&](fmgpu_position* out, uint64_t cap, uint64_t* count, fmgpu_hit* hits, uint64_t hcap, uint64_t* hcount, uint8_t* stratum) {
        return fmgpu_map(index.handle, buf.data(), off.data(), nq, &flat.what, out, cap, count, hits, hcap, hcount, stratum, nullptr, nullptr, nullptr);
    });
}
// Both strands (include/fmgpu.h: fmgpu_map_strands): fmc::map(index, reads, query, strands) maps every read and its reverse complement, the second strand made on the
// device.  qidx and MapResult::stratum count in the doubled batch: read = qidx >> 1, strand = qidx & 1; position.pos is where the searched string lies (strand 1: the
// leftmost position of the reverse complement).  pair = true: the best stratum per read — once either strand is found, neither goes on.  Strands::dna5() is the
// complement of the ranks $ A C G T.  bothStrands(seqs, complement) is the same doubled batch on the host: a symbol c < complement.size() becomes complement[c], any
// other stays as it is.
struct Strands {
    std::vector<uint8_t> complement;
    bool pair{false};
    static auto dna5(bool pair = false) -> Strands { return Strands{{0, 4, 3, 2, 1}, pair}; }
    auto c() const -> fmgpu_strands { return fmgpu_strands{complement.data(), static_cast<int32_t>(complement.size()), pair ? 1 : 0}; }
};
template <typename Queries>
auto bothStrands(Queries const& seqs, std::vector<uint8_t> const& complement) -> std::vector<std::vector<uint8_t>> {
    std::vector<std::vector<uint8_t>> out;
    for (auto const& s : seqs) {
        auto& fwd = out.emplace_back();
        for (auto c : s) fwd.push_back(static_cast<uint8_t>(c));
        std::vector<uint8_t> rev(fwd.rbegin(), fwd.rend());
        for (auto& c : rev) if (c < complement.size()) c = complement[c];
        out.push_back(std::move(rev));
    }
    return out;
}
template <typename Index, typename Queries>
auto map(Index const& index, Queries const& queries, MapQuery const& query, Strands const& strands) -> MapResult {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(queries, buf, off);
    size_t nq = off.size() - 1;
    detail::FlatMapQuery flat{query};
    fmgpu_strands st = strands.c();
    return detail::run_map(2 * nq, query.locate, [&](fmgpu_position* out, uint64_t cap, uint64_t* count, fmgpu_hit* hits, uint64_t hcap, uint64_t* hcount, uint8_t* stratum) {
        return fmgpu_map_strands(index.handle, buf.data(), off.data(), nq, &flat.what, &st, out, cap, count, hits, hcap, hcount, stratum, nullptr, nullptr, nullptr);
    });
}
template <typename Index>
auto map(Index const& index, PackedQueries const& queries, MapQuery const& query) -> MapResult {
    size_t nq = queries.size();
    detail::FlatMapQuery flat{query};
    return detail::run_map(nq, query.locate, [&](fmgpu_position* out, uint64_t cap, uint64_t* count, fmgpu_hit* hits, uint64_t hcap, uint64_t* hcount, uint8_t* stratum) {
        return fmgpu_map_q4(index.handle, queries.packed.data(), queries.qoff.data(), nq, &flat.what, out, cap, count, hits, hcap, hcount, stratum, nullptr, nullptr, nullptr);
    });
}

// Positions as text (include/fmgpu.h: fmgpu_positions_format): fmc::formatPositions(positions, spec[, readNames, seqNames]) is one line per located position, formatted
// on the device.  The default FormatSpec writes `qidx seq_id pos errors`, the line the reference's example prints per hit.  strands = true reads qidx as fmc::map with
// Strands numbers it (Column::Read and Column::ReadName use qidx >> 1, Column::Strand is '-' for an odd qidx); nameStop ends a name in front of its first blank; posAdd
// is added to pos.  A NameTable is the names back to back plus one span per row: built from strings, or from the bytes and spans a parse returned.
struct FormatSpec {
    enum class Column : uint8_t { Qidx = FMGPU_COL_QIDX, SeqId = FMGPU_COL_SEQ_ID, Pos = FMGPU_COL_POS, Errors = FMGPU_COL_ERRORS, Hit = FMGPU_COL_HIT,
                                  Read = FMGPU_COL_READ, Strand = FMGPU_COL_STRAND, ReadName = FMGPU_COL_READ_NAME, SeqName = FMGPU_COL_SEQ_NAME };
    std::vector<Column> columns{Column::Qidx, Column::SeqId, Column::Pos, Column::Errors};
    char     sep{' '};
    bool     strands{false};
    bool     nameStop{false};
    uint64_t posAdd{0};
};
struct NameTable {
    std::vector<uint8_t>         bytes;
    std::vector<fmgpu_text_span> spans;
    NameTable() = default;
    explicit NameTable(std::vector<std::string> const& names) {
        for (auto const& n : names) {
            spans.push_back(fmgpu_text_span{bytes.size(), n.size()});
            bytes.insert(bytes.end(), n.begin(), n.end());
        }
    }
    NameTable(std::string_view text, std::vector<fmgpu_text_span> spans_) : bytes(text.begin(), text.end()), spans(std::move(spans_)) {}
    auto c() const -> fmgpu_name_table { return fmgpu_name_table{bytes.empty() ? nullptr : bytes.data(), bytes.size(), spans.empty() ? nullptr : spans.data(), spans.size()}; }
};
inline auto formatPositions(std::vector<fmgpu_position> const& positions, FormatSpec const& spec = {}, NameTable const* readNames = nullptr,
                            NameTable const* seqNames = nullptr) -> std::string {
    if (spec.columns.empty() || spec.columns.size() > 8) throw std::runtime_error("fmindex-collection (gpu): a line has 1 .. 8 columns");
    fmgpu_format_spec s{};
    s.n_cols = static_cast<int32_t>(spec.columns.size());
    for (size_t c = 0; c < spec.columns.size(); ++c) s.cols[c] = static_cast<uint8_t>(spec.columns[c]);
    s.sep = static_cast<uint8_t>(spec.sep); s.strand_shift = spec.strands ? 1 : 0; s.name_stop = spec.nameStop ? 1 : 0; s.pos_add = spec.posAdd;
    fmgpu_name_table rt{}, qt{};
    if (readNames) { rt = readNames->c(); s.read_names = &rt; }
    if (seqNames) { qt = seqNames->c(); s.seq_names = &qt; }
    uint64_t bytes = 0;
    detail::check(fmgpu_positions_format(positions.data(), positions.size(), &s, nullptr, 0, &bytes, nullptr, nullptr));      // the counting call sizes the text exactly
    std::string text(bytes, '\0');
    if (bytes) detail::check(fmgpu_positions_format(positions.data(), positions.size(), &s, reinterpret_cast<uint8_t*>(text.data()), bytes, &bytes, nullptr, nullptr));
    return text;
}

// Positions as SAM (include/fmgpu.h: fmgpu_positions_sam, fmgpu_sam_header): fmc::formatSam(positions, reads, spec) is the alignment lines of the positions fmc::map
// returned for `reads` (the FORWARD batch: any range of reads, a ParsedQueries among them), formatted on the device; fmc::samHeader(names, lengths, program) is the
// header in front of them.  spec.strands = the Strands the reads were mapped with (qidx counts both strands; an odd one is written reversed and complemented with flag
// 16).  Without a table QNAME and RNAME are numbers and QUAL is '*'.  cigar = true states that the search was ungapped: "<m>M".
struct CharTable {
    std::array<uint8_t, 256> map;
    // value firstRank + i -> letters[i], every other value (255, the Foreign symbol, among them) -> other
    explicit CharTable(std::string_view letters = "ACGT", uint8_t firstRank = 1, char other = 'N') {
        map.fill(static_cast<uint8_t>(other));
        for (size_t i = 0; i < letters.size(); ++i) map[firstRank + i] = static_cast<uint8_t>(letters[i]);
    }
    auto set(uint8_t value, char byte) -> CharTable& { map[value] = static_cast<uint8_t>(byte); return *this; }
    static auto dna5() -> CharTable { return CharTable{}.set(0, '$'); }       // the inverse of SymbolTable::dna5()
};
struct SamSpec {
    CharTable        charOf{CharTable::dna5()};
    Strands const*   strands{nullptr};
    NameTable const* readNames{nullptr};
    NameTable const* quals{nullptr};
    NameTable const* seqNames{nullptr};
    bool    cigar{true};
    bool    emitUnmapped{true};
    bool    secondarySeq{false};
    uint8_t mapqUnique{60}, mapqMulti{0};
};
struct SamText {
    std::string           text;
    std::vector<uint64_t> lineOffsets;                                       // lines + 1 entries where asked for, else empty
};
template <typename Queries>
auto formatSam(std::vector<fmgpu_position> const& positions, Queries const& reads, SamSpec const& spec = {}, bool wantLineOffsets = false) -> SamText {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(reads, buf, off);
    fmgpu_sam_spec s{};
    s.qbuf = buf.data(); s.qoff = off.data(); s.nq = off.size() - 1; s.char_of = spec.charOf.map.data();
    fmgpu_strands st{};
    fmgpu_name_table rt{}, qt{}, nt{};
    if (spec.strands) { st = spec.strands->c(); s.strands = &st; }
    if (spec.readNames) { rt = spec.readNames->c(); s.read_names = &rt; }
    if (spec.quals) { qt = spec.quals->c(); s.quals = &qt; }
    if (spec.seqNames) { nt = spec.seqNames->c(); s.seq_names = &nt; }
    s.cigar = spec.cigar ? 1 : 0; s.emit_unmapped = spec.emitUnmapped ? 1 : 0; s.secondary_seq = spec.secondarySeq ? 1 : 0;
    s.mapq_unique = spec.mapqUnique; s.mapq_multi = spec.mapqMulti;
    uint64_t bytes = 0, lines = 0;
    detail::check(fmgpu_positions_sam(positions.data(), positions.size(), &s, nullptr, 0, &bytes, nullptr, &lines, nullptr));        // the counting call sizes the text exactly
    SamText out;
    out.text.assign(bytes, '\0');
    if (wantLineOffsets) out.lineOffsets.assign(lines + 1, 0);
    if (bytes) detail::check(fmgpu_positions_sam(positions.data(), positions.size(), &s, reinterpret_cast<uint8_t*>(out.text.data()), bytes, &bytes,
                                                 wantLineOffsets ? out.lineOffsets.data() : nullptr, &lines, nullptr));
    return out;
}
inline auto samHeader(NameTable const& seqNames, std::vector<uint64_t> const& lengths, char const* program = nullptr) -> std::string {
    if (seqNames.spans.size() < lengths.size()) throw std::runtime_error("fmindex-collection (gpu): a name per sequence length");
    fmgpu_name_table const t = seqNames.c();
    uint64_t bytes = 0;
    detail::check(fmgpu_sam_header(&t, lengths.data(), lengths.size(), program, nullptr, 0, &bytes));
    std::string text(bytes, '\0');
    detail::check(fmgpu_sam_header(&t, lengths.data(), lengths.size(), program, reinterpret_cast<uint8_t*>(text.data()), bytes, &bytes));
    return text;
}

// Paired-end mates (include/fmgpu.h: fmgpu_positions_mates): fmc::joinMates(positionsA, readsA, positionsB, readsB, spec) joins the positions fmc::map returned for
// the two mates of every fragment — mate A of fragment f is read f of readsA, mate B read f of readsB — to concordant pairs, on the device; the overload without a
// second batch takes one interleaved batch whose reads 2f and 2f + 1 are the mates.  Only the lengths of the reads are used.  spec.strands = the positions come from a
// both-strand call (qidx counts both strands); without strands every strand is 0 and Orientation::FR finds nothing.
struct MatesSpec {
    enum class Orientation : uint8_t { FR = FMGPU_MATES_FR, Any = FMGPU_MATES_ANY };
    bool        strands{true};
    Orientation orientation{Orientation::FR};
    uint64_t    minTlen{0}, maxTlen{1000};                                   // inclusive
    bool        best{false};                                                 // only a fragment's pairs with the fewest errors
    uint64_t    maxRecords{0};                                               // > 0: a fragment one of whose mates has more records is not joined (class 5)
};
struct MatePairs {
    std::vector<fmgpu_mate_pair> pairs;                                      // fragments ascending, inside a fragment by a, then by (pos of b, b)
    std::vector<uint64_t>        offsets;                                    // fragments + 1 entries: each fragment's first pair
    std::vector<uint8_t>         classes;                                    // per fragment: 0 no record, 1 only A, 2 only B, 3 no concordant pair, 4 paired, 5 not joined
};
namespace detail {
inline auto joinMates(std::vector<fmgpu_position> const& a, std::vector<uint64_t> const& offA, std::vector<fmgpu_position> const* b, std::vector<uint64_t> const* offB,
                      MatesSpec const& spec) -> MatePairs {
    size_t const reads = offA.size() - 1;
    if (b ? offB->size() != offA.size() : reads % 2 != 0) throw std::runtime_error("fmindex-collection (gpu): one read of each batch per fragment");
    fmgpu_mates_spec s{};
    s.qoff_a = offA.data(); s.qoff_b = b ? offB->data() : nullptr; s.n_fragments = b ? reads : reads / 2;
    s.min_tlen = spec.minTlen; s.max_tlen = spec.maxTlen; s.max_records = spec.maxRecords;
    s.strand_shift = spec.strands ? 1 : 0; s.interleaved = b ? 0 : 1; s.orientation = static_cast<uint8_t>(spec.orientation); s.best = spec.best ? 1 : 0;
    fmgpu_position const* pb = b && !b->empty() ? b->data() : nullptr;
    fmgpu_position const* pa = a.empty() ? nullptr : a.data();
    uint64_t count = 0;
    detail::check(fmgpu_positions_mates(pa, a.size(), pb, b ? b->size() : 0, &s, nullptr, 0, &count, nullptr, nullptr, nullptr));     // the counting call sizes the pairs exactly
    MatePairs out;
    out.pairs.resize(count); out.offsets.assign(s.n_fragments + 1, 0); out.classes.assign(s.n_fragments, 0);
    detail::check(fmgpu_positions_mates(pa, a.size(), pb, b ? b->size() : 0, &s, count ? out.pairs.data() : nullptr, count, &count, out.offsets.data(),
                                        out.classes.empty() ? nullptr : out.classes.data(), nullptr));
    return out;
}
}  // namespace detail
template <typename QueriesA, typename QueriesB>
auto joinMates(std::vector<fmgpu_position> const& positionsA, QueriesA const& readsA, std::vector<fmgpu_position> const& positionsB, QueriesB const& readsB,
               MatesSpec const& spec = {}) -> MatePairs {
    std::vector<uint8_t> bufA, bufB; std::vector<uint64_t> offA, offB;
    detail::flatten(readsA, bufA, offA);
    detail::flatten(readsB, bufB, offB);
    return detail::joinMates(positionsA, offA, &positionsB, &offB, spec);
}
template <typename Queries>
auto joinMates(std::vector<fmgpu_position> const& positions, Queries const& interleavedReads, MatesSpec const& spec = {}) -> MatePairs {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(interleavedReads, buf, off);
    return detail::joinMates(positions, off, nullptr, nullptr, spec);
}

// Seed chains (include/fmgpu.h: fmgpu_seeds_chain): fmc::chainSeeds(positions, spans, spec) joins the located seeds of every query — the positions of
// index.locateHits for the hit records of fmgpu_search_smems, with that call's seed spans — to collinear chains on the device, best first inside a query.
// spec.queries counts the queries in the numbering of qidx (twice the reads for a both-strand batch).
struct ChainSpec {
    uint64_t queries{0};
    uint32_t maxGap{5000}, maxSkew{500};                                     // a link needs 1 <= dt, dq <= maxGap and |dt - dq| <= maxSkew
    double   gapCost{0.5};                                                   // per base of skew, kept in 8 fractional bits
    uint32_t maxLookback{64};                                                // 1 .. 256 candidates per anchor
    uint32_t minScore{0}, minAnchors{1};
    uint32_t maxChains{0};                                                   // > 0: the best maxChains of a query
    uint32_t maxAnchors{0};                                                  // > 0: a query with more anchors is left out (class 3)
    bool     wantAnchors{true};
};
struct SeedChains {
    std::vector<fmgpu_chain> chains;                                         // queries ascending, inside a query by descending score, then by the first anchor's place
    std::vector<uint64_t>    offsets;                                        // queries + 1 entries: each query's first chain
    std::vector<uint8_t>     classes;                                        // per query: 0 no anchor, 1 chained, 2 nothing past the filters, 3 left out by maxAnchors
    std::vector<uint32_t>    anchors;                                        // chain k's anchors, indices into positions: [chains[k].first, + chains[k].n_anchors)
};
inline auto chainSeeds(std::vector<fmgpu_position> const& positions, std::vector<fmgpu_seed_span> const& spans, ChainSpec const& spec) -> SeedChains {
    if (!(spec.gapCost >= 0.0) || spec.gapCost > 256.0) throw std::runtime_error("fmindex-collection (gpu): gapCost lies in 0 .. 256");
    fmgpu_chain_spec s{};
    s.nq = spec.queries; s.max_gap = spec.maxGap; s.max_skew = spec.maxSkew; s.gap_cost_q8 = static_cast<uint32_t>(spec.gapCost * 256.0 + 0.5);
    s.max_lookback = spec.maxLookback; s.min_score = spec.minScore; s.min_anchors = spec.minAnchors; s.max_chains = spec.maxChains; s.max_anchors = spec.maxAnchors;
    fmgpu_position const* p = positions.empty() ? nullptr : positions.data();
    fmgpu_seed_span const* sp = spans.empty() ? nullptr : spans.data();
    uint64_t count = 0;
    detail::check(fmgpu_seeds_chain(p, positions.size(), sp, spans.size(), &s, nullptr, 0, &count, nullptr, nullptr, nullptr, nullptr));     // the counting call sizes the chains exactly
    SeedChains out;
    out.chains.resize(count); out.offsets.assign(s.nq + 1, 0); out.classes.assign(s.nq, 0);
    if (spec.wantAnchors) out.anchors.assign(positions.size(), 0);
    detail::check(fmgpu_seeds_chain(p, positions.size(), sp, spans.size(), &s, count ? out.chains.data() : nullptr, count, &count,
                                    out.anchors.empty() ? nullptr : out.anchors.data(), out.offsets.data(), out.classes.empty() ? nullptr : out.classes.data(), nullptr));
    uint64_t used = 0;
    for (auto const& c : out.chains) used += c.n_anchors;
    if (spec.wantAnchors) out.anchors.resize(used);
    return out;
}

// Chain alignments (include/fmgpu.h: fmgpu_chains_align): fmc::alignChains(index, chains, positions, spans, reads, spec) aligns every chain of fmc::chainSeeds between
// its ends on the device — the anchors are exact matches, the gaps between them small banded dynamic programs — and returns one record per chain and the operations
// of all chains, len << 4 | op with BAM's codes.  `reads` is the batch in the numbering of qidx (the doubled batch for both-strand mapping).  The text under every
// chain comes from ONE extract call on `index` (the extract table is built for the call if the index lacks it, and dropped again); the overload without an index takes
// the windows as (text, offsets): window c at text[offsets[c] .. offsets[c + 1]).
struct AlignSpec {
    uint32_t band{64};                                                       // diagonals on either side of a gap's own: 0 .. 65535
    uint32_t maxGapLen{5000};                                                // 0 .. 65535: a gap with more read or text symbols leaves its chain out (status 1)
    uint64_t maxCells{uint64_t{1} << 24};                                    // 1 .. 2^30: so does a gap whose band holds more cells
};
struct ChainAlignments {
    std::vector<fmgpu_chain_alignment> alignments;                           // one per chain, in chain order
    std::vector<uint32_t>              ops;                                  // chain k's at [alignments[k].first_op, + alignments[k].n_ops)
    // the CIGAR string of chain k: with '=' and 'X', or (extended = false, for SAM) both folded into 'M'; "*" for a chain that was left out
    auto cigar(size_t k, bool extended = true) const -> std::string {
        auto const& r = alignments.at(k);
        if (r.n_ops == 0) return "*";
        std::string out;
        uint64_t run = 0; char last = 0;
        auto flush = [&]() { if (run) out += std::to_string(run) + last; run = 0; };
        for (uint64_t i = r.first_op; i < r.first_op + r.n_ops; ++i) {
            const uint32_t op = ops[i] & 15u;
            char c = op == FMGPU_OP_I ? 'I' : op == FMGPU_OP_D ? 'D' : op == FMGPU_OP_S ? 'S' : op == FMGPU_OP_EQ ? '=' : 'X';
            if (!extended && (c == '=' || c == 'X')) c = 'M';
            if (c != last) flush();
            last = c; run += ops[i] >> 4;
        }
        flush();
        return out;
    }
};
inline auto alignChains(SeedChains const& chains, std::vector<fmgpu_position> const& positions, std::vector<fmgpu_seed_span> const& spans,
                        std::vector<std::vector<uint8_t>> const& reads, std::vector<uint8_t> const& text, std::vector<uint64_t> const& textOffsets,
                        AlignSpec const& spec = {}) -> ChainAlignments {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(reads, buf, off);
    if (buf.empty()) buf.push_back(0);
    fmgpu_align_spec s{};
    s.nq = reads.size(); s.band = spec.band; s.max_gap_len = spec.maxGapLen; s.max_cells = spec.maxCells;
    ChainAlignments out;
    const uint64_t n = chains.chains.size();
    if (n && textOffsets.size() != n + 1) throw std::runtime_error("fmindex-collection (gpu): alignChains takes one text window per chain");
    out.alignments.resize(n);
    std::vector<uint8_t> none(1, 0);
    uint8_t const* t = text.empty() ? none.data() : text.data();
    auto call = [&](uint32_t* ops, uint64_t capacity, uint64_t* count) {
        return fmgpu_chains_align(chains.chains.data(), n, chains.anchors.data(), chains.anchors.size(), positions.data(), positions.size(), spans.data(), spans.size(),
                                  buf.data(), off.data(), t, textOffsets.data(), &s, out.alignments.data(), ops, capacity, count, nullptr);
    };
    uint64_t count = 0;
    detail::check(call(nullptr, 0, &count));                                 // the counting call sizes the operations exactly
    out.ops.resize(count);
    if (count) detail::check(call(out.ops.data(), count, &count));
    return out;
}
template <typename Index>
auto alignChains(Index const& index, SeedChains const& chains, std::vector<fmgpu_position> const& positions, std::vector<fmgpu_seed_span> const& spans,
                 std::vector<std::vector<uint8_t>> const& reads, AlignSpec const& spec = {}) -> ChainAlignments {
    std::vector<fmgpu_text_range> ranges;
    std::vector<uint64_t> offsets(1, 0);
    for (auto const& c : chains.chains) { ranges.push_back(fmgpu_text_range{c.seq_id, c.tbeg, c.tend - c.tbeg}); offsets.push_back(offsets.back() + (c.tend - c.tbeg)); }
    std::vector<uint8_t> text;
    if (!ranges.empty()) text = detail::extractWithTable(index, ranges);
    return alignChains(chains, positions, spans, reads, text, offsets, spec);
}

// Paired-end SAM (include/fmgpu.h: fmgpu_positions_sam_mates): fmc::formatSamMates(positionsA, readsA, positionsB, readsB, pairs, spec) is two alignment lines per
// fragment, line 2f for mate A and line 2f + 1 for mate B, with the mate fields filled in (flags 1, 2, 8, 32, 64, 128, RNEXT, PNEXT, TLEN), formatted on the device from
// the positions fmc::map returned for the two FORWARD batches and the pairs fmc::joinMates made of them (its result, or any array of pair records).  A fragment with
// pairs takes the one with the fewest errors, the first among equals, and is proper; elsewhere each mate takes its own primary record.  The overload without a second
// batch takes one interleaved batch whose reads 2f and 2f + 1 are the mates.  An ArrayView is a pointer and a count in host or device memory; a std::vector converts.
// readNames are the names of batch A; stripMateSuffix removes a trailing "/1" or "/2" from QNAME.  The counting call sizes the text, as in fmc::formatSam.
template <typename T>
struct ArrayView {
    T const* data{nullptr};
    size_t   size{0};
    ArrayView() = default;
    ArrayView(T const* d, size_t n) : data{n ? d : nullptr}, size{n} {}
    ArrayView(std::vector<T> const& v) : ArrayView{v.data(), v.size()} {}                     // NOLINT: a vector is a view of itself
};
struct SamMatesSpec {
    CharTable        charOf{CharTable::dna5()};
    Strands const*   strands{nullptr};
    NameTable const* readNames{nullptr};
    NameTable const* qualsA{nullptr};
    NameTable const* qualsB{nullptr};                                        // stays null for an interleaved batch
    NameTable const* seqNames{nullptr};
    bool    cigar{true};
    bool    stripMateSuffix{true};
    uint8_t mapqUnique{60}, mapqMulti{0};
};
namespace detail {
inline auto formatSamMates(ArrayView<fmgpu_position> a, ArrayView<fmgpu_position> b, ArrayView<fmgpu_mate_pair> pairs, std::vector<uint8_t> const& bufA,
                           std::vector<uint64_t> const& offA, std::vector<uint8_t> const* bufB, std::vector<uint64_t> const* offB, SamMatesSpec const& spec,
                           bool wantLineOffsets) -> SamText {
    size_t const reads = offA.size() - 1;
    if (bufB ? offB->size() != offA.size() : reads % 2 != 0) throw std::runtime_error("fmindex-collection (gpu): one read of each batch per fragment");
    fmgpu_sam_mates_spec s{};
    s.qbuf_a = bufA.data(); s.qoff_a = offA.data(); s.n_fragments = bufB ? reads : reads / 2; s.char_of = spec.charOf.map.data();
    if (bufB) { s.qbuf_b = bufB->data(); s.qoff_b = offB->data(); }
    if (s.n_fragments && !s.qbuf_a) s.qbuf_a = reinterpret_cast<uint8_t const*>(offA.data());        // (batches without a symbol: never read through)
    if (s.n_fragments && bufB && !s.qbuf_b) s.qbuf_b = reinterpret_cast<uint8_t const*>(offB->data());
    fmgpu_strands st{};
    fmgpu_name_table rt{}, qa{}, qb{}, nt{};
    if (spec.strands) { st = spec.strands->c(); s.strands = &st; }
    if (spec.readNames) { rt = spec.readNames->c(); s.read_names = &rt; }
    if (spec.qualsA) { qa = spec.qualsA->c(); s.quals_a = &qa; }
    if (spec.qualsB) { qb = spec.qualsB->c(); s.quals_b = &qb; }
    if (spec.seqNames) { nt = spec.seqNames->c(); s.seq_names = &nt; }
    s.interleaved = bufB ? 0 : 1; s.cigar = spec.cigar ? 1 : 0; s.strip_mate_suffix = spec.stripMateSuffix ? 1 : 0;
    s.mapq_unique = spec.mapqUnique; s.mapq_multi = spec.mapqMulti;
    uint64_t bytes = 0;
    detail::check(fmgpu_positions_sam_mates(a.data, a.size, b.data, b.size, pairs.data, pairs.size, &s, nullptr, 0, &bytes, nullptr, nullptr));      // the counting call sizes the text exactly
    SamText out;
    out.text.assign(bytes, '\0');
    if (wantLineOffsets) out.lineOffsets.assign(2 * s.n_fragments + 1, 0);
    if (bytes) detail::check(fmgpu_positions_sam_mates(a.data, a.size, b.data, b.size, pairs.data, pairs.size, &s, reinterpret_cast<uint8_t*>(out.text.data()), bytes, &bytes,
                                                       wantLineOffsets ? out.lineOffsets.data() : nullptr, nullptr));
    return out;
}
}  // namespace detail
template <typename QueriesA, typename QueriesB>
auto formatSamMates(ArrayView<fmgpu_position> positionsA, QueriesA const& readsA, ArrayView<fmgpu_position> positionsB, QueriesB const& readsB,
                    ArrayView<fmgpu_mate_pair> pairs, SamMatesSpec const& spec = {}, bool wantLineOffsets = false) -> SamText {
    std::vector<uint8_t> bufA, bufB; std::vector<uint64_t> offA, offB;
    detail::flatten(readsA, bufA, offA);
    detail::flatten(readsB, bufB, offB);
    return detail::formatSamMates(positionsA, positionsB, pairs, bufA, offA, &bufB, &offB, spec, wantLineOffsets);
}
template <typename QueriesA, typename QueriesB>
auto formatSamMates(ArrayView<fmgpu_position> positionsA, QueriesA const& readsA, ArrayView<fmgpu_position> positionsB, QueriesB const& readsB, MatePairs const& joined,
                    SamMatesSpec const& spec = {}, bool wantLineOffsets = false) -> SamText {
    return formatSamMates(positionsA, readsA, positionsB, readsB, ArrayView<fmgpu_mate_pair>{joined.pairs}, spec, wantLineOffsets);
}
template <typename Queries>
auto formatSamMates(ArrayView<fmgpu_position> positions, Queries const& interleavedReads, ArrayView<fmgpu_mate_pair> pairs, SamMatesSpec const& spec = {},
                    bool wantLineOffsets = false) -> SamText {
    std::vector<uint8_t> buf; std::vector<uint64_t> off;
    detail::flatten(interleavedReads, buf, off);
    return detail::formatSamMates(positions, {}, pairs, buf, off, nullptr, nullptr, spec, wantLineOffsets);
}
template <typename Queries>
auto formatSamMates(ArrayView<fmgpu_position> positions, Queries const& interleavedReads, MatePairs const& joined, SamMatesSpec const& spec = {},
                    bool wantLineOffsets = false) -> SamText {
    return formatSamMates(positions, interleavedReads, ArrayView<fmgpu_mate_pair>{joined.pairs}, spec, wantLineOffsets);
}

// A feed (include/fmgpu.h: fmgpu_feed_*): host batches searched chunk by chunk on one index, upload, search and download overlapped.  What a caller that holds its
// queries in host memory — the reference's Sequences — should search through: `fmc::Feed feed{index}; feed.search_no_errors(queries, delegate);`.  A Sequences object
// (reads of one-byte symbols, each contiguous) goes down through the `_v` calls without being flattened, a PackedQueries through `_q4`.  The delegates are called as by
// the free functions of the same names, which stay as they are.  One feed serves one call at a time; the index must outlive it.
template <typename Index>
struct Feed {
    fmgpu_feed_t handle{nullptr};
    Index const* index{nullptr};
    explicit Feed(Index const& idx, fmgpu_feed_config const& config = {}) : index{&idx} { detail::check(fmgpu_feed_create(idx.handle, &config, &handle)); }
    Feed(Feed const&) = delete;
    Feed& operator=(Feed const&) = delete;
    Feed(Feed&& o) noexcept : handle{o.handle}, index{o.index} { o.handle = nullptr; }
    ~Feed() { if (handle) fmgpu_feed_destroy(handle); }

    struct Info { uint64_t pinnedBytes, deviceBytes, lastChunks, lastStagedBytes, lastUploadedBytes; };
    auto info() const -> Info {
        Info i{};
        detail::check(fmgpu_feed_info(handle, &i.pinnedBytes, &i.deviceBytes, &i.lastChunks, &i.lastStagedBytes, &i.lastUploadedBytes));
        return i;
    }

    // search_no_errors::search(index, queries, delegate(qidx, cursor)): only non-empty cursors are reported
    template <typename Queries, typename Delegate>
    void search_no_errors(Queries const& queries, Delegate&& delegate) const {
        std::vector<uint8_t const*> reads; std::vector<uint64_t> lens;
        scattered(queries, reads, lens);
        size_t nq = reads.size();
        std::vector<uint64_t> lb(nq), len(nq);
        detail::check(fmgpu_feed_search_exact_v(handle, reads.data(), lens.data(), nq, lb.data(), len.data(), nullptr));
        reportExact(lb, len, delegate);
    }
    template <typename Delegate>
    void search_no_errors(PackedQueries const& queries, Delegate&& delegate) const {
        size_t nq = queries.size();
        std::vector<uint64_t> lb(nq), len(nq);
        detail::check(fmgpu_feed_search_exact_q4(handle, queries.packed.data(), queries.qoff.data(), nq, lb.data(), len.data(), nullptr));
        reportExact(lb, len, delegate);
    }
    // search_ng26::search<Edit>(index, queries, scheme, partition, delegate(qidx, cursor, errors), n)
    template <bool Edit = true, typename Queries, typename Delegate>
    void search_ng26(Queries const& queries, search_scheme::Scheme const& scheme, std::vector<size_t> const& partition, Delegate&& delegate,
                     size_t n = std::numeric_limits<size_t>::max()) const {
        std::vector<uint8_t const*> reads; std::vector<uint64_t> lens;
        scattered(queries, reads, lens);
        size_t nq = reads.size();
        if (scheme.empty() || nq == 0 || n == 0) return;
        size_t P = scheme[0].pi.size();
        std::vector<uint64_t> pi, l, u, part(partition.begin(), partition.end());
        for (auto const& s : scheme) {
            if (s.pi.size() != P) throw std::runtime_error("fmindex-collection (gpu): searches of a scheme must have the same number of parts");
            pi.insert(pi.end(), s.pi.begin(), s.pi.end()); l.insert(l.end(), s.l.begin(), s.l.end()); u.insert(u.end(), s.u.begin(), s.u.end());
        }
        fmgpu_scheme sc{static_cast<int32_t>(scheme.size()), static_cast<int32_t>(P), pi.data(), l.data(), u.data(), part.empty() ? nullptr : part.data(), Edit ? 1 : 0, 0};
        auto hits = detail::run_hits(nq, [&](fmgpu_hit* out, uint64_t cap, uint64_t* count) {
            return fmgpu_feed_search_scheme_v(handle, reads.data(), lens.data(), nq, &sc, n, out, cap, count, nullptr);
        });
        detail::report(*index, hits, delegate);
    }
    // (the scheme kernels read bytes: a packed batch is unpacked on the host first)
    template <bool Edit = true, typename Delegate>
    void search_ng26(PackedQueries const& queries, search_scheme::Scheme const& scheme, std::vector<size_t> const& partition, Delegate&& delegate,
                     size_t n = std::numeric_limits<size_t>::max()) const {
        search_ng26<Edit>(queries.unpack(), scheme, partition, std::forward<Delegate>(delegate), n);
    }
    // fmc::map chunk by chunk (fmgpu_feed_map_v): the same MapResult, the device-side hit and position buffers bounded by the chunk
    template <typename Queries>
    auto map(Queries const& queries, MapQuery const& query) const -> MapResult {
        std::vector<uint8_t const*> reads; std::vector<uint64_t> lens;
        scattered(queries, reads, lens);
        size_t nq = reads.size();
        detail::FlatMapQuery flat{query};
        return detail::run_map(nq, query.locate, [&](fmgpu_position* out, uint64_t cap, uint64_t* count, fmgpu_hit* hits, uint64_t hcap, uint64_t* hcount, uint8_t* stratum) {
            return fmgpu_feed_map_v(handle, reads.data(), lens.data(), nq, &flat.what, out, cap, count, hits, hcap, hcount, stratum, nullptr, nullptr);
        });
    }
    // both strands chunk by chunk (fmgpu_feed_map_strands; the batch is flattened: there is no `_v` form): what fmc::map(index, queries, query, strands) returns
    template <typename Queries>
    auto map(Queries const& queries, MapQuery const& query, Strands const& strands) const -> MapResult {
        std::vector<uint8_t> buf; std::vector<uint64_t> off;
        detail::flatten(queries, buf, off);
        size_t nq = off.size() - 1;
        detail::FlatMapQuery flat{query};
        fmgpu_strands st = strands.c();
        return detail::run_map(2 * nq, query.locate, [&](fmgpu_position* out, uint64_t cap, uint64_t* count, fmgpu_hit* hits, uint64_t hcap, uint64_t* hcount, uint8_t* stratum) {
            return fmgpu_feed_map_strands(handle, buf.data(), off.data(), nq, &flat.what, &st, out, cap, count, hits, hcap, hcount, stratum, nullptr, nullptr);
        });
    }
    // The bytes of a read file to positions (fmgpu_feed_map_text): what fmc::map(index, parseQueries(text, format, table), query) returns plus the name and quality
    // spans and the length of every read, without the batch ever visiting the host: the text travels in windows of chunkBytes (0 = 64 MiB), each parsed and mapped
    // on the device.  final = false: only the records the text proves complete; `consumed` tells where the next call starts.  A text error throws, naming the line.
    struct TextResult : MapResult {
        std::vector<fmgpu_text_span> names, quals;                    // spans into the text
        std::vector<uint64_t> lens;                                   // symbols of every read
        uint64_t symbols{0}, consumed{0}, foreign{0};
        auto size() const -> size_t { return lens.size(); }
        auto name(std::string_view text, size_t q) const -> std::string_view { return text.substr(names[q].offset, names[q].len); }
        auto quality(std::string_view text, size_t q) const -> std::string_view { return text.substr(quals[q].offset, quals[q].len); }
    };
#ifdef __cpp_lib_span
    auto mapText(std::span<uint8_t const> text, TextFormat format, SymbolTable const& table, MapQuery const& query, bool final = true, uint64_t chunkBytes = 0) const -> TextResult {
        return mapText(ByteView{text.data(), text.size()}, format, table, query, final, chunkBytes);
    }
#endif
    auto mapText(std::string_view text, TextFormat format, SymbolTable const& table, MapQuery const& query, bool final = true, uint64_t chunkBytes = 0) const -> TextResult {
        return mapText(ByteView{reinterpret_cast<uint8_t const*>(text.data()), text.size()}, format, table, query, final, chunkBytes);
    }
    struct ByteView {                                                 // (what std::span<uint8_t const> is from C++20 on: this header also serves C++17)
        uint8_t const* first; size_t count;
        auto data() const -> uint8_t const* { return first; }
        auto size() const -> size_t { return count; }
    };
    // both strands of every read of the file (fmgpu_feed_map_text_strands): stratum holds two entries per read, names / quals / lens stay per read of the file
    auto mapText(std::string_view text, TextFormat format, SymbolTable const& table, MapQuery const& query, Strands const& strands, bool final = true,
                 uint64_t chunkBytes = 0) const -> TextResult {
        return mapText(ByteView{reinterpret_cast<uint8_t const*>(text.data()), text.size()}, format, table, query, final, chunkBytes, &strands);
    }
    auto mapText(ByteView text, TextFormat format, SymbolTable const& table, MapQuery const& query, Strands const& strands, bool final = true,
                 uint64_t chunkBytes = 0) const -> TextResult {
        return mapText(text, format, table, query, final, chunkBytes, &strands);
    }
    auto mapText(ByteView text, TextFormat format, SymbolTable const& table, MapQuery const& query, bool final = true, uint64_t chunkBytes = 0,
                 Strands const* strands = nullptr) const -> TextResult {
        detail::FlatMapQuery flat{query};
        fmgpu_strands st = strands ? strands->c() : fmgpu_strands{};
        const uint64_t mult = strands ? 2 : 1;
        TextResult r;
        uint64_t rcap = std::max<uint64_t>(1024, text.size() / 64), cap = query.locate ? std::max<uint64_t>(4 * rcap, text.size() / 16) : 0;
        uint64_t hcap = std::max<uint64_t>(4 * rcap, text.size() / 16), count = 0, hcount = 0;
        fmgpu_parse_result res{};
        for (int round = 0; round < 2; ++round) {                     // the counts are exact also on FMGPU_ERR_CAPACITY, so a second call with them fits
            r.positions.resize(cap); r.hits.resize(hcap);
            r.stratum.assign(mult * rcap, 255); r.names.resize(rcap); r.quals.resize(rcap); r.lens.resize(rcap);
            int rc = strands ? fmgpu_feed_map_text_strands(handle, text.data(), text.size(), static_cast<int32_t>(format), final ? 1 : 0, table.map.data(), chunkBytes, &flat.what,
                                                           &st, r.positions.data(), cap, &count, r.hits.data(), hcap, &hcount, r.stratum.data(), r.names.data(), r.quals.data(),
                                                           r.lens.data(), rcap, &res, nullptr, nullptr)
                             : fmgpu_feed_map_text(handle, text.data(), text.size(), static_cast<int32_t>(format), final ? 1 : 0, table.map.data(), chunkBytes, &flat.what,
                                                   r.positions.data(), cap, &count, r.hits.data(), hcap, &hcount, r.stratum.data(), r.names.data(), r.quals.data(), r.lens.data(), rcap,
                                                   &res, nullptr, nullptr);
            if (rc == FMGPU_ERR_CAPACITY && round == 0) { cap = std::max(cap, count); hcap = std::max(hcap, hcount); rcap = std::max<uint64_t>(rcap, res.reads); continue; }
            detail::check(rc);
            break;
        }
        r.positions.resize(count); r.hits.resize(hcount);
        r.stratum.resize(mult * res.reads); r.names.resize(res.reads); r.quals.resize(res.reads); r.lens.resize(res.reads);
        r.symbols = res.symbols; r.consumed = res.consumed; r.foreign = res.foreign;
        return r;
    }

  private:
    template <typename Queries>
    static void scattered(Queries const& queries, std::vector<uint8_t const*>& reads, std::vector<uint64_t>& lens) {
        for (auto const& q : queries) {
            static_assert(sizeof(*q.data()) == 1, "a feed takes reads of one-byte symbols, each contiguous in memory");
            reads.push_back(reinterpret_cast<uint8_t const*>(q.data()));
            lens.push_back(q.size());
        }
    }
    template <typename Delegate>
    void reportExact(std::vector<uint64_t> const& lb, std::vector<uint64_t> const& len, Delegate&& delegate) const {
        using cursor_t = select_cursor_t<Index>;
        for (size_t q = 0; q < lb.size(); ++q) {
            if (len[q] == 0) continue;
            cursor_t cur{};
            cur.index = index; cur.lb = lb[q]; cur.len = len[q];
            delegate(q, cur);
        }
    }
};
template <typename Index> Feed(Index const&) -> Feed<Index>;
template <typename Index> Feed(Index const&, fmgpu_feed_config const&) -> Feed<Index>;

// Library options (include/fmgpu.h: fmgpu_option) — what a new handle is given, which of several result-identical kernels serves a call; the library reads no
// environment variable.  setOption(FMGPU_OPT_LF_TABLE, 0) before an index is made keeps it the plain configuration (occurrence tables + sampled suffix array).
inline void setOption(fmgpu_option option, int64_t value) { detail::check(fmgpu_set_option(static_cast<int32_t>(option), value)); }
inline auto getOption(fmgpu_option option) -> int64_t { int64_t v{}; detail::check(fmgpu_get_option(static_cast<int32_t>(option), &v)); return v; }

// One index file on several GPUs of this process (include/fmgpu.h: fmgpu_replicas_*): loadReplicas<Index>(file, {0, 1, 2, 3}) reads the file ONCE, onto the first
// listed device, and copies the handle to the others device to device (peerCopies() tells how many replicas were made that way; empty list: every visible device);
// searches cut the batch into contiguous ranges, one per replica, run them concurrently and report in batch order.
// `front()` is the first replica as an Index (locate and cursor steps go through it with its device current).
template <typename Index>
struct Replicas {
    fmgpu_replicas_t handle{nullptr};
    Index first{};
    Replicas() = default;
    Replicas(Replicas const&) = delete;
    Replicas& operator=(Replicas const&) = delete;
    Replicas(Replicas&& o) noexcept : handle{o.handle}, first{std::move(o.first)} { o.handle = nullptr; o.first.handle = nullptr; }
    ~Replicas() { first.handle = nullptr; if (handle) fmgpu_replicas_destroy(handle); }       // (the first replica's handle is borrowed from the set)
    auto size() const -> size_t { int32_t n{}; detail::check(fmgpu_replicas_info(handle, &n, nullptr, 0, nullptr)); return static_cast<size_t>(n); }
    auto front() const -> Index const& { return first; }
    auto peerCopies() const -> size_t { int32_t n{}; detail::check(fmgpu_replicas_peer_copies(handle, &n)); return static_cast<size_t>(n); }
    // search_no_errors::search over the replicas: delegate(qidx, cursor) for every non-empty cursor, in batch order
    template <typename Queries, typename Delegate>
    void searchNoErrors(Queries const& queries, Delegate&& delegate) const {
        std::vector<uint8_t> buf; std::vector<uint64_t> off;
        detail::flatten(queries, buf, off);
        size_t nq = off.size() - 1;
        std::vector<uint64_t> lb(nq), len(nq);
        detail::check(fmgpu_replicas_search_exact(handle, buf.data(), off.data(), nq, lb.data(), len.data(), nullptr));
        using cursor_t = select_cursor_t<Index>;
        for (size_t q = 0; q < nq; ++q) {
            if (len[q] == 0) continue;
            cursor_t cur{};
            cur.index = &first; cur.lb = lb[q]; cur.len = len[q];
            delegate(q, cur);
        }
    }
};
template <typename Index>
auto loadReplicas(std::string const& fileName, std::vector<int32_t> const& devices = {}) -> Replicas<Index> {
    Replicas<Index> r;
    detail::check(fmgpu_replicas_load(fileName.c_str(), devices.empty() ? nullptr : devices.data(), static_cast<int32_t>(devices.size()), &r.handle));
    detail::check(fmgpu_replicas_info(r.handle, nullptr, nullptr, 0, &r.first.handle));
    int32_t sigma{}, bidir{};
    detail::check(fmgpu_index_info(r.first.handle, &r.first.n, &sigma, nullptr, &bidir, nullptr));
    if (static_cast<size_t>(sigma) != Index::Sigma || (bidir != 0) != Index::IsBidirectional)
        throw std::runtime_error("loadReplicas: " + fileName + " holds an index of Sigma " + std::to_string(sigma) + (bidir ? " (BiFMIndex)" : " (FMIndex)"));
    return r;
}

}  // namespace fmc
