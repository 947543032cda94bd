// fmc::map and fmc::Feed::map (include/fmc_gpu.hpp: one fmgpu_map / fmgpu_feed_map_v call each) against the reports of fmc::Search: on the reference's fixture text
// (search/checkSearches.cpp, as in test_fmc_gpu.cpp) and on a larger batch, for exact search, Hamming and edit distance, with and without maxResults; then the
// best-stratum ladder against search_ng26::search_best located cursor by cursor.  Exit 77 without a device (everything here needs one).
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cstdio>
#include <random>
#include <tuple>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;
using Report = std::vector<std::tuple<size_t, size_t, size_t, size_t>>;      // qidx, seqId, pos, errors

template <typename Index>
static Report viaSearch(Index const& index, Reads const& reads, bool edit, size_t errors, std::optional<size_t> maxResults) {
    Report out;
    auto rep = [&](size_t qidx, size_t sid, size_t pos, size_t e) { out.emplace_back(qidx, sid, pos, e); };
    fmc::Search{index, reads, edit, errors, maxResults, rep}();
    return out;
}
static Report reportOf(fmc::MapResult const& r) {
    Report out;
    for (auto const& p : r.positions) {
        out.emplace_back(p.qidx, p.seq_id, p.pos, p.errors);
        CHECK(p.hit < r.hits.size() && r.hits[p.hit].qidx == p.qidx);
    }
    return out;
}

int main() {
    namespace ss = fmc::search_scheme;
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return 77; }

    {   // the fixture: reads of 2 symbols, which fmc::Search searches with h2(errors + 1, 0, errors)
        uint8_t const A = 1, B = 2, C = 3;
        auto input = Reads{{A, A, A, C, A, A, A, B, A, A, A}, {A, A, A, B, A, A, A, C, A, A, A}};
        auto queries = Reads{{C, C}, {B, B}};
        fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{input, /*samplingRate*/ 1, /*threadNbr*/ 1};
        fmc::Feed feed{index, fmgpu_feed_config{1, 0, 0, 0, 0, 0}};                     // one read per chunk
        for (bool edit : {true, false}) {
            auto want = viaSearch(index, queries, edit, 1, {});
            CHECK(want.size() == 8);
            auto q = fmc::MapQuery::search(1, edit, {}, 2);
            CHECK(reportOf(fmc::map(index, queries, q)) == want);
            CHECK(reportOf(feed.map(queries, q)) == want);
            CHECK(reportOf(fmc::map(index, fmc::PackedQueries::pack(queries, 5), q)) == want);
            auto want3 = viaSearch(index, queries, edit, 1, 3);
            CHECK(want3.size() == 6);
            auto q3 = fmc::MapQuery::search(1, edit, 3, 2);
            CHECK(reportOf(fmc::map(index, queries, q3)) == want3);
            CHECK(reportOf(feed.map(queries, q3)) == want3);
        }
        auto r = fmc::map(index, queries, fmc::MapQuery::search(0));                     // no occurrence of CC / BB
        CHECK(r.positions.empty() && r.hits.empty() && r.stratum == std::vector<uint8_t>({255, 255}));
        CHECK(viaSearch(index, queries, true, 0, {}).empty());
    }

    // a larger batch: reads of 32 symbols of a random text with 0 .. 3 substitutions, some with a foreign symbol, one empty
    std::mt19937 rng(11);
    Reads text(2);
    for (auto& t : text) { t.resize(1500); for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4); }
    fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{text, 4, 1};
    Reads reads;
    for (size_t i = 0; i < 150; ++i) {
        size_t const at = rng() % (1500 - 32);
        Reads::value_type r(text[i % 2].begin() + at, text[i % 2].begin() + at + 32);
        for (size_t e = 0; e < i % 4; ++e) r[rng() % 32] = static_cast<uint8_t>(1 + rng() % 4);
        if (i % 29 == 0) r[rng() % 32] = 9;
        reads.push_back(r);
    }
    reads.push_back({});
    fmc::Feed feed{index, fmgpu_feed_config{16, 0, 3, 0, 0, 0}};
    for (bool edit : {true, false}) {
        for (size_t errors : {size_t{0}, size_t{1}, size_t{2}}) {
            for (std::optional<size_t> maxResults : {std::optional<size_t>{}, std::optional<size_t>{2}}) {
                auto want = viaSearch(index, reads, edit, errors, maxResults);
                // (the documented deviation of fmgpu_hits_from_intervals: search_no_errors reports the empty read's cursor, the whole index; fmgpu_map leaves it out)
                if (errors == 0 && !maxResults)
                    want.erase(std::remove_if(want.begin(), want.end(), [&](auto const& t) { return std::get<0>(t) == reads.size() - 1; }), want.end());
                CHECK(errors < 2 || want.size() > reads.size() / 2);
                auto q = fmc::MapQuery::search(errors, edit, maxResults);
                CHECK(reportOf(fmc::map(index, reads, q)) == want);
                CHECK(reportOf(feed.map(reads, q)) == want);
                q.firstRecords = 1;                                                    // the library's scratch grows: the same reports
                CHECK(reportOf(fmc::map(index, reads, q)) == want);
            }
        }
    }
    {   // the best-stratum ladder: fmc::map against search_ng26::search_best located cursor by cursor (same order: callback order, rows ascending)
        auto ladder = std::vector<std::tuple<ss::Scheme, std::vector<size_t>>>{};
        for (size_t k = 0; k < 3; ++k) ladder.emplace_back(ss::generator::h2(k + 2, 0, k), std::vector<size_t>{});
        Report want;
        fmc::search_ng26::search_best<false>(index, reads, ladder, [&](size_t qidx, auto const& cursor, size_t e) {
            for (auto [sid, spos, offset] : fmc::LocateLinear{index, cursor}) want.emplace_back(qidx, sid, spos + offset, e);
        });
        auto r = fmc::map(index, reads, fmc::MapQuery::ladder(2, false));
        CHECK(!want.empty() && reportOf(r) == want);
        CHECK(reportOf(feed.map(reads, fmc::MapQuery::ladder(2, false))) == want);
        size_t per[4] = {0, 0, 0, 0};
        for (auto s : r.stratum) ++per[s == 255 ? 3 : s];
        CHECK(per[0] > 0 && per[1] > 0 && per[2] > 0 && per[3] > 0 && r.stratum.size() == reads.size());
        auto q = fmc::MapQuery::ladder(2, false);
        q.locate = false;
        auto h = fmc::map(index, reads, q);
        CHECK(h.positions.empty() && h.hits.size() == r.hits.size());
    }

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
