// The best-hit ladders of include/fmc_gpu.hpp on one fmgpu_search_best* call each: the reference's fixture ladders (search/checkSearches.cpp "search ng21, all
// search_best" / "all search_best_n", as in test_fmc_gpu.cpp) through the Sequences overloads and through the PackedQueries overloads, with the same located
// results; then a larger batch, bytes against packed.  Exit 77 without a device (everything here needs one).
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cstdio>
#include <random>
#include <tuple>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;
using Results = std::vector<std::tuple<size_t, size_t, size_t>>;

int main() {
    namespace ss = fmc::search_scheme;
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return 77; }

    {   // the fixture with A, B, C = 1, 2, 3 (a packed batch needs sigma <= 15; the located positions do not depend on the symbols' names)
        uint8_t const A = 1, B = 2, C = 3;
        auto input = Reads{{A, A, A, C, A, A, A, B, A, A, A}, {A, A, A, B, A, A, A, C, A, A, A}};
        auto queries = Reads{{C, C}, {B, B}};
        auto packed = fmc::PackedQueries::pack(queries, 5);
        fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{input, /*samplingRate*/ 1, /*threadNbr*/ 1};
        auto results = Results{};
        auto locate_all = [&](auto qidx, auto cursor, auto errors) {
            (void)errors;
            for (auto [sid, spos, offset] : fmc::LocateLinear{index, cursor}) results.emplace_back(qidx, sid, spos + offset);
        };
        auto sorted = [&]() { auto r = results; std::sort(r.begin(), r.end()); results.clear(); return r; };
        auto ex = [&](size_t minK, size_t maxK) { return ss::expand(ss::generator::pigeon_opt(minK, maxK), queries[0].size()); };
        auto all8 = Results{{0, 0, 3}, {0, 0, 3}, {0, 1, 7}, {0, 1, 7}, {1, 0, 7}, {1, 0, 7}, {1, 1, 3}, {1, 1, 3}};
        auto top3 = Results{{0, 0, 3}, {0, 1, 7}, {0, 1, 7}, {1, 0, 7}, {1, 0, 7}, {1, 1, 3}};
        fmc::search_ng21::search_best(index, queries, std::vector{ex(0, 0), ex(1, 1), ex(2, 2)}, locate_all);
        CHECK(sorted() == all8);
        fmc::search_ng21::search_best(index, packed, std::vector{ex(0, 0), ex(1, 1), ex(2, 2)}, locate_all);
        CHECK(sorted() == all8);
        fmc::search_ng21::search_best_n(index, queries, std::vector{ex(0, 0), ex(1, 1)}, 3, locate_all);
        CHECK(sorted() == top3);
        fmc::search_ng21::search_best_n(index, packed, std::vector{ex(0, 0), ex(1, 1)}, 3, locate_all);
        CHECK(sorted() == top3);
        // search_ng26::search_best with the explicit list: the same ladder un-expanded (Hamming distance: the fixture's substitutions)
        auto ladder = std::vector<std::tuple<ss::Scheme, std::vector<size_t>>>{};
        for (size_t k = 0; k < 2; ++k) ladder.emplace_back(ss::generator::pigeon_opt(k, k), ss::createUniformPartition(ss::generator::pigeon_opt(k, k), queries[0].size()));
        auto expected = Results{{0, 0, 2}, {0, 0, 3}, {0, 1, 6}, {0, 1, 7}, {1, 0, 6}, {1, 0, 7}, {1, 1, 2}, {1, 1, 3}};     // checkSearches.cpp:14-72, one substitution
        fmc::search_ng26::search_best<false>(index, queries, ladder, locate_all);
        CHECK(sorted() == expected);
        fmc::search_ng26::search_best<false>(index, packed, ladder, locate_all);
        CHECK(sorted() == expected);
        fmc::search_ng26::search_best<false>(index, packed, ladder, locate_all, 0);      // n = 0: nothing is reported (SearchNg26.h:408-409)
        CHECK(results.empty());
    }

    // a larger batch: reads of a random text with 0 .. 2 substitutions, some with a foreign symbol, one empty — bytes against packed, record for record
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
    auto const packed = fmc::PackedQueries::packOnDevice(reads, 5);
    auto const bytes = packed.unpack();
    using Row = std::tuple<size_t, uint64_t, uint64_t, size_t>;
    std::vector<Row> a, b;
    auto into = [](std::vector<Row>& v) { return [&v](size_t q, auto const& c, size_t e) { v.emplace_back(q, c.lb, c.len, e); }; };
    auto ladder = std::vector<std::tuple<ss::Scheme, std::vector<size_t>>>{};
    for (size_t k = 0; k < 3; ++k) ladder.emplace_back(ss::generator::h2(k + 2, 0, k), std::vector<size_t>{});
    for (size_t n : {std::numeric_limits<size_t>::max(), size_t{2}}) {
        a.clear(); b.clear();
        fmc::search_ng26::search_best<true>(index, bytes, ladder, into(a), n);
        fmc::search_ng26::search_best<true>(index, packed, ladder, into(b), n);
        CHECK(a.size() > reads.size() / 2 && a == b);
        size_t errors[3] = {0, 0, 0};
        for (auto const& r : a) if (std::get<3>(r) < 3) ++errors[std::get<3>(r)];
        CHECK(errors[0] > 0 && errors[1] > 0 && errors[2] > 0);                        // every stratum of the ladder reported
    }
    auto ex = [&](size_t k) { return ss::expand(ss::generator::pigeon_opt(k, k), 32); };
    a.clear(); b.clear();
    fmc::search_ng21::search_best(index, bytes, std::vector{ex(0), ex(1), ex(2)}, into(a));
    fmc::search_ng21::search_best(index, packed, std::vector{ex(0), ex(1), ex(2)}, into(b));
    CHECK(a.size() > reads.size() / 2 && a == b);
    a.clear(); b.clear();
    fmc::search_ng21::search_best_n(index, bytes, std::vector{ex(0), ex(1), ex(2)}, 2, into(a));
    fmc::search_ng21::search_best_n(index, packed, std::vector{ex(0), ex(1), ex(2)}, 2, into(b));
    CHECK(!a.empty() && a == b);

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
