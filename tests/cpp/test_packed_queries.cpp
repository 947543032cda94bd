// fmc::PackedQueries (include/fmc_gpu.hpp): the host packer against the format's literal, the device packer against the host packer, and the search overloads
// that take a packed batch against the same searches on the Sequences.  Exit 77 without a device (the host checks have run by then).
#include "../../include/fmc_gpu.hpp"

#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;

int main() {
    {   // the format, as include/fmgpu.h states it
        auto pq = fmc::PackedQueries::pack(Reads{{1, 2, 3}, {4, 0}}, 5);
        CHECK((pq.packed == std::vector<uint8_t>{0x21, 0x43, 0x00}));
        CHECK((pq.qoff == std::vector<uint64_t>{0, 3, 5}) && pq.size() == 2);
        pq = fmc::PackedQueries::pack(Reads{{9, 1, 255}}, 5);
        CHECK((pq.packed == std::vector<uint8_t>{0x1f, 0x0f}));
        pq = fmc::PackedQueries::pack(Reads{{1, 2, 3}, {}, {4, 9}}, 5, {0, 4, 3, 2, 1});
        auto both = fmc::PackedQueries::pack(Reads{{1, 2, 3}, {2, 3, 4}, {}, {}, {4, 9}, {255, 1}}, 5);
        CHECK(pq.packed == both.packed && pq.qoff == both.qoff);
        CHECK((pq.unpack() == Reads{{1, 2, 3}, {2, 3, 4}, {}, {}, {4, 255}, {255, 1}}));
        bool threw = false;
        try { (void)fmc::PackedQueries::pack(Reads{{1}}, 16); } catch (std::exception const&) { threw = true; }
        CHECK(threw);
    }
    if (failures) return 1;
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("host checks passed; no device\n"); return 77; }

    std::mt19937 rng(7);
    Reads text(3);
    for (auto& t : text) { t.resize(1500); for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4); }
    fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{text, 4, 1};
    Reads reads;
    for (size_t i = 0; i < 120; ++i) {
        size_t const m = i % 3 == 0 ? 33 : 32 + i % 2, at = rng() % (1500 - m);
        Reads::value_type r(text[i % 3].begin() + at, text[i % 3].begin() + at + m);
        r.resize(32);
        if (i % 5 == 0) r[rng() % 32] = static_cast<uint8_t>(1 + rng() % 4);
        if (i % 17 == 0) r[rng() % 32] = 9;
        reads.push_back(r);
    }
    std::vector<uint8_t> const comp{0, 4, 3, 2, 1};
    auto const host = fmc::PackedQueries::pack(reads, 5, comp), dev = fmc::PackedQueries::packOnDevice(reads, 5, comp);
    CHECK(host.packed == dev.packed && host.qoff == dev.qoff);
    auto const bytes = host.unpack();

    using Row = std::tuple<size_t, uint64_t, uint64_t, size_t>;
    std::vector<Row> a, b;
    fmc::search_no_errors::search(index, bytes, [&](size_t q, auto const& c) { a.emplace_back(q, c.lb, c.len, 0); });
    fmc::search_no_errors::search(index, dev, [&](size_t q, auto const& c) { b.emplace_back(q, c.lb, c.len, 0); });
    CHECK(!a.empty() && a == b);
    a.clear(); b.clear();
    auto const scheme = fmc::search_scheme::generator::h2(3, 0, 1);
    fmc::search_ng26::search<false>(index, bytes, scheme, {}, [&](size_t q, auto const& c, size_t e) { a.emplace_back(q, c.lb, c.len, e); });
    fmc::search_ng26::search<false>(index, dev, scheme, {}, [&](size_t q, auto const& c, size_t e) { b.emplace_back(q, c.lb, c.len, e); });
    CHECK(a.size() > reads.size() / 2 && a == b);
    a.clear(); b.clear();
    fmc::search<true>(index, bytes, 1, [&](size_t q, auto const& c, size_t e) { a.emplace_back(q, c.lb, c.len, e); });
    fmc::search<true>(index, dev, 1, [&](size_t q, auto const& c, size_t e) { b.emplace_back(q, c.lb, c.len, e); });
    CHECK(!a.empty() && a == b);
    a.clear(); b.clear();
    auto const expanded = fmc::search_scheme::expand(fmc::search_scheme::generator::pigeon_opt(0, 1), 32);
    fmc::search_ng21::search(index, bytes, expanded, [&](size_t q, auto const& c, size_t e) { a.emplace_back(q, c.lb, c.len, e); });
    fmc::search_ng21::search(index, dev, expanded, [&](size_t q, auto const& c, size_t e) { b.emplace_back(q, c.lb, c.len, e); });
    CHECK(!a.empty() && a == b);
    a.clear(); b.clear();
    fmc::search_ng21::search_n(index, bytes, expanded, 2, [&](size_t q, auto const& c, size_t e) { a.emplace_back(q, c.lb, c.len, e); });
    fmc::search_ng21::search_n(index, dev, expanded, 2, [&](size_t q, auto const& c, size_t e) { b.emplace_back(q, c.lb, c.len, e); });
    CHECK(!a.empty() && a == b);

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
