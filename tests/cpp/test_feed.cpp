// fmc::Feed (include/fmc_gpu.hpp) against the free functions of the mirror: search_no_errors and search_ng26 over a Sequences object (through the `_v` calls, not
// flattened) and over a PackedQueries, for several chunkings — the same callbacks in the same order.  Exit 77 without a device (the host checks have run by then).
#include "../../include/fmc_gpu.hpp"

#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;
using Row = std::tuple<size_t, uint64_t, uint64_t, size_t>;

int main() {
    {   // the planner needs no device
        uint64_t const qoff[5] = {1, 4, 4, 9, 30};
        uint64_t first[5] = {}, chunks = 0;
        CHECK(fmgpu_feed_plan(qoff, 4, 2, 10, first, 4, &chunks) == 0 && chunks == 3 && first[0] == 0 && first[1] == 2 && first[2] == 3 && first[3] == 4);
        CHECK(fmgpu_feed_plan(qoff, 4, 0, 10, first, 4, &chunks) == FMGPU_ERR_INVALID);
        fmgpu_feed_t f = nullptr;
        CHECK(fmgpu_feed_create(nullptr, nullptr, &f) == FMGPU_ERR_INVALID && f == nullptr);
    }
    if (failures) return 1;
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("host checks passed; no device\n"); return 77; }

    std::mt19937 rng(7);
    Reads text(3);
    for (auto& t : text) { t.resize(1500); for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4); }
    fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{text, 4, 1};
    Reads reads;
    for (size_t i = 0; i < 90; ++i) {
        size_t const m = i % 11 == 0 ? 0 : 20 + i % 45, at = rng() % (1500 - m);
        Reads::value_type r(text[i % 3].begin() + at, text[i % 3].begin() + at + m);
        if (m && i % 5 == 0) r[rng() % m] = static_cast<uint8_t>(1 + rng() % 4);
        if (m && i % 17 == 0) r[rng() % m] = 9;
        reads.push_back(r);
    }
    auto const packed = fmc::PackedQueries::pack(reads, 5);
    auto const scheme = fmc::search_scheme::generator::h2(3, 0, 1);

    std::vector<Row> exact, hamming, edit, two;
    fmc::search_no_errors::search(index, reads, [&](size_t q, auto const& c) { exact.emplace_back(q, c.lb, c.len, 0); });
    fmc::search_ng26::search<false>(index, reads, scheme, {}, [&](size_t q, auto const& c, size_t e) { hamming.emplace_back(q, c.lb, c.len, e); });
    fmc::search_ng26::search<true>(index, reads, scheme, {}, [&](size_t q, auto const& c, size_t e) { edit.emplace_back(q, c.lb, c.len, e); });
    fmc::search_ng26::search<true>(index, reads, scheme, {}, [&](size_t q, auto const& c, size_t e) { two.emplace_back(q, c.lb, c.len, e); }, 2);
    CHECK(exact.size() > 20 && hamming.size() > exact.size() && edit.size() > hamming.size() && two.size() < edit.size());

    for (uint64_t chunkReads : {uint64_t{1}, uint64_t{7}, uint64_t{0}}) {
        fmgpu_feed_config cfg{};
        cfg.chunk_reads = chunkReads;
        cfg.pack4 = chunkReads == 7;
        fmc::Feed feed{index, cfg};
        std::vector<Row> got;
        feed.search_no_errors(reads, [&](size_t q, auto const& c) { got.emplace_back(q, c.lb, c.len, 0); });
        CHECK(got == exact);
        CHECK(feed.info().lastChunks == (chunkReads ? (reads.size() + chunkReads - 1) / chunkReads : 1));
        got.clear();
        feed.search_no_errors(packed, [&](size_t q, auto const& c) { got.emplace_back(q, c.lb, c.len, 0); });
        CHECK(got == exact);
        got.clear();
        feed.search_ng26<false>(reads, scheme, {}, [&](size_t q, auto const& c, size_t e) { got.emplace_back(q, c.lb, c.len, e); });
        CHECK(got == hamming);
        got.clear();
        feed.search_ng26<true>(reads, scheme, {}, [&](size_t q, auto const& c, size_t e) { got.emplace_back(q, c.lb, c.len, e); });
        CHECK(got == edit);
        got.clear();
        feed.search_ng26<true>(packed.unpack(), scheme, {}, [&](size_t q, auto const& c, size_t e) { got.emplace_back(q, c.lb, c.len, e); }, 2);
        CHECK(got == two);
        got.clear();
        feed.search_no_errors(Reads{}, [&](size_t q, auto const& c) { got.emplace_back(q, c.lb, c.len, 0); });
        CHECK(got.empty());
    }
    fmc::Feed plain{index};                                       // (deduced, default configuration)
    CHECK(plain.info().deviceBytes == 0);

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
