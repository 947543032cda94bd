// index.locateHits and fmc::Search (search/search.h:48-75) on top of fmgpu_locate_hits, against the per-cursor LocateLinear loop (locate.h:14-57) that
// fmc::Search stood for.  Linked with -Wl,--wrap=fmgpu_locate,--wrap=fmgpu_locate_hits: the wrappers count the ABI calls, so that a batch is seen to be
// located by ONE call.  `test_locate_hits time <reads>` prints the wall time of fmc::Search against the per-cursor loop instead of checking.
// Needs a GPU; exit code 0 = all checks passed, 77 = no GPU (host-only compile check).
#include "../../include/fmc_gpu.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <optional>
#include <random>
#include <string>
#include <tuple>
#include <vector>

extern "C" {
int __real_fmgpu_locate(fmgpu_index_t h, const uint64_t* rows, uint64_t count, uint64_t* out_seq, uint64_t* out_pos, uint64_t* out_steps, fmgpu_stats* stats, void* stream);
int __real_fmgpu_locate_hits(fmgpu_index_t h, const fmgpu_hit* hits, uint64_t count, fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                             fmgpu_stats* stats, void* stream);
static size_t g_locate_calls = 0, g_locate_hits_calls = 0;
int __wrap_fmgpu_locate(fmgpu_index_t h, const uint64_t* rows, uint64_t count, uint64_t* out_seq, uint64_t* out_pos, uint64_t* out_steps, fmgpu_stats* stats, void* stream) {
    ++g_locate_calls;
    return __real_fmgpu_locate(h, rows, count, out_seq, out_pos, out_steps, stats, stream);
}
int __wrap_fmgpu_locate_hits(fmgpu_index_t h, const fmgpu_hit* hits, uint64_t count, fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                             fmgpu_stats* stats, void* stream) {
    ++g_locate_hits_calls;
    return __real_fmgpu_locate_hits(h, hits, count, out, capacity, out_count, stats, stream);
}
}

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

using Report = std::vector<std::tuple<size_t, size_t, size_t, size_t>>;
using Index = fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16>;

static std::vector<std::vector<uint8_t>> makeText(size_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<uint8_t> t(n);
    for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4);
    for (size_t copy = 1; copy <= 5; ++copy)                                  // a five-copy repeat: cursors of several rows
        std::copy(t.begin(), t.begin() + n / 20, t.begin() + copy * (n / 6));
    return {t};
}
static std::vector<std::vector<uint8_t>> makeReads(std::vector<uint8_t> const& t, size_t count, size_t len, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<std::vector<uint8_t>> reads;
    for (size_t i = 0; i < count; ++i) {
        size_t p = rng() % (t.size() - len);
        std::vector<uint8_t> q(t.begin() + p, t.begin() + p + len);
        for (size_t s = rng() % 3; s > 0; --s) q[rng() % len] = static_cast<uint8_t>(1 + rng() % 4);
        reads.push_back(q);
    }
    return reads;
}
// what fmc::Search reported before it located through fmgpu_locate_hits: one LocateLinear per reported cursor
template <typename Queries>
static Report perCursor(Index const& index, Queries const& reads, bool edit, size_t errors, std::optional<size_t> maxResults) {
    Report out;
    auto report = [&](size_t qidx, auto const& cursor, size_t e) {
        for (auto [sid, spos, offset] : fmc::LocateLinear{index, cursor}) out.emplace_back(qidx, sid, spos + offset, e);
    };
    if (maxResults) { if (edit) fmc::search_n<true>(index, reads, errors, *maxResults, report); else fmc::search_n<false>(index, reads, errors, *maxResults, report); }
    else { if (edit) fmc::search<true>(index, reads, errors, report); else fmc::search<false>(index, reads, errors, report); }
    return out;
}
template <typename Queries>
static Report viaSearch(Index const& index, Queries const& reads, bool edit, size_t errors, std::optional<size_t> maxResults) {
    Report out;
    auto rep = [&](size_t qidx, size_t sid, size_t pos, size_t e) { out.emplace_back(qidx, sid, pos, e); };
    fmc::Search{index, reads, edit, errors, maxResults, rep}();
    return out;
}

int main(int argc, char** argv) {
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("No GPU: compiled only\n"); return 77; }
    auto const text = makeText(200'000, 7);
    auto const index = Index{text, 16, 1};
    if (argc > 2 && std::string(argv[1]) == "time") {
        auto const reads = makeReads(text[0], std::stoul(argv[2]), 101, 3);
        for (int edit = 0; edit < 2; ++edit) {
            auto t0 = std::chrono::steady_clock::now();
            auto a = perCursor(index, reads, edit, 2, std::nullopt);
            auto t1 = std::chrono::steady_clock::now();
            g_locate_calls = g_locate_hits_calls = 0;
            auto b = viaSearch(index, reads, edit, 2, std::nullopt);
            auto t2 = std::chrono::steady_clock::now();
            std::printf("%s k=2, %zu reads, %zu positions: per-cursor loop %.3f s, fmc::Search %.3f s (%zu fmgpu_locate_hits calls, %zu fmgpu_locate calls), same=%d\n",
                        edit ? "edit" : "hamming", reads.size(), b.size(), std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count(),
                        g_locate_hits_calls, g_locate_calls, int(a == b));
        }
        return 0;
    }
    {   // index.locateHits equals the LocateLinear loop, record for record
        auto const reads = makeReads(text[0], 400, 30, 11);
        std::vector<fmgpu_hit> hits;
        Report loop;
        fmc::search<true>(index, reads, 2, [&](size_t qidx, auto const& cursor, size_t e) {
            fmgpu_hit h{}; h.qidx = qidx; h.lb = cursor.lb; h.len = cursor.len; h.errors = static_cast<uint32_t>(e);
            hits.push_back(h);
            for (auto [sid, spos, offset] : fmc::LocateLinear{index, cursor}) loop.emplace_back(qidx, sid, spos + offset, e);
        });
        auto const pos = index.locateHits(hits);
        CHECK(pos.size() == loop.size()); CHECK(loop.size() > hits.size());
        for (size_t i = 0; i < pos.size() && i < loop.size(); ++i) {
            CHECK(std::get<0>(loop[i]) == pos[i].qidx); CHECK(std::get<1>(loop[i]) == pos[i].seq_id);
            CHECK(std::get<2>(loop[i]) == pos[i].pos); CHECK(std::get<3>(loop[i]) == pos[i].errors);
            CHECK(hits[pos[i].hit].qidx == pos[i].qidx);
        }
        CHECK(index.locateHits({}).empty());
    }
    {   // fmc::Search equals the loop: Hamming and edit distance, with and without maxResults
        auto const reads = makeReads(text[0], 600, 40, 5);
        for (int edit = 0; edit < 2; ++edit)
            for (size_t errors : {size_t{0}, size_t{1}, size_t{2}})
                for (auto maxResults : {std::optional<size_t>{}, std::optional<size_t>{3}}) {
                    auto const want = perCursor(index, reads, edit, errors, maxResults);
                    auto const got = viaSearch(index, reads, edit, errors, maxResults);
                    CHECK(!want.empty()); CHECK(got == want);
                    if (got != want) {
                        size_t i = 0;
                        while (i < got.size() && i < want.size() && got[i] == want[i]) ++i;
                        std::printf("edit %d errors %zu maxResults %d: %zu vs %zu records, first difference at %zu", edit, errors, int(bool(maxResults)), got.size(), want.size(), i);
                        if (i < got.size() && i < want.size())
                            std::printf(": got (%zu %zu %zu %zu) want (%zu %zu %zu %zu)", std::get<0>(got[i]), std::get<1>(got[i]), std::get<2>(got[i]), std::get<3>(got[i]),
                                        std::get<0>(want[i]), std::get<1>(want[i]), std::get<2>(want[i]), std::get<3>(want[i]));
                        std::printf("\n");
                    }
                }
    }
    {   // a batch of 10 000 reads: ONE fmgpu_locate_hits call, no fmgpu_locate call
        auto const reads = makeReads(text[0], 10'000, 101, 9);
        g_locate_calls = g_locate_hits_calls = 0;
        auto const got = viaSearch(index, reads, true, 2, std::nullopt);
        CHECK(g_locate_hits_calls == 1); CHECK(g_locate_calls == 0); CHECK(got.size() >= reads.size());
        g_locate_calls = g_locate_hits_calls = 0;
        auto const want = perCursor(index, reads, true, 2, std::nullopt);
        CHECK(g_locate_calls > 1000); CHECK(got == want);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
