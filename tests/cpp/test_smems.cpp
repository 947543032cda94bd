// fmc::search_smems on top of fmgpu_search_smems (include/fmc_gpu.hpp), against a loop of std::search over the sequences the index was built from.
// Needs a GPU; exit code 0 = all checks passed, 77 = no GPU (host-only compile check).
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

using Seq = std::vector<uint8_t>;
using Seed = std::tuple<size_t, size_t, size_t, size_t>;           // qidx, qbeg, qlen, rows

// occurrences of read[beg, end) in the sequences (a sequence holds no delimiter: no match spans two of them)
static size_t occurrences(std::vector<Seq> const& seqs, Seq const& read, size_t beg, size_t end) {
    size_t n = 0;
    for (auto const& s : seqs)
        for (auto it = s.begin(); (it = std::search(it, s.end(), read.begin() + beg, read.begin() + end)) != s.end(); ++it) ++n;
    return n;
}

// the SMEMs of every read from the definition: L[e] = the longest break-free match ending at e; an SMEM ends where the next end's match is no longer
static std::vector<Seed> brute(std::vector<Seq> const& seqs, std::vector<Seq> const& reads, size_t sigma, size_t minLen, size_t maxRows) {
    std::vector<Seed> out;
    for (size_t q = 0; q < reads.size(); ++q) {
        auto const& r = reads[q];
        std::vector<size_t> L(r.size(), 0);
        for (size_t e = 0; e < r.size(); ++e)
            for (size_t l = 1; l <= e + 1; ++l) {
                uint8_t c = r[e + 1 - l];
                if (c < 1 || c >= sigma || occurrences(seqs, r, e + 1 - l, e + 1) == 0) break;
                L[e] = l;
            }
        for (size_t e = 0; e < r.size(); ++e) {
            if (L[e] == 0 || (e + 1 < r.size() && L[e + 1] > L[e])) continue;
            size_t rows = occurrences(seqs, r, e + 1 - L[e], e + 1);
            if (L[e] >= std::max<size_t>(minLen, 1) && (maxRows == 0 || rows <= maxRows)) out.emplace_back(q, e + 1 - L[e], L[e], rows);
        }
    }
    return out;
}

template <typename Index>
static void check(Index const& index, std::vector<Seq> const& seqs, size_t sigma, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<Seq> reads;
    for (size_t k = 0; k < 40; ++k) {                               // windows of the text with a few substitutions, breaks in every fourth read
        auto const& s = seqs[k % seqs.size()];
        size_t len = 1 + rng() % 90, at = rng() % (s.size() - len);
        Seq r(s.begin() + at, s.begin() + at + len);
        for (size_t m = rng() % 3; m > 0; --m) r[rng() % len] = static_cast<uint8_t>(1 + rng() % (sigma - 1));
        if (k % 4 == 3) r[rng() % len] = k % 8 == 3 ? 0 : static_cast<uint8_t>(sigma);
        reads.push_back(r);
    }
    reads.push_back({});
    reads.push_back(seqs[2]);
    for (auto [minLen, maxRows] : {std::pair<size_t, size_t>{1, 0}, {6, 0}, {1, 2}}) {
        std::vector<Seed> got;
        fmc::search_smems(index, reads, minLen, maxRows, [&](size_t qidx, auto cursor, size_t qbeg, size_t qlen) { got.emplace_back(qidx, qbeg, qlen, cursor.count()); });
        CHECK(got == brute(seqs, reads, sigma, minLen, maxRows));
        CHECK(!got.empty());
        if (sigma <= 15) {
            std::vector<Seed> packed;
            fmc::search_smems(index, fmc::PackedQueries::pack(reads, sigma), minLen, maxRows,
                              [&](size_t qidx, auto cursor, size_t qbeg, size_t qlen) { packed.emplace_back(qidx, qbeg, qlen, cursor.count()); });
            CHECK(packed == got);
        }
    }
    // the cursor of a seed is the cursor of an exact search for it
    std::vector<Seq> parts; std::vector<std::pair<size_t, size_t>> cursors;
    fmc::search_smems(index, reads, 1, 0, [&](size_t qidx, auto cursor, size_t qbeg, size_t qlen) {
        parts.emplace_back(reads[qidx].begin() + qbeg, reads[qidx].begin() + qbeg + qlen);
        cursors.emplace_back(cursor.lb, cursor.len);
    });
    size_t seen = 0;
    fmc::search_no_errors::search(index, parts, [&](size_t q, auto cursor) { CHECK(cursors[q] == std::make_pair(size_t(cursor.lb), size_t(cursor.len))); ++seen; });
    CHECK(seen == parts.size());
    fmc::search_smems(index, std::vector<Seq>{}, 1, 0, [&](size_t, auto, size_t, size_t) { CHECK(false); });
}

int main() {
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("No GPU: compiled only\n"); return 77; }
    auto makeSeqs = [](size_t sigma, uint32_t seed) {
        std::mt19937 rng(seed);
        std::vector<Seq> seqs;
        for (size_t len : {300, 120, 200}) {
            Seq s(len);
            for (size_t i = 0; i < len; ++i) s[i] = seqs.size() == 1 ? static_cast<uint8_t>(1 + i % 3) : static_cast<uint8_t>(1 + rng() % (sigma - 1));   // (the second one: a tandem repeat)
            seqs.push_back(s);
        }
        return seqs;
    };
    {
        auto const seqs = makeSeqs(5, 3);
        auto index = fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16>{seqs, 16, 1};
        check(index, seqs, 5, 1);
    }
    {
        auto const seqs = makeSeqs(21, 4);
        auto index = fmc::FMIndex<21, fmc::string::Wavelet>{seqs, 4, 1};
        check(index, seqs, 21, 2);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
