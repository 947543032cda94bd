// fmc::search_hamming_sm (include/fmc_gpu.hpp) on top of fmgpu_search_hamming_sm: the masks of ScoringMatrix (checked on the host), then on a small BiFMIndex<21> the
// reference test's matrix against a brute-force scorer over the sequences, the identity matrix against search_ng26::search<false>, and the IUPAC helper on a BiFMIndex<5>.
// Needs a GPU for the searches; exit code 0 = all checks passed, 77 = no GPU (the mask checks passed, the rest was compiled only).
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cstdio>
#include <map>
#include <random>
#include <tuple>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

using Seq = std::vector<uint8_t>;
namespace sm = fmc::search_hamming_sm;

static uint32_t bits(std::initializer_list<int> ranks) { uint32_t m = 0; for (int r : ranks) m |= 1u << r; return m; }

static auto referenceTestMatrix() {
    auto m = sm::ScoringMatrix<28, 21>{};       // (the seven calls of the reference's test)
    m.setCost(21,  5, 0); m.setCost(22, 13, 0); m.setCost(23,  4, 0); m.setCost(24,  7, 0);
    m.setCost(25, 12, 0); m.setCost(26, 17, 0); m.setCost(27, 19, 0);
    return m;
}

static void checkMasks() {
    auto d = sm::ScoringMatrix<5>{};
    CHECK((d.freeMask == std::array<uint32_t, 5>{0, 2, 4, 8, 16}));
    CHECK((d.costMask == std::array<uint32_t, 5>{0, 0b11100, 0b11010, 0b10110, 0b01110}));
    auto m = referenceTestMatrix();
    uint32_t every = 0;
    for (int r = 1; r < 21; ++r) every |= 1u << r;
    int const extra[7] = {5, 13, 4, 7, 12, 17, 19};
    CHECK(m.freeMask[0] == 0 && m.costMask[0] == 0);
    for (size_t q = 1; q < 21; ++q) CHECK(m.freeMask[q] == 1u << q && m.costMask[q] == (every & ~(1u << q)));
    for (size_t k = 0; k < 7; ++k) CHECK(m.freeMask[21 + k] == 1u << extra[k] && m.costMask[21 + k] == (every & ~(1u << extra[k])));
    auto raw = m.raw();
    CHECK(raw.query_sigma == 28 && raw.reserved == 0 && raw.free_mask == m.freeMask.data() && raw.cost_mask == m.costMask.data());
    auto i = sm::iupacDna();
    CHECK(i.freeMask[5] == bits({1, 3}) && i.costMask[5] == bits({2, 4}));            // R = A | G
    CHECK(i.freeMask[11] == bits({2, 3, 4}) && i.costMask[11] == bits({1}));          // B = not A
    CHECK(i.freeMask[15] == bits({1, 2, 3, 4}) && i.costMask[15] == 0);               // N
    CHECK(i.freeMask[3] == bits({3}) && i.costMask[3] == bits({1, 2, 4}) && i.freeMask[0] == 0 && i.costMask[0] == 0);
    bool threw = false;
    try { i.setCost(16, 1, 0); } catch (std::runtime_error const&) { threw = true; }
    CHECK(threw);
}

// rows per (qidx, errors): every window of a sequence that the masks pair with the read at <= maxErrors errors (no mask pairs the delimiter: no window spans two sequences);
// a read shorter than the scheme has parts reports nothing
template <typename SM>
static auto brute(std::vector<Seq> const& seqs, std::vector<Seq> const& reads, SM const& m, size_t maxErrors, size_t parts) {
    std::map<std::pair<size_t, size_t>, size_t> out;
    for (size_t q = 0; q < reads.size(); ++q) {
        auto const& r = reads[q];
        if (r.size() < parts) continue;
        for (auto const& s : seqs)
            for (size_t at = 0; at + r.size() <= s.size(); ++at) {
                size_t e = 0;
                for (size_t j = 0; j < r.size() && e <= maxErrors; ++j) {
                    uint32_t f = r[j] < m.freeMask.size() ? m.freeMask[r[j]] : 0, c = r[j] < m.costMask.size() ? m.costMask[r[j]] : 0;
                    if ((f >> s[at + j]) & 1u) continue;
                    e += ((c >> s[at + j]) & 1u) ? 1 : maxErrors + 1;
                }
                if (e <= maxErrors) ++out[{q, e}];
            }
    }
    return out;
}

template <typename Index, typename SM>
static void checkAgainstBrute(Index const& index, std::vector<Seq> const& seqs, std::vector<Seq> const& reads, SM const& m, size_t K) {
    // one search, so no occurrence is reported twice: the rows per (qidx, errors) are the brute force's
    std::map<std::pair<size_t, size_t>, size_t> got;
    size_t lastQ = 0, calls = 0;
    sm::search(index, reads, fmc::search_scheme::generator::backtracking(K + 1, 0, K), m, [&](size_t qidx, auto cursor, size_t e) {
        CHECK(qidx >= lastQ && cursor.count() > 0 && e <= K);       // ascending qidx: the reference's callback order
        lastQ = qidx; ++calls;
        got[{qidx, e}] += cursor.count();
    });
    auto const want = brute(seqs, reads, m, K, K + 1);
    CHECK(got == want);
    if (got != want) {
        std::printf("  %zu (qidx, errors) pairs reported, %zu expected\n", got.size(), want.size());
        for (auto const& [key, rows] : want) if (!got.count(key) || got.at(key) != rows) { std::printf("  first difference: qidx %zu errors %zu: %zu rows reported, %zu expected\n", key.first, key.second, got.count(key) ? got.at(key) : 0, rows); break; }
    }
    CHECK(calls >= reads.size() / 3);
    // a scheme of several searches finds the same (qidx, errors) pairs
    std::map<std::pair<size_t, size_t>, size_t> viaH2;
    sm::search(index, reads, fmc::search_scheme::generator::h2(K + 2, 0, K), m, [&](size_t qidx, auto cursor, size_t e) { viaH2[{qidx, e}] += cursor.count(); });
    CHECK(viaH2.size() == got.size());
    for (auto const& [key, rows] : got) CHECK(viaH2.count(key) && viaH2[key] >= rows);
    // n = 1: one row per query that has any
    std::map<size_t, size_t> perQuery, limited;
    for (auto const& [key, rows] : got) perQuery[key.first] += rows;
    sm::search(index, reads, fmc::search_scheme::generator::h2(K + 2, 0, K), m, [&](size_t qidx, auto cursor, size_t) { limited[qidx] += cursor.count(); }, 1);
    CHECK(limited.size() == perQuery.size());
    for (auto const& [q, rows] : limited) CHECK(rows == 1);
    sm::search(index, std::vector<Seq>{}, fmc::search_scheme::generator::h2(K + 2, 0, K), m, [&](size_t, auto, size_t) { CHECK(false); });
}

int main() {
    checkMasks();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("No GPU: compiled only\n"); return 77; }
    auto makeSeqs = [](size_t sigma, uint32_t seed) {
        std::mt19937 rng(seed);
        std::vector<Seq> seqs;
        for (size_t len : {900, 140, 200}) {
            Seq s(len);
            for (size_t i = 0; i < len; ++i) s[i] = seqs.size() == 1 ? static_cast<uint8_t>(1 + (i * i + 3 * i) % 7 % (sigma - 1)) : static_cast<uint8_t>(1 + rng() % (sigma - 1));
            seqs.push_back(s);
        }
        return seqs;
    };
    auto makeReads = [](std::vector<Seq> const& seqs, size_t sigma, uint32_t seed) {
        std::mt19937 rng(seed);
        std::vector<Seq> reads;
        for (size_t k = 0; k < 30; ++k) {
            auto const& s = seqs[k % seqs.size()];
            size_t len = 12 + rng() % 20, at = rng() % (s.size() - len);
            Seq r(s.begin() + at, s.begin() + at + len);
            for (size_t mu = k % 3; mu > 0; --mu) r[rng() % len] = static_cast<uint8_t>(1 + rng() % (sigma - 1));
            reads.push_back(r);
        }
        reads.push_back({});
        reads.push_back({1});
        return reads;
    };
    {   // the reference test's matrix on BiFMIndex<21>: codes 21 .. 27 stand for one residue each
        auto const seqs = makeSeqs(21, 3);
        auto index = fmc::BiFMIndex<21, fmc::string::InterleavedBitvector16>{seqs, 4, 1};
        auto reads = makeReads(seqs, 21, 1);
        auto const m = referenceTestMatrix();
        std::map<uint8_t, uint8_t> codeOf;
        for (size_t q = 21; q < 28; ++q) for (size_t r = 1; r < 21; ++r) if ((m.freeMask[q] >> r) & 1u) codeOf[static_cast<uint8_t>(r)] = static_cast<uint8_t>(q);
        size_t recoded = 0;
        for (auto& r : reads) for (auto& c : r) if (codeOf.count(c) && (++recoded % 2)) c = codeOf[c];
        CHECK(recoded > 20);
        reads[4][3] = 28; reads[7][0] = 255;                         // bytes without a row pair with nothing
        checkAgainstBrute(index, seqs, reads, m, 1);
        // the identity matrix is search_ng26::search<false>: the same delegate calls
        auto plain = makeReads(seqs, 21, 2);
        auto scheme = fmc::search_scheme::generator::pigeon_opt(0, 1);
        using Call = std::tuple<size_t, size_t, size_t, size_t>;
        std::vector<Call> a, b;
        sm::search(index, plain, scheme, sm::ScoringMatrix<21>{}, [&](size_t q, auto cur, size_t e) { a.emplace_back(q, cur.lb, cur.len, e); });
        fmc::search_ng26::search<false>(index, plain, scheme, {}, [&](size_t q, auto cur, size_t e) { b.emplace_back(q, cur.lb, cur.len, e); });
        std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
        CHECK(a == b && a.size() >= 10);
    }
    {   // the IUPAC helper on BiFMIndex<5>
        auto const seqs = makeSeqs(5, 5);
        auto index = fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16>{seqs, 4, 1};
        auto reads = makeReads(seqs, 5, 6);
        auto const m = sm::iupacDna();
        std::mt19937 rng(9);
        for (auto& r : reads) {
            if (r.size() < 8) continue;
            r[rng() % r.size()] = 15;                                // N
            size_t p = rng() % r.size();
            if (r[p] == 1 || r[p] == 3) r[p] = 5;                    // R where the read holds A or G
            if (rng() % 4 == 0) r[rng() % r.size()] = static_cast<uint8_t>(5 + rng() % 11);
        }
        checkAgainstBrute(index, seqs, reads, m, 2);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
