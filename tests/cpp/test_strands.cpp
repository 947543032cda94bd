// Both strands through include/fmc_gpu.hpp: fmc::bothStrands and the hand-over of fmc::Strands on the host (checked everywhere), then on a device
// fmc::map(index, reads, query, strands), fmc::Feed::map(reads, query, strands) and fmc::Feed::mapText(text, ..., strands) against fmc::map on bothStrands(reads), and
// the pair ladder against search_ng26::search_best_pairs located cursor by cursor.  Exit 77 without a device, after the host checks.
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <tuple>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;
using Report = std::vector<std::tuple<size_t, size_t, size_t, size_t>>;      // qidx, seqId, pos, errors

static Report reportOf(fmc::MapResult const& r) {
    Report out;
    for (auto const& p : r.positions) {
        out.emplace_back(p.qidx, p.seq_id, p.pos, p.errors);
        CHECK(p.hit < r.hits.size() && r.hits[p.hit].qidx == p.qidx);
    }
    return out;
}
static bool sameResult(fmc::MapResult const& a, fmc::MapResult const& b) {
    if (a.stratum != b.stratum || a.hits.size() != b.hits.size() || a.positions.size() != b.positions.size()) return false;
    for (size_t i = 0; i < a.hits.size(); ++i) if (std::memcmp(&a.hits[i], &b.hits[i], sizeof(fmgpu_hit)) != 0) return false;
    for (size_t i = 0; i < a.positions.size(); ++i) if (std::memcmp(&a.positions[i], &b.positions[i], sizeof(fmgpu_position)) != 0) return false;
    return true;
}

int main() {
    namespace ss = fmc::search_scheme;

    {   // the host mirror: no device needed
        static_assert(sizeof(fmgpu_strands) == 16, "fmgpu_strands is 16 bytes");
        auto st = fmc::Strands::dna5(true);
        fmgpu_strands c = st.c();
        CHECK(c.complement == st.complement.data() && c.n == 5 && c.pair == 1);
        CHECK(fmc::Strands::dna5().c().pair == 0 && (st.complement == std::vector<uint8_t>{0, 4, 3, 2, 1}));
        auto both = fmc::bothStrands(Reads{{1, 2, 2, 4, 5, 255, 0}, {}, {3}}, st.complement);
        CHECK((both == Reads{{1, 2, 2, 4, 5, 255, 0}, {0, 255, 5, 1, 3, 3, 4}, {}, {}, {3}, {2}}));
        CHECK((fmc::bothStrands(Reads{{0, 1, 2}}, std::vector<uint8_t>{7}) == Reads{{0, 1, 2}, {2, 1, 7}}));
        CHECK(fmc::bothStrands(Reads{}, st.complement).empty());
        // the argument checks of the C calls that come before the device
        fmgpu_map_query what{};
        uint64_t cnt = 7, one[2] = {0, 0};
        uint8_t byte = 0;
        CHECK(fmgpu_map_strands(nullptr, &byte, one, 1, &what, nullptr, nullptr, 0, &cnt, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID);
        fmgpu_strands bad = st.c();
        bad.pair = 2;
        CHECK(fmgpu_map_strands(nullptr, &byte, one, 1, &what, &bad, nullptr, 0, &cnt, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID);
        CHECK(fmgpu_map_strands(nullptr, nullptr, nullptr, 0, &what, &c, nullptr, 0, &cnt, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == 0 && cnt == 0);
        CHECK(fmgpu_queries_strands(&byte, one, uint64_t{1} << 30, st.complement.data(), 5, &byte, one, nullptr) == FMGPU_ERR_UNSUPPORTED);
    }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return failures ? 1 : 77; }

    // reads of 32 symbols of a random text with 0 .. 3 substitutions, every other one reverse-complemented, some with a foreign symbol, one empty
    std::mt19937 rng(13);
    Reads text(2);
    for (auto& t : text) { t.resize(1500); for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4); }
    fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{text, 4, 1};
    auto const dna = fmc::Strands::dna5().complement;
    Reads reads;
    for (size_t i = 0; i < 120; ++i) {
        size_t const at = rng() % (1500 - 32);
        Reads::value_type r(text[i % 2].begin() + at, text[i % 2].begin() + at + 32);
        for (size_t e = 0; e < i % 4; ++e) r[rng() % 32] = static_cast<uint8_t>(1 + rng() % 4);
        if (i % 29 == 0) r[rng() % 32] = 9;
        if (i % 2) r = fmc::bothStrands(Reads{r}, dna)[1];
        reads.push_back(r);
    }
    reads.push_back({});
    auto const doubled = fmc::bothStrands(reads, dna);
    fmc::Feed feed{index, fmgpu_feed_config{16, 0, 3, 0, 0, 0}};

    for (auto const& q : {fmc::MapQuery::search(0), fmc::MapQuery::ladder(2, false), fmc::MapQuery::ladder(1, true)}) {
        auto want = fmc::map(index, doubled, q);                                           // pair = false: fmc::map on the host-doubled batch
        CHECK(!want.positions.empty() && want.stratum.size() == 2 * reads.size());
        CHECK(sameResult(fmc::map(index, reads, q, fmc::Strands::dna5(false)), want));
        CHECK(sameResult(feed.map(reads, q, fmc::Strands::dna5(false)), want));
    }
    {   // pair = true: search_ng26::search_best_pairs on the host-doubled batch, located cursor by cursor
        auto ladder = std::vector<std::tuple<ss::Scheme, std::vector<size_t>>>{};
        for (size_t k = 0; k < 3; ++k) ladder.emplace_back(ss::generator::h2(k + 2, 0, k), std::vector<size_t>{});
        Report want, independent;
        fmc::search_ng26::search_best_pairs<false>(index, doubled, ladder, [&](size_t qidx, auto const& cursor, size_t e) {
            for (auto [sid, spos, offset] : fmc::LocateLinear{index, cursor}) want.emplace_back(qidx, sid, spos + offset, e);
        });
        fmc::search_ng26::search_best<false>(index, doubled, ladder, [&](size_t qidx, auto const& cursor, size_t e) {
            for (auto [sid, spos, offset] : fmc::LocateLinear{index, cursor}) independent.emplace_back(qidx, sid, spos + offset, e);
        });
        auto r = fmc::map(index, reads, fmc::MapQuery::ladder(2, false), fmc::Strands::dna5(true));
        CHECK(!want.empty() && reportOf(r) == want && want.size() <= independent.size());
        CHECK(sameResult(feed.map(reads, fmc::MapQuery::ladder(2, false), fmc::Strands::dna5(true)), r));
        for (size_t q = 0; q < reads.size(); ++q) CHECK(r.stratum[2 * q] == r.stratum[2 * q + 1]);

        // the same reads as a FASTA file through Feed::mapText
        std::string fasta;
        for (size_t i = 0; i < reads.size(); ++i) {
            fasta += ">r" + std::to_string(i) + "\n";
            for (auto c : reads[i]) fasta += c >= 1 && c <= 4 ? "ACGT"[c - 1] : 'N';
            fasta += "\n";
        }
        auto table = fmc::SymbolTable::dna5();
        auto parsed = fmc::parseQueries(fasta, fmc::TextFormat::Fasta, table);
        for (bool pair : {false, true}) {
            auto wantText = fmc::map(index, parsed, fmc::MapQuery::ladder(2, false), fmc::Strands::dna5(pair));
            auto t = feed.mapText(fasta, fmc::TextFormat::Fasta, table, fmc::MapQuery::ladder(2, false), fmc::Strands::dna5(pair), true, 257);
            CHECK(t.size() == reads.size() && t.stratum.size() == 2 * reads.size() && sameResult(t, wantText));
            CHECK(feed.info().lastUploadedBytes == fasta.size());
            CHECK(t.name(fasta, 5) == "r5" && t.lens[5] == 32);
        }
        auto plain = feed.mapText(fasta, fmc::TextFormat::Fasta, table, fmc::MapQuery::ladder(2, false), true, 257);       // the feed still serves the plain call
        CHECK(plain.stratum.size() == reads.size() && sameResult(plain, fmc::map(index, parsed, fmc::MapQuery::ladder(2, false))));
    }

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
