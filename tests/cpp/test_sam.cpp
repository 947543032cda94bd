// SAM records through include/fmc_gpu.hpp: the mirror struct, fmc::CharTable and fmc::samHeader on the host (checked everywhere, with the argument checks of
// fmgpu_positions_sam that come before the device), then on a device fmc::formatSam against a snprintf loop: both strands, ties for the primary record, unmapped
// reads, names and qualities from strings and from the spans of a parse.  Exit 77 without a device, after the host checks.
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;

static std::string upToBlank(std::string const& n) {
    auto const s = n.substr(0, std::min(n.find(' '), n.find('\t')));
    return s.empty() ? "*" : s;
}

// the same contract with snprintf: what a caller's own loop would write
static std::string hostSam(std::vector<fmgpu_position> const& positions, Reads const& reads, fmc::SamSpec const& spec, std::vector<std::string> const* readNames,
                           std::vector<std::string> const* quals, std::vector<std::string> const* seqNames, std::vector<uint64_t>* offsets = nullptr) {
    unsigned const shift = spec.strands ? 1 : 0;
    std::string out;
    char buf[128];
    size_t i = 0;
    if (offsets) offsets->assign(1, 0);
    for (size_t r = 0; r < reads.size(); ++r) {
        size_t const first = i;
        while (i < positions.size() && (positions[i].qidx >> shift) == r) ++i;
        size_t const m = reads[r].size();
        std::string const qname = readNames ? upToBlank((*readNames)[r]) : std::to_string(r);
        auto seqOf = [&](bool reverse) {
            std::string s;
            for (size_t j = 0; j < m; ++j) {
                uint8_t c = reads[r][reverse ? m - 1 - j : j];
                if (reverse && c < spec.strands->complement.size()) c = spec.strands->complement[c];
                s += static_cast<char>(spec.charOf.map[c]);
            }
            return s;
        };
        auto qualOf = [&](bool reverse, std::string const& seq) {
            if (!quals || (*quals)[r].empty() || seq == "*") return std::string{"*"};
            std::string q = (*quals)[r];
            if (reverse) std::reverse(q.begin(), q.end());
            return q;
        };
        if (first == i) {
            if (spec.emitUnmapped) {
                std::string const seq = m ? seqOf(false) : "*";
                out += qname + "\t4\t*\t0\t0\t*\t*\t0\t0\t" + seq + "\t" + qualOf(false, seq) + "\n";
                if (offsets) offsets->push_back(out.size());
            }
            continue;
        }
        uint32_t least = UINT32_MAX;
        size_t primary = first, atLeast = 0;
        for (size_t k = first; k < i; ++k) if (positions[k].errors < least) { least = positions[k].errors; primary = k; }
        for (size_t k = first; k < i; ++k) atLeast += positions[k].errors == least;
        for (size_t k = first; k < i; ++k) {
            auto const& p = positions[k];
            bool const reverse = shift && (p.qidx & 1), secondary = k != primary;
            std::string const seq = m == 0 || (secondary && !spec.secondarySeq) ? "*" : seqOf(reverse);
            std::string const rname = seqNames ? upToBlank((*seqNames)[p.seq_id]) : std::to_string(p.seq_id);
            std::string const cigar = spec.cigar && m ? std::to_string(m) + "M" : "*";
            unsigned const mapq = !secondary && atLeast == 1 ? spec.mapqUnique : spec.mapqMulti;
            std::snprintf(buf, sizeof buf, "\t%u\t", (reverse ? 16u : 0u) | (secondary ? 256u : 0u));
            out += qname + buf + rname;
            std::snprintf(buf, sizeof buf, "\t%" PRIu64 "\t%u\t", p.pos + 1, mapq);
            out += buf + cigar + "\t*\t0\t0\t" + seq + "\t" + qualOf(reverse, seq);
            std::snprintf(buf, sizeof buf, "\tNM:i:%u\tNH:i:%zu\n", p.errors, i - first);
            out += buf;
            if (offsets) offsets->push_back(out.size());
        }
    }
    return out;
}

int main() {
    {   // the host mirror: no device needed
        static_assert(sizeof(fmgpu_sam_spec) == 72, "the size include/fmgpu.h states");
        static_assert(offsetof(fmgpu_sam_spec, qoff) == 8 && offsetof(fmgpu_sam_spec, nq) == 16 && offsetof(fmgpu_sam_spec, char_of) == 24 && offsetof(fmgpu_sam_spec, strands) == 32 &&
                      offsetof(fmgpu_sam_spec, read_names) == 40 && offsetof(fmgpu_sam_spec, quals) == 48 && offsetof(fmgpu_sam_spec, seq_names) == 56 &&
                      offsetof(fmgpu_sam_spec, cigar) == 64 && offsetof(fmgpu_sam_spec, mapq_multi) == 68 && offsetof(fmgpu_sam_spec, reserved) == 69, "field offsets");
        fmc::SamSpec spec;
        CHECK(spec.cigar && spec.emitUnmapped && !spec.secondarySeq && spec.mapqUnique == 60 && spec.mapqMulti == 0 && !spec.strands && !spec.readNames && !spec.quals && !spec.seqNames);
        auto const chars = fmc::CharTable::dna5();
        auto const symbols = fmc::SymbolTable::dna5();
        for (char c : std::string{"$ACGT"}) CHECK(chars.map[symbols.map[static_cast<unsigned char>(c)]] == static_cast<uint8_t>(c));
        CHECK(chars.map[255] == 'N' && chars.map[7] == 'N');
        // the header: host code
        fmc::NameTable const names{std::vector<std::string>{"chr1 homo sapiens", "chrM\tx"}};
        CHECK(fmc::samHeader(names, {248956422, 16569}, "prog") == "@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:248956422\n@SQ\tSN:chrM\tLN:16569\n@PG\tID:prog\n");
        CHECK(fmc::samHeader(fmc::NameTable{}, {}) == "@HD\tVN:1.6\tSO:unknown\n");
        bool threw = false;
        try { (void)fmc::samHeader(fmc::NameTable{std::vector<std::string>{"a", " b"}}, {1, 2}); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "sequence 1 has an empty name") != nullptr; }
        CHECK(threw);
        // no line: no text, behind the checks
        CHECK(fmc::formatSam({}, Reads{}).text.empty());
        fmc::SamSpec quiet; quiet.emitUnmapped = false;
        auto const none = fmc::formatSam({}, Reads{{1, 2}, {3}}, quiet, true);
        CHECK(none.text.empty() && none.lineOffsets == std::vector<uint64_t>{0});
        // the argument checks that come before the device
        std::vector<fmgpu_position> one(1);
        uint8_t const q[2] = {1, 2};
        uint64_t const off[2] = {0, 2};
        uint64_t bytes = 7;
        fmgpu_sam_spec s{};
        CHECK(fmgpu_positions_sam(one.data(), 1, nullptr, nullptr, 0, &bytes, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "spec is null"));
        CHECK(fmgpu_positions_sam(one.data(), 1, &s, nullptr, 0, &bytes, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "char_of is null"));
        s.char_of = chars.map.data(); s.nq = 1;
        CHECK(fmgpu_positions_sam(one.data(), 1, &s, nullptr, 0, &bytes, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "qbuf is null"));
        s.qbuf = q; s.qoff = off;
        CHECK(fmgpu_positions_sam(nullptr, 1, &s, nullptr, 0, &bytes, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "positions is null"));
        s.cigar = 2;
        CHECK(fmgpu_positions_sam(one.data(), 1, &s, nullptr, 0, &bytes, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "cigar"));
        s.cigar = 1; s.reserved[2] = 1;
        CHECK(fmgpu_positions_sam(one.data(), 1, &s, nullptr, 0, &bytes, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "reserved"));
    }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return failures ? 1 : 77; }

    std::mt19937_64 rng(29);
    std::vector<std::string> const seqNames{"chr1", "chr2 assembled", "", "chrM"};
    Reads reads;
    std::vector<std::string> readNames, quals;
    std::vector<fmgpu_position> positions;
    for (size_t r = 0; r < 600; ++r) {
        size_t const m = r % 37 == 0 ? 0 : r == 300 ? 20000 : 1 + rng() % 150;
        auto& read = reads.emplace_back(m);
        for (auto& c : read) c = rng() % 50 == 0 ? 255 : static_cast<uint8_t>(1 + rng() % 4);
        readNames.push_back(r % 13 == 0 ? "" : "read" + std::to_string(r) + (r % 2 ? " 1:N:0" : ""));
        std::string q(r % 7 == 0 ? 0 : m, '!');
        for (auto& c : q) c = static_cast<char>(33 + rng() % 94);
        quals.push_back(q);
        size_t const records = r % 5 == 0 ? 0 : r == 301 ? 700 : 1 + rng() % 3;
        for (size_t k = 0; k < records; ++k) {
            fmgpu_position p{};
            p.qidx = 2 * r + rng() % 2; p.seq_id = rng() % seqNames.size(); p.pos = rng() >> (rng() % 64); p.errors = static_cast<uint32_t>(rng() % 3);
            p.hit = static_cast<uint32_t>(positions.size());
            positions.push_back(p);
        }
    }
    fmc::NameTable const rt{readNames}, qt{quals}, nt{seqNames};
    auto const strands = fmc::Strands::dna5(true);
    for (int variant = 0; variant < 4; ++variant) {
        fmc::SamSpec spec;
        spec.strands = &strands;
        if (variant != 1) { spec.readNames = &rt; spec.quals = &qt; spec.seqNames = &nt; }
        spec.secondarySeq = variant >= 2; spec.cigar = variant != 3; spec.emitUnmapped = variant != 3; spec.mapqUnique = 40 + variant; spec.mapqMulti = variant;
        std::vector<uint64_t> offsets;
        auto const want = hostSam(positions, reads, spec, spec.readNames ? &readNames : nullptr, spec.quals ? &quals : nullptr, spec.seqNames ? &seqNames : nullptr, &offsets);
        auto const got = fmc::formatSam(positions, reads, spec, true);
        CHECK(got.text == want);
        CHECK(got.lineOffsets == offsets);
    }
    {   // without strands: qidx is the read; all reads unmapped
        std::vector<fmgpu_position> plain(positions.begin(), positions.begin() + 200);
        for (auto& p : plain) p.qidx >>= 1;
        fmc::SamSpec spec;
        spec.readNames = &rt;
        CHECK(fmc::formatSam(plain, reads, spec).text == hostSam(plain, reads, spec, &readNames, nullptr, nullptr));
        CHECK(fmc::formatSam({}, reads, spec).text == hostSam({}, reads, spec, &readNames, nullptr, nullptr));
    }
    {   // names and qualities as the spans of a parse: the text is the tables' bytes
        std::string fastq;
        std::vector<std::string> names, qs;
        for (size_t i = 0; i < 10; ++i) {
            names.push_back("q" + std::to_string(i) + " extra");
            qs.push_back(std::string{"IJKLMNOP"}.substr(0, 4 + i % 5));
            fastq += "@" + names.back() + "\n" + std::string{"ACGTNACG"}.substr(0, 4 + i % 5) + "\n+\n" + qs.back() + "\n";
        }
        auto parsed = fmc::parseQueries(fastq, fmc::TextFormat::Fastq, fmc::SymbolTable::dna5());
        fmc::NameTable const fromNames{fastq, parsed.names}, fromQuals{fastq, parsed.quals};
        Reads parsedReads;
        for (auto const& r : parsed) parsedReads.emplace_back(r.begin(), r.end());
        std::vector<fmgpu_position> few;
        for (size_t i = 0; i < 10; i += 2) { fmgpu_position p{}; p.qidx = 2 * i + (i % 4 == 0); p.seq_id = i % 4; p.pos = 1000 * i; few.push_back(p); }
        fmc::SamSpec spec;
        spec.strands = &strands; spec.readNames = &fromNames; spec.quals = &fromQuals; spec.seqNames = &nt;
        CHECK(parsed.size() == 10 && fmc::formatSam(few, parsed, spec).text == hostSam(few, parsedReads, spec, &names, &qs, &seqNames));
    }
    {   // a read beyond the batch, a read out of order: the lowest offending record is named; the next call succeeds
        fmc::SamSpec spec;
        spec.strands = &strands;
        auto bad = positions;
        bad[900].qidx = 2 * reads.size(); bad[400].qidx = 2 * reads.size() + 5;
        bool threw = false;
        try { (void)fmc::formatSam(bad, reads, spec); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "record 400 ") != nullptr; }
        CHECK(threw);
        bad = positions; bad[500].qidx = 0;
        threw = false;
        try { (void)fmc::formatSam(bad, reads, spec); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "record 500 ") != nullptr; }
        CHECK(threw);
        CHECK(fmc::formatSam(positions, reads, spec).text == hostSam(positions, reads, spec, nullptr, nullptr, nullptr));
    }

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
