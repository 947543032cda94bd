// Positions as text through include/fmc_gpu.hpp: the mirror structs and fmc::NameTable on the host (checked everywhere, with the argument checks of
// fmgpu_positions_format that come before the device), then on a device fmc::formatPositions against a snprintf loop: the example's line, every column, names from
// strings and from the spans of a parse, both strands.  Exit 77 without a device, after the host checks.
#include "../../include/fmc_gpu.hpp"

#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Col = fmc::FormatSpec::Column;

// the same contract with snprintf: what a caller's own loop would write
static std::string hostFormat(std::vector<fmgpu_position> const& positions, fmc::FormatSpec const& spec, std::vector<std::string> const* reads = nullptr,
                              std::vector<std::string> const* seqs = nullptr) {
    auto stop = [&](std::string const& n) { return spec.nameStop ? n.substr(0, std::min(n.find(' '), n.find('\t'))) : n; };
    std::string out;
    char buf[32];
    for (auto const& p : positions) {
        uint64_t const read = spec.strands ? p.qidx >> 1 : p.qidx;
        for (size_t c = 0; c < spec.columns.size(); ++c) {
            uint64_t v = 0;
            bool number = true;
            switch (spec.columns[c]) {
                case Col::Qidx: v = p.qidx; break;
                case Col::SeqId: v = p.seq_id; break;
                case Col::Pos: v = p.pos + spec.posAdd; break;
                case Col::Errors: v = p.errors; break;
                case Col::Hit: v = p.hit; break;
                case Col::Read: v = read; break;
                case Col::Strand: out += spec.strands && (p.qidx & 1) ? '-' : '+'; number = false; break;
                case Col::ReadName: out += stop((*reads)[read]); number = false; break;
                case Col::SeqName: out += stop((*seqs)[p.seq_id]); number = false; break;
            }
            if (number) { std::snprintf(buf, sizeof buf, "%" PRIu64, v); out += buf; }
            out += c + 1 < spec.columns.size() ? spec.sep : '\n';
        }
    }
    return out;
}

int main() {
    {   // the host mirror: no device needed
        static_assert(sizeof(fmgpu_format_spec) == 40 && sizeof(fmgpu_name_table) == 32 && sizeof(fmgpu_position) == 32, "the sizes include/fmgpu.h states");
        static_assert(offsetof(fmgpu_format_spec, cols) == 4 && offsetof(fmgpu_format_spec, sep) == 12 && offsetof(fmgpu_format_spec, reserved) == 15 &&
                      offsetof(fmgpu_format_spec, pos_add) == 16 && offsetof(fmgpu_format_spec, read_names) == 24 && offsetof(fmgpu_format_spec, seq_names) == 32, "field offsets");
        fmc::FormatSpec spec;
        CHECK((spec.columns == std::vector<Col>{Col::Qidx, Col::SeqId, Col::Pos, Col::Errors}) && spec.sep == ' ' && !spec.strands && !spec.nameStop && spec.posAdd == 0);
        CHECK(static_cast<int>(Col::SeqName) == FMGPU_COL_SEQ_NAME && static_cast<int>(Col::Strand) == FMGPU_COL_STRAND);
        fmc::NameTable names{std::vector<std::string>{"ab", "", "xyz"}};
        auto c = names.c();
        CHECK(c.n_bytes == 5 && c.count == 3 && c.bytes == names.bytes.data() && c.spans == names.spans.data());
        CHECK(names.spans[1].offset == 2 && names.spans[1].len == 0 && names.spans[2].offset == 2 && names.spans[2].len == 3);
        fmc::NameTable fromText{"@r0 x\nACGT\n", {fmgpu_text_span{1, 4}}};
        CHECK(fromText.c().n_bytes == 11 && fromText.c().count == 1);
        CHECK(fmc::NameTable{}.c().bytes == nullptr && fmc::NameTable{}.c().spans == nullptr);
        // no record: no text, before anything else is looked at
        CHECK(fmc::formatPositions({}).empty());
        // the argument checks that come before the device
        std::vector<fmgpu_position> one(1);
        uint64_t bytes = 7;
        fmgpu_format_spec s{};
        s.n_cols = 1;
        CHECK(fmgpu_positions_format(one.data(), 1, nullptr, nullptr, 0, &bytes, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "spec is null"));
        CHECK(fmgpu_positions_format(nullptr, 1, &s, nullptr, 0, &bytes, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "positions is null"));
        s.n_cols = 9;
        CHECK(fmgpu_positions_format(one.data(), 1, &s, nullptr, 0, &bytes, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "n_cols"));
        s.n_cols = 1; s.cols[0] = FMGPU_COL_READ_NAME;
        CHECK(fmgpu_positions_format(one.data(), 1, &s, nullptr, 0, &bytes, nullptr, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "read_names"));
        bool threw = false;
        try { fmc::FormatSpec nine; nine.columns.assign(9, Col::Qidx); (void)fmc::formatPositions(one, nine); } catch (std::runtime_error const&) { threw = true; }
        CHECK(threw);
    }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return failures ? 1 : 77; }

    std::mt19937_64 rng(23);
    std::vector<std::string> const readNames{"read0 first", "r1", "", "read3\tlane 2", "a-rather-long-read-name-of-more-than-sixty-four-bytes-so-that-its-wave-copies-it/1"};
    std::vector<std::string> const seqNames{"chr1", "chr2 assembled", "chrM"};
    std::vector<fmgpu_position> positions(1500);
    for (size_t i = 0; i < positions.size(); ++i) {
        auto& p = positions[i];
        p.qidx = rng() % (2 * readNames.size());
        p.seq_id = rng() % seqNames.size();
        p.pos = rng() >> (rng() % 64);
        p.errors = static_cast<uint32_t>(rng() >> (32 + rng() % 32));
        p.hit = static_cast<uint32_t>(i);
    }
    positions[7].pos = UINT64_MAX; positions[8].pos = 0; positions[9].pos = 9999999999ull;
    fmc::NameTable const reads{readNames}, seqs{seqNames};

    {   // the example's line: "%zu %zu %zu %zu\n"
        std::string want;
        char buf[128];
        for (auto const& p : positions) {
            std::snprintf(buf, sizeof buf, "%zu %zu %zu %zu\n", static_cast<size_t>(p.qidx), static_cast<size_t>(p.seq_id), static_cast<size_t>(p.pos), static_cast<size_t>(p.errors));
            want += buf;
        }
        CHECK(fmc::formatPositions(positions) == want);
        CHECK(hostFormat(positions, fmc::FormatSpec{}) == want);
    }
    for (bool stop : {false, true}) {
        fmc::FormatSpec spec{{Col::ReadName, Col::SeqName, Col::Pos, Col::Strand, Col::Read, Col::Errors, Col::Hit, Col::Qidx}, '\t', true, stop, 1};
        CHECK(fmc::formatPositions(positions, spec, &reads, &seqs) == hostFormat(positions, spec, &readNames, &seqNames));
    }
    {   // strands off: every qidx is its own read
        std::vector<fmgpu_position> few(positions.begin(), positions.begin() + 300);
        for (auto& p : few) p.qidx %= readNames.size();
        fmc::FormatSpec spec{{Col::Read, Col::Strand, Col::ReadName, Col::Pos, Col::Pos}, ' ', false, true, UINT64_MAX};
        CHECK(fmc::formatPositions(few, spec, &reads) == hostFormat(few, spec, &readNames));
    }
    {   // names as the spans of a parse: the text is the table's bytes
        std::string fastq;
        for (size_t i = 0; i < 10; ++i) fastq += "@q" + std::to_string(i) + " extra\nACGT\n+\nIIII\n";
        auto parsed = fmc::parseQueries(fastq, fmc::TextFormat::Fastq, fmc::SymbolTable::dna5());
        fmc::NameTable fromParse{fastq, parsed.names};
        std::vector<std::string> names;
        for (size_t i = 0; i < 10; ++i) names.push_back("q" + std::to_string(i) + " extra");
        std::vector<fmgpu_position> few(positions.begin(), positions.begin() + 300);
        fmc::FormatSpec spec{{Col::ReadName, Col::Pos}, '\t', true, true, 0};
        CHECK(parsed.names.size() == 10 && fmc::formatPositions(few, spec, &fromParse) == hostFormat(few, spec, &names));
    }
    {   // a row beyond the table: the lowest offending record is named
        auto bad = positions;
        bad[900].qidx = 2 * readNames.size(); bad[400].qidx = 2 * readNames.size() + 5;
        fmc::FormatSpec spec{{Col::ReadName}, ' ', true, false, 0};
        bool threw = false;
        try { (void)fmc::formatPositions(bad, spec, &reads); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "record 400 ") != nullptr; }
        CHECK(threw);
        CHECK(fmc::formatPositions(positions, spec, &reads) == hostFormat(positions, spec, &readNames));      // the next call succeeds
    }

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
