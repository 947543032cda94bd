// fmc::parseQueries (include/fmc_gpu.hpp): the symbol tables on the host; on a GPU FASTA and FASTQ text parsed on the device, the parsed batch searched, packed and
// mapped like the Sequences it spells, names and qualities read back through the spans, chunked parsing, and the text error a malformed file throws.
// Exit 77 without a device (the host checks have run by then).
#include "../../include/fmc_gpu.hpp"

#include <cstdio>
#include <random>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;

static Reads asReads(fmc::ParsedQueries const& p) {
    Reads out;
    for (auto const& r : p) out.emplace_back(r.begin(), r.end());
    return out;
}

int main() {
    {   // the ready-made tables
        auto const t = fmc::SymbolTable::dna5();
        CHECK(t.map['$'] == 0 && t.map['A'] == 1 && t.map['c'] == 2 && t.map['G'] == 3 && t.map['t'] == 4 && t.map['N'] == fmc::SymbolTable::Foreign && t.map['\n'] == 255);
        CHECK(fmc::SymbolTable::dna5(true).map['N'] == 1 && fmc::SymbolTable::dna6().map['n'] == 5 && fmc::SymbolTable::dna6().map['-'] == 255);
        auto const p = fmc::SymbolTable::protein();
        CHECK(p.map['A'] == 1 && p.map['Y'] == 20 && p.map['y'] == 20 && p.map['B'] == 255 && p.map['$'] == 0);
        auto const d = fmc::SymbolTable{"ab", 3, false, 9, " -"}.set('z', 0);
        CHECK(d.map['a'] == 3 && d.map['b'] == 4 && d.map['A'] == 9 && d.map[' '] == fmc::SymbolTable::Drop && d.map['-'] == fmc::SymbolTable::Drop && d.map['z'] == 0);
    }
    if (failures) return 1;
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("host checks passed; no device\n"); return 77; }

    std::mt19937 rng(11);
    Reads text(2);
    for (auto& t : text) { t.resize(1200); for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4); }
    fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{text, 4, 1};
    Reads reads;
    for (size_t i = 0; i < 60; ++i) {
        size_t const m = i == 7 ? 0 : 20 + rng() % 40, at = rng() % (1200 - 60);
        reads.emplace_back(text[i % 2].begin() + at, text[i % 2].begin() + at + m);
    }
    std::string fasta, fastq;
    char const* letters = "$ACGT";
    for (size_t i = 0; i < reads.size(); ++i) {
        std::string s;
        for (auto c : reads[i]) s.push_back(letters[c]);
        fasta += ">read " + std::to_string(i) + "\n";
        for (size_t k = 0; k < s.size(); k += 23) fasta += s.substr(k, 23) + (i % 2 ? "\r\n" : "\n");
        fastq += "@read " + std::to_string(i) + "\n" + s + "\n+\n" + std::string(s.size(), static_cast<char>('!' + i % 40)) + "\n";
    }
    auto const dna = fmc::SymbolTable::dna5();
    auto const fromFasta = fmc::parseQueries(fasta, fmc::TextFormat::Fasta, dna), fromFastq = fmc::parseQueries(fastq, fmc::TextFormat::Fastq, dna);
    CHECK(asReads(fromFasta) == reads && asReads(fromFastq) == reads);
    CHECK(fromFasta.consumed == fasta.size() && fromFastq.consumed == fastq.size() && fromFasta.foreign == 0 && fromFastq.foreign == 0);
    CHECK(fromFastq.size() == reads.size() && fromFastq[3].size() == reads[3].size() && fromFastq[7].empty());
    CHECK(fromFasta.name(fasta, 12) == "read 12" && fromFastq.name(fastq, 59) == "read 59");
    CHECK(fromFastq.quality(fastq, 5) == std::string(reads[5].size(), '!' + 5) && fromFasta.quality(fasta, 5).empty());

    // the parsed batch where a Sequences object goes: exact search, a scheme search, the device packer, fmc::map, a feed
    using Row = std::tuple<size_t, uint64_t, uint64_t, size_t>;
    std::vector<Row> a, b;
    fmc::search_no_errors::search(index, reads, [&](size_t q, auto const& c) { a.emplace_back(q, c.lb, c.len, 0); });
    fmc::search_no_errors::search(index, fromFastq, [&](size_t q, auto const& c) { b.emplace_back(q, c.lb, c.len, 0); });
    CHECK(a.size() >= reads.size() - 1 && a == b);
    a.clear(); b.clear();
    auto const scheme = fmc::search_scheme::generator::h2(3, 0, 1);
    fmc::search_ng26::search<false>(index, reads, scheme, {}, [&](size_t q, auto const& c, size_t e) { a.emplace_back(q, c.lb, c.len, e); });
    fmc::search_ng26::search<false>(index, fromFasta, scheme, {}, [&](size_t q, auto const& c, size_t e) { b.emplace_back(q, c.lb, c.len, e); });
    CHECK(!a.empty() && a == b);
    std::vector<uint8_t> const comp{0, 4, 3, 2, 1};
    auto const packedReads = fmc::PackedQueries::packOnDevice(reads, 5, comp), packedParsed = fmc::PackedQueries::packOnDevice(fromFastq, 5, comp);
    CHECK(packedReads.packed == packedParsed.packed && packedReads.qoff == packedParsed.qoff);
    fmc::MapQuery query;
    auto const m1 = fmc::map(index, reads, query), m2 = fmc::map(index, fromFasta, query);
    CHECK(!m1.positions.empty() && m1.positions.size() == m2.positions.size());
    for (size_t i = 0; i < m1.positions.size() && i < m2.positions.size(); ++i)
        CHECK(m1.positions[i].qidx == m2.positions[i].qidx && m1.positions[i].seq_id == m2.positions[i].seq_id && m1.positions[i].pos == m2.positions[i].pos);
    a.clear(); b.clear();
    fmc::Feed feed{index};
    feed.search_no_errors(reads, [&](size_t q, auto const& c) { a.emplace_back(q, c.lb, c.len, 0); });
    feed.search_no_errors(fromFastq, [&](size_t q, auto const& c) { b.emplace_back(q, c.lb, c.len, 0); });
    CHECK(!a.empty() && a == b);

    {   // a file in two chunks: the first half proves some records complete, the rest starts at `consumed`
        std::string_view const whole{fastq};
        auto const head = fmc::parseQueries(whole.substr(0, fastq.size() / 2 + 3), fmc::TextFormat::Fastq, dna, false);
        auto const tail = fmc::parseQueries(whole.substr(head.consumed), fmc::TextFormat::Fastq, dna);
        auto joined = asReads(head);
        for (auto const& r : asReads(tail)) joined.push_back(r);
        CHECK(head.size() > 10 && tail.size() > 10 && head.consumed <= fastq.size() / 2 + 3 && joined == reads);
    }
    {   // symbols outside the alphabet, dropped bytes, LINES
        auto const p = fmc::parseQueries("AC-GN\n\nT T\n", fmc::TextFormat::Lines, fmc::SymbolTable{"ACGT", 1, true, fmc::SymbolTable::Foreign, "- "});
        CHECK((asReads(p) == Reads{{1, 2, 3, 255}, {}, {4, 4}}) && p.foreign == 1);
    }
    {   // the text errors
        std::string what;
        try { (void)fmc::parseQueries("@a\nAC\n+\nII\n@b\nGT\n+\nIII\n", fmc::TextFormat::Fastq, dna); } catch (std::runtime_error const& e) { what = e.what(); }
        std::printf("thrown: %s\n", what.c_str());
        CHECK(what.find("line 7") != std::string::npos && what.find("offset 19") != std::string::npos);
        what.clear();
        try { (void)fmc::parseQueries("ACGT\n>a\nAC\n", fmc::TextFormat::Fasta, dna); } catch (std::runtime_error const& e) { what = e.what(); }
        std::printf("thrown: %s\n", what.c_str());
        CHECK(what.find("line 0") != std::string::npos);
    }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
