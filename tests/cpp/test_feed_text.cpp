// fmc::Feed::mapText (include/fmc_gpu.hpp, fmgpu_feed_map_text): the bytes of a FASTA and of a FASTQ file mapped through a feed, window by window, against
// fmc::map(index, fmc::parseQueries(text, ...), query) on the whole text, with the names, quality lines and lengths of the whole-text parse.
// Exit 77 without a device.
#include "../../include/fmc_gpu.hpp"

#include <cstdio>
#include <cstring>
#include <random>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

template <typename T>
static bool sameBytes(std::vector<T> const& a, std::vector<T> const& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main() {
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return 77; }

    using Reads = std::vector<std::vector<uint8_t>>;
    std::mt19937 rng(23);
    Reads text(2);
    for (auto& t : text) { t.resize(1500); for (auto& c : t) c = static_cast<uint8_t>(1 + rng() % 4); }
    fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16> index{text, 4, 1};
    std::string fasta, fastq;
    char const* letters = "$ACGT";
    for (size_t i = 0; i < 70; ++i) {
        size_t const m = i == 9 ? 0 : 20 + rng() % 45, at = rng() % (1500 - 70);
        std::string s;
        for (size_t k = 0; k < m; ++k) s.push_back(letters[text[i % 2][at + k]]);
        if (m && i % 3 == 0) s[rng() % m] = "ACGT"[rng() % 4];              // a substitution: found by the ladder's second or third scheme
        if (m && i % 11 == 0) s[m / 2] = 'N';                               // a foreign byte
        char const* eol = i % 4 == 1 ? "\r\n" : "\n";
        fasta += ">read " + std::to_string(i) + eol;
        for (size_t k = 0; k < s.size(); k += 17) fasta += s.substr(k, 17) + eol;
        fastq += "@read " + std::to_string(i) + eol + s + eol + "+" + eol + std::string(s.size(), static_cast<char>('!' + i % 40)) + eol;
    }
    fasta.pop_back();                                                       // the last record ends the file without a newline
    auto const dna = fmc::SymbolTable::dna5();
    auto const query = fmc::MapQuery::ladder(2, false);

    struct Case { std::string const* text; fmc::TextFormat format; };
    for (auto const& c : {Case{&fasta, fmc::TextFormat::Fasta}, Case{&fastq, fmc::TextFormat::Fastq}}) {
        auto const parsed = fmc::parseQueries(*c.text, c.format, dna);
        auto const want = fmc::map(index, parsed, query);
        CHECK(parsed.size() == 70 && !want.positions.empty() && want.positions.size() >= want.hits.size());
        fmgpu_feed_config config{};
        config.slots = 3;
        fmc::Feed feed{index, config};
        for (uint64_t chunkBytes : {uint64_t{16}, uint64_t{257}, uint64_t{0}}) {
            auto const got = feed.mapText(std::string_view{*c.text}, c.format, dna, query, true, chunkBytes);
            CHECK(sameBytes(got.positions, want.positions) && sameBytes(got.hits, want.hits) && got.stratum == want.stratum);
            CHECK(sameBytes(got.names, parsed.names) && sameBytes(got.quals, parsed.quals));
            CHECK(got.size() == parsed.size() && got.consumed == parsed.consumed && got.foreign == parsed.foreign && got.symbols == parsed.qbuf.size());
            for (size_t q = 0; q < got.size() && q < parsed.size(); ++q) CHECK(got.lens[q] == parsed[q].size());
            CHECK(got.name(*c.text, 12) == "read 12" && got.quality(*c.text, 5) == parsed.quality(*c.text, 5));
            uint64_t const B = chunkBytes ? chunkBytes : (uint64_t{64} << 20);
            CHECK(feed.info().lastChunks == (c.text->size() + B - 1) / B && feed.info().lastUploadedBytes == c.text->size());
        }
        // the bytes as they lie in a buffer of uint8_t, and a text that is not final: the last record stays for the next call
        auto const* bytes = reinterpret_cast<uint8_t const*>(c.text->data());
        using Feed = fmc::Feed<fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16>>;
        auto const head = feed.mapText(Feed::ByteView{bytes, c.text->size()}, c.format, dna, query, false, 64);
        auto const headParsed = fmc::parseQueries(*c.text, c.format, dna, false);
        CHECK(head.size() == headParsed.size() && head.consumed == headParsed.consumed && head.size() >= 69 && sameBytes(head.names, headParsed.names));
    }
    {   // a text error names the line of the whole text
        std::string bad = fastq;
        size_t const at = bad.find("\n+", bad.size() / 2);
        bad[at + 1] = '-';
        fmc::Feed feed{index};
        bool thrown = false;
        try { (void)feed.mapText(std::string_view{bad}, fmc::TextFormat::Fastq, dna, query, true, 64); }
        catch (std::exception const& e) {
            thrown = true;
            size_t line = 0;
            for (size_t i = 0; i <= at; ++i) line += bad[i] == '\n';
            CHECK(std::string{e.what()}.find("text error in line " + std::to_string(line) + " ") != std::string::npos);
        }
        CHECK(thrown);
        CHECK(feed.mapText(std::string_view{fastq}, fmc::TextFormat::Fastq, dna, query).size() == 70);         // the feed serves a good call afterwards
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
