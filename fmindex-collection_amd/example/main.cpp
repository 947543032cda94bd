// The reference's `example` harness (src/example/main.cpp, with its command line and FASTA reader) on the GPU path — same behaviour, own code:
// FASTA -> ranks, reverse complements, BiFMIndex<5, InterleavedBitvector16> at sampling rate 16, one search per k in
// [min_k, max_k] with the chosen algorithm and search-scheme generator, LocateLinear of every reported cursor, the same
// statistics line and the same `--save_output` file ("queryId seqId pos" per located row, in callback order).
//
// Same flags as the reference.  What differs:
//   * the index is built on the GPU at every start (seconds for a human genome) instead of being cached in `<fasta>.tab.dense.index`
//     (a cereal archive, not read or written here); --partialBuildUp, --threads and --ext are accepted and have nothing to switch;
//   * --algo: `ng21` (all four modes, main.cpp:176-185), `noerror` (:213-215), and `ng26` (search_ng26::search, Edit = true, over the
//     un-expanded scheme with a uniform partition) are available; the other research variants are not part of this build;
//   * --gen: backtracking, pigeon, pigeon_opt, h2-k1, h2-k2, h2-k3 (generator/all.h:35-96); `<name>_dyn` stretches the scheme to the read length by expandByWNC (Edit = true, sigma 4, 3e9 rows: main.cpp:116) instead of uniformly;
//   * locating is one batched call over all rows of all cursors (the rows and their order are the reference's);
//   * --packed (not in the reference): the reads are packed once, 4 bits per symbol, and searched in that form (the `_q4` entry points); the reverse
//     complements are made on the device while packing (fmgpu_queries_pack4) instead of on the host.  The output is the same, byte for byte.
//   * --feed (not in the reference): `noerror` and `ng26` (mode all) search through an fmc::Feed — the reads go to the device chunk by chunk, upload, search and
//     download overlapped, the Sequences object is not flattened; with --packed the packed batch goes through the feed.  The output is the same, byte for byte.
//   * --mode map (not in the reference): search, callback order and locate as ONE fmgpu_map call (fmc::map) — `noerror` as exact search, `ng26` / `ng21` as the best-hit
//     ladder of `besthits`; with --feed through fmgpu_feed_map_v (fmc::Feed::map), chunk by chunk.  --save_output then holds "queryId seqId pos errors" per located row,
//     in the reference's report order (fmc::Search's reportFunc arguments).
//   * --mode map --feed --device-parse --no-reverse (no trimming, no read limit, not ng21): the bytes of the query file go through the feed as they are
//     (fmgpu_feed_map_text through fmc::Feed::mapText); the reads are never vectors on the host.  The same --save_output file as without --device-parse.
//   * --pair-strands (not in the reference; --mode map, not --packed): the reverse complements are made on the device and the ladder stops for a read once either of its
//     strands is found (fmgpu_map_strands with pair = 1 through fmc::map / fmc::Feed::map with an fmc::Strands).  queryId in --save_output then counts read by read,
//     2 * read + strand, instead of the forward reads followed by the reverse complements.  With --feed --device-parse (no trimming, no read limit, not ng21) the
//     bytes of the query file go through fmgpu_feed_map_text_strands.
//   * --device-format (not in the reference; --mode map): the --save_output file is formatted on the device (fmgpu_positions_format through fmc::formatPositions) instead
//     of by the fprintf loop.  The file is the same, byte for byte.  fmc::map returns host vectors, so the records are staged up again for it: this flag proves that
//     the two writers agree, not that one is faster (tools/format_probe.py measures that on records that are resident on the device).
//   * --sam (not in the reference; --mode map, not --packed): the --save_output file is a SAM file: the header (fmgpu_sam_header through fmc::samHeader: one @SQ line
//     per sequence of --index, named up to its first blank) followed by the records made on the device (fmgpu_positions_sam through fmc::formatSam) from the positions
//     and the searched batch.  QNAME is the read's number in that batch and QUAL is '*' (the default reader keeps neither names nor qualities); CIGAR is "<m>M" for
//     noerror and '*' otherwise (the ladders of this harness are edit-distance searches).  With --pair-strands a read and its reverse complement are one read (flag 16);
//     without it every read of the searched batch, the reverse complements the harness appends included, is a read of its own.
//   * --mates <second query file> (not in the reference; --mode map, not --sam, --feed, --packed, --device-format or --queries): read i of --query and read i of
//     --mates are the two mates of fragment i.  Both files are mapped as --mode map maps one, and the positions are joined on the device (fmgpu_positions_mates
//     through fmc::joinMates) with --min_tlen / --max_tlen (0 / 1000): with both strands a pair is concordant in FR orientation, with --no-reverse in any.
//     --save_output gets "fragment seqId posA strandA posB strandB tlen errors" per pair, strands as + / -.
//   * --chain-seeds (not in the reference; --mode map, not --packed, --feed, --pair-strands, --device-format, --sam or --mates): in place of the scheme search the
//     seeds of every read (fmgpu_search_smems: --min_seed, default 19; --max_seed_rows, default 50) are located (fmgpu_locate_hits) and joined to collinear chains on
//     the device (fmgpu_seeds_chain through fmc::chainSeeds).  --save_output gets "qidx seq_id tbeg tend qbeg qend score n_anchors" per chain.
//   * --align-chains (not in the reference; only with --chain-seeds): every chain is aligned between its ends on the device (fmgpu_chains_align through
//     fmc::alignChains, the text under the chains read from the index); each line of --save_output gains "status n_match n_mismatch n_ins n_del cigar".
//   * --paired-sam (not in the reference; only with --mates): the --save_output file is a paired-end SAM file instead of the pair lines: the header of --sam
//     followed by two records per fragment made on the device (fmgpu_positions_sam_mates through fmc::formatSamMates) from the positions of the two files and the
//     joined pairs: a fragment with pairs takes the one with the fewest errors and is proper, elsewhere each mate takes its primary record.  QNAME = the fragment's
//     number, RNAME as under --sam.
//   * --device-parse (not in the reference): the --query file is read as bytes and parsed on the device (fmgpu_queries_parse through fmc::parseQueries); its first byte
//     chooses FASTA ('>') or FASTQ ('@', read only this way).  On a well-formed FASTA — ends in a newline, no '>' inside sequence lines, no '\r' — the output is the
//     same, byte for byte.  Elsewhere the device rules differ from the reader below: a '\r' in front of a newline belongs to the line end (the reader takes it for
//     a symbol), a '>' that is not the first byte of its line is an ordinary byte (the reader starts a record there), a last line without a newline keeps its last
//     base (the reader drops the file's last byte), and a name line at the very end of the file is an empty read (the reader yields no record).  The --index file keeps the reader below.
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <iterator>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

// ---- command line --------------------------------------------------------------------------------------------------------------
// What the reference's example accepts (its argp.h), described as a table: flag, whether a value follows, what the value does.  Numbers are
// read as floating point and truncated, so "--queries 1e5" works as it does there; a flag that needs a value but is the last token, and any
// token that is no flag, is reported as "unknown commandline <token>".
enum class HitMode { all, besthits, map };
struct Options {
    std::string referenceFasta, readsFasta, outputFile, matesFasta;
    std::vector<std::string> algorithms;
    std::string schemeName = "h2-k2";
    bool schemeDyn = false;
    size_t firstK = 0, lastK = 6, stepK = 1;
    size_t readLimit = 0, trimTo = 0, hitsPerRead = 0;          // 0 = no limit
    size_t minTlen = 0, maxTlen = 1000;                          // --mates: the template lengths of a concordant pair, inclusive
    size_t minSeed = 19, maxSeedRows = 50;                       // --chain-seeds: the shortest seed kept, the most rows a kept seed may have (0 = no limit)
    bool withReverseComplement = true, unknownToA = false, wantHelp = false, packed = false, feed = false, deviceParse = false, pairStrands = false, deviceFormat = false, sam = false, pairedSam = false, chainSeeds = false, alignChains = false;
    HitMode hitMode = HitMode::all;
};

size_t asCount(char const* text) { return static_cast<size_t>(std::strtod(text, nullptr)); }

struct FlagRule {
    char const* name;
    bool takesValue;
    void (*apply)(Options&, char const*);
};
FlagRule const kFlags[] = {
    {"--index", true, [](Options& o, char const* v) { o.referenceFasta = v; }},
    {"--query", true, [](Options& o, char const* v) { o.readsFasta = v; }},
    {"--save_output", true, [](Options& o, char const* v) { o.outputFile = v; }},
    {"--algo", true, [](Options& o, char const* v) { o.algorithms.emplace_back(v); }},
    {"--gen", true, [](Options& o, char const* v) {
         o.schemeName = v;
         static std::string const suffix = "_dyn";
         if (o.schemeName.size() > suffix.size() && o.schemeName.compare(o.schemeName.size() - suffix.size(), suffix.size(), suffix) == 0) {
             o.schemeName.erase(o.schemeName.size() - suffix.size());
             o.schemeDyn = true;
         }
     }},
    {"--min_k", true, [](Options& o, char const* v) { o.firstK = asCount(v); }},
    {"--max_k", true, [](Options& o, char const* v) { o.lastK = asCount(v); }},
    {"--stepSize_k", true, [](Options& o, char const* v) { o.stepK = asCount(v); }},
    {"--queries", true, [](Options& o, char const* v) { o.readLimit = asCount(v); }},
    {"--read_length", true, [](Options& o, char const* v) { o.trimTo = asCount(v); }},
    {"--maxhitperquery", true, [](Options& o, char const* v) { o.hitsPerRead = asCount(v); }},
    {"--mode", true, [](Options& o, char const* v) {
         std::string const m = v;
         if (m == "all") o.hitMode = HitMode::all;
         else if (m == "besthits") o.hitMode = HitMode::besthits;
         else if (m == "map") o.hitMode = HitMode::map;
         else throw std::runtime_error("invalid mode \"" + m + "\", must be any of \"all\", \"besthits\", \"map\"");
     }},
    {"--no-reverse", false, [](Options& o, char const*) { o.withReverseComplement = false; }},
    {"--convertUnknownChar", false, [](Options& o, char const*) { o.unknownToA = true; }},
    {"--help", false, [](Options& o, char const*) { o.wantHelp = true; }},
    {"--packed", false, [](Options& o, char const*) { o.packed = true; }},
    {"--feed", false, [](Options& o, char const*) { o.feed = true; }},
    {"--device-parse", false, [](Options& o, char const*) { o.deviceParse = true; }},
    {"--pair-strands", false, [](Options& o, char const*) { o.pairStrands = true; }},
    {"--device-format", false, [](Options& o, char const*) { o.deviceFormat = true; }},
    {"--sam", false, [](Options& o, char const*) { o.sam = true; }},
    {"--mates", true, [](Options& o, char const* v) { o.matesFasta = v; }},
    {"--paired-sam", false, [](Options& o, char const*) { o.pairedSam = true; }},
    {"--min_tlen", true, [](Options& o, char const* v) { o.minTlen = asCount(v); }},
    {"--max_tlen", true, [](Options& o, char const* v) { o.maxTlen = asCount(v); }},
    {"--chain-seeds", false, [](Options& o, char const*) { o.chainSeeds = true; }},
    {"--align-chains", false, [](Options& o, char const*) { o.alignChains = true; }},
    {"--min_seed", true, [](Options& o, char const* v) { o.minSeed = asCount(v); }},
    {"--max_seed_rows", true, [](Options& o, char const* v) { o.maxSeedRows = asCount(v); }},
    // accepted for compatibility; nothing to switch in this build (no index cache file, no host threads, one String type)
    {"--ext", true, [](Options&, char const*) {}},
    {"--threads", true, [](Options&, char const*) {}},
    {"--partialBuildUp", false, [](Options&, char const*) {}},
};

Options parseCommandLine(int argc, char const* const* argv) {
    Options o;
    for (int at = 1; at < argc; ++at) {
        std::string const token = argv[at];
        FlagRule const* rule = nullptr;
        for (auto const& f : kFlags) if (token == f.name) { rule = &f; break; }
        if (!rule || (rule->takesValue && at + 1 >= argc)) throw std::runtime_error("unknown commandline " + token);
        rule->apply(o, rule->takesValue ? argv[++at] : nullptr);
    }
    return o;
}

// ---- FASTA ------------------------------------------------------------------------------------------------------------------------
// The reader the example uses, by its observable rules: the file must begin with '>'; a name line runs to the next newline; every other
// byte of a record is a symbol — $ A C G T (either case) are ranks 0..4, N is rank 5 when the alphabet has six symbols, newlines are
// dropped, any other byte is rank 1 (5 with six symbols) under --convertUnknownChar and an "unknown alphabet" error without it; a '>'
// anywhere in the sequence part starts the next record; the very last byte of the file ends the last record and is never a symbol itself
// (a file whose last line has no newline loses its last base); a name line that runs to the end of the file yields no record.
enum ByteClass : uint8_t { kSymbol0 = 0, /* 1..5: that rank */ kSkip = 6, kOther = 7 };
std::array<uint8_t, 256> byteClasses(size_t sigma) {
    std::array<uint8_t, 256> t;
    t.fill(kOther);
    t[static_cast<unsigned char>('\n')] = kSkip;
    t[static_cast<unsigned char>('$')] = 0;
    char const* letters = "ACGT";
    for (uint8_t r = 0; r < 4; ++r) {
        t[static_cast<unsigned char>(letters[r])] = static_cast<uint8_t>(r + 1);
        t[static_cast<unsigned char>(letters[r] - 'A' + 'a')] = static_cast<uint8_t>(r + 1);
    }
    if (sigma == 6) t[static_cast<unsigned char>('N')] = t[static_cast<unsigned char>('n')] = 5;
    return t;
}

std::vector<std::vector<uint8_t>> readFasta(std::string const& path, size_t sigma, bool unknownToA) {
    std::vector<std::vector<uint8_t>> records;
    if (path.empty() || !std::filesystem::exists(path)) return records;
    std::ifstream in{path, std::ios::binary};
    std::vector<char> bytes{std::istreambuf_iterator<char>{in}, std::istreambuf_iterator<char>{}};
    if (bytes.empty() || bytes[0] != '>') throw std::runtime_error("can't read fasta file");
    auto const classes = byteClasses(sigma);
    uint8_t const fallback = sigma == 6 ? 5 : 1;
    size_t const size = bytes.size();
    size_t at = 0;
    while (at < size) {                                            // `at` stands on the '>' of a name line
        while (at < size && bytes[at] != '\n') ++at;
        ++at;                                                      // first byte of the sequence part
        if (at >= size) break;
        std::vector<uint8_t> ranks;
        for (; at + 1 < size && bytes[at] != '>'; ++at) {
            uint8_t const cls = classes[static_cast<unsigned char>(bytes[at])];
            if (cls < kSkip) ranks.push_back(cls);
            else if (cls == kOther) {
                if (!unknownToA) throw std::runtime_error("unknown alphabet");
                ranks.push_back(fallback);
            }
        }
        records.push_back(std::move(ranks));
        if (at + 1 >= size) break;                                 // stopped on the last byte of the file
    }
    return records;
}

// --device-parse: the same ranks from the raw bytes of a FASTA or FASTQ file, parsed on the device (the line rules of fmgpu_queries_parse, include/fmgpu.h)
std::vector<std::vector<uint8_t>> readQueriesOnDevice(std::string const& path, size_t sigma, bool unknownToA) {
    std::vector<std::vector<uint8_t>> records;
    if (path.empty() || !std::filesystem::exists(path)) return records;
    std::ifstream in{path, std::ios::binary};
    std::string const bytes{std::istreambuf_iterator<char>{in}, std::istreambuf_iterator<char>{}};
    if (bytes.empty() || (bytes[0] != '>' && bytes[0] != '@')) throw std::runtime_error("can't read fasta file");
    auto const table = sigma == 6 ? fmc::SymbolTable::dna6(unknownToA) : fmc::SymbolTable::dna5(unknownToA);
    auto const parsed = fmc::parseQueries(bytes, bytes[0] == '@' ? fmc::TextFormat::Fastq : fmc::TextFormat::Fasta, table);
    if (parsed.foreign > 0) throw std::runtime_error("unknown alphabet");
    records.reserve(parsed.size());
    for (auto const& read : parsed) records.emplace_back(read.begin(), read.end());
    return records;
}

// --sam: the names of the sequences of a FASTA file, by the reader's rules above (a name line starts a record only if a sequence part follows it), without the
// blanks in front of them
std::vector<std::string> readFastaNames(std::string const& path) {
    std::vector<std::string> names;
    std::ifstream in{path, std::ios::binary};
    std::string const bytes{std::istreambuf_iterator<char>{in}, std::istreambuf_iterator<char>{}};
    size_t const size = bytes.size();
    size_t at = 0;
    while (at < size) {
        size_t const from = at + 1;
        while (at < size && bytes[at] != '\n') ++at;
        std::string name = bytes.substr(std::min(from, at), at - std::min(from, at));
        name.erase(0, name.find_first_not_of(" \t"));
        ++at;
        if (at >= size) break;
        names.push_back(name);
        while (at + 1 < size && bytes[at] != '>') ++at;
        if (at + 1 >= size) break;
    }
    return names;
}

// every read followed by its reverse complement (A <-> T, C <-> G; other ranks stay)
std::vector<std::vector<uint8_t>> withReverseComplements(std::vector<std::vector<uint8_t>> const& reads) {
    static uint8_t const complement[6] = {0, 4, 3, 2, 1, 5};
    std::vector<std::vector<uint8_t>> both;
    both.reserve(2 * reads.size());
    for (auto const& r : reads) {
        both.push_back(r);
        std::vector<uint8_t> rc(r.rbegin(), r.rend());
        for (auto& c : rc) if (c < 6) c = complement[c];
        both.push_back(std::move(rc));
    }
    return both;
}

// ---- search-scheme generators by name (the ones this build has; the reference's list is search_scheme/generator/all.h:35-96) ----------------
fmc::search_scheme::Scheme schemeByName(std::string const& name, size_t minErrors, size_t maxErrors) {
    namespace g = fmc::search_scheme::generator;
    struct Entry { char const* name; fmc::search_scheme::Scheme (*make)(size_t, size_t); };
    static Entry const table[] = {
        {"backtracking", [](size_t lo, size_t hi) { return g::backtracking(1, lo, hi); }},
        {"pigeon", [](size_t lo, size_t hi) { return g::pigeon_trivial(lo, hi); }},
        {"pigeon_opt", [](size_t lo, size_t hi) { return g::pigeon_opt(lo, hi); }},
        {"h2-k1", [](size_t lo, size_t hi) { return g::h2(hi + 1, lo, hi); }},
        {"h2-k2", [](size_t lo, size_t hi) { return g::h2(hi + 2, lo, hi); }},
        {"h2-k3", [](size_t lo, size_t hi) { return g::h2(hi + 3, lo, hi); }},
    };
    for (auto const& e : table) if (name == e.name) return e.make(minErrors, maxErrors);
    std::string known;
    for (auto const& e : table) known += std::string(known.empty() ? "" : ", ") + e.name;
    throw std::runtime_error("unknown search scheme generator \"" + name + "\" (this build has: " + known + ")");
}

struct StopWatch {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double reset() {
        auto n = std::chrono::steady_clock::now();
        double d = std::chrono::duration<double>(n - t).count();
        t = n;
        return d;
    }
};

// ---- one run of the harness ---------------------------------------------------------------------------------------------------------
// What the reference's main loop does for one (algorithm, k) pair, in this order: search (every reported cursor is a Hit), locate every row of
// every cursor (one batched device call here; the rows and their order are those of the per-cursor LocateLinear loops), count, print the
// statistics line, write the optional output file.
constexpr size_t Sigma = 5;                                      // $ A C G T (src/example/utils.h:81-85)
using Index = fmc::BiFMIndex<Sigma, fmc::string::InterleavedBitvector16>;
enum class Algorithm { ng21, ng26, noerror };

Algorithm algorithmByName(std::string const& name) {
    if (name == "ng21") return Algorithm::ng21;
    if (name == "ng26") return Algorithm::ng26;
    if (name == "noerror") return Algorithm::noerror;
    throw std::runtime_error("algorithm \"" + name + "\" is not part of this build (available: ng21, ng26, noerror)");
}

Index openIndex(Options const& config) {
    std::printf("start loading %s ...", "str");                  // (the one String of the example: InterleavedBitvector16)
    std::fflush(stdout);
    auto reference = readFasta(config.referenceFasta, Sigma, config.unknownToA);
    if (reference.empty()) throw std::runtime_error("no sequences in --index " + config.referenceFasta);
    Index index{reference, /*samplingRate*/ 16, /*threads*/ 1};   // built on the GPU at every start (seconds for a human genome)
    std::printf("done\n");
    return index;
}

struct Hit { size_t read; uint64_t firstRow, rows; size_t errors; };
struct Placement {
    size_t read, sequence, position, errors;
    bool operator<(Placement const& o) const { return std::tie(read, sequence, position, errors) < std::tie(o.read, o.sequence, o.position, o.errors); }
    bool operator==(Placement const& o) const { return std::tie(read, sequence, position, errors) == std::tie(o.read, o.sequence, o.position, o.errors); }
};

struct Run {
    Options const& config;
    Index index;
    fmc::NameTable referenceNames{};                             // --sam: the names and lengths of the sequences of --index
    std::vector<uint64_t> referenceLengths{};
    std::vector<std::vector<uint8_t>> const* mateReads{nullptr};  // --mates: the reads of the second file, loaded, doubled and trimmed as the first's

    // a scheme stretched to the read length: uniformly, or (--gen <name>_dyn) part by part where the weighted node count grows least — with the constants
    // the reference's example passes (src/example/main.cpp:116, :135: Edit = true, sigma 4, 3e9 rows)
    fmc::search_scheme::Scheme stretch(fmc::search_scheme::Scheme const& scheme, size_t len) const {
        return config.schemeDyn ? fmc::search_scheme::expandByWNC<true>(scheme, len, 4, 3'000'000'000) : fmc::search_scheme::expand(scheme, len);
    }

    // Queries: the reads as Sequences, or as fmc::PackedQueries (--packed); firstLength = the length of read 0
    template <typename Queries>
    std::vector<Hit> search(Algorithm kind, size_t k, Queries const& reads, size_t firstLength) const {
        std::vector<Hit> hits;
        auto collect = [&](size_t read, auto const& cursor, size_t errors) { hits.push_back({read, cursor.lb, cursor.len, errors}); };
        size_t const perRead = config.hitsPerRead == 0 ? std::numeric_limits<size_t>::max() : config.hitsPerRead;
        auto schemesUpTo = [&](auto&& make) {                      // best-hit modes try 0, 1, .. k errors in turn
            using T = decltype(make(size_t{}));
            std::vector<T> list;
            for (size_t j = 0; j <= k; ++j) list.push_back(make(j));
            return list;
        };
        switch (kind) {
        case Algorithm::noerror:
            if (config.feed) fmc::Feed{index}.search_no_errors(reads, [&](size_t read, auto const& cursor) { collect(read, cursor, 0); });
            else fmc::search_no_errors::search(index, reads, [&](size_t read, auto const& cursor) { collect(read, cursor, 0); });
            break;
        case Algorithm::ng26: {
            if (config.hitMode == HitMode::all && config.feed) fmc::Feed{index}.search_ng26<true>(reads, schemeByName(config.schemeName, 0, k), {}, collect, perRead);
            else if (config.hitMode == HitMode::all) fmc::search_ng26::search<true>(index, reads, schemeByName(config.schemeName, 0, k), {}, collect, perRead);
            else fmc::search_ng26::search_best<true>(index, reads, schemesUpTo([&](size_t j) {
                     return std::tuple<fmc::search_scheme::Scheme, std::vector<size_t>>{schemeByName(config.schemeName, j, j), {}}; }), collect, perRead);
            break;
        }
        case Algorithm::ng21: {
            size_t const len = firstLength;
            if (config.hitMode == HitMode::all) {
                auto const expanded = stretch(schemeByName(config.schemeName, 0, k), len);
                if (config.hitsPerRead == 0) fmc::search_ng21::search(index, reads, expanded, collect);
                else fmc::search_ng21::search_n(index, reads, expanded, config.hitsPerRead, collect);
            } else {
                auto const ladder = schemesUpTo([&](size_t j) { return stretch(schemeByName(config.schemeName, j, j), len); });
                if (config.hitsPerRead == 0) fmc::search_ng21::search_best(index, reads, ladder, collect);
                else fmc::search_ng21::search_best_n(index, reads, ladder, config.hitsPerRead, collect);
            }
            break;
        }
        }
        return hits;
    }

    std::vector<Placement> locate(std::vector<Hit> const& hits) const {
        std::vector<fmgpu_hit> cursors(hits.size());
        for (size_t i = 0; i < hits.size(); ++i) { cursors[i].qidx = hits[i].read; cursors[i].lb = hits[i].firstRow; cursors[i].len = hits[i].rows; }
        auto const where = index.locateHits(cursors);                   // every row of every hit, in hit order: one call
        std::vector<Placement> placed;
        placed.reserve(where.size());
        for (auto const& p : where) {
            auto const& h = hits[p.hit];
            placed.push_back({h.read, static_cast<uint32_t>(p.seq_id), p.pos, h.errors});
        }
        return placed;
    }

    // --mode map: the whole path as one fmgpu_map call (with --feed: fmgpu_feed_map_v); a packed batch goes through a feed as bytes
    // --pair-strands: the example's own complement rule (ranks 0 .. 5: A <-> T, C <-> G, the others stay), the pair ladder
    static fmc::Strands pairStrands() { return fmc::Strands{{0, 4, 3, 2, 1, 5}, true}; }
    template <typename Queries>
    fmc::MapResult mapThroughFeed(Queries const& reads, fmc::MapQuery const& query) const {
        return config.pairStrands ? fmc::Feed{index}.map(reads, query, pairStrands()) : fmc::Feed{index}.map(reads, query);
    }
    fmc::MapResult mapThroughFeed(fmc::PackedQueries const& reads, fmc::MapQuery const& query) const { return fmc::Feed{index}.map(reads.unpack(), query); }

    template <typename Queries>
    fmc::MapResult mapAtOnce(Queries const& reads, fmc::MapQuery const& query) const {
        if constexpr (std::is_same_v<Queries, fmc::PackedQueries>) return fmc::map(index, reads, query);
        else return config.pairStrands ? fmc::map(index, reads, query, pairStrands()) : fmc::map(index, reads, query);
    }
    template <typename Queries>
    void oneErrorBudgetMapped(Algorithm kind, size_t k, Queries const& reads, size_t firstLength) const {
        StopWatch clock;
        fmc::MapQuery query;
        if (config.hitsPerRead != 0) query.maxResults = config.hitsPerRead;
        if (kind == Algorithm::ng26) {
            query.kind = fmc::MapQuery::Kind::Schemes;
            for (size_t j = 0; j <= k; ++j) query.schemes.emplace_back(schemeByName(config.schemeName, j, j), std::vector<size_t>{});
        } else if (kind == Algorithm::ng21) {
            query.kind = fmc::MapQuery::Kind::Ng21;
            for (size_t j = 0; j <= k; ++j) query.expanded.push_back(stretch(schemeByName(config.schemeName, j, j), firstLength));
        }
        if constexpr (!std::is_same_v<Queries, fmc::PackedQueries>) if (mateReads) return matesMapped(reads, query, k, clock);
        if constexpr (!std::is_same_v<Queries, fmc::PackedQueries>) if (config.chainSeeds) return seedsChained(reads, k, clock);
        auto const mapped = config.feed ? mapThroughFeed(reads, query) : mapAtOnce(reads, query);
        double const tMap = clock.reset();
        std::string sam;
        if constexpr (!std::is_same_v<Queries, fmc::PackedQueries>) if (config.sam && !config.outputFile.empty()) sam = samFile(mapped, reads, kind == Algorithm::noerror);
        reportMapped(mapped, (config.pairStrands ? 2 : 1) * reads.size(), k, tMap, sam);
    }

    // --mates: both files mapped as --mode map maps one, then the positions of the two mates of every fragment (read i of either file) joined on the device
    // (fmgpu_positions_mates through fmc::joinMates).  A batch with both strands counts 2 * read + strand, whether the reverse complements were made here (every read
    // followed by its reverse complement) or on the device (--pair-strands): concordant is FR then; with --no-reverse every strand is 0 and any order counts.
    // --save_output gets "fragment seqId posA strandA posB strandB tlen errors" per pair, written by a loop here.
    void matesMapped(std::vector<std::vector<uint8_t>> const& reads, fmc::MapQuery const& query, size_t k, StopWatch& clock) const {
        auto const first = mapAtOnce(reads, query);
        auto const second = mapAtOnce(*mateReads, query);
        double const tMap = clock.reset();
        bool const bothStrands = config.pairStrands || config.withReverseComplement, doubled = bothStrands && !config.pairStrands;
        auto forward = [&](std::vector<std::vector<uint8_t>> const& batch) {
            if (!doubled) return batch;
            std::vector<std::vector<uint8_t>> every;
            for (size_t i = 0; i < batch.size(); i += 2) every.push_back(batch[i]);
            return every;
        };
        fmc::MatesSpec spec;
        spec.strands = bothStrands;
        spec.orientation = bothStrands ? fmc::MatesSpec::Orientation::FR : fmc::MatesSpec::Orientation::Any;
        spec.minTlen = config.minTlen; spec.maxTlen = config.maxTlen;
        auto const joined = fmc::joinMates(first.positions, forward(reads), second.positions, forward(*mateReads), spec);
        double const tJoin = clock.reset();
        size_t const factor = config.pairStrands ? 2 : 1;
        printMapped(first, factor * reads.size(), k, tMap / 2);
        printMapped(second, factor * mateReads->size(), k, tMap / 2);
        size_t const paired = static_cast<size_t>(std::count(joined.classes.begin(), joined.classes.end(), uint8_t{4}));
        std::printf("%-15s %3zu: %10.3gs - pairs: %10zu in %10zu of %10zu fragments\n", "mates", k, tJoin, joined.pairs.size(), paired, joined.classes.size());
        if (config.outputFile.empty()) return;
        std::string sam;                                                // --paired-sam: two records per fragment, made on the device from the positions and the pairs
        if (config.pairedSam) {
            auto const strands = pairStrands();
            fmc::SamMatesSpec samSpec;
            if (bothStrands) samSpec.strands = &strands;
            samSpec.seqNames = &referenceNames;
            samSpec.cigar = query.kind == fmc::MapQuery::Kind::Exact;             // (the exact search is ungapped, as under --sam)
            auto recordsA = first.positions, recordsB = second.positions;
            for (auto* records : {&recordsA, &recordsB}) for (auto& p : *records) p.seq_id = static_cast<uint32_t>(p.seq_id);      // (what the other files print of it)
            sam = fmc::samHeader(referenceNames, referenceLengths, "fmindex-collection-gpu-example") +
                  fmc::formatSamMates(recordsA, forward(reads), recordsB, forward(*mateReads), joined, samSpec).text;
        }
        auto* out = std::fopen(config.outputFile.c_str(), "w");
        if (!out) throw std::runtime_error("cannot write " + config.outputFile);
        if (config.pairedSam) {
            bool const written = std::fwrite(sam.data(), 1, sam.size(), out) == sam.size();
            std::fclose(out);
            if (!written) throw std::runtime_error("cannot write " + config.outputFile);
            return;
        }
        for (auto const& p : joined.pairs) {
            auto const& a = first.positions[p.a];
            auto const& b = second.positions[p.b];
            std::fprintf(out, "%zu %zu %zu %c %zu %c %zu %zu\n", static_cast<size_t>(p.fragment), static_cast<size_t>(static_cast<uint32_t>(a.seq_id)), static_cast<size_t>(a.pos),
                         bothStrands && (a.qidx & 1) ? '-' : '+', static_cast<size_t>(b.pos), bothStrands && (b.qidx & 1) ? '-' : '+', static_cast<size_t>(p.tlen),
                         static_cast<size_t>(p.errors));
        }
        std::fclose(out);
    }

    // --chain-seeds: in place of the scheme search the seeds of every read (fmgpu_search_smems through fmc::search_smems: --min_seed, --max_seed_rows), located
    // (fmgpu_locate_hits) and joined to collinear chains on the device (fmgpu_seeds_chain through fmc::chainSeeds).  Every read of the batch is a query of its own,
    // a reverse complement too.  --save_output gets "qidx seq_id tbeg tend qbeg qend score n_anchors" per chain, in the call's output order.
    void seedsChained(std::vector<std::vector<uint8_t>> const& reads, size_t k, StopWatch& clock) const {
        std::vector<fmgpu_hit> seeds;
        std::vector<fmgpu_seed_span> spans;
        fmc::search_smems(index, reads, config.minSeed, config.maxSeedRows, [&](size_t read, auto const& cursor, size_t qbeg, size_t qlen) {
            fmgpu_hit h{};
            h.qidx = read; h.lb = cursor.lb; h.len = cursor.len;
            seeds.push_back(h);
            spans.push_back({static_cast<uint32_t>(qbeg), static_cast<uint32_t>(qlen)});
        });
        double const tSeeds = clock.reset();
        auto const anchors = index.locateHits(seeds);
        double const tLocate = clock.reset();
        fmc::ChainSpec spec;
        spec.queries = reads.size();
        spec.wantAnchors = config.alignChains;
        auto const chained = fmc::chainSeeds(anchors, spans, spec);
        double const tChain = clock.reset();
        // --align-chains: every chain aligned between its ends (fmgpu_chains_align through fmc::alignChains, the text read from the index); the lines of --save_output
        // gain "status n_match n_mismatch n_ins n_del cigar"
        fmc::ChainAlignments aligned;
        if (config.alignChains) aligned = fmc::alignChains(index, chained, anchors, spans, reads);
        double const tAlign = clock.reset();
        size_t const with = static_cast<size_t>(std::count(chained.classes.begin(), chained.classes.end(), uint8_t{1}));
        std::printf("%-15s %3zu: %10.3gs (%10.3gs +%10.3gs +%10.3gs ) - seeds: %10zu anchors: %10zu chains: %10zu in %10zu of %10zu queries\n", "chain-seeds", k,
                    tSeeds + tLocate + tChain, tSeeds, tLocate, tChain, seeds.size(), anchors.size(), chained.chains.size(), with, reads.size());
        if (config.alignChains) {
            size_t out = 0;
            for (auto const& r : aligned.alignments) out += r.status != 0;
            std::printf("%-15s %3zu: %10.3gs - chains: %10zu left out: %10zu operations: %10zu\n", "align-chains", k, tAlign, aligned.alignments.size(), out, aligned.ops.size());
        }
        if (config.outputFile.empty()) return;
        auto* out = std::fopen(config.outputFile.c_str(), "w");
        if (!out) throw std::runtime_error("cannot write " + config.outputFile);
        for (size_t i = 0; i < chained.chains.size(); ++i) {
            auto const& c = chained.chains[i];
            std::fprintf(out, "%zu %zu %zu %zu %zu %zu %zu %zu", static_cast<size_t>(c.qidx), static_cast<size_t>(static_cast<uint32_t>(c.seq_id)), static_cast<size_t>(c.tbeg),
                         static_cast<size_t>(c.tend), static_cast<size_t>(c.qbeg), static_cast<size_t>(c.qend), static_cast<size_t>(c.score), static_cast<size_t>(c.n_anchors));
            if (config.alignChains) {
                auto const& r = aligned.alignments[i];
                std::fprintf(out, " %zu %zu %zu %zu %zu %s", static_cast<size_t>(r.status), static_cast<size_t>(r.n_match), static_cast<size_t>(r.n_mismatch),
                             static_cast<size_t>(r.n_ins), static_cast<size_t>(r.n_del), aligned.cigar(i).c_str());
            }
            std::fputc('\n', out);
        }
        std::fclose(out);
    }

    // --mode map --feed --device-parse without reverse complements: the bytes of the query file go through the feed as they are (fmgpu_feed_map_text through
    // fmc::Feed::mapText): parsed and mapped on the device window by window, no read ever a vector on the host
    void oneErrorBudgetMappedText(Algorithm kind, size_t k, std::string const& text) const {
        StopWatch clock;
        fmc::MapQuery query;
        if (config.hitsPerRead != 0) query.maxResults = config.hitsPerRead;
        if (kind == Algorithm::ng26) {
            query.kind = fmc::MapQuery::Kind::Schemes;
            for (size_t j = 0; j <= k; ++j) query.schemes.emplace_back(schemeByName(config.schemeName, j, j), std::vector<size_t>{});
        }
        auto const table = Sigma == 6 ? fmc::SymbolTable::dna6(config.unknownToA) : fmc::SymbolTable::dna5(config.unknownToA);
        auto const format = text[0] == '@' ? fmc::TextFormat::Fastq : fmc::TextFormat::Fasta;
        auto const mapped = config.pairStrands ? fmc::Feed{index}.mapText(std::string_view{text}, format, table, query, pairStrands())
                                               : fmc::Feed{index}.mapText(std::string_view{text}, format, table, query);
        if (mapped.foreign > 0) throw std::runtime_error("unknown alphabet");
        double const tMap = clock.reset();
        std::string sam;                                                // (the records need the reads: the text is parsed once more)
        if (config.sam && !config.outputFile.empty()) sam = samFile(mapped, fmc::parseQueries(text, format, table), kind == Algorithm::noerror);
        reportMapped(mapped, (config.pairStrands ? 2 : 1) * mapped.size(), k, tMap, sam);
    }

    // --sam: the header and the records of the batch that was searched
    template <typename Queries>
    std::string samFile(fmc::MapResult const& mapped, Queries const& reads, bool ungapped) const {
        auto const strands = pairStrands();
        fmc::SamSpec spec;
        if (config.pairStrands) spec.strands = &strands;
        spec.seqNames = &referenceNames;
        spec.cigar = ungapped;
        auto records = mapped.positions;
        for (auto& p : records) p.seq_id = static_cast<uint32_t>(p.seq_id);           // (what the other files print of it)
        return fmc::samHeader(referenceNames, referenceLengths, "fmindex-collection-gpu-example") + fmc::formatSam(records, reads, spec).text;
    }

    void printMapped(fmc::MapResult const& mapped, size_t nreads, size_t k, double tMap) const {
        struct { size_t n; size_t size() const { return n; } } const reads{nreads};
        std::vector<Placement> distinct;
        distinct.reserve(mapped.positions.size());
        for (auto const& p : mapped.positions) distinct.push_back({static_cast<size_t>(p.qidx), static_cast<uint32_t>(p.seq_id), static_cast<size_t>(p.pos), p.errors});
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        std::unordered_set<size_t> readsWithHits;
        for (auto const& h : mapped.hits) readsWithHits.insert(config.pairStrands ? h.qidx / 2 : h.qidx > reads.size() / 2 ? h.qidx - reads.size() / 2 : h.qidx);
        std::printf("%-15s %3zu: %10.3gs (%10.3gs+%10.3gs) %10.3gq/s - results: %10zu/%10zu/%10zu/%10zu - mem: %13zu\n", "str", k, tMap, tMap, 0.0,
                    reads.size() / tMap, mapped.positions.size(), mapped.positions.size(), distinct.size(), readsWithHits.size(), size_t{0});
    }

    void reportMapped(fmc::MapResult const& mapped, size_t nreads, size_t k, double tMap, std::string const& sam = {}) const {
        printMapped(mapped, nreads, k, tMap);
        if (config.outputFile.empty()) return;
        auto* out = std::fopen(config.outputFile.c_str(), "w");
        if (!out) throw std::runtime_error("cannot write " + config.outputFile);
        if (config.sam) {
            if (std::fwrite(sam.data(), 1, sam.size(), out) != sam.size()) { std::fclose(out); throw std::runtime_error("cannot write " + config.outputFile); }
        } else if (config.deviceFormat) {                               // the same lines made on the device (the default FormatSpec: qidx seq_id pos errors)
            auto records = mapped.positions;
            for (auto& p : records) p.seq_id = static_cast<uint32_t>(p.seq_id);       // (what the loop below prints of it)
            auto const text = fmc::formatPositions(records);
            if (std::fwrite(text.data(), 1, text.size(), out) != text.size()) { std::fclose(out); throw std::runtime_error("cannot write " + config.outputFile); }
        } else {
            for (auto const& p : mapped.positions)
                std::fprintf(out, "%zu %zu %zu %zu\n", static_cast<size_t>(p.qidx), static_cast<size_t>(static_cast<uint32_t>(p.seq_id)), static_cast<size_t>(p.pos), static_cast<size_t>(p.errors));
        }
        std::fclose(out);
    }

    template <typename Queries>
    void oneErrorBudget(Algorithm kind, size_t k, Queries const& reads, size_t firstLength) const {
        if (config.hitMode == HitMode::map) return oneErrorBudgetMapped(kind, k, reads, firstLength);
        StopWatch clock;
        auto const hits = search(kind, k, reads, firstLength);
        double const tSearch = clock.reset();
        auto const placed = locate(hits);
        double const tLocate = clock.reset();

        auto distinct = placed;
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        std::unordered_set<size_t> readsWithHits;                  // a read and its reverse complement (second half of the batch) count once
        for (auto const& h : hits) readsWithHits.insert(h.read > reads.size() / 2 ? h.read - reads.size() / 2 : h.read);
        std::printf("%-15s %3zu: %10.3gs (%10.3gs+%10.3gs) %10.3gq/s - results: %10zu/%10zu/%10zu/%10zu - mem: %13zu\n", "str", k, tSearch + tLocate, tSearch, tLocate,
                    reads.size() / (tSearch + tLocate), placed.size(), placed.size(), distinct.size(), readsWithHits.size(), size_t{0});
        if (config.outputFile.empty()) return;
        auto* out = std::fopen(config.outputFile.c_str(), "w");
        if (!out) throw std::runtime_error("cannot write " + config.outputFile);
        for (auto const& p : placed) std::fprintf(out, "%zu %zu %zu\n", p.read, p.sequence, p.position);
        std::fclose(out);
    }
};

}  // namespace

int main(int argc, char const* const* argv) try {
    auto config = parseCommandLine(argc, argv);
    if (config.wantHelp) {
        std::printf("Usage:\n"
                    "./example --index somefile.fasta\n"
                    "   this will only build the index for somefile.fasta (on the GPU; nothing is written)\n"
                    "\n"
                    "./example --index somefile.fasta\\\n"
                    "          --query queryfile.fasta\\\n"
                    "          --algo [ng21, ng26, noerror]\\\n"
                    "          --gen <backtracking|pigeon|pigeon_opt|h2-k1|h2-k2|h2-k3>\\\n"
                    "          --queries <int> (maximal of number of queries)\\\n"
                    "          --read_length <int> (shorten all queries to this length)\\\n"
                    "          --save_output <file> (saves output at the end)\\\n"
                    "          --min_k <int> (minimal number of errors)\\\n"
                    "          --max_k <int> (maximal number of errors)\\\n"
                    "          --stepSize_k <int> (steps of errors)\\\n"
                    "          --no-reverse (don't use reverse compliment)\\\n"
                    "          --mode [all, besthits, map] (all: all hits with k errors (default), besthits: all hits with the lowest hit,\\\n"
                    "                 map: besthits as one search-order-locate call on the device; --save_output gets \"queryId seqId pos errors\")\\\n"
                    "          --packed (search the reads in the 4-bit packed form; reverse complements are made on the device)\\\n"
                    "          --feed (noerror, ng26, and every algorithm under --mode map: search through a feed, chunk by chunk)\\\n"
                    "          --device-parse (parse the query file on the device; FASTA or FASTQ by its first byte, '>' or '@'.  Same output on a\\\n"
                    "                 well-formed FASTA.  Unlike the default reader: \"\\r\\n\" ends a line, a '>' inside a line is an ordinary byte,\\\n"
                    "                 a last line without a newline keeps its last base, a name line at the end of the file is an empty read)\\\n"
                    "          --pair-strands (--mode map: reverse complements made on the device, best stratum per read: once either strand of a\\\n"
                    "                 read is found, neither is searched with more errors; queryId = 2 * read + strand)\\\n"
                    "          --device-format (--mode map: the --save_output file is formatted on the device; the same file, byte for byte)\\\n"
                    "          --sam (--mode map, not --packed: the --save_output file is a SAM file, the header and the records made on the device;\\\n"
                    "                 QNAME = the read's number in the searched batch, with --pair-strands one read for both strands)\\\n"
                    "          --mates <second queryfile> (--mode map, not --sam, --feed, --packed, --device-format or --queries: read i of the two files are\\\n"
                    "                 the mates of fragment i; both files are mapped and their positions joined on the device: --save_output gets\\\n"
                    "                 \"fragment seqId posA strandA posB strandB tlen errors\" per concordant pair (opposite strands, the forward mate\\\n"
                    "                 upstream; with --no-reverse any order))\\\n"
                    "          --paired-sam (only with --mates: the --save_output file is a paired-end SAM file, the header of --sam and two records per\\\n"
                    "                 fragment made on the device: the pair with the fewest errors where there is one, else each mate's best record)\\\n"
                    "          --min_tlen <int> --max_tlen <int> (--mates: the template lengths of a concordant pair, inclusive; 0 and 1000)\\\n"
                    "          --chain-seeds (--mode map, not --packed, --feed, --pair-strands, --device-format, --sam or --mates: in place of the scheme search\\\n"
                    "                 the seeds of every read are located and joined to collinear chains on the device: --save_output gets\\\n"
                    "                 \"qidx seq_id tbeg tend qbeg qend score n_anchors\" per chain)\\\n"
                    "          --align-chains (only with --chain-seeds: every chain aligned between its ends on the device; each line of --save_output gains\\\n"
                    "                 \"status n_match n_mismatch n_ins n_del cigar\")\\\n"
                    "          --min_seed <int> --max_seed_rows <int> (--chain-seeds: the shortest seed kept, the most rows of a kept seed; 19 and 50)\\\n"
                    "          --maxhitperquery <int> (some int, 0 = infinite hits)\n");
        return 0;
    }
    bool const needsFirstLength = std::any_of(config.algorithms.begin(), config.algorithms.end(), [](auto const& a) { return algorithmByName(a) == Algorithm::ng21; });
    if (config.pairStrands && (config.hitMode != HitMode::map || config.packed)) throw std::runtime_error("--pair-strands needs --mode map and byte reads (no --packed)");
    if (config.deviceFormat && config.hitMode != HitMode::map) throw std::runtime_error("--device-format needs --mode map");
    if (config.sam && (config.hitMode != HitMode::map || config.packed || config.deviceFormat)) throw std::runtime_error("--sam needs --mode map, byte reads (no --packed) and no --device-format");
    if (!config.matesFasta.empty() && config.hitMode != HitMode::map) throw std::runtime_error("--mates needs --mode map");
    if (!config.matesFasta.empty() && (config.sam || config.feed)) throw std::runtime_error("--mates does not go with --sam or --feed: pairs are joined from the positions of two whole batches");
    if (!config.matesFasta.empty() && (config.packed || config.deviceFormat || config.readLimit != 0)) throw std::runtime_error("--mates needs byte reads (no --packed), no --device-format and no --queries");
    if (config.pairedSam && config.matesFasta.empty()) throw std::runtime_error("--paired-sam needs --mates");
    if (config.minTlen > config.maxTlen) throw std::runtime_error("--min_tlen lies above --max_tlen");
    if (config.chainSeeds && config.hitMode != HitMode::map) throw std::runtime_error("--chain-seeds needs --mode map");
    if (config.alignChains && !config.chainSeeds) throw std::runtime_error("--align-chains needs --chain-seeds");
    if (config.chainSeeds && (config.packed || config.feed || config.pairStrands || config.deviceFormat || config.sam || !config.matesFasta.empty()))
        throw std::runtime_error("--chain-seeds needs byte reads (no --packed) and does not go with --feed, --pair-strands, --device-format, --sam or --mates");
    auto withReference = [&](Run& run) {                              // --sam: what the header and RNAME are made of
        if (!config.sam && !config.pairedSam) return;
        auto const reference = readFasta(config.referenceFasta, Sigma, config.unknownToA);
        run.referenceNames = fmc::NameTable{readFastaNames(config.referenceFasta)};
        for (auto const& s : reference) run.referenceLengths.push_back(s.size());
        if (run.referenceNames.spans.size() != run.referenceLengths.size()) throw std::runtime_error("--sam: the names and the sequences of --index do not pair up");
    };
    if (config.hitMode == HitMode::map && config.feed && config.deviceParse && (!config.withReverseComplement || config.pairStrands) && !config.packed && config.readLimit == 0 &&
        config.trimTo == 0 && !needsFirstLength && !config.readsFasta.empty() && std::filesystem::exists(config.readsFasta)) {
        std::ifstream in{config.readsFasta, std::ios::binary};
        std::string const text{std::istreambuf_iterator<char>{in}, std::istreambuf_iterator<char>{}};
        if (text.empty() || (text[0] != '>' && text[0] != '@')) throw std::runtime_error("can't read fasta file");
        std::printf("loaded %zu bytes of query text\n", text.size());
        Run run{config, openIndex(config)};
        withReference(run);
        for (auto const& algorithm : config.algorithms) {
            std::printf("using algorithm %s\n", algorithm.c_str());
            for (size_t k = config.firstK; k <= config.lastK; k += config.stepK) run.oneErrorBudgetMappedText(algorithmByName(algorithm), k, text);
        }
        return 0;
    }
    auto reads = config.deviceParse ? readQueriesOnDevice(config.readsFasta, Sigma, config.unknownToA) : readFasta(config.readsFasta, Sigma, config.unknownToA);
    // --packed: both strands come out of the device packer, unless reads get trimmed (the reference trims the doubled batch, and a trimmed reverse
    // complement is not the reverse complement of the trimmed read: then the strands are made here and only packed)
    bool const trims = config.trimTo != 0 && std::any_of(reads.begin(), reads.end(), [&](auto const& r) { return r.size() > config.trimTo; });
    bool const strandsOnDevice = (config.packed && config.withReverseComplement && !trims) || config.pairStrands;
    size_t const strands = strandsOnDevice ? 2 : 1;
    if (config.withReverseComplement && !strandsOnDevice) reads = withReverseComplements(reads);
    if (!reads.empty()) {
        std::printf("loaded %zu queries (incl reverse complements)\n", strands * reads.size());
        std::printf("%-15s: %10s  (%10s +%10s ) %10s    - results: %10s/%10s/%10s/%10s - mem: %13s\n", "name", "time_search + time_locate", "time_search",
                    "time_locate", "(time_search+time_locate)/queries.size()", "resultCt", "results.size()", "uniqueResults.size()", "readIds.size()", "memory");
    }
    Run run{config, openIndex(config)};
    withReference(run);
    size_t const limit = config.readLimit != 0 ? config.readLimit : std::numeric_limits<size_t>::max();     // (of the doubled batch)
    if (strands * reads.size() > limit) reads.resize((limit + strands - 1) / strands);
    if (config.trimTo != 0) for (auto& r : reads) if (r.size() > config.trimTo) r.resize(config.trimTo);
    std::vector<std::vector<uint8_t>> mates;
    if (!config.matesFasta.empty()) {
        if (!std::filesystem::exists(config.matesFasta)) throw std::runtime_error("--mates: no file " + config.matesFasta);
        mates = config.deviceParse ? readQueriesOnDevice(config.matesFasta, Sigma, config.unknownToA) : readFasta(config.matesFasta, Sigma, config.unknownToA);
        if (config.withReverseComplement && !strandsOnDevice) mates = withReverseComplements(mates);
        if (config.trimTo != 0) for (auto& r : mates) if (r.size() > config.trimTo) r.resize(config.trimTo);
        if (mates.size() != reads.size()) throw std::runtime_error("--mates: the two files do not hold the same number of reads");
        std::printf("loaded %zu mates (incl reverse complements)\n", strands * mates.size());
        run.mateReads = &mates;
    }
    fmc::PackedQueries packed;
    if (config.packed) {
        packed = strandsOnDevice ? fmc::PackedQueries::packOnDevice(reads, Sigma, {0, 4, 3, 2, 1}) : fmc::PackedQueries::pack(reads, Sigma);
        if (packed.size() > limit) packed.qoff.resize(limit + 1);      // (an odd limit ends the batch on a forward read)
    }
    for (auto const& algorithm : config.algorithms) {
        std::printf("using algorithm %s\n", algorithm.c_str());
        auto const kind = algorithmByName(algorithm);
        if (reads.empty()) continue;
        for (size_t k = config.firstK; k <= config.lastK; k += config.stepK) {
            if (config.packed) run.oneErrorBudget(kind, k, packed, reads[0].size());
            else run.oneErrorBudget(kind, k, reads, reads[0].size());
        }
    }
    return 0;
} catch (std::exception const& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
}
