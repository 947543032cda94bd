// Paired-end SAM records through include/fmc_gpu.hpp: the mirror struct and the argument checks of fmgpu_positions_sam_mates that come before the device (checked
// everywhere), then on a device fmc::formatSamMates against fixed lines: the worked example of include/fmgpu.h, the six situations of a fragment written by hand (the
// lines tests/test_sam_mates_host.py holds the model against), the same fragments as one interleaved batch, from vectors, from joinMates' result and from device
// memory.  Exit 77 without a device, after the host checks.
#include "../../include/fmc_gpu.hpp"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;

static fmgpu_position record(uint64_t qidx, uint64_t seq, uint64_t pos, uint32_t errors) {
    fmgpu_position p{};
    p.qidx = qidx; p.seq_id = seq; p.pos = pos; p.errors = errors;
    return p;
}
static fmgpu_mate_pair pairOf(uint64_t fragment, uint32_t a, uint32_t b) {
    fmgpu_mate_pair p{};
    p.fragment = fragment; p.a = a; p.b = b;                    // tlen, errors and flags are not read
    return p;
}

int main() {
    {   // the host mirror: no device needed
        static_assert(sizeof(fmgpu_sam_mates_spec) == 96, "the size include/fmgpu.h states");
        static_assert(offsetof(fmgpu_sam_mates_spec, qoff_a) == 8 && offsetof(fmgpu_sam_mates_spec, qbuf_b) == 16 && offsetof(fmgpu_sam_mates_spec, qoff_b) == 24 &&
                      offsetof(fmgpu_sam_mates_spec, n_fragments) == 32 && offsetof(fmgpu_sam_mates_spec, char_of) == 40 && offsetof(fmgpu_sam_mates_spec, strands) == 48 &&
                      offsetof(fmgpu_sam_mates_spec, read_names) == 56 && offsetof(fmgpu_sam_mates_spec, quals_a) == 64 && offsetof(fmgpu_sam_mates_spec, quals_b) == 72 &&
                      offsetof(fmgpu_sam_mates_spec, seq_names) == 80 && offsetof(fmgpu_sam_mates_spec, interleaved) == 88 && offsetof(fmgpu_sam_mates_spec, cigar) == 89 &&
                      offsetof(fmgpu_sam_mates_spec, strip_mate_suffix) == 90 && offsetof(fmgpu_sam_mates_spec, mapq_unique) == 91 &&
                      offsetof(fmgpu_sam_mates_spec, mapq_multi) == 92 && offsetof(fmgpu_sam_mates_spec, reserved) == 93, "field offsets");
        fmc::SamMatesSpec spec;
        CHECK(spec.cigar && spec.stripMateSuffix && spec.mapqUnique == 60 && spec.mapqMulti == 0 && !spec.strands && !spec.readNames && !spec.qualsA && !spec.qualsB && !spec.seqNames);
        // no fragment: no text, behind the checks
        CHECK(fmc::formatSamMates({}, Reads{}, {}, Reads{}, std::vector<fmgpu_mate_pair>{}).text.empty());
        auto const none = fmc::formatSamMates({}, Reads{}, fmc::MatePairs{}, {}, true);
        CHECK(none.text.empty() && none.lineOffsets == std::vector<uint64_t>{0});
        bool threw = false;
        try { (void)fmc::formatSamMates({}, Reads{{1}, {2}, {3}}, fmc::MatePairs{}); } catch (std::runtime_error const&) { threw = true; }      // an odd interleaved batch
        CHECK(threw);
        // the argument checks that come before the device
        std::vector<fmgpu_position> one(1);
        std::vector<fmgpu_mate_pair> pr(1);
        uint8_t const q[2] = {1, 2};
        uint64_t const off[2] = {0, 2};
        uint64_t bytes = 7;
        auto const chars = fmc::CharTable::dna5();
        fmgpu_sam_mates_spec s{};
        auto call = [&](fmgpu_position const* a, fmgpu_position const* b, fmgpu_mate_pair const* p, fmgpu_sam_mates_spec const* sp) {
            return fmgpu_positions_sam_mates(a, 1, b, b ? 1 : 0, p, 1, sp, nullptr, 0, &bytes, nullptr, nullptr);
        };
        CHECK(call(one.data(), one.data(), pr.data(), nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "spec is null"));
        CHECK(call(one.data(), one.data(), pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "char_of is null"));
        s.char_of = chars.map.data(); s.n_fragments = 1;
        CHECK(call(one.data(), one.data(), pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "qbuf_a is null"));
        s.qbuf_a = q; s.qoff_a = off;
        CHECK(call(one.data(), one.data(), pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "qbuf_b is null in separate mode"));
        s.qbuf_b = q; s.qoff_b = off;
        CHECK(call(nullptr, one.data(), pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "positions_a is null"));
        CHECK(call(one.data(), one.data(), nullptr, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "pairs is null"));
        s.interleaved = 1;
        CHECK(call(one.data(), nullptr, pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "must be null in interleaved mode"));
        s.interleaved = 0; s.strip_mate_suffix = 2;
        CHECK(call(one.data(), one.data(), pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "strip_mate_suffix"));
        s.strip_mate_suffix = 1; s.reserved[1] = 1;
        CHECK(call(one.data(), one.data(), pr.data(), &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "reserved"));
        CHECK(bytes == 7);
    }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return failures ? 1 : 77; }

    auto const strands = fmc::Strands::dna5(true);
    {   // the worked example of the header text
        fmc::SamMatesSpec spec;
        spec.strands = &strands;
        std::vector<fmgpu_position> const a{record(0, 0, 10, 0)}, b{record(1, 0, 50, 1)};
        auto const got = fmc::formatSamMates(a, Reads{{1, 2, 3, 4}}, b, Reads{{3, 3, 4, 1}}, std::vector<fmgpu_mate_pair>{pairOf(0, 0, 0)}, spec, true);
        std::string const lineA = "0\t99\t0\t11\t60\t4M\t=\t51\t44\tACGT\t*\tNM:i:0\tNH:i:1\n", lineB = "0\t147\t0\t51\t60\t4M\t=\t11\t-44\tTACC\t*\tNM:i:1\tNH:i:1\n";
        CHECK(got.text == lineA + lineB);
        CHECK((got.lineOffsets == std::vector<uint64_t>{0, lineA.size(), lineA.size() + lineB.size()}));
    }
    // six fragments, one per situation: a proper pair (the second pair record has fewer errors), both mates on chr2 without a pair, chr1 and chrM, only A (two equally
    // good records), only B, neither
    Reads const readsA{{1, 2, 3, 4}, {1, 1, 2}, {4, 4, 4, 1, 2}, {2, 3, 2}, {3, 3, 3, 1}, {1, 4}}, readsB{{3, 3, 4, 1, 1}, {2, 2, 2, 2}, {1, 2, 1}, {4, 1, 4, 1}, {2, 2, 1}, {4, 4, 4}};
    std::vector<std::string> const names{"f0/1 first", "f1/1", "f2/1", "f3/1", "f4/1\tx", "f5/1"}, qualsA{"ABCD", "EFG", "HIJKL", "MNO", "PQRS", "TU"},
                                   qualsB{"abcde", "fghi", "jkl", "mnop", "qrs", "tuv"}, seqs{"chr1 one", "chr2", "chrM"};
    std::vector<fmgpu_position> const recA{record(0, 0, 100, 1), record(0, 0, 400, 0), record(2, 1, 30, 0), record(5, 0, 7, 2), record(6, 2, 9, 0), record(7, 2, 90, 0)},
                                      recB{record(1, 0, 150, 1), record(1, 0, 460, 0), record(2, 1, 10, 1), record(4, 2, 7, 0), record(9, 1, 0, 3)};
    std::vector<fmgpu_mate_pair> const pairs{pairOf(0, 0, 0), pairOf(0, 1, 1)};
    std::vector<std::string> const six{"f0\t99\tchr1\t401\t60\t4M\t=\t461\t65\tACGT\tABCD\tNM:i:0\tNH:i:2\n",
                                       "f0\t147\tchr1\t461\t60\t5M\t=\t401\t-65\tTTACC\tedcba\tNM:i:0\tNH:i:2\n",
                                       "f1\t65\tchr2\t31\t60\t3M\t=\t11\t-23\tAAC\tEFG\tNM:i:0\tNH:i:1\n",
                                       "f1\t129\tchr2\t11\t60\t4M\t=\t31\t23\tCCCC\tfghi\tNM:i:1\tNH:i:1\n",
                                       "f2\t81\tchr1\t8\t60\t5M\tchrM\t8\t0\tGTAAA\tLKJIH\tNM:i:2\tNH:i:1\n",
                                       "f2\t161\tchrM\t8\t60\t3M\tchr1\t8\t0\tACA\tjkl\tNM:i:0\tNH:i:1\n",
                                       "f3\t73\tchrM\t10\t0\t3M\t=\t10\t0\tCGC\tMNO\tNM:i:0\tNH:i:2\n",
                                       "f3\t133\tchrM\t10\t0\t*\t=\t10\t0\tTATA\tmnop\n",
                                       "f4\t101\tchr2\t1\t0\t*\t=\t1\t0\tGGGA\tPQRS\n",
                                       "f4\t153\tchr2\t1\t60\t3M\t=\t1\t0\tTGG\tsrq\tNM:i:3\tNH:i:1\n",
                                       "f5\t77\t*\t0\t0\t*\t*\t0\t0\tAT\tTU\n",
                                       "f5\t141\t*\t0\t0\t*\t*\t0\t0\tTTT\ttuv\n"};
    std::string want;
    std::vector<uint64_t> offsets{0};
    for (auto const& line : six) { want += line; offsets.push_back(want.size()); }
    fmc::NameTable const rt{names}, qa{qualsA}, qb{qualsB}, nt{seqs};
    fmc::SamMatesSpec spec;
    spec.strands = &strands; spec.readNames = &rt; spec.qualsA = &qa; spec.qualsB = &qb; spec.seqNames = &nt;
    {
        auto const got = fmc::formatSamMates(recA, readsA, recB, readsB, pairs, spec, true);
        CHECK(got.text == want);
        CHECK(got.lineOffsets == offsets);
        fmc::MatePairs joined;                                  // what joinMates returns: its pairs are taken
        joined.pairs = pairs;
        CHECK(fmc::formatSamMates(recA, readsA, recB, readsB, joined, spec).text == want);
    }
    {   // the records and the pairs in device memory
        void *da = nullptr, *db = nullptr, *dp = nullptr;
        CHECK(fmgpu_malloc(&da, recA.size() * sizeof recA[0]) == 0 && fmgpu_malloc(&db, recB.size() * sizeof recB[0]) == 0 && fmgpu_malloc(&dp, pairs.size() * sizeof pairs[0]) == 0);
        CHECK(fmgpu_memcpy_h2d(da, recA.data(), recA.size() * sizeof recA[0]) == 0 && fmgpu_memcpy_h2d(db, recB.data(), recB.size() * sizeof recB[0]) == 0 &&
              fmgpu_memcpy_h2d(dp, pairs.data(), pairs.size() * sizeof pairs[0]) == 0);
        auto const got = fmc::formatSamMates(fmc::ArrayView<fmgpu_position>{static_cast<fmgpu_position const*>(da), recA.size()}, readsA,
                                             fmc::ArrayView<fmgpu_position>{static_cast<fmgpu_position const*>(db), recB.size()}, readsB,
                                             fmc::ArrayView<fmgpu_mate_pair>{static_cast<fmgpu_mate_pair const*>(dp), pairs.size()}, spec);
        CHECK(got.text == want);
        fmgpu_free(da); fmgpu_free(db); fmgpu_free(dp);
    }
    {   // the same fragments as one interleaved batch: reads 2f and 2f + 1, every index into the one array; the names and qualities of both mates in one table each
        Reads reads;
        std::vector<std::string> names2, quals2;
        for (size_t f = 0; f < 6; ++f) { reads.push_back(readsA[f]); reads.push_back(readsB[f]); names2.push_back(names[f]); names2.push_back("mate2"); quals2.push_back(qualsA[f]); quals2.push_back(qualsB[f]); }
        std::vector<fmgpu_position> rec;
        std::vector<uint32_t> newA, newB;
        size_t ia = 0, ib = 0;
        for (uint64_t read = 0; read < 12; ++read) {
            auto const& from = read % 2 ? recB : recA;
            size_t& i = read % 2 ? ib : ia;
            for (; i < from.size() && (from[i].qidx >> 1) == read / 2; ++i) {
                (read % 2 ? newB : newA).push_back(static_cast<uint32_t>(rec.size()));
                rec.push_back(record(2 * read + (from[i].qidx & 1), from[i].seq_id, from[i].pos, from[i].errors));
            }
        }
        std::vector<fmgpu_mate_pair> both;
        for (auto const& p : pairs) both.push_back(pairOf(p.fragment, newA[p.a], newB[p.b]));
        fmc::NameTable const rt2{names2}, q2{quals2};
        fmc::SamMatesSpec one = spec;
        one.readNames = &rt2; one.qualsA = &q2; one.qualsB = nullptr;
        auto const got = fmc::formatSamMates(rec, reads, both, one, true);
        CHECK(got.text == want);
        CHECK(got.lineOffsets == offsets);
    }
    {   // a pair that names a record of another fragment is refused with its index; the next call succeeds
        auto bad = pairs;
        bad.push_back(pairOf(1, 0, 2));
        bool threw = false;
        try { (void)fmc::formatSamMates(recA, readsA, recB, readsB, bad, spec); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "pair 2 ") != nullptr; }
        CHECK(threw);
        CHECK(fmc::formatSamMates(recA, readsA, recB, readsB, pairs, spec).text == want);
    }

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
