// fmc::reconstructText (utils.h:672-703) and index.extract on top of fmgpu_extract (include/fmc_gpu.hpp), against the sequences the index was built from.
// Needs a GPU; exit code 0 = all checks passed, 77 = no GPU (host-only compile check).
#include "../../include/fmc_gpu.hpp"

#include <cstdio>
#include <random>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static std::vector<std::vector<uint8_t>> makeSeqs(size_t count, size_t sigma, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<std::vector<uint8_t>> seqs;
    for (size_t i = 0; i < count; ++i) {
        size_t len = i == 0 ? 0 : i == 1 ? 5000 : rng() % 300;
        std::vector<uint8_t> s(len);
        for (auto& c : s) c = static_cast<uint8_t>(1 + rng() % (sigma - 1));
        seqs.push_back(s);
    }
    return seqs;
}

template <typename Index>
static void check(Index& index, std::vector<std::vector<uint8_t>> const& seqs, uint32_t seed) {
    CHECK(fmc::reconstructText(index) == seqs);
    for (size_t r = 0; r < seqs.size(); r += 37) {                              // sentinel row r: the text of the sequence its delimiter ends (one per sequence)
        auto [seqId, pos, steps] = index.locate(r);
        CHECK(pos + steps == seqs[seqId].size());
        CHECK(fmc::reconstructText(index, r) == seqs[seqId]);
    }
    index.accelerateExtract();
    std::mt19937 rng(seed);
    std::vector<fmgpu_text_range> ranges;
    std::vector<uint8_t> want;
    for (size_t k = 0; k < 2000; ++k) {
        size_t s = rng() % seqs.size(), len = seqs[s].size();
        size_t a = rng() % (len + 1), b = rng() % (len + 1);
        if (a > b) std::swap(a, b);
        ranges.push_back(fmgpu_text_range{s, a, b - a});
        want.insert(want.end(), seqs[s].begin() + a, seqs[s].begin() + b);
    }
    CHECK(index.extract(ranges) == want);
    CHECK(index.extract({}).empty());
    CHECK(fmc::reconstructText(index) == seqs);                                // with the table kept
    index.accelerateExtract(false);
}

int main() {
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("No GPU: compiled only\n"); return 77; }
    {
        auto const seqs = makeSeqs(200, 5, 3);
        auto index = fmc::BiFMIndex<5, fmc::string::InterleavedBitvector16>{seqs, 16, 1};
        check(index, seqs, 1);
    }
    {
        auto const seqs = makeSeqs(100, 21, 4);
        auto index = fmc::FMIndex<21, fmc::string::Wavelet>{seqs, 4, 1};
        check(index, seqs, 2);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
