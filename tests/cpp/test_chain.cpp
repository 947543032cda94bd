// Seed chains through include/fmc_gpu.hpp: the two mirror structs and the argument checks of fmgpu_seeds_chain that come before the device (checked everywhere),
// then on a device fmc::chainSeeds against the cases tests/test_chain_cpp.py wrote out with the plain-Python model (tests/chain_model.py): argv[1] names the file.
// Exit 77 without a device, after the host checks.
#include "../../include/fmc_gpu.hpp"

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <fstream>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main(int argc, char** argv) {
    {   // the host mirror: no device needed
        static_assert(sizeof(fmgpu_chain) == 56 && offsetof(fmgpu_chain, seq_id) == 8 && offsetof(fmgpu_chain, tbeg) == 16 && offsetof(fmgpu_chain, tend) == 24 &&
                      offsetof(fmgpu_chain, qbeg) == 32 && offsetof(fmgpu_chain, qend) == 36 && offsetof(fmgpu_chain, score) == 40 && offsetof(fmgpu_chain, n_anchors) == 44 &&
                      offsetof(fmgpu_chain, first) == 48 && offsetof(fmgpu_chain, flags) == 52, "the record include/fmgpu.h states");
        static_assert(sizeof(fmgpu_chain_spec) == 48 && offsetof(fmgpu_chain_spec, max_gap) == 8 && offsetof(fmgpu_chain_spec, max_skew) == 12 &&
                      offsetof(fmgpu_chain_spec, gap_cost_q8) == 16 && offsetof(fmgpu_chain_spec, max_lookback) == 20 && offsetof(fmgpu_chain_spec, min_score) == 24 &&
                      offsetof(fmgpu_chain_spec, min_anchors) == 28 && offsetof(fmgpu_chain_spec, max_chains) == 32 && offsetof(fmgpu_chain_spec, max_anchors) == 36 &&
                      offsetof(fmgpu_chain_spec, reserved) == 40, "field offsets");
        fmc::ChainSpec spec;
        CHECK(spec.queries == 0 && spec.maxGap == 5000 && spec.maxSkew == 500 && spec.gapCost == 0.5 && spec.maxLookback == 64 && spec.minScore == 0 &&
              spec.minAnchors == 1 && spec.maxChains == 0 && spec.maxAnchors == 0 && spec.wantAnchors);
        // no query, no anchor: nothing
        auto none = fmc::chainSeeds({}, {}, spec);
        CHECK(none.chains.empty() && none.classes.empty() && none.anchors.empty() && none.offsets == std::vector<uint64_t>{0});
        spec.queries = 3;
        none = fmc::chainSeeds({}, {}, spec);
        CHECK(none.chains.empty() && none.classes == std::vector<uint8_t>(3, 0) && none.offsets == std::vector<uint64_t>(4, 0));
        // what the mirror and the call refuse before the device
        std::vector<fmgpu_position> one(1);
        std::vector<fmgpu_seed_span> span(1);
        for (int bad = 0; bad < 4; ++bad) {
            fmc::ChainSpec s;
            s.queries = 1;
            if (bad == 0) s.maxGap = 0;
            if (bad == 1) s.maxSkew = 0x80000000u;
            if (bad == 2) s.maxLookback = 257;
            if (bad == 3) s.gapCost = 256.5;
            bool threw = false;
            try { (void)fmc::chainSeeds(one, span, s); } catch (std::runtime_error const&) { threw = true; }
            CHECK(threw);
        }
        uint64_t count = 7;
        fmgpu_chain_spec s{};
        s.nq = 1; s.max_gap = 1; s.max_skew = 1; s.max_lookback = 1;
        CHECK(fmgpu_seeds_chain(one.data(), 1, span.data(), 1, nullptr, nullptr, 0, &count, nullptr, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID &&
              std::strstr(fmgpu_last_error(), "spec is null"));
        CHECK(fmgpu_seeds_chain(nullptr, 1, span.data(), 1, &s, nullptr, 0, &count, nullptr, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID &&
              std::strstr(fmgpu_last_error(), "positions is null"));
        CHECK(fmgpu_seeds_chain(one.data(), 1, nullptr, 1, &s, nullptr, 0, &count, nullptr, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID &&
              std::strstr(fmgpu_last_error(), "spans is null"));
        s.reserved[7] = 1;
        CHECK(fmgpu_seeds_chain(one.data(), 1, span.data(), 1, &s, nullptr, 0, &count, nullptr, nullptr, nullptr, nullptr) == FMGPU_ERR_INVALID &&
              std::strstr(fmgpu_last_error(), "reserved"));
    }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return failures ? 1 : 77; }
    if (argc < 2) { std::printf("FAILED: no case file\n"); return 1; }

    std::ifstream in(argv[1]);
    size_t cases = 0, chains_seen = 0;
    in >> cases;
    CHECK(in.good() && cases > 0);
    for (size_t c = 0; c < cases && in.good(); ++c) {
        fmc::ChainSpec spec;
        uint64_t count = 0, n_spans = 0, q8 = 0, n = 0;
        in >> spec.queries >> count >> n_spans >> spec.maxGap >> spec.maxSkew >> q8 >> spec.maxLookback >> spec.minScore >> spec.minAnchors >> spec.maxChains >> spec.maxAnchors;
        spec.gapCost = static_cast<double>(q8) / 256.0;
        std::vector<fmgpu_position> positions(count);
        std::vector<fmgpu_seed_span> spans(n_spans);
        for (auto& p : positions) { in >> p.qidx >> p.seq_id >> p.pos >> p.hit; p.errors = 3; }
        for (auto& s : spans) in >> s.qbeg >> s.qlen;
        fmc::SeedChains want;
        in >> n;
        want.chains.resize(n);
        for (auto& k : want.chains) in >> k.qidx >> k.seq_id >> k.tbeg >> k.tend >> k.qbeg >> k.qend >> k.score >> k.n_anchors >> k.first >> k.flags;
        want.offsets.resize(spec.queries + 1);
        for (auto& o : want.offsets) in >> o;
        want.classes.resize(spec.queries);
        for (auto& k : want.classes) { unsigned v = 0; in >> v; k = static_cast<uint8_t>(v); }
        in >> n;
        want.anchors.resize(n);
        for (auto& a : want.anchors) in >> a;
        CHECK(!in.fail());
        auto const got = fmc::chainSeeds(positions, spans, spec);
        CHECK(got.offsets == want.offsets && got.classes == want.classes && got.anchors == want.anchors && got.chains.size() == want.chains.size());
        CHECK(got.chains.size() == want.chains.size() && (want.chains.empty() || std::memcmp(got.chains.data(), want.chains.data(), want.chains.size() * sizeof(fmgpu_chain)) == 0));
        spec.wantAnchors = false;
        CHECK(fmc::chainSeeds(positions, spans, spec).anchors.empty());
        chains_seen += want.chains.size();
        if (c == 0 && count > 2) {   // a query beyond the batch: the lowest offending record is named; the next call succeeds
            auto bad = positions;
            bad[count - 1].qidx = spec.queries; bad[count - 2].qidx = spec.queries + 5;
            bool threw = false;
            try { (void)fmc::chainSeeds(bad, spans, spec); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), ("record " + std::to_string(count - 2) + " ").c_str()) != nullptr; }
            CHECK(threw);
            CHECK(fmc::chainSeeds(positions, spans, spec).offsets == want.offsets);
        }
    }
    CHECK(chains_seen > 100);

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
