// Paired-end mates through include/fmc_gpu.hpp: the two mirror structs and the argument checks of fmgpu_positions_mates that come before the device (checked
// everywhere), then on a device fmc::joinMates against a host double loop: separate batches and the interleaved one, both orientations, best, maxRecords, a fragment
// with hundreds of records per mate.  Exit 77 without a device, after the host checks.
#include "../../include/fmc_gpu.hpp"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <random>
#include <tuple>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

using Reads = std::vector<std::vector<uint8_t>>;
using Positions = std::vector<fmgpu_position>;

// the same contract as a caller's own loops would write it: every record of mate A against every record of mate B
static fmc::MatePairs hostJoin(Positions const& a, Reads const& readsA, Positions const& b, Reads const& readsB, fmc::MatesSpec const& spec, bool interleaved) {
    unsigned const shift = spec.strands ? 1 : 0;
    size_t const n = interleaved ? readsA.size() / 2 : readsA.size();
    auto run = [&](Positions const& p, size_t read) {
        auto const lo = std::partition_point(p.begin(), p.end(), [&](fmgpu_position const& x) { return (x.qidx >> shift) < read; });
        auto const hi = std::partition_point(p.begin(), p.end(), [&](fmgpu_position const& x) { return (x.qidx >> shift) <= read; });
        return std::pair<size_t, size_t>{lo - p.begin(), hi - p.begin()};
    };
    fmc::MatePairs out;
    for (size_t f = 0; f < n; ++f) {
        out.offsets.push_back(out.pairs.size());
        size_t const ra = interleaved ? 2 * f : f, rb = interleaved ? 2 * f + 1 : f;
        auto const [a0, a1] = run(a, ra);
        auto const [b0, b1] = run(b, rb);
        if (a0 == a1 || b0 == b1) { out.classes.push_back(a0 == a1 && b0 == b1 ? 0 : b0 == b1 ? 1 : 2); continue; }
        if (spec.maxRecords && (a1 - a0 > spec.maxRecords || b1 - b0 > spec.maxRecords)) { out.classes.push_back(5); continue; }
        uint64_t const ma = readsA[ra].size(), mb = readsB[rb].size();
        std::vector<fmgpu_mate_pair> found;
        for (size_t i = a0; i < a1; ++i) {
            std::vector<std::tuple<uint64_t, size_t, fmgpu_mate_pair>> mine;
            for (size_t j = b0; j < b1; ++j) {
                uint64_t const pa = a[i].pos, pb = b[j].pos, ea = pa + ma, eb = pb + mb, sa = shift ? a[i].qidx & 1 : 0, sb = shift ? b[j].qidx & 1 : 0;
                uint64_t const tlen = std::max(ea, eb) - std::min(pa, pb);
                if (a[i].seq_id != b[j].seq_id || tlen < spec.minTlen || tlen > spec.maxTlen) continue;
                if (spec.orientation == fmc::MatesSpec::Orientation::FR) {
                    if (sa == sb) continue;
                    uint64_t const pf = sa ? pb : pa, ef = sa ? eb : ea, pr = sa ? pa : pb, er = sa ? ea : eb;
                    if (pf > pr || ef > er) continue;
                }
                mine.emplace_back(pb, j, fmgpu_mate_pair{f, tlen, static_cast<uint32_t>(i), static_cast<uint32_t>(j), a[i].errors + b[j].errors, pa <= pb ? 1u : 0u});
            }
            std::sort(mine.begin(), mine.end(), [](auto const& x, auto const& y) { return std::tie(std::get<0>(x), std::get<1>(x)) < std::tie(std::get<0>(y), std::get<1>(y)); });
            for (auto const& m : mine) found.push_back(std::get<2>(m));
        }
        if (spec.best && !found.empty()) {
            uint32_t least = UINT32_MAX;
            for (auto const& p : found) least = std::min(least, p.errors);
            found.erase(std::remove_if(found.begin(), found.end(), [&](fmgpu_mate_pair const& p) { return p.errors != least; }), found.end());
        }
        out.classes.push_back(found.empty() ? 3 : 4);
        out.pairs.insert(out.pairs.end(), found.begin(), found.end());
    }
    out.offsets.push_back(out.pairs.size());
    return out;
}

static bool same(fmc::MatePairs const& x, fmc::MatePairs const& y) {
    return x.offsets == y.offsets && x.classes == y.classes && x.pairs.size() == y.pairs.size() &&
           (x.pairs.empty() || std::memcmp(x.pairs.data(), y.pairs.data(), x.pairs.size() * sizeof(fmgpu_mate_pair)) == 0);
}

int main() {
    {   // the host mirror: no device needed
        static_assert(sizeof(fmgpu_mate_pair) == 32 && offsetof(fmgpu_mate_pair, tlen) == 8 && offsetof(fmgpu_mate_pair, a) == 16 && offsetof(fmgpu_mate_pair, b) == 20 &&
                      offsetof(fmgpu_mate_pair, errors) == 24 && offsetof(fmgpu_mate_pair, flags) == 28, "the record include/fmgpu.h states");
        static_assert(sizeof(fmgpu_mates_spec) == 56 && offsetof(fmgpu_mates_spec, qoff_b) == 8 && offsetof(fmgpu_mates_spec, n_fragments) == 16 &&
                      offsetof(fmgpu_mates_spec, min_tlen) == 24 && offsetof(fmgpu_mates_spec, max_tlen) == 32 && offsetof(fmgpu_mates_spec, max_records) == 40 &&
                      offsetof(fmgpu_mates_spec, strand_shift) == 48 && offsetof(fmgpu_mates_spec, interleaved) == 49 && offsetof(fmgpu_mates_spec, orientation) == 50 &&
                      offsetof(fmgpu_mates_spec, best) == 51 && offsetof(fmgpu_mates_spec, reserved) == 52, "field offsets");
        fmc::MatesSpec spec;
        CHECK(spec.strands && spec.orientation == fmc::MatesSpec::Orientation::FR && spec.minTlen == 0 && spec.maxTlen == 1000 && !spec.best && spec.maxRecords == 0);
        // no fragment: nothing, before anything else is looked at
        auto const none = fmc::joinMates({}, Reads{}, {}, Reads{});
        CHECK(none.pairs.empty() && none.classes.empty() && none.offsets == std::vector<uint64_t>{0});
        CHECK(fmc::joinMates({}, Reads{}).offsets == std::vector<uint64_t>{0});
        bool threw = false;
        try { (void)fmc::joinMates({}, Reads{{1}}, {}, Reads{}); } catch (std::runtime_error const&) { threw = true; }
        CHECK(threw);
        threw = false;
        try { (void)fmc::joinMates({}, Reads{{1}, {2}, {3}}); } catch (std::runtime_error const&) { threw = true; }
        CHECK(threw);
        // the argument checks that come before the device
        Positions one(1);
        uint64_t const off[2] = {0, 2};
        uint64_t count = 7;
        fmgpu_mates_spec s{};
        s.n_fragments = 1;
        auto call = [&](fmgpu_position const* pa, fmgpu_position const* pb, uint64_t cb, fmgpu_mates_spec const* sp) {
            return fmgpu_positions_mates(pa, 1, pb, cb, sp, nullptr, 0, &count, nullptr, nullptr, nullptr);
        };
        CHECK(call(one.data(), one.data(), 1, nullptr) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "spec is null"));
        CHECK(call(one.data(), one.data(), 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "qoff_a is null"));
        s.qoff_a = off;
        CHECK(call(one.data(), one.data(), 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "qoff_b is null in separate mode"));
        s.qoff_b = off; s.interleaved = 1;
        CHECK(call(one.data(), nullptr, 0, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "qoff_b must be null"));
        s.interleaved = 0; s.orientation = 2;
        CHECK(call(one.data(), one.data(), 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "orientation"));
        s.orientation = 0; s.min_tlen = 2; s.max_tlen = 1;
        CHECK(call(one.data(), one.data(), 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "min_tlen"));
        s.min_tlen = 0; s.reserved[3] = 1;
        CHECK(call(one.data(), one.data(), 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "reserved"));
        s.reserved[3] = 0;
        CHECK(call(nullptr, one.data(), 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "positions_a is null"));
        CHECK(call(one.data(), nullptr, 1, &s) == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), "positions_b is null"));
    }
    int ndev = 0;
    if (fmgpu_device_count(&ndev) != 0 || ndev == 0) { std::printf("no device\n"); return failures ? 1 : 77; }

    std::mt19937_64 rng(31);
    size_t const n = 300;
    Reads readsA, readsB, readsI;
    Positions a, b, both;
    for (size_t f = 0; f < n; ++f) {
        readsA.emplace_back(30 + rng() % 120, uint8_t{1});
        readsB.emplace_back(30 + rng() % 120, uint8_t{2});
        readsI.push_back(readsA.back()); readsI.push_back(readsB.back());
        for (int mate = 0; mate < 2; ++mate) {
            size_t const records = f % 7 == static_cast<size_t>(mate) ? 0 : f == 150 ? 400 : 1 + rng() % 4;
            for (size_t k = 0; k < records; ++k) {
                fmgpu_position p{};
                uint64_t const strand = rng() % 2;
                p.qidx = 2 * f + strand; p.seq_id = rng() % 2; p.pos = (f % 3 ? 0 : uint64_t{1} << 33) + rng() % 1500; p.errors = static_cast<uint32_t>(rng() % 3);
                (mate ? b : a).push_back(p);
                p.qidx = 2 * (2 * f + mate) + strand;
                both.push_back(p);
            }
        }
    }
    for (int variant = 0; variant < 5; ++variant) {
        fmc::MatesSpec spec;
        spec.orientation = variant % 2 ? fmc::MatesSpec::Orientation::Any : fmc::MatesSpec::Orientation::FR;
        spec.best = variant == 2 || variant == 3;
        spec.maxRecords = variant == 4 ? 3 : 0;
        spec.minTlen = variant == 1 ? 200 : 0; spec.maxTlen = variant == 1 ? 700 : 1000;
        auto const want = hostJoin(a, readsA, b, readsB, spec, false);
        auto const got = fmc::joinMates(a, readsA, b, readsB, spec);
        CHECK(same(got, want));
        CHECK(variant == 4 ? want.classes[150] == 5 : !want.pairs.empty());
        CHECK(same(fmc::joinMates(both, readsI, spec), hostJoin(both, readsI, both, readsI, spec, true)));
    }
    {   // without strands FR finds nothing and Any pairs; no record on one side
        Positions pa(a.begin(), a.begin() + 100), pb(b.begin(), b.begin() + 100);
        for (auto& p : pa) p.qidx >>= 1;
        for (auto& p : pb) p.qidx >>= 1;
        fmc::MatesSpec spec;
        spec.strands = false;
        CHECK(fmc::joinMates(pa, readsA, pb, readsB, spec).pairs.empty());
        spec.orientation = fmc::MatesSpec::Orientation::Any;
        auto const want = hostJoin(pa, readsA, pb, readsB, spec, false);
        CHECK(!want.pairs.empty() && same(fmc::joinMates(pa, readsA, pb, readsB, spec), want));
        CHECK(same(fmc::joinMates({}, readsA, pb, readsB, spec), hostJoin({}, readsA, pb, readsB, spec, false)));
        CHECK(same(fmc::joinMates(pa, readsA, {}, readsB, spec), hostJoin(pa, readsA, {}, readsB, spec, false)));
    }
    {   // a read beyond the batch, a read out of order: the array and the lowest offending record are named; the next call succeeds
        auto bad = b;
        bad[500].qidx = 2 * n; bad[200].qidx = 2 * n + 5;
        bool threw = false;
        try { (void)fmc::joinMates(a, readsA, bad, readsB); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "positions_b: record 200 ") != nullptr; }
        CHECK(threw);
        bad = a; bad[300].qidx = 0;
        threw = false;
        try { (void)fmc::joinMates(bad, readsA, b, readsB); } catch (std::runtime_error const& e) { threw = std::strstr(e.what(), "positions_a: record 300 ") != nullptr; }
        CHECK(threw);
        CHECK(same(fmc::joinMates(a, readsA, b, readsB), hostJoin(a, readsA, b, readsB, {}, false)));
    }

    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
