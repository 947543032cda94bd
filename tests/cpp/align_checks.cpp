// The paths of fmgpu_chains_align that return before the first device call, as a stand-alone program for a sanitizer build of the host side of
// fmindex-collection_amd/csrc/fmgpu_align.hip (the program's own copy of the call is the one that runs; the helpers it calls come from libfmgpu.so):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         fmindex-collection_amd/csrc/fmgpu_align.hip tests/cpp/align_checks.cpp -o align_checks -fsanitize=address,undefined \
//         -Lfmindex-collection_amd -lfmgpu -Wl,-rpath,$PWD/fmindex-collection_amd && ./align_checks
// It needs no device and is never loaded into another process.  tests/test_align_cpp.py builds and runs it.
#include "../../include/fmgpu.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool refused(int rc, const char* word) { return rc == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), word) != nullptr; }

int main() {
    std::vector<fmgpu_chain> chains(2);
    std::vector<uint32_t> anchors(2, 0);
    std::vector<fmgpu_position> rec(2);
    std::vector<fmgpu_seed_span> spans(2);
    std::vector<uint8_t> q(8, 1), t(8, 1);
    std::vector<uint64_t> qoff(3, 0), toff(3, 0);
    std::vector<fmgpu_chain_alignment> out(2);
    std::memset(out.data(), 0xAA, out.size() * sizeof(fmgpu_chain_alignment));
    std::vector<uint32_t> ops(4, 0xAAAAAAAAu);
    uint64_t n = 7;
    auto spec = []() {
        fmgpu_align_spec s{};
        s.nq = 2; s.band = 64; s.max_gap_len = 5000; s.max_cells = uint64_t{1} << 24;
        return s;
    };
    // which: the array handed in as null (-1: none)
    auto call = [&](const fmgpu_align_spec* s, int which = -1, uint64_t n_chains = 2, uint64_t n_anchor = 2, uint64_t count = 2, uint64_t n_spans = 2) {
        return fmgpu_chains_align(which == 0 ? nullptr : chains.data(), n_chains, which == 1 ? nullptr : anchors.data(), n_anchor, which == 2 ? nullptr : rec.data(), count,
                                  which == 3 ? nullptr : spans.data(), n_spans, which == 4 ? nullptr : q.data(), which == 5 ? nullptr : qoff.data(),
                                  which == 6 ? nullptr : t.data(), which == 7 ? nullptr : toff.data(), s, which == 8 ? nullptr : out.data(), which == 9 ? nullptr : ops.data(), 4,
                                  &n, nullptr);
    };
    fmgpu_align_spec good = spec(), s;

    CHECK(refused(call(nullptr), "spec is null"));
    CHECK(refused(fmgpu_chains_align(chains.data(), 2, anchors.data(), 2, rec.data(), 2, spans.data(), 2, q.data(), qoff.data(), t.data(), toff.data(), &good, out.data(),
                                     ops.data(), 4, nullptr, nullptr), "out_ops_count is null"));
    for (uint32_t bad : {65536u, 0x80000000u, 0xffffffffu}) {
        s = good; s.band = bad; CHECK(refused(call(&s), "band must lie in 0 .. 65535"));
        s = good; s.max_gap_len = bad; CHECK(refused(call(&s), "max_gap_len must lie in 0 .. 65535"));
    }
    for (uint64_t bad : {uint64_t{0}, (uint64_t{1} << 30) + 1, ~uint64_t{0}}) { s = good; s.max_cells = bad; CHECK(refused(call(&s), "max_cells must lie in 1 .. 2^30")); }
    for (int k = 0; k < 8; ++k) { s = good; s.reserved[k] = 1; CHECK(refused(call(&s), "reserved must be 0")); }
    const char* const names[9] = {"chains", "anchors", "positions", "spans", "qbuf", "qoff", "tbuf", "toff", "out"};
    for (int k = 0; k < 9; ++k) CHECK(refused(call(&good, k), (std::string(names[k]) + " is null while n_chains > 0").c_str()));
    CHECK(refused(call(&good, 9), "out_ops is null while ops_capacity > 0"));
    for (int k = 0; k < 4; ++k) {
        uint64_t counts[4] = {2, 2, 2, 2};
        counts[k] = k % 2 ? uint64_t{1} << 40 : (uint64_t{1} << 32) - 256;
        n = 7;
        CHECK(call(&good, -1, counts[0], counts[1], counts[2], counts[3]) == FMGPU_ERR_UNSUPPORTED && n == 0 && std::strstr(fmgpu_last_error(), "2^32 - 256") != nullptr);
    }
    // the accepted ends of every range, without a chain: nothing to do, nothing written, and null arrays are fine
    s = good; s.nq = 0; s.band = 0; s.max_gap_len = 0; s.max_cells = 1;
    n = 7;
    CHECK(call(&s, -1, 0) == 0 && n == 0);
    s = good; s.band = 65535; s.max_gap_len = 65535; s.max_cells = uint64_t{1} << 30;
    n = 7;
    CHECK(fmgpu_chains_align(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &s, nullptr, nullptr, 0, &n, nullptr) == 0 && n == 0);
    s = good; s.band = 65536;
    CHECK(refused(call(&s, -1, 0), "band must lie in"));                // the checks come first without a chain, too
    for (auto const& r : out) { fmgpu_chain_alignment filled; std::memset(&filled, 0xAA, sizeof filled); CHECK(std::memcmp(&r, &filled, sizeof r) == 0); }
    for (uint32_t w : ops) CHECK(w == 0xAAAAAAAAu);
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
