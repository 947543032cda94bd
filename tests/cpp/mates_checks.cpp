// The paths of fmgpu_positions_mates that return before the first device call, as a stand-alone program for a sanitizer build of the host side of
// fmindex-collection_amd/csrc/fmgpu_mates.hip (the program's own copy of the call is the one that runs; the helpers it calls come from libfmgpu.so):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         fmindex-collection_amd/csrc/fmgpu_mates.hip tests/cpp/mates_checks.cpp -o mates_checks -fsanitize=address,undefined \
//         -Lfmindex-collection_amd -lfmgpu -Wl,-rpath,$PWD/fmindex-collection_amd && ./mates_checks
// It needs no device and is never loaded into another process.
#include "../../include/fmgpu.h"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static bool refused(int rc, const char* word) { return rc == FMGPU_ERR_INVALID && std::strstr(fmgpu_last_error(), word) != nullptr; }

int main() {
    std::vector<fmgpu_position> rec(2);
    std::vector<fmgpu_mate_pair> out(4);
    std::memset(out.data(), 0xAA, out.size() * sizeof(fmgpu_mate_pair));
    std::vector<uint64_t> qoff{0, 4, 8};
    uint64_t n = 7;
    auto spec = [&]() {
        fmgpu_mates_spec s{};
        s.qoff_a = qoff.data(); s.qoff_b = qoff.data(); s.n_fragments = 2; s.max_tlen = 1000; s.strand_shift = 1;
        return s;
    };
    auto call = [&](const fmgpu_mates_spec* s) { return fmgpu_positions_mates(rec.data(), 2, rec.data(), 2, s, out.data(), 4, &n, nullptr, nullptr, nullptr); };
    fmgpu_mates_spec good = spec(), s;

    CHECK(refused(call(nullptr), "spec is null"));
    CHECK(refused(fmgpu_positions_mates(rec.data(), 2, rec.data(), 2, &good, out.data(), 4, nullptr, nullptr, nullptr, nullptr), "out_count is null"));
    s = good; s.qoff_a = nullptr; CHECK(refused(call(&s), "qoff_a is null"));
    for (uint8_t bad : {uint8_t{2}, uint8_t{255}}) {
        s = good; s.strand_shift = bad; CHECK(refused(call(&s), "strand_shift"));
        s = good; s.interleaved = bad; CHECK(refused(call(&s), "interleaved must be"));
        s = good; s.orientation = bad; CHECK(refused(call(&s), "orientation"));
        s = good; s.best = bad; CHECK(refused(call(&s), "best must be"));
    }
    for (int k = 0; k < 4; ++k) { s = good; s.reserved[k] = 1; CHECK(refused(call(&s), "reserved")); }
    s = good; s.min_tlen = 1001; CHECK(refused(call(&s), "min_tlen lies above max_tlen"));
    s = good; s.min_tlen = s.max_tlen = UINT64_MAX; s.qoff_b = nullptr; CHECK(refused(call(&s), "qoff_b is null in separate mode"));
    s = good; s.interleaved = 1; CHECK(refused(call(&s), "qoff_b must be null in interleaved mode"));
    s.qoff_b = nullptr; CHECK(refused(call(&s), "positions_b must be null with count_b = 0"));
    CHECK(refused(fmgpu_positions_mates(rec.data(), 2, nullptr, 1, &s, out.data(), 4, &n, nullptr, nullptr, nullptr), "positions_b must be null with count_b = 0"));
    CHECK(refused(fmgpu_positions_mates(nullptr, 2, nullptr, 0, &s, out.data(), 4, &n, nullptr, nullptr, nullptr), "positions_a is null"));
    CHECK(refused(fmgpu_positions_mates(nullptr, 2, rec.data(), 2, &good, out.data(), 4, &n, nullptr, nullptr, nullptr), "positions_a is null"));
    CHECK(refused(fmgpu_positions_mates(rec.data(), 2, nullptr, 2, &good, out.data(), 4, &n, nullptr, nullptr, nullptr), "positions_b is null"));
    CHECK(refused(fmgpu_positions_mates(rec.data(), 2, rec.data(), 2, &good, nullptr, 4, &n, nullptr, nullptr, nullptr), "out is null"));
    n = 7;
    CHECK(fmgpu_positions_mates(rec.data(), (uint64_t{1} << 32) - 256, rec.data(), 2, &good, nullptr, 0, &n, nullptr, nullptr, nullptr) == FMGPU_ERR_UNSUPPORTED && n == 0);
    CHECK(fmgpu_positions_mates(rec.data(), 2, rec.data(), uint64_t{1} << 40, &good, nullptr, 0, &n, nullptr, nullptr, nullptr) == FMGPU_ERR_UNSUPPORTED);
    s = good; s.n_fragments = (uint64_t{1} << 31) - 1;
    CHECK(fmgpu_positions_mates(rec.data(), 2, rec.data(), 2, &s, nullptr, 0, &n, nullptr, nullptr, nullptr) == FMGPU_ERR_UNSUPPORTED);
    // no fragment: 0 before anything else is looked at
    uint64_t off[2] = {9, 9};
    fmgpu_mates_spec none{};
    none.strand_shift = 9; none.reserved[0] = 1; none.min_tlen = 2;
    n = 7;
    CHECK(fmgpu_positions_mates(nullptr, 5, nullptr, 5, &none, nullptr, 5, &n, off, nullptr, nullptr) == 0 && n == 0 && off[0] == 0 && off[1] == 9);
    n = 7;
    CHECK(fmgpu_positions_mates(nullptr, 0, nullptr, 0, &none, nullptr, 0, &n, nullptr, nullptr, nullptr) == 0 && n == 0);
    for (auto const& p : out) { fmgpu_mate_pair filled; std::memset(&filled, 0xAA, sizeof filled); CHECK(std::memcmp(&p, &filled, sizeof p) == 0); }
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
