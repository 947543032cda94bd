// The paths of fmgpu_positions_format that return before the first device call, as a stand-alone program for a sanitizer build of the host side of
// fmindex-collection_amd/csrc/fmgpu_format.hip (the program's own copy of the call is the one that runs; the helpers it calls come from libfmgpu.so):
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         fmindex-collection_amd/csrc/fmgpu_format.hip tests/cpp/format_checks.cpp -o format_checks -fsanitize=address,undefined \
//         -Lfmindex-collection_amd -lfmgpu -Wl,-rpath,$PWD/fmindex-collection_amd && ./format_checks
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
    std::vector<uint8_t> out(64, 0xAA), bytes(4);
    std::vector<fmgpu_text_span> spans(1);
    uint64_t n = 7;
    auto spec = [](int32_t n_cols, std::initializer_list<uint8_t> cols) {
        fmgpu_format_spec s{};
        s.n_cols = n_cols; s.sep = ' ';
        size_t k = 0;
        for (auto c : cols) s.cols[k++] = c;
        return s;
    };
    auto call = [&](const fmgpu_format_spec* s) { return fmgpu_positions_format(rec.data(), 2, s, out.data(), 64, &n, nullptr, nullptr); };
    fmgpu_format_spec good = spec(4, {0, 1, 2, 3}), s;

    CHECK(refused(call(nullptr), "spec is null"));
    CHECK(refused(fmgpu_positions_format(nullptr, 2, &good, out.data(), 64, &n, nullptr, nullptr), "positions is null"));
    CHECK(refused(fmgpu_positions_format(rec.data(), 2, &good, out.data(), 64, nullptr, nullptr, nullptr), "out_bytes is null"));
    CHECK(refused(fmgpu_positions_format(rec.data(), 2, &good, nullptr, 64, &n, nullptr, nullptr), "out is null"));
    for (int32_t bad : {0, 9, -1, INT32_MIN, INT32_MAX}) { s = spec(bad, {0}); CHECK(refused(call(&s), "n_cols")); }
    s = spec(8, {0, 1, 2, 3, 4, 5, 6, 9}); CHECK(refused(call(&s), "unknown column code 9"));
    s = spec(1, {255}); CHECK(refused(call(&s), "unknown column code 255"));
    s = good; s.strand_shift = 2; CHECK(refused(call(&s), "strand_shift"));
    s = good; s.name_stop = 255; CHECK(refused(call(&s), "name_stop"));
    s = good; s.reserved = 1; CHECK(refused(call(&s), "reserved"));
    s = spec(1, {FMGPU_COL_READ_NAME}); CHECK(refused(call(&s), "needs the read_names table"));
    s = spec(2, {0, FMGPU_COL_SEQ_NAME}); CHECK(refused(call(&s), "needs the seq_names table"));
    fmgpu_name_table t{nullptr, 4, spans.data(), 1};
    s = spec(1, {FMGPU_COL_READ_NAME}); s.read_names = &t; CHECK(refused(call(&s), "read_names table has no bytes"));
    t = fmgpu_name_table{bytes.data(), 4, nullptr, 1};
    s = spec(1, {FMGPU_COL_SEQ_NAME}); s.seq_names = &t; CHECK(refused(call(&s), "seq_names table has no spans"));
    CHECK(fmgpu_positions_format(rec.data(), uint64_t{1} << 32, &good, nullptr, 0, &n, nullptr, nullptr) == FMGPU_ERR_UNSUPPORTED);
    // no record: 0 before anything else is looked at
    uint64_t off[2] = {9, 9};
    n = 7;
    CHECK(fmgpu_positions_format(nullptr, 0, nullptr, nullptr, 0, &n, off, nullptr) == 0 && n == 0 && off[0] == 0 && off[1] == 9);
    CHECK(fmgpu_positions_format(nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr) == 0);
    for (auto b : out) CHECK(b == 0xAA);
    if (failures) return 1;
    std::printf("all checks passed\n");
    return 0;
}
