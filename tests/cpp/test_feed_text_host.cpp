// The arithmetic of a text feed (fmindex-collection_amd/csrc/fmgpu_feed_host.h: windows, piece finality, the headroom policy, the piece-size limit) against a
// restatement of the rule of include/fmgpu.h (fmgpu_feed_map_text, "Pieces").  Stand-alone: no device, no library; tests/test_feed_text_host.py builds it plain and
// with -fsanitize=address,undefined and runs it as a program.
#include "../../fmindex-collection_amd/csrc/fmgpu_feed_host.h"

#include <cstdio>
#include <utility>

namespace fh = fmgpu_feed_host;

static int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the rule, byte by byte: window c is text[c B, min((c + 1) B, bytes)), c = 0 .. ceil(bytes / B) - 1
static std::vector<std::pair<uint64_t, uint64_t>> windows_by_the_rule(uint64_t bytes, uint64_t B) {
    std::vector<std::pair<uint64_t, uint64_t>> w;
    for (uint64_t a = 0; a < bytes; a += B) w.push_back({a, bytes - a < B ? bytes : a + B});
    return w;
}

static void check_windows(uint64_t bytes, uint64_t B) {
    const auto want = windows_by_the_rule(bytes, B);
    CHECK(fh::text_windows(bytes, B) == want.size());
    uint64_t covered = 0;
    for (uint64_t c = 0; c < want.size(); ++c) {
        CHECK(fh::text_window_begin(c, B) == want[c].first);
        CHECK(fh::text_window_end(bytes, c, B) == want[c].second);
        CHECK(want[c].first == covered && want[c].second > want[c].first && want[c].second - want[c].first <= B);
        covered = want[c].second;
        for (int32_t final = 0; final < 2; ++final) CHECK(fh::text_piece_final(c, want.size(), final) == (final && c + 1 == want.size()));
    }
    CHECK(covered == bytes);
}

int main() {
    // B: 0 is the default of 64 MiB, every other value is itself (1 .. 15 are refused by the call, kTextMinWindow)
    CHECK(fh::text_window_bytes(0) == (64ull << 20) && fh::text_window_bytes(16) == 16 && fh::text_window_bytes(4097) == 4097 && fh::kTextMinWindow == 16);
    // bytes a multiple of B, one more than a multiple, B > bytes, B = 16, one byte, and a text beyond 2^32 bytes in default windows
    for (unsigned long long B : {16ull, 17ull, 64ull, 257ull, 4096ull})
        for (unsigned long long bytes : {1ull, 15ull, 16ull, 17ull, B - 1, B, B + 1, 3 * B, 3 * B + 1, 7 * B - 1, 1000ull, 4095ull, 4097ull}) check_windows(bytes, B);
    check_windows(0, 16);
    CHECK(fh::text_windows(0, 16) == 0);
    check_windows((5ull << 30) + 3, fh::text_window_bytes(0));
    CHECK(fh::text_windows((5ull << 30) + 3, 64ull << 20) == 81);
    CHECK(fh::text_windows(~0ull, 16) == (~0ull >> 4) + 1 && fh::text_window_end(~0ull, ~0ull >> 4, 16) == ~0ull);      // no overflow at the top of the range

    // the headroom: a window's worth, at most 1 MiB, a multiple of 16; unchanged while a carry fits (0, H), at least twice a carry that does not (H + 1)
    for (uint64_t B : {16ull, 17ull, 64ull, 257ull, 4096ull, 1ull << 20, (1ull << 20) + 1, 64ull << 20}) {
        const uint64_t H = fh::text_headroom(B);
        CHECK(H % 16 == 0 && H >= (B < (1ull << 20) ? B : (1ull << 20)) && H < (B < (1ull << 20) ? B : (1ull << 20)) + 16);
        CHECK(fh::text_headroom_for(H, 0) == H && fh::text_headroom_for(H, 1) == H && fh::text_headroom_for(H, H) == H);
        const uint64_t G = fh::text_headroom_for(H, H + 1);
        CHECK(G % 16 == 0 && G >= 2 * (H + 1) && G < 2 * (H + 1) + 16);
        CHECK(fh::text_headroom_for(G, H + 1) == G && fh::text_headroom_for(G, G) == G);                                 // grown once, it serves
    }
    // growth by doubling: a carry that grows by B bytes per piece (no record ends) regrows a slot O(log) times
    {
        uint64_t H = fh::text_headroom(16), regrown = 0;
        for (uint64_t carry = 0; carry <= 1ull << 20; carry += 16) { const uint64_t G = fh::text_headroom_for(H, carry); regrown += G != H; H = G; }
        CHECK(regrown <= 17 && H >= 1ull << 20);
    }

    // a piece holds at most 2^32 - 2 bytes: carry + window
    const uint64_t M = 0xfffffffeull;
    CHECK(fh::kTextMaxPiece == M);
    CHECK(fh::text_piece_fits(0, M) && !fh::text_piece_fits(0, M + 1) && fh::text_piece_fits(M, 0) && !fh::text_piece_fits(M + 1, 0));
    CHECK(fh::text_piece_fits(M - 16, 16) && !fh::text_piece_fits(M - 15, 16) && fh::text_piece_fits(1, M - 1) && !fh::text_piece_fits(2, M - 1));
    CHECK(!fh::text_piece_fits(~0ull, 1) && !fh::text_piece_fits(1, ~0ull) && !fh::text_piece_fits(~0ull, ~0ull));        // no wrap-around

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
