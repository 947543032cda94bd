// tools/format_probe.py, the baseline leg: the example's output loop (fmindex-collection_amd/example/main.cpp, reportMapped: four "%zu" per located position) formatting
// into a memory buffer instead of a file, on one core.  Built by the probe with g++ -O2 -shared; returns the bytes written.
#include <cstddef>
#include <cstdint>
#include <cstdio>

struct Position { uint64_t qidx, seq_id, pos; uint32_t errors, hit; };

extern "C" uint64_t format_loop(Position const* positions, uint64_t count, char* out, uint64_t capacity) {
    uint64_t at = 0;
    for (uint64_t i = 0; i < count; ++i) {
        auto const& p = positions[i];
        int const n = std::snprintf(out + at, capacity - at, "%zu %zu %zu %zu\n", static_cast<size_t>(p.qidx), static_cast<size_t>(static_cast<uint32_t>(p.seq_id)),
                                    static_cast<size_t>(p.pos), static_cast<size_t>(p.errors));
        if (n < 0 || static_cast<uint64_t>(n) >= capacity - at) return 0;
        at += static_cast<uint64_t>(n);
    }
    return at;
}
