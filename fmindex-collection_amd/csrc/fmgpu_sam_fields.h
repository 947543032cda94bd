// fmgpu_sam_fields.h — what the SAM writers share (fmgpu_sam.hip, fmgpu_sam_mates.hip): the search of a window's lines by a whole wave, the short fields of a line
// formatted into the LDS window of fmgpu_positions.h, and the copy of SEQ and QUAL by whole waves (put_run).  Everything is force-inlined into the kernels of the
// including unit.
#pragma once
#include "fmgpu_positions.h"
#include "fmgpu_pieces.h"

namespace fmgpu {

// the last index i of a[0 .. n - 1] with a[i] <= key (strict: a[i] < key), a non-decreasing and a[0] passing; by the whole wave, 64 probes per step
__device__ __forceinline__ uint64_t wave_search(const uint64_t* __restrict__ a, uint64_t n, uint64_t key, bool strict) {
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63u) / 64u, at = lo + lane * step;
        bool pass = false;
        if (at < hi) { const uint64_t v = a[at]; pass = strict ? v < key : v <= key; }
        const uint64_t passing = (uint64_t)__popcll(__ballot(pass));          // (a prefix of the lanes, lane 0 among them)
        lo += (passing - 1) * step;
        hi = lo + step < hi ? lo + step : hi;
    }
    return lo;
}

// the fields of a line in a Window (fmgpu_positions.h) whose positions count from the 16-byte piece of the output address that holds the text's first byte: each
// returns the position behind what it wrote
__device__ __forceinline__ uint64_t field_decimal(const Window& w, uint64_t at, uint64_t v, uint32_t sep) {
    const uint32_t d = digits10(v);
    put_decimal(w, v, at + d);
    w.put(at + d, sep);
    return at + d + 1;
}
__device__ __forceinline__ uint64_t field_text(const Window& w, uint64_t at, const char* s, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) w.put(at + k, (uint32_t)(uint8_t)s[k]);
    return at + n;
}
// a name by its lane, the part inside the window: without a table the number in decimal, '*' for an empty name (src == nullptr)
__device__ __forceinline__ uint64_t field_name(const Window& w, uint64_t hi, uint64_t at, const uint8_t* src, uint32_t n, bool numbered, uint64_t number) {
    if (!src && numbered) return field_decimal(w, at, number, '\t');
    if (!src) { w.put(at, '*'); w.put(at + 1, '\t'); return at + 2; }
    uint32_t j0, j1;
    window_clip(w.lo, hi, at, n, &j0, &j1);
    for (uint32_t j = j0; j < j1; ++j) w.lds[at + j - w.lo] = src[j];
    w.put(at + n, '\t');
    return at + n + 1;
}

// `len` bytes at position `at`, the part inside the window, copied by the wave, eight lanes to a field: a lane makes up to 16 bytes of the line from the aligned
// 16-byte pieces that hold their source, reversed in registers where `rev` (byte j of the line is byte len - 1 - j of src), each sent through the strand's 256 entries
// of tab (nullptr: as it is).  Every lane of the wave calls it; a lane without such a field passes len = 0.
__device__ __forceinline__ void put_run(const Window& w, uint64_t hi, const uint8_t* src, uint32_t len, uint64_t at, uint32_t rev, const uint8_t* tab) {
    uint32_t j0, j1;                                        // bytes j0 .. j1 - 1 of the field lie in the window
    window_clip(w.lo, hi, at, len, &j0, &j1);
    unsigned long long todo = __ballot(j1 > j0);
    const uint32_t lane = threadIdx.x & 63u, slot = lane >> 3, sub = lane & 7u;
    while (todo) {                                          // eight fields per round, eight lanes (128 bytes a step) each
        unsigned long long mine = todo;
        for (uint32_t k = 0; k < slot; ++k) mine &= mine - 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) todo &= todo - 1;
        const int l = mine ? __ffsll((long long)mine) - 1 : 0;
        const unsigned long long s = __shfl((unsigned long long)reinterpret_cast<uintptr_t>(src), l), p = __shfl((unsigned long long)at, l);
        const uint32_t b = (uint32_t)__shfl((int)j0, l), e = (uint32_t)__shfl((int)j1, l), n = (uint32_t)__shfl((int)len, l), r = (uint32_t)__shfl((int)rev, l);
        const uint8_t* from = reinterpret_cast<const uint8_t*>((uintptr_t)s);
        const uint8_t* tr = tab ? tab + 256u * r : nullptr;
        for (uint32_t c = b + 16u * sub; mine && c < e; c += 128u) {
            const uint32_t k = e - c < 16u ? e - c : 16u;
            Piece v;
            if (!r) v = load_bytes(from + c, k);
            else {
                const Piece f = load_bytes(from + (n - c - k), k);
                v = piece_shr(Piece{__builtin_bswap64(f.hi), __builtin_bswap64(f.lo)}, 16u - k);
            }
            for (uint32_t x = 0; x < k; ++x) {
                uint32_t byte = (uint32_t)((x < 8u ? v.lo >> (8u * x) : v.hi >> (8u * (x - 8u))) & 255u);
                if (tr) byte = tr[byte];
                w.lds[p + c + x - w.lo] = (uint8_t)byte;
            }
        }
    }
}

}  // namespace fmgpu
