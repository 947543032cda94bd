// fmgpu_pieces.h — sixteen bytes in two registers: what the passes that copy and reverse runs of symbol bytes (fmgpu_strands.hip, fmgpu_sam.hip) load, shift and mask.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace fmgpu {

// sixteen bytes as two words, byte k of the piece = byte k & 7 of word k >> 3
struct Piece { uint64_t lo, hi; };
__device__ __forceinline__ Piece piece_shr(Piece v, uint32_t bytes) {      // bytes in [0, 16]
    if (bytes >= 16u) return Piece{0, 0};
    if (bytes >= 8u) { v.lo = v.hi; v.hi = 0; bytes -= 8u; }
    if (bytes) { const uint32_t b = 8u * bytes; v.lo = (v.lo >> b) | (v.hi << (64u - b)); v.hi >>= b; }
    return v;
}
__device__ __forceinline__ Piece piece_shl(Piece v, uint32_t bytes) {      // bytes in [0, 16]
    if (bytes >= 16u) return Piece{0, 0};
    if (bytes >= 8u) { v.hi = v.lo; v.lo = 0; bytes -= 8u; }
    if (bytes) { const uint32_t b = 8u * bytes; v.hi = (v.hi << b) | (v.lo >> (64u - b)); v.lo <<= b; }
    return v;
}
__device__ __forceinline__ Piece piece_low(Piece v, uint32_t bytes) {      // the low `bytes` bytes, 1 .. 16
    if (bytes < 8u) { v.lo &= (1ull << (8u * bytes)) - 1ull; v.hi = 0; }
    else if (bytes < 16u) v.hi &= bytes == 8u ? 0ull : (1ull << (8u * (bytes - 8u))) - 1ull;
    return v;
}
// bytes p[0 .. n - 1], 1 <= n <= 16, from the one or two aligned 16-byte pieces that hold them (each holds a byte of the range: no piece lies outside the pages of the buffer)
__device__ __forceinline__ Piece load_bytes(const uint8_t* p, uint32_t n) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const uint32_t sh = (uint32_t)(a & 15u);
    const uint4* w = reinterpret_cast<const uint4*>(a - sh);
    const uint4 A = w[0];
    uint64_t x0 = (uint64_t)A.x | ((uint64_t)A.y << 32), x1 = (uint64_t)A.z | ((uint64_t)A.w << 32), x2 = 0, x3 = 0;
    if (sh + n > 16u) { const uint4 B = w[1]; x2 = (uint64_t)B.x | ((uint64_t)B.y << 32); x3 = (uint64_t)B.z | ((uint64_t)B.w << 32); }
    if (sh >= 8u) { x0 = x1; x1 = x2; x2 = x3; }
    const uint32_t b = 8u * (sh & 7u);
    Piece v;
    v.lo = b ? (x0 >> b) | (x1 << (64u - b)) : x0;
    v.hi = b ? (x1 >> b) | (x2 << (64u - b)) : x1;
    return piece_low(v, n);
}

}  // namespace fmgpu
