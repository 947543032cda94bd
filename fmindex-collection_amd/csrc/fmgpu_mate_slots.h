// fmgpu_mate_slots.h — what the two calls on paired-end mates share (fmgpu_mates.hip, fmgpu_sam_mates.hip): the layout "fragment f owns slots 2f (mate A) and 2f + 1
// (mate B)"; separate record arrays A and B fill the even and the odd slots, an interleaved array's reads 2f and 2f + 1 ARE the slots.  With it: the limits, the first
// eight error words, the records pass, the staging of the two sides and the report of those words.  Who sets the QOFF words and which words a later pass waits for is each
// unit's own: the latter decides which pass may index by a read number that nobody has checked.
#pragma once
#include "fmgpu_positions.h"

namespace fmgpu {

constexpr uint64_t kMaxMateRecords = (1ull << 32) - 256;
constexpr uint64_t kMaxFragments = (1ull << 31) - 1;        // two slots (lines) per fragment, numbered in 32 bits
constexpr uint64_t kPosLimit = 1ull << 62;

// the error words both calls start with, in the order they are reported, one word for array A and one for array B each: the lowest record whose read lies beyond the
// batch; whose read lies below its predecessor's; the lowest read whose offsets decrease; the lowest record whose pos is 2^62 or more
enum : int { E_RANGE = 0, E_ORDER = 2, E_QOFF = 4, E_POS = 6, E_MATE_WORDS = 8 };

// record i of the `count` records p of side `side`: read number in range and not below its predecessor's, pos < 2^62 (an offender atomicMin's i into its word of err), and
// the first and the last record of its slot from the boundaries between neighbours.  Returns the slot; kNone: the record names no read of the batch and is to be skipped.
__device__ __forceinline__ uint64_t mate_record(const fmgpu_position* __restrict__ p, uint64_t count, uint64_t i, int side, uint32_t shift, uint64_t reads, bool interleaved,
                                                unsigned long long* err, uint32_t* first, uint32_t* end) {
    uint64_t read;
    bool starts, ends;
    if (!run_edges(p, count, i, shift, reads, &err[E_RANGE + side], &err[E_ORDER + side], &read, &starts, &ends)) return kNone;
    if (p[i].pos >= kPosLimit) atomicMin(&err[E_POS + side], (unsigned long long)i);
    const uint64_t slot = interleaved ? read : 2 * read + (uint64_t)side;
    if (starts) first[slot] = (uint32_t)i;
    if (ends) end[slot] = (uint32_t)i + 1u;
    return slot;
}

// ---- host side
// the record arrays and the offsets of the two sides in device memory (n fragments); interleaved: side B is side A, whose batch holds 2 n reads
inline int stage_mate_sides(const fmgpu_position* pa, uint64_t ca, const fmgpu_position* pb, uint64_t cb, const uint64_t* qa, const uint64_t* qb, uint64_t n, bool interleaved,
                            Staged* spos, Staged* soff, const fmgpu_position** dpos, const uint64_t** dqoff, hipStream_t stream) {
    int rc;
    if ((rc = spos[0].in(pa, ca * sizeof(fmgpu_position), stream)) || (rc = soff[0].in(qa, ((interleaved ? 2 * n : n) + 1) * 8, stream))) return rc;
    if (!interleaved && ((rc = spos[1].in(pb, cb * sizeof(fmgpu_position), stream)) || (rc = soff[1].in(qb, (n + 1) * 8, stream)))) return rc;
    for (int s = 0; s < 2; ++s) { dpos[s] = (const fmgpu_position*)spos[interleaved ? 0 : s].dev; dqoff[s] = (const uint64_t*)soff[interleaved ? 0 : s].dev; }
    return 0;
}

// what the first eight error words say, as call `fn` reports it: the kinds in the order of the words, array A before array B; 0: none is set
inline int mate_errors(const uint64_t* err, const char* fn) {
    static const struct { int word; const char* who[2]; const char* what; } kKinds[4] = {
        {E_RANGE, {"positions_a: record ", "positions_b: record "}, " names a read beyond the batch"},
        {E_ORDER, {"positions_a: record ", "positions_b: record "}, " names a read below its predecessor's"},
        {E_QOFF, {"qoff_a: read ", "qoff_b: read "}, " has an offset above its successor's"},
        {E_POS, {"positions_a: record ", "positions_b: record "}, " has a pos of 2^62 or more"}};
    for (const auto& k : kKinds) for (int s = 0; s < 2; ++s) if (err[k.word + s] != kNone)
        return fail(FMGPU_ERR_INVALID, std::string(fn) + ": " + k.who[s] + std::to_string(err[k.word + s]) + k.what);
    return 0;
}

}  // namespace fmgpu
