// fmgpu_mates.hip — fmgpu_positions_mates (include/fmgpu.h): the located positions of the two mates of paired-end fragments joined to concordant pairs on the device.
// Nothing here depends on the row width or on an index.  A fragment f owns two slots, 2f (mate A) and 2f + 1 (mate B): in separate mode record arrays A and B fill the
// even and the odd slots, in interleaved mode reads 2f and 2f + 1 of the one array ARE the slots, so every pass behind the first sees one layout.  The passes:
//  k_mates_records    one lane per record of each array: read number in range and not below its predecessor's, pos < 2^62 (an offending record atomicMin's its index
//                     into an error word), the first and the last record of each slot from the boundaries between neighbours
//  k_mates_qoff       one lane per read of each batch: the offsets do not decrease
//  k_mates_classes    one lane per fragment: classes 0, 1, 2 and 5; a fragment that will be joined is marked 3 for now
//  (the B-side records ordered by (read, seq_id, pos, index): three stable hipcub radix sorts of index values, by pos, by seq_id, by read, a gather in front of each)
//  k_mates_compact    one lane per B-side record in that order: seq_id, pos with the strand in bit 63, pos + m, index and errors as one 32-byte record, so that the
//                     walks load neither the record array nor the offsets of batch B
//  k_mates_walk<MIN>  (best only) one lane per A-side record of a joined fragment: atomicMin of the error sum over its concordant records into the fragment's word
//  k_mates_walk<COUNT> the same walk, counting: a bisection of the slot's ordered records to the first one with the A-record's seq_id and pos >= p(a) - max_tlen, then
//                     one step per record up to pos <= p(a) + max_tlen (tlen >= |p(a) - p(b)|: nothing outside the window can be concordant)
//  (hipcub exclusive scan of the counts to 64-bit pair offsets per A-side record)
//  k_mates_fragments  one lane per fragment: its pair count from the offsets of its first and behind its last A-record, classes 3 and 4
//  (hipcub exclusive scan of those to out_off; the total and the error words are read back together, once)
//  k_mates_walk<WRITE> the same walk again: each lane writes its pairs behind its offset as whole 32-byte records
// Every pass behind the first two reads the error words and does nothing once one is set: a batch that is out of order indexes nothing.
// Scratch: 37 bytes per fragment (its two slots among them), 12 bytes per A-side record, 56 bytes per B-side record, plus hipcub's own; freed on return.
// The slots, the first pass, the staging of the two sides and the report of the error words are fmgpu_mate_slots.h's, shared with fmgpu_sam_mates.hip; the run boundaries
// (run_edges) and the hipcub calls written once (cub_size, cub_run) are fmgpu_positions.h's.
#include "fmgpu_mate_slots.h"

namespace fmgpu {
namespace {

constexpr uint64_t kStrandBit = 1ull << 63;

enum : int { E_WORDS = E_MATE_WORDS };                      // the error words behind out_off's scratch: fmgpu_mate_slots.h's eight
enum : uint8_t { CLS_NONE = 0, CLS_ONLY_A = 1, CLS_ONLY_B = 2, CLS_DISCORDANT = 3, CLS_PAIRED = 4, CLS_SKIPPED = 5 };
enum : int { WALK_MIN = 0, WALK_COUNT = 1, WALK_WRITE = 2 };

struct Sorted { uint64_t seq, pos_s, end; uint32_t idx, errors; };     // a B-side record as the walks read it: pos_s = pos | strand << 63, end = pos + m
static_assert(sizeof(Sorted) == 32, "two 16-byte pieces");

struct MatesArgs {
    const fmgpu_position *pa, *pb;                          // (interleaved: pb = pa, count_b = count_a, qoff_b = qoff_a)
    uint64_t count_a, count_b;
    const uint64_t *qoff_a, *qoff_b;
    uint64_t n, reads;                                      // fragments; reads of a batch (n, interleaved 2 n)
    uint64_t min_tlen, max_tlen, max_records;
    uint8_t shift, interleaved, any, best;
    uint32_t *first, *end;                                  // per slot: its first record, one behind its last
    uint32_t* fbest;                                        // per fragment: the minimal error sum of its concordant pairs (best)
    uint8_t* cls;                                           // per fragment
    uint32_t* cnt;                                          // count_a + 1: the pairs of each A-side record
    uint64_t* rstart;                                       // count_a + 1: its first pair
    uint64_t *fcount, *foff;                                // n + 1: the pairs of each fragment, its first pair; foff[n] = the number of pairs
    unsigned long long* err;                                // E_WORDS words, behind foff
    Sorted* sb;                                             // count_b
};

__device__ __forceinline__ bool failed(const MatesArgs& a) {
    unsigned long long all = kNone;
#pragma unroll
    for (int k = 0; k < E_WORDS; ++k) all &= a.err[k];
    return all != kNone;
}

__global__ __launch_bounds__(256) void k_mates_records(MatesArgs a, int side) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t count = side ? a.count_b : a.count_a;
    if (i < count) (void)mate_record(side ? a.pb : a.pa, count, i, side, a.shift, a.reads, a.interleaved, a.err, a.first, a.end);
}

__global__ __launch_bounds__(256) void k_mates_qoff(MatesArgs a, int side) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.reads) return;
    const uint64_t* __restrict__ q = side ? a.qoff_b : a.qoff_a;
    if (q[r + 1] < q[r]) atomicMin(&a.err[E_QOFF + side], (unsigned long long)r);
}

__device__ __forceinline__ uint32_t slot_records(const MatesArgs& a, uint64_t slot) { return a.first[slot] != kNoRecord32 ? a.end[slot] - a.first[slot] : 0u; }

__global__ __launch_bounds__(256) void k_mates_classes(MatesArgs a) {
    if (failed(a)) return;
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    const uint32_t na = slot_records(a, 2 * f), nb = slot_records(a, 2 * f + 1);
    uint8_t c = CLS_DISCORDANT;
    if (!na && !nb) c = CLS_NONE;
    else if (!nb) c = CLS_ONLY_A;
    else if (!na) c = CLS_ONLY_B;
    else if (a.max_records && (na > a.max_records || nb > a.max_records)) c = CLS_SKIPPED;
    a.cls[f] = c;
}

// the keys of the three sorts: nothing here is indexed by a read number, so these run whatever the first pass found
__global__ __launch_bounds__(256) void k_mates_key_pos(MatesArgs a, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count_b) return;
    keys[i] = a.pb[i].pos; vals[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_mates_key_seq(MatesArgs a, const uint32_t* __restrict__ vals, uint64_t* __restrict__ keys) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.count_b) return;
    keys[j] = a.pb[vals[j]].seq_id;
}
__global__ __launch_bounds__(256) void k_mates_key_read(MatesArgs a, const uint32_t* __restrict__ vals, uint32_t* __restrict__ keys) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.count_b) return;
    keys[j] = (uint32_t)(a.pb[vals[j]].qidx >> a.shift);
}

__global__ __launch_bounds__(256) void k_mates_compact(MatesArgs a, const uint32_t* __restrict__ order) {
    if (failed(a)) return;
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.count_b) return;
    const uint32_t idx = order[j];
    const fmgpu_position r = a.pb[idx];
    const uint64_t read = r.qidx >> a.shift, m = a.qoff_b[read + 1] - a.qoff_b[read];
    const uint64_t strand = a.shift ? r.qidx & 1u : 0u;
    ulonglong2* const dst = reinterpret_cast<ulonglong2*>(a.sb + j);
    dst[0] = make_ulonglong2(r.seq_id, r.pos | (strand ? kStrandBit : 0ull));
    dst[1] = make_ulonglong2(r.pos + m, (unsigned long long)idx | ((unsigned long long)r.errors << 32));
}

__device__ __forceinline__ Sorted load_sorted(const Sorted* __restrict__ s, uint64_t j) {
    const ulonglong2 x = reinterpret_cast<const ulonglong2*>(s + j)[0], y = reinterpret_cast<const ulonglong2*>(s + j)[1];
    return Sorted{x.x, x.y, y.x, (uint32_t)y.y, (uint32_t)(y.y >> 32)};
}

template <int MODE>
__global__ __launch_bounds__(256) void k_mates_walk(MatesArgs a, fmgpu_mate_pair* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.count_a) return;
    if (i == a.count_a || failed(a)) { if (MODE == WALK_COUNT) a.cnt[i] = 0; return; }
    const fmgpu_position rec = a.pa[i];
    const uint64_t read = rec.qidx >> a.shift;
    const uint64_t f = a.interleaved ? read >> 1 : read;
    if ((a.interleaved && (read & 1u)) || a.cls[f] != (MODE == WALK_WRITE ? CLS_PAIRED : CLS_DISCORDANT)) { if (MODE == WALK_COUNT) a.cnt[i] = 0; return; }
    const uint64_t p_a = rec.pos, e_a = p_a + (a.qoff_a[read + 1] - a.qoff_a[read]), s_a = a.shift ? rec.qidx & 1u : 0u;
    const uint64_t lo = p_a > a.max_tlen ? p_a - a.max_tlen : 0, hi = a.max_tlen >= kPosLimit ? kNone : p_a + a.max_tlen;     // (p_a < 2^62: no wrap)
    const uint64_t b1 = a.end[2 * f + 1];
    uint64_t l = a.first[2 * f + 1], h = b1;
    while (l < h) {                                         // the first record of the slot with (seq_id, pos) >= (seq_id of a, lo)
        const uint64_t mid = (l + h) >> 1;
        const ulonglong2 k = reinterpret_cast<const ulonglong2*>(a.sb + mid)[0];
        if (k.x < rec.seq_id || (k.x == rec.seq_id && (k.y & ~kStrandBit) < lo)) l = mid + 1; else h = mid;
    }
    const uint32_t want = a.best && MODE != WALK_MIN ? a.fbest[f] : 0u;
    uint32_t count = 0, least = 0xffffffffu;
    bool any_pair = false;
    uint64_t at = MODE == WALK_WRITE ? a.rstart[i] : 0;
    for (uint64_t j = l; j < b1; ++j) {
        const Sorted s = load_sorted(a.sb, j);
        const uint64_t p_b = s.pos_s & ~kStrandBit, s_b = s.pos_s >> 63;
        if (s.seq != rec.seq_id || p_b > hi) break;
        const uint64_t tlen = (e_a > s.end ? e_a : s.end) - (p_a < p_b ? p_a : p_b);
        if (tlen < a.min_tlen || tlen > a.max_tlen) continue;
        if (!a.any) {                                       // FR: the strand-0 mate lies upstream and neither end of it passes the other mate's
            if (s_a == s_b) continue;
            const uint64_t pf = s_a ? p_b : p_a, ef = s_a ? s.end : e_a, pr = s_a ? p_a : p_b, er = s_a ? e_a : s.end;
            if (pf > pr || ef > er) continue;
        }
        const uint32_t sum = rec.errors + s.errors;
        if (MODE == WALK_MIN) { least = sum < least ? sum : least; any_pair = true; continue; }
        if (a.best && sum != want) continue;
        if (MODE == WALK_WRITE) {
            fmgpu_mate_pair pair;
            pair.fragment = f; pair.tlen = tlen; pair.a = (uint32_t)i; pair.b = s.idx; pair.errors = sum; pair.flags = p_a <= p_b ? 1u : 0u;
            out[at++] = pair;
        }
        ++count;
    }
    if (MODE == WALK_MIN && any_pair) atomicMin(&a.fbest[f], least);
    if (MODE == WALK_COUNT) a.cnt[i] = count;
}

__global__ __launch_bounds__(256) void k_mates_fragments(MatesArgs a) {
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f > a.n) return;
    uint64_t c = 0;
    if (f < a.n && !failed(a) && a.cls[f] == CLS_DISCORDANT) {
        c = a.rstart[a.end[2 * f]] - a.rstart[a.first[2 * f]];
        if (c) a.cls[f] = CLS_PAIRED;
    }
    a.fcount[f] = c;
}

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_positions_mates(const fmgpu_position* positions_a, uint64_t count_a, const fmgpu_position* positions_b, uint64_t count_b, const fmgpu_mates_spec* spec,
                          fmgpu_mate_pair* out, uint64_t capacity, uint64_t* out_count, uint64_t* out_off, uint8_t* out_class, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!spec) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_mates: spec is null");
    if (!out_count) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_mates: out_count is null");
    const uint64_t n = spec->n_fragments;
    if (n == 0) { *out_count = 0; return first_offset_zero(out_off, stream); }         // no fragment: nothing else is looked at
    if (!spec->qoff_a) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: qoff_a is null");
    if (spec->strand_shift > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: strand_shift must be 0 or 1");
    if (spec->interleaved > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: interleaved must be 0 or 1");
    if (spec->orientation > FMGPU_MATES_ANY) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: orientation must be FMGPU_MATES_FR or FMGPU_MATES_ANY");
    if (spec->best > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: best must be 0 or 1");
    if (spec->reserved[0] || spec->reserved[1] || spec->reserved[2] || spec->reserved[3]) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: reserved must be 0");
    if (spec->min_tlen > spec->max_tlen) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: min_tlen lies above max_tlen");
    if (spec->interleaved) {
        if (spec->qoff_b) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: qoff_b must be null in interleaved mode");
        if (positions_b || count_b) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_mates: positions_b must be null with count_b = 0 in interleaved mode");
    } else {
        if (!spec->qoff_b) return fail(FMGPU_ERR_INVALID, "fmgpu_mates_spec: qoff_b is null in separate mode");
        if (count_b && !positions_b) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_mates: positions_b is null while count_b > 0");
    }
    if (count_a && !positions_a) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_mates: positions_a is null while count_a > 0");
    if (!out && capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_mates: out is null while capacity > 0");
    *out_count = 0;
    if (count_a >= kMaxMateRecords || count_b >= kMaxMateRecords)
        return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_mates: count_a and count_b must each stay below 2^32 - 256");
    if (n >= kMaxFragments) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_mates: n_fragments must stay below 2^31 - 1");

    MatesArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.reads = spec->interleaved ? 2 * n : n;
    a.count_a = count_a; a.count_b = spec->interleaved ? count_a : count_b;
    a.min_tlen = spec->min_tlen; a.max_tlen = spec->max_tlen; a.max_records = spec->max_records;
    a.shift = spec->strand_shift; a.interleaved = spec->interleaved; a.any = spec->orientation == FMGPU_MATES_ANY; a.best = spec->best;

    int rc;
    Staged spos[2], soff[2], sout;
    const fmgpu_position* dpos[2];
    const uint64_t* dqoff[2];
    if ((rc = stage_mate_sides(positions_a, count_a, positions_b, count_b, spec->qoff_a, spec->qoff_b, n, spec->interleaved, spos, soff, dpos, dqoff, stream))) return rc;
    a.pa = dpos[0]; a.pb = dpos[1]; a.qoff_a = dqoff[0]; a.qoff_b = dqoff[1];
    const uint64_t ca = a.count_a, cb = a.count_b;
    const bool join = ca && cb;                                     // without a record on either side there is nothing to order or to walk

    // per slot: first, end; per fragment: fbest (4), cls (1), fcount and foff (8 each, one entry more); the error words behind foff
    DBuf slots, frags, offs, arec, keys, vals, sorted, tmp;
    if ((rc = slots.alloc(2 * n * 8)) || (rc = frags.alloc(n * 5)) || (rc = offs.alloc((2 * (n + 1) + E_WORDS) * 8)) || (rc = arec.alloc((ca + 1) * 12))) return rc;
    a.first = slots.as<uint32_t>(); a.end = a.first + 2 * n;
    a.fbest = frags.as<uint32_t>(); a.cls = reinterpret_cast<uint8_t*>(a.fbest + n);
    a.fcount = offs.as<uint64_t>(); a.foff = a.fcount + (n + 1);
    a.err = reinterpret_cast<unsigned long long*>(a.foff + (n + 1));
    a.rstart = arec.as<uint64_t>(); a.cnt = reinterpret_cast<uint32_t*>(a.rstart + (ca + 1));
    uint64_t *k0 = nullptr, *k1 = nullptr;
    uint32_t *v0 = nullptr, *v1 = nullptr;
    int read_bits = 1;
    while (read_bits < 32 && (a.reads - 1) >> read_bits) ++read_bits;

    Widened counts(a.cnt, Widen{});
    auto scan_counts = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, counts, a.rstart, (size_t)(ca + 1), stream); };
    auto scan_fragments = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, a.fcount, a.foff, (size_t)(n + 1), stream); };
    auto sort_pos = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, v0, v1, (size_t)cb, 0, 62, stream); };
    auto sort_seq = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, v1, v0, (size_t)cb, 0, 64, stream); };
    auto sort_read = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, (uint32_t*)k0, (uint32_t*)k1, v0, v1, (size_t)cb, 0, read_bits, stream); };
    size_t tb = 0;
    FM_HIP(cub_size(&tb, scan_counts, scan_fragments));
    if (join) {
        if ((rc = keys.alloc(cb * 16)) || (rc = vals.alloc(cb * 8)) || (rc = sorted.alloc(cb * sizeof(Sorted)))) return rc;
        k0 = keys.as<uint64_t>(); k1 = k0 + cb; v0 = vals.as<uint32_t>(); v1 = v0 + cb;
        a.sb = sorted.as<Sorted>();
        FM_HIP(cub_size(&tb, sort_pos, sort_seq, sort_read));
    }
    if ((rc = tmp.alloc(tb))) return rc;

    FM_HIP(hipMemsetAsync(a.first, 0xff, 2 * n * 4, stream));
    FM_HIP(hipMemsetAsync(a.fbest, 0xff, n * 4, stream));
    FM_HIP(hipMemsetAsync(a.err, 0xff, E_WORDS * 8, stream));
    if (ca) {
        FM_GRID(g, ca);
        k_mates_records<<<g, dim3(256), 0, stream>>>(a, 0);
        FM_LAUNCHED("k_mates_records");
    }
    if (!spec->interleaved && cb) {
        FM_GRID(g, cb);
        k_mates_records<<<g, dim3(256), 0, stream>>>(a, 1);
        FM_LAUNCHED("k_mates_records");
    }
    {
        FM_GRID(g, a.reads);
        k_mates_qoff<<<g, dim3(256), 0, stream>>>(a, 0);
        FM_LAUNCHED("k_mates_qoff");
        if (!spec->interleaved) { k_mates_qoff<<<g, dim3(256), 0, stream>>>(a, 1); FM_LAUNCHED("k_mates_qoff"); }
    }
    FM_GRID(fgrid, n + 1);
    k_mates_classes<<<fgrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_mates_classes");
    FM_GRID(agrid, ca + 1);
    if (join) {
        FM_GRID(bgrid, cb);
        k_mates_key_pos<<<bgrid, dim3(256), 0, stream>>>(a, k0, v0);
        FM_LAUNCHED("k_mates_key_pos");
        FM_HIP(cub_run(sort_pos, tmp));                             // v1: by pos, then index
        k_mates_key_seq<<<bgrid, dim3(256), 0, stream>>>(a, v1, k0);
        FM_LAUNCHED("k_mates_key_seq");
        FM_HIP(cub_run(sort_seq, tmp));                             // v0: by seq_id, stable
        k_mates_key_read<<<bgrid, dim3(256), 0, stream>>>(a, v0, (uint32_t*)k0);
        FM_LAUNCHED("k_mates_key_read");
        FM_HIP(cub_run(sort_read, tmp));                            // v1: by read, stable: the order
        k_mates_compact<<<bgrid, dim3(256), 0, stream>>>(a, v1);
        FM_LAUNCHED("k_mates_compact");
        if (a.best) { k_mates_walk<WALK_MIN><<<agrid, dim3(256), 0, stream>>>(a, nullptr); FM_LAUNCHED("k_mates_walk"); }
        k_mates_walk<WALK_COUNT><<<agrid, dim3(256), 0, stream>>>(a, nullptr);
        FM_LAUNCHED("k_mates_walk");
    } else FM_HIP(hipMemsetAsync(a.cnt, 0, (ca + 1) * 4, stream));
    FM_HIP(cub_run(scan_counts, tmp));
    k_mates_fragments<<<fgrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_mates_fragments");
    FM_HIP(cub_run(scan_fragments, tmp));
    uint64_t back[1 + E_WORDS];                                     // the number of pairs and the error words: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, a.foff + n, sizeof back, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if ((rc = mate_errors(back + 1, "fmgpu_positions_mates"))) return rc;
    const uint64_t total = back[0];
    *out_count = total;
    if (out_off) FM_HIP(hipMemcpyAsync(out_off, a.foff, (n + 1) * 8, hipMemcpyDefault, stream));
    if (out_class) FM_HIP(hipMemcpyAsync(out_class, a.cls, n, hipMemcpyDefault, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (!out && !capacity) return 0;
    if (total > capacity) return fail(FMGPU_ERR_CAPACITY, std::to_string(total) + " pairs: more than `capacity`");
    if (!total) return 0;
    if ((rc = sout.out(out, total * sizeof(fmgpu_mate_pair), stream))) return rc;
    k_mates_walk<WALK_WRITE><<<agrid, dim3(256), 0, stream>>>(a, (fmgpu_mate_pair*)sout.dev);
    FM_LAUNCHED("k_mates_walk");
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
