// fmgpu_positions.h — what the calls on located positions share (fmgpu_format.hip, fmgpu_sam.hip, fmgpu_mates.hip, fmgpu_sam_mates.hip, fmgpu_chain.hip): records and
// the runs of a read in a sorted record array, digit counts, name tables and their row lookup, the LDS window a workgroup formats text into and how it leaves as aligned
// 16-byte stores, and on the host a hipcub call written once for sizing and running, the end of a text call behind its read-back and the odds and ends around them.
// Nothing here depends on the row width or on an index.  Everything on the device side is force-inlined into the kernels of the including unit.
#pragma once
#include "fmgpu_common.h"

#include <hipcub/hipcub.hpp>

namespace fmgpu {

constexpr uint64_t kNone = ~0ull;                           // an error word that no offender has lowered; a 64-bit "nothing"
constexpr uint32_t kNoRecord32 = 0xffffffffu;               // a read, slot or fragment without a record

static __device__ const uint64_t kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                                               100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                               100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};

// decimal digits of v (0 has one): floor(log10) estimated from the bit length (1233 / 4096 ~ log10 2), corrected by one compare
static __device__ __forceinline__ uint32_t digits10(uint64_t v) {
    v |= 1ull;
    const uint32_t t = ((64u - (uint32_t)__clzll((long long)v)) * 1233u) >> 12;
    return t + 1u - (v < kPow10[t] ? 1u : 0u);
}

__device__ __forceinline__ fmgpu_position load_record(const fmgpu_position* __restrict__ p, uint64_t i, int aligned16) {
    fmgpu_position r;
    if (aligned16) {
        const ulonglong2 a = reinterpret_cast<const ulonglong2*>(p)[2 * i], b = reinterpret_cast<const ulonglong2*>(p)[2 * i + 1];
        r.qidx = a.x; r.seq_id = a.y; r.pos = b.x; r.errors = (uint32_t)b.y; r.hit = (uint32_t)(b.y >> 32);
    } else r = p[i];                                        // (a caller's device array at an odd multiple of 8)
    return r;
}

// record i of p[0 .. count - 1], an array sorted by read (qidx >> shift).  A read of `reads` and more atomicMin's i into *range and the record is to be skipped
// (false); a read below its predecessor's atomicMin's i into *order.  *first / *last: the record starts / ends the run of its read, from its two neighbours.
__device__ __forceinline__ bool run_edges(const fmgpu_position* __restrict__ p, uint64_t count, uint64_t i, uint32_t shift, uint64_t reads, unsigned long long* range,
                                          unsigned long long* order, uint64_t* read, bool* first, bool* last) {
    const uint64_t r = p[i].qidx >> shift;
    *read = r;
    if (r >= reads) { atomicMin(range, (unsigned long long)i); return false; }
    const uint64_t before = i ? p[i - 1].qidx >> shift : ~0ull, behind = i + 1 < count ? p[i + 1].qidx >> shift : ~0ull;
    if (i && before > r) atomicMin(order, (unsigned long long)i);
    *first = before != r; *last = behind != r;
    return true;
}

// the device view of an fmgpu_name_table
struct NameTable { const uint8_t* bytes; uint64_t n_bytes; const fmgpu_text_span* spans; uint64_t count; };
constexpr uint64_t kMaxRowBytes = 1ull << 31;               // a row of this many bytes is refused
enum : uint32_t { ROW_OK = 0, ROW_BEYOND = 1, ROW_SPAN = 2, ROW_LONG = 3 };     // the row lies beyond the table; its span leaves the table's bytes; it is too long

// row `row` of a table: where its bytes start and how many count (stop: up to the first ' ' or '\t').  Checked in the order of the codes; what is refused has no bytes.
__device__ __forceinline__ uint32_t table_row(const NameTable& t, uint64_t row, bool stop, const uint8_t** src, uint32_t* len) {
    *src = t.bytes; *len = 0;
    if (row >= t.count) return ROW_BEYOND;
    const uint64_t o = t.spans[row].offset, n = t.spans[row].len;
    if (n > t.n_bytes || o > t.n_bytes - n) return ROW_SPAN;
    if (n >= kMaxRowBytes) return ROW_LONG;
    const uint8_t* s = t.bytes + o;
    uint64_t m = n;                                         // (counted in the span's own 64 bits)
    if (stop) for (uint64_t j = 0; j < n; ++j) { const uint8_t b = s[j]; if (b == ' ' || b == '\t') { m = j; break; } }
    *src = s; *len = (uint32_t)m;
    return ROW_OK;
}

constexpr uint32_t kTextWindow = 16384;                     // bytes of LDS a workgroup formats into (a multiple of 16)

struct Window {                                             // positions count from a 16-byte piece of the output address; the window holds [lo, lo + kTextWindow)
    uint8_t* lds; uint64_t lo;
    __device__ __forceinline__ void put(uint64_t at, uint32_t b) const { const uint64_t k = at - lo; if (k < kTextWindow) lds[k] = (uint8_t)b; }
};

// v in decimal, its last digit at end - 1: divisions by constants, in 32 bits once the value is below 2^32 (nine digits at a time above)
__device__ __forceinline__ void put_decimal(const Window& w, uint64_t v, uint64_t end) {
    while (v >> 32) {
        const uint64_t q = v / 1000000000ull;
        uint32_t r = (uint32_t)(v - q * 1000000000ull);
#pragma unroll
        for (int k = 0; k < 9; ++k) { w.put(--end, '0' + r % 10u); r /= 10u; }
        v = q;                                              // (>= 4: the loop never leaves a zero behind)
    }
    uint32_t x = (uint32_t)v;
    do { w.put(--end, '0' + x % 10u); x /= 10u; } while (x);
}

// a run of `len` bytes at position `at` against the window's positions [lo, hi): bytes j0 .. j1 - 1 of the run lie inside (none: j0 = j1 = 0)
__device__ __forceinline__ void window_clip(uint64_t lo, uint64_t hi, uint64_t at, uint32_t len, uint32_t* j0, uint32_t* j1) {
    *j0 = 0; *j1 = 0;
    if (len && at < hi && at + len > lo) { *j0 = at < lo ? (uint32_t)(lo - at) : 0u; *j1 = at + len > hi ? (uint32_t)(hi - at) : len; }
}

// positions [from, hi) of the window at lo (lo <= from, lo a multiple of 16, gbase + lo 16-byte aligned) leave LDS for gbase by the 256 lanes of the workgroup: aligned
// 16-byte stores, a piece that [from, hi) covers in part byte by byte.  Nothing is stored below `from` or at `hi` and behind.  The caller synchronises in front of it.
__device__ __forceinline__ void window_flush(const uint8_t* lds, uint8_t* gbase, uint64_t lo, uint64_t from, uint64_t hi) {
    const uint32_t pieces = (uint32_t)((hi - lo + 15u) / 16u);
    for (uint32_t j = threadIdx.x; j < pieces; j += 256u) {
        const uint64_t p0 = lo + 16u * j;
        if (p0 >= from && p0 + 16u <= hi) *reinterpret_cast<uint4*>(gbase + p0) = *reinterpret_cast<const uint4*>(lds + 16u * j);
        else for (uint32_t k = 0; k < 16u; ++k) if (p0 + k >= from && p0 + k < hi) gbase[p0 + k] = lds[16u * j + k];
    }
}

// ---- host side
struct Widen { __host__ __device__ uint64_t operator()(uint32_t v) const { return v; } };      // 32-bit lengths and counts scanned to 64-bit offsets
using Widened = hipcub::TransformInputIterator<uint64_t, Widen, const uint32_t*>;

// a hipcub call is written once, as a callable (void* tmp, size_t& bytes) -> hipError_t around it: asked without a buffer it states the temporary bytes it takes
// (cub_size folds those of several calls into the most that any of them takes and ends at the first that fails), with a buffer of that size it runs (cub_run)
template <class... Calls> inline hipError_t cub_size(size_t* most, Calls&&... calls) {
    hipError_t e = hipSuccess;
    auto one = [&](auto& call) { size_t bytes = 0; e = call(nullptr, bytes); if (bytes > *most) *most = bytes; return e == hipSuccess; };
    (void)(one(calls) && ...);
    return e;
}
template <class Call> inline hipError_t cub_run(Call&& call, const DBuf& tmp) {
    size_t bytes = tmp.bytes;
    return call(tmp.p, bytes);
}

// nothing to report: out_off[0] = 0, in host or device memory
inline int first_offset_zero(uint64_t* out_off, hipStream_t stream) {
    if (!out_off) return 0;
    if (!is_device_pointer(out_off)) { out_off[0] = 0; return 0; }
    FM_HIP(hipMemsetAsync(out_off, 0, 8, stream));
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

// the end of a text call behind its one read-back: `total` bytes in `lines` lines whose offsets stand at doff.  *out_bytes and out_line_off are written, the counting
// call (no out, no capacity) ends here and so does one whose capacity is too small; otherwise `out` is staged and *write says that the caller's write pass is due.
// (The SAM writers stage their read batches behind this, so `out` is allocated in front of them; an empty text stages nothing.)
inline int text_tail(uint64_t total, const uint64_t* doff, uint64_t lines, uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* out_line_off, Staged& sout,
                     hipStream_t stream, bool* write) {
    *write = false;
    *out_bytes = total;
    if (out_line_off) FM_HIP(hipMemcpyAsync(out_line_off, doff, (lines + 1) * 8, hipMemcpyDefault, stream));
    if (!out && !capacity) { FM_HIP(hipStreamSynchronize(stream)); return 0; }
    if (total > capacity) {
        FM_HIP(hipStreamSynchronize(stream));
        return fail(FMGPU_ERR_CAPACITY, "the text takes " + std::to_string(total) + " bytes: more than `capacity`");
    }
    if (const int rc = sout.out(out, total, stream)) { (void)hipStreamSynchronize(stream); return rc; }
    *write = true;
    return 0;
}
// the windows of kTextWindow bytes that `total` bytes at dout touch, counted from the 16-byte piece of the address that holds the first byte
inline uint64_t text_windows(const void* dout, uint64_t total) { return ((reinterpret_cast<uintptr_t>(dout) & 15u) + total + kTextWindow - 1) / kTextWindow; }

// a table that is given (null: nothing to check) has bytes and spans where it states some; spec: the struct the message names, which: the table's member
inline int check_name_table(const fmgpu_name_table* t, const char* spec, const char* which) {
    if (!t) return 0;
    if (!t->bytes && t->n_bytes) return fail(FMGPU_ERR_INVALID, std::string(spec) + ": the " + which + " table has no bytes but n_bytes > 0");
    if (!t->spans && t->count) return fail(FMGPU_ERR_INVALID, std::string(spec) + ": the " + which + " table has no spans but count > 0");
    return 0;
}

// the table's two arrays in device memory (used in place where they are there already), as the kernels' view of them
inline int stage_name_table(const fmgpu_name_table* t, Staged& bytes, Staged& spans, hipStream_t stream, NameTable* out) {
    int rc;
    if ((rc = bytes.in(t->bytes, t->n_bytes, stream)) || (rc = spans.in(t->spans, t->count * sizeof(fmgpu_text_span), stream))) return rc;
    *out = NameTable{(const uint8_t*)bytes.dev, t->n_bytes, (const fmgpu_text_span*)spans.dev, t->count};
    return 0;
}

}  // namespace fmgpu
