// fmgpu_format.hip — fmgpu_positions_format (include/fmgpu.h): located hits to text lines on the device, the mirror image of fmgpu_queries_parse.  Nothing here depends on
// the row width or on an index.  Three passes over the records:
//  k_format_measure  one lane per record: the record as two 16-byte loads, digit counts from clz and one compare against a power of ten, name lengths from the spans (with
//                    name_stop: a scan of the name for its first blank) -> the line's length as one 32-bit word; an offending record atomicMin's its index into an error word
//  (hipcub exclusive scan of the lengths to 64-bit offsets; the entry behind the last record is the size of the text, read back once together with the error words)
//  k_format_write    a workgroup takes 256 consecutive records = one contiguous range of the output, formats them into LDS at the range's own position modulo 16 of the
//                    OUTPUT ADDRESS, and streams LDS to global memory as aligned 16-byte stores; only the head and tail of the range leave byte by byte.  A range larger
//                    than the LDS window (long names) is walked window by window; a name of 64 bytes and more is copied by its whole wave.
// Scratch: 12 bytes per record (the length word and the offset) and the scan's own, freed on return.
#include "fmgpu_common.h"

#include <hipcub/hipcub.hpp>

namespace fmgpu {

constexpr uint32_t kFormatWindow = 16384;                   // bytes of LDS a workgroup formats into (a multiple of 16)
constexpr uint32_t kWaveCopyFrom = 64;                      // a name this long is copied by the 64 lanes of its wave
constexpr uint64_t kNoRecord = ~0ull;
constexpr uint64_t kMaxNameBytes = 1ull << 31;

struct FormatNames { const uint8_t* bytes; uint64_t n_bytes; const fmgpu_text_span* spans; uint64_t count; };
struct FormatArgs {
    int32_t n_cols;
    uint8_t cols[8];
    uint8_t sep, strand_shift, name_stop, use_read_names, use_seq_names;
    uint64_t pos_add;
    FormatNames read_names, seq_names;
};

__device__ const uint64_t kPow10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull,
                                        100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull,
                                        100000000000000000ull, 1000000000000000000ull, 10000000000000000000ull};

// decimal digits of v (0 has one): floor(log10) estimated from the bit length (1233 / 4096 ~ log10 2), corrected by one compare
__device__ __forceinline__ uint32_t digits10(uint64_t v) {
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

enum : uint32_t { NAME_OK = 0, NAME_ROW = 1, NAME_SPAN = 2, NAME_LONG = 3 };
// row `row` of a name table: where its bytes start and how many count (name_stop: up to the first ' ' or '\t')
__device__ __forceinline__ uint32_t name_of(const FormatNames& t, uint64_t row, uint32_t stop, const uint8_t** src, uint32_t* len) {
    *src = t.bytes; *len = 0;
    if (row >= t.count) return NAME_ROW;
    const uint64_t o = t.spans[row].offset, n = t.spans[row].len;
    if (n > t.n_bytes || o > t.n_bytes - n) return NAME_SPAN;
    if (n >= kMaxNameBytes) return NAME_LONG;
    const uint8_t* s = t.bytes + o;
    uint32_t m = (uint32_t)n;
    if (stop) for (uint32_t j = 0; j < m; ++j) { const uint8_t b = s[j]; if (b == ' ' || b == '\t') { m = j; break; } }
    *src = s; *len = m;
    return NAME_OK;
}

// tail: [0] the lowest record whose name row lies beyond its table, [1] ... whose span leaves the table's bytes, [2] ... whose name or line is too long
__global__ __launch_bounds__(256) void k_format_measure(const fmgpu_position* __restrict__ pos, uint64_t count, FormatArgs a, int aligned16, uint32_t* __restrict__ lens,
                                                        unsigned long long* __restrict__ tail) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > count) return;
    if (i == count) { lens[i] = 0; return; }
    const fmgpu_position r = load_record(pos, i, aligned16);
    const uint64_t read = r.qidx >> a.strand_shift;
    uint32_t bad = NAME_OK, rn = 0, sn = 0;
    const uint8_t* src;
    if (a.use_read_names) bad = name_of(a.read_names, read, a.name_stop, &src, &rn);
    if (a.use_seq_names) { const uint32_t b = name_of(a.seq_names, r.seq_id, a.name_stop, &src, &sn); if (b && (!bad || b < bad)) bad = b; }
    uint64_t n = (uint64_t)a.n_cols;                        // the separators and the '\n'
    for (int c = 0; c < a.n_cols; ++c) {
        switch (a.cols[c]) {
            case FMGPU_COL_QIDX: n += digits10(r.qidx); break;
            case FMGPU_COL_SEQ_ID: n += digits10(r.seq_id); break;
            case FMGPU_COL_POS: n += digits10(r.pos + a.pos_add); break;
            case FMGPU_COL_ERRORS: n += digits10(r.errors); break;
            case FMGPU_COL_HIT: n += digits10(r.hit); break;
            case FMGPU_COL_READ: n += digits10(read); break;
            case FMGPU_COL_STRAND: n += 1; break;
            case FMGPU_COL_READ_NAME: n += rn; break;
            default: n += sn; break;
        }
    }
    if (!bad && (n >> 32)) bad = NAME_LONG;
    if (bad) { atomicMin(&tail[bad - 1], (unsigned long long)i); n = 0; }
    lens[i] = (uint32_t)n;
}

struct Window {                                             // positions count from the range's first byte rounded down to a 16-byte piece of the output address
    uint8_t* lds; uint64_t lo;
    __device__ __forceinline__ void put(uint64_t at, uint32_t b) const { const uint64_t k = at - lo; if (k < kFormatWindow) lds[k] = (uint8_t)b; }
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

// `len` bytes of src at position `at`, the part inside the window: by the lane itself, or (64 bytes and more) by the wave, one byte per lane and step.  Every lane of
// the wave calls it; a lane without a name passes len = 0.
__device__ __forceinline__ void put_name(const Window& w, uint64_t hi, const uint8_t* src, uint32_t len, uint64_t at) {
    uint32_t j0 = 0, j1 = 0;                                // bytes j0 .. j1 - 1 of the name lie in the window
    if (len && at < hi && at + len > w.lo) { j0 = at < w.lo ? (uint32_t)(w.lo - at) : 0u; j1 = at + len > hi ? (uint32_t)(hi - at) : len; }
    const bool wide = j1 - j0 >= kWaveCopyFrom;
    if (!wide) for (uint32_t j = j0; j < j1; ++j) w.lds[at + j - w.lo] = src[j];
    unsigned long long todo = __ballot(wide);
    const uint32_t lane = threadIdx.x & 63u;
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const unsigned long long s = __shfl((unsigned long long)reinterpret_cast<uintptr_t>(src), l), p = __shfl((unsigned long long)at, l);
        const uint32_t b = (uint32_t)__shfl((int)j0, l), e = (uint32_t)__shfl((int)j1, l);
        const uint8_t* from = reinterpret_cast<const uint8_t*>((uintptr_t)s);
        for (uint32_t j = b + lane; j < e; j += 64u) w.lds[p + j - w.lo] = from[j];
    }
}

__global__ __launch_bounds__(256) void k_format_write(const fmgpu_position* __restrict__ pos, uint64_t count, FormatArgs a, int aligned16, const uint64_t* __restrict__ off,
                                                      uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kFormatWindow];
    const uint64_t first = (uint64_t)blockIdx.x * 256u, i = first + threadIdx.x;
    const uint64_t last = first + 256u < count ? first + 256u : count;
    const bool live = i < count;
    const uint64_t b0 = off[first], b1 = off[last];
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(out + b0) & 15u);
    const uint64_t extent = shift + (b1 - b0);              // the range in positions: [shift, extent)
    uint8_t* const gbase = out + b0 - shift;                // position 0: 16-byte aligned, never stored to below position `shift`

    fmgpu_position r = {0, 0, 0, 0, 0};
    uint64_t begin = 0, end = 0, read = 0;
    const uint8_t *rsrc = nullptr, *ssrc = nullptr;
    uint32_t rn = 0, sn = 0;
    if (live) {
        r = load_record(pos, i, aligned16);
        begin = off[i] - b0 + shift; end = off[i + 1] - b0 + shift;
        read = r.qidx >> a.strand_shift;
        if (a.use_read_names) (void)name_of(a.read_names, read, a.name_stop, &rsrc, &rn);
        if (a.use_seq_names) (void)name_of(a.seq_names, r.seq_id, a.name_stop, &ssrc, &sn);
    }
    for (uint64_t lo = 0; lo < extent; lo += kFormatWindow) {
        const uint64_t hi = lo + kFormatWindow < extent ? lo + kFormatWindow : extent;
        const Window w{lds, lo};
        const bool mine = live && begin < hi && end > lo;
        uint64_t at = begin;
        for (int c = 0; c < a.n_cols; ++c) {                // (uniform: every lane of a wave reaches put_name's ballot)
            const uint32_t col = a.cols[c];
            if (col == FMGPU_COL_READ_NAME) { put_name(w, hi, rsrc, mine ? rn : 0u, at); at += rn; }
            else if (col == FMGPU_COL_SEQ_NAME) { put_name(w, hi, ssrc, mine ? sn : 0u, at); at += sn; }
            else if (col == FMGPU_COL_STRAND) { if (mine) w.put(at, a.strand_shift && (r.qidx & 1u) ? '-' : '+'); at += 1; }
            else {
                const uint64_t v = col == FMGPU_COL_QIDX ? r.qidx : col == FMGPU_COL_SEQ_ID ? r.seq_id : col == FMGPU_COL_POS ? r.pos + a.pos_add
                                 : col == FMGPU_COL_ERRORS ? r.errors : col == FMGPU_COL_HIT ? r.hit : read;
                const uint32_t d = digits10(v);
                if (mine) put_decimal(w, v, at + d);
                at += d;
            }
            if (mine) w.put(at, c + 1 < a.n_cols ? a.sep : (uint32_t)'\n');
            at += 1;
        }
        __syncthreads();
        const uint64_t from = lo > shift ? lo : shift;      // what this window holds of the range: positions [from, hi)
        const uint32_t pieces = (uint32_t)((hi - lo + 15u) / 16u);
        for (uint32_t j = threadIdx.x; j < pieces; j += 256u) {
            const uint64_t p0 = lo + 16u * j;
            if (p0 >= from && p0 + 16u <= hi) *reinterpret_cast<uint4*>(gbase + p0) = *reinterpret_cast<const uint4*>(lds + 16u * j);
            else for (uint32_t k = 0; k < 16u; ++k) if (p0 + k >= from && p0 + k < hi) gbase[p0 + k] = lds[16u * j + k];
        }
        __syncthreads();
    }
}

struct WidenLength { __host__ __device__ uint64_t operator()(uint32_t v) const { return v; } };
using Lengths = hipcub::TransformInputIterator<uint64_t, WidenLength, const uint32_t*>;

static int check_names(const fmgpu_name_table* t, const char* which) {
    if (!t) return fail(FMGPU_ERR_INVALID, std::string("fmgpu_format_spec: a ") + which + " column needs the " + which + " table");
    if (!t->bytes && t->n_bytes) return fail(FMGPU_ERR_INVALID, std::string("fmgpu_format_spec: the ") + which + " table has no bytes but n_bytes > 0");
    if (!t->spans && t->count) return fail(FMGPU_ERR_INVALID, std::string("fmgpu_format_spec: the ") + which + " table has no spans but count > 0");
    return 0;
}

}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_positions_format(const fmgpu_position* positions, uint64_t count, const fmgpu_format_spec* spec, uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                           uint64_t* out_line_off, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (count == 0) {
        if (out_bytes) *out_bytes = 0;
        if (!out_line_off) return 0;
        if (!is_device_pointer(out_line_off)) { out_line_off[0] = 0; return 0; }
        FM_HIP(hipMemsetAsync(out_line_off, 0, 8, stream));
        FM_HIP(hipStreamSynchronize(stream));
        return 0;
    }
    if (!spec) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_format: spec is null");
    if (!positions) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_format: positions is null");
    if (!out_bytes) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_format: out_bytes is null");
    if (!out && capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_format: out is null while capacity > 0");
    if (spec->n_cols < 1 || spec->n_cols > 8) return fail(FMGPU_ERR_INVALID, "fmgpu_format_spec: n_cols must be in [1, 8]");
    bool read_names = false, seq_names = false;
    for (int c = 0; c < spec->n_cols; ++c) {
        if (spec->cols[c] > FMGPU_COL_SEQ_NAME) return fail(FMGPU_ERR_INVALID, "fmgpu_format_spec: unknown column code " + std::to_string((int)spec->cols[c]));
        read_names |= spec->cols[c] == FMGPU_COL_READ_NAME;
        seq_names |= spec->cols[c] == FMGPU_COL_SEQ_NAME;
    }
    if (spec->strand_shift > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_format_spec: strand_shift must be 0 or 1");
    if (spec->name_stop > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_format_spec: name_stop must be 0 or 1");
    if (spec->reserved) return fail(FMGPU_ERR_INVALID, "fmgpu_format_spec: reserved must be 0");
    int rc;
    if (read_names && (rc = check_names(spec->read_names, "read_names"))) return rc;
    if (seq_names && (rc = check_names(spec->seq_names, "seq_names"))) return rc;
    *out_bytes = 0;
    FM_GRID(mgrid, count + 1);                                      // (2^32 records and more are refused here, before anything is staged)

    FormatArgs a;
    std::memset(&a, 0, sizeof a);
    a.n_cols = spec->n_cols;
    std::memcpy(a.cols, spec->cols, 8);
    a.sep = spec->sep; a.strand_shift = spec->strand_shift; a.name_stop = spec->name_stop; a.pos_add = spec->pos_add;
    a.use_read_names = read_names; a.use_seq_names = seq_names;
    Staged spos, sbytes[2], sspans[2], sout;
    if ((rc = spos.in(positions, count * sizeof(fmgpu_position), stream))) return rc;
    for (int k = 0; k < 2; ++k) {
        if (!(k ? seq_names : read_names)) continue;
        const fmgpu_name_table* t = k ? spec->seq_names : spec->read_names;
        if ((rc = sbytes[k].in(t->bytes, t->n_bytes, stream)) || (rc = sspans[k].in(t->spans, t->count * sizeof(fmgpu_text_span), stream))) return rc;
        (k ? a.seq_names : a.read_names) = FormatNames{(const uint8_t*)sbytes[k].dev, t->n_bytes, (const fmgpu_text_span*)sspans[k].dev, t->count};
    }
    const fmgpu_position* dpos = (const fmgpu_position*)spos.dev;
    const int aligned16 = (reinterpret_cast<uintptr_t>(dpos) & 15u) == 0;

    DBuf lens, off, tmp;                                            // off: count + 1 offsets, the three error words behind them
    if ((rc = lens.alloc((count + 1) * 4)) || (rc = off.alloc((count + 4) * 8))) return rc;
    uint64_t* const doff = off.as<uint64_t>();
    Lengths lengths(lens.as<uint32_t>(), WidenLength{});
    size_t tb = 0;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, lengths, doff, (size_t)(count + 1), stream));
    if ((rc = tmp.alloc(tb))) return rc;
    FM_HIP(hipMemsetAsync(doff + count + 1, 0xff, 24, stream));
    k_format_measure<<<mgrid, dim3(256), 0, stream>>>(dpos, count, a, aligned16, lens.as<uint32_t>(), reinterpret_cast<unsigned long long*>(doff + count + 1));
    FM_LAUNCHED("k_format_measure");
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, lengths, doff, (size_t)(count + 1), stream));
    uint64_t back[4] = {0, 0, 0, 0};                                // the size of the text and the error words: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, doff + count, 32, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (back[1] != kNoRecord || back[2] != kNoRecord) {
        const bool row = back[1] <= back[2];                        // (of one record, the row is looked at first)
        return fail(FMGPU_ERR_INVALID, "fmgpu_positions_format: record " + std::to_string(row ? back[1] : back[2]) +
                                       (row ? " names a row beyond its name table" : " has a name span that leaves the table's bytes"));
    }
    if (back[3] != kNoRecord) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_format: record " + std::to_string(back[3]) + " has a name of 2^31 bytes or more (or a line of 2^32)");
    const uint64_t total = back[0];
    *out_bytes = total;
    if (out_line_off) FM_HIP(hipMemcpyAsync(out_line_off, doff, (count + 1) * 8, hipMemcpyDefault, stream));
    if (!out && !capacity) { FM_HIP(hipStreamSynchronize(stream)); return 0; }
    if (total > capacity) {
        FM_HIP(hipStreamSynchronize(stream));
        return fail(FMGPU_ERR_CAPACITY, "the text takes " + std::to_string(total) + " bytes: more than `capacity`");
    }
    if ((rc = sout.out(out, total, stream))) { (void)hipStreamSynchronize(stream); return rc; }
    FM_GRID(wgrid, ((count + 255) / 256) * 256);
    k_format_write<<<wgrid, dim3(256), 0, stream>>>(dpos, count, a, aligned16, doff, (uint8_t*)sout.dev);
    FM_LAUNCHED("k_format_write");
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
