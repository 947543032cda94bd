// fmgpu_format.hip — fmgpu_positions_format (include/fmgpu.h): located hits to text lines on the device, the mirror image of fmgpu_queries_parse.  Nothing here depends on
// the row width or on an index.  Three passes over the records:
//  k_format_measure  one lane per record: the record as two 16-byte loads, digit counts from clz and one compare against a power of ten, name lengths from the spans (with
//                    name_stop: a scan of the name for its first blank) -> the line's length as one 32-bit word; an offending record atomicMin's its index into an error word
//  (hipcub exclusive scan of the lengths to 64-bit offsets; the entry behind the last record is the size of the text, read back once together with the error words)
//  k_format_write    a workgroup takes 256 consecutive records = one contiguous range of the output, formats them into LDS at the range's own position modulo 16 of the
//                    OUTPUT ADDRESS, and streams LDS to global memory as aligned 16-byte stores; only the head and tail of the range leave byte by byte.  A range larger
//                    than the LDS window (long names) is walked window by window; a name of 64 bytes and more is copied by its whole wave.
// Scratch: 12 bytes per record (the length word and the offset) and the scan's own, freed on return.
// The record loads, digit counts, name tables, the LDS window and its stores and the end of the call behind its read-back are fmgpu_positions.h's, shared with fmgpu_sam.hip
// and fmgpu_sam_mates.hip; here: the columns and how a name is copied.
#include "fmgpu_positions.h"

namespace fmgpu {

constexpr uint32_t kWaveCopyFrom = 64;                      // a name this long is copied by the 64 lanes of its wave
constexpr uint64_t kNoRecord = ~0ull;

struct FormatArgs {
    int32_t n_cols;
    uint8_t cols[8];
    uint8_t sep, strand_shift, name_stop, use_read_names, use_seq_names;
    uint64_t pos_add;
    NameTable read_names, seq_names;
};

// tail: [0] the lowest record whose name row lies beyond its table, [1] ... whose span leaves the table's bytes, [2] ... whose name or line is too long
__global__ __launch_bounds__(256) void k_format_measure(const fmgpu_position* __restrict__ pos, uint64_t count, FormatArgs a, int aligned16, uint32_t* __restrict__ lens,
                                                        unsigned long long* __restrict__ tail) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > count) return;
    if (i == count) { lens[i] = 0; return; }
    const fmgpu_position r = load_record(pos, i, aligned16);
    const uint64_t read = r.qidx >> a.strand_shift;
    uint32_t bad = ROW_OK, rn = 0, sn = 0;                  // (the ROW_* codes number the words of tail from 1)
    const uint8_t* src;
    if (a.use_read_names) bad = table_row(a.read_names, read, a.name_stop, &src, &rn);
    if (a.use_seq_names) { const uint32_t b = table_row(a.seq_names, r.seq_id, a.name_stop, &src, &sn); if (b && (!bad || b < bad)) bad = b; }
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
    if (!bad && (n >> 32)) bad = ROW_LONG;
    if (bad) { atomicMin(&tail[bad - 1], (unsigned long long)i); n = 0; }
    lens[i] = (uint32_t)n;
}

// `len` bytes of src at position `at`, the part inside the window: by the lane itself, or (64 bytes and more) by the wave, one byte per lane and step.  Every lane of
// the wave calls it; a lane without a name passes len = 0.
__device__ __forceinline__ void put_name(const Window& w, uint64_t hi, const uint8_t* src, uint32_t len, uint64_t at) {
    uint32_t j0, j1;                                        // bytes j0 .. j1 - 1 of the name lie in the window
    window_clip(w.lo, hi, at, len, &j0, &j1);
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
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTextWindow];
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
        if (a.use_read_names) (void)table_row(a.read_names, read, a.name_stop, &rsrc, &rn);
        if (a.use_seq_names) (void)table_row(a.seq_names, r.seq_id, a.name_stop, &ssrc, &sn);
    }
    for (uint64_t lo = 0; lo < extent; lo += kTextWindow) {
        const uint64_t hi = lo + kTextWindow < extent ? lo + kTextWindow : extent;
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
        window_flush(lds, gbase, lo, lo > shift ? lo : shift, hi);      // what this window holds of the range: positions [max(lo, shift), hi)
        __syncthreads();
    }
}

static int check_names(const fmgpu_name_table* t, const char* which) {
    if (!t) return fail(FMGPU_ERR_INVALID, std::string("fmgpu_format_spec: a ") + which + " column needs the " + which + " table");
    return check_name_table(t, "fmgpu_format_spec", which);
}

}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_positions_format(const fmgpu_position* positions, uint64_t count, const fmgpu_format_spec* spec, uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                           uint64_t* out_line_off, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (count == 0) {
        if (out_bytes) *out_bytes = 0;
        return first_offset_zero(out_line_off, stream);
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
    if (read_names && (rc = stage_name_table(spec->read_names, sbytes[0], sspans[0], stream, &a.read_names))) return rc;
    if (seq_names && (rc = stage_name_table(spec->seq_names, sbytes[1], sspans[1], stream, &a.seq_names))) return rc;
    const fmgpu_position* dpos = (const fmgpu_position*)spos.dev;
    const int aligned16 = (reinterpret_cast<uintptr_t>(dpos) & 15u) == 0;

    DBuf lens, off, tmp;                                            // off: count + 1 offsets, the three error words behind them
    if ((rc = lens.alloc((count + 1) * 4)) || (rc = off.alloc((count + 4) * 8))) return rc;
    uint64_t* const doff = off.as<uint64_t>();
    Widened lengths(lens.as<uint32_t>(), Widen{});
    auto scan_lengths = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, lengths, doff, (size_t)(count + 1), stream); };
    size_t tb = 0;
    FM_HIP(cub_size(&tb, scan_lengths));
    if ((rc = tmp.alloc(tb))) return rc;
    FM_HIP(hipMemsetAsync(doff + count + 1, 0xff, 24, stream));
    k_format_measure<<<mgrid, dim3(256), 0, stream>>>(dpos, count, a, aligned16, lens.as<uint32_t>(), reinterpret_cast<unsigned long long*>(doff + count + 1));
    FM_LAUNCHED("k_format_measure");
    FM_HIP(cub_run(scan_lengths, tmp));
    uint64_t back[4] = {0, 0, 0, 0};                                // the size of the text and the error words: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, doff + count, 32, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (back[1] != kNoRecord || back[2] != kNoRecord) {
        const bool row = back[1] <= back[2];                        // (of one record, the row is looked at first)
        return fail(FMGPU_ERR_INVALID, "fmgpu_positions_format: record " + std::to_string(row ? back[1] : back[2]) +
                                       (row ? " names a row beyond its name table" : " has a name span that leaves the table's bytes"));
    }
    if (back[3] != kNoRecord) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_format: record " + std::to_string(back[3]) + " has a name of 2^31 bytes or more (or a line of 2^32)");
    bool write;
    if ((rc = text_tail(back[0], doff, count, out, capacity, out_bytes, out_line_off, sout, stream, &write)) || !write) return rc;
    FM_GRID(wgrid, ((count + 255) / 256) * 256);
    k_format_write<<<wgrid, dim3(256), 0, stream>>>(dpos, count, a, aligned16, doff, (uint8_t*)sout.dev);
    FM_LAUNCHED("k_format_write");
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
