// fmgpu_sam.hip — fmgpu_positions_sam and fmgpu_sam_header (include/fmgpu.h): located hits to SAM records on the device.  Nothing here depends on the row width or
// on an index.  A line is about 220 bytes for 101 bp reads, most of them copied read and quality bytes, so the path is a stream whose stores dominate.  The passes:
//  k_sam_records  one lane per record: read number in range and not below its predecessor's (an offending record atomicMin's its index into an error word), the first
//                 and the last record of each read from the boundaries between neighbours, atomicMin of (errors, index) per read = its primary record
//  k_sam_count    one lane per record: how many records of the read carry its minimal errors (MAPQ)
//  k_sam_reads    one lane per read: the offsets of the batch do not decrease; the lines of the read (its records, or one unmapped line)
//  (hipcub exclusive scan of the line counts: each read's first line)
//  k_sam_measure  one lane per line of the bound count + nq (the number of lines is known on the device only): the line's length as one 32-bit word, names, quality
//                 spans and lengths checked; a line behind the last one measures 0
//  (hipcub exclusive scan of the lengths to 64-bit offsets; the size of the text, the number of lines and the error words are read back together, once)
//  k_sam_write    the OUTPUT is cut into windows of 16 KiB aligned to 16 bytes of the output address, one per workgroup: each wave finds the lines that touch
//                 the window and their reads by searches of 64 probes per step, a lane per line formats the short fields of its part inside the window into LDS, the
//                 waves copy SEQ and QUAL, eight lanes to a field (aligned 16-byte loads, strand 1 reversed in registers, the symbol-to-character tables in LDS), and the
//                 window leaves as aligned 16-byte stores: only the first and last bytes of the text leave byte by byte.  Equal windows balance a heavy-tailed batch by construction.
// Every pass behind the first reads the error words and does nothing once one is set: a batch that is out of order indexes nothing.
// Scratch: 32 bytes per read and 12 bytes per line of the bound, plus the scans' own, freed on return.
// The record loads and run boundaries, digit counts, name tables, the LDS window and its stores and the end of the call behind its read-back are fmgpu_positions.h's, shared
// with fmgpu_format.hip, fmgpu_mates.hip, fmgpu_sam_mates.hip and fmgpu_chain.hip; a line's defects, names and quality string, the frame of the write kernel, the field_*
// helpers and the copy of SEQ and QUAL (put_run) are fmgpu_sam_fields.h's, shared with fmgpu_sam_mates.hip; here: SAM's line (describe).
#include "fmgpu_sam_fields.h"

namespace fmgpu {
namespace {

constexpr uint64_t kMaxSamLines = (1ull << 32) - 256;

// the error words behind the offsets: the lowest record whose read is >= nq; whose read lies below its predecessor's; the lowest read whose offsets decrease; the lowest
// (line << 8 | code) the measure pass refuses as invalid; ... as unsupported (the codes: fmgpu_sam_fields.h); and (no error) the number of lines
enum : int { E_RANGE = 0, E_ORDER = 1, E_QOFF = 2, E_LINE = 3, E_LONG = 4, E_LINES = 5, E_WORDS = 6 };

struct SamArgs {
    const fmgpu_position* pos; uint64_t count;
    const uint8_t* qbuf; const uint64_t* qoff; uint64_t nq;
    NameTable read_names, quals, seq_names;
    uint8_t shift, use_read_names, use_quals, use_seq_names, cigar, emit_unmapped, secondary_seq, mapq_unique, mapq_multi;
    int aligned16;                                          // the records may be loaded as 16-byte pieces
    unsigned long long* key;                                // per read: (errors << 32 | record) of its primary record
    uint32_t *first, *end, *nmin;                           // per read: its first record, one behind its last, its records with the minimal errors
    uint32_t* lcount;                                       // nq + 1: the lines of each read
    uint64_t* lstart;                                       // nq + 1: each read's first line; [nq] = the number of lines
    unsigned long long* err;                                // E_WORDS words
    uint64_t bound;                                         // count + (emit_unmapped ? nq : 0) >= the number of lines
};

__device__ __forceinline__ bool failed(const SamArgs& a) { return (a.err[E_RANGE] & a.err[E_ORDER] & a.err[E_QOFF]) != kNone; }

__global__ __launch_bounds__(256) void k_sam_records(SamArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    uint64_t read;
    bool first, last;
    if (!run_edges(a.pos, a.count, i, a.shift, a.nq, &a.err[E_RANGE], &a.err[E_ORDER], &read, &first, &last)) return;
    if (first) a.first[read] = (uint32_t)i;
    if (last) a.end[read] = (uint32_t)i + 1u;
    atomicMin(&a.key[read], ((unsigned long long)a.pos[i].errors << 32) | (unsigned long long)i);
}

__global__ __launch_bounds__(256) void k_sam_count(SamArgs a) {
    if (failed(a)) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint64_t read = a.pos[i].qidx >> a.shift;
    if ((uint32_t)(a.key[read] >> 32) == a.pos[i].errors) atomicAdd(&a.nmin[read], 1u);
}

__global__ __launch_bounds__(256) void k_sam_reads(SamArgs a) {
    if ((a.err[E_RANGE] & a.err[E_ORDER]) != kNone) return;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > a.nq) return;
    if (r == a.nq) { a.lcount[r] = 0; return; }
    if (a.qoff[r + 1] < a.qoff[r]) atomicMin(&a.err[E_QOFF], (unsigned long long)r);
    const uint32_t f = a.first[r];
    a.lcount[r] = f != kNoRecord32 ? a.end[r] - f : (uint32_t)a.emit_unmapped;
}

// one line of the output: where it comes from and how long its fields are
struct Line {
    uint32_t bad, toolong;
    bool mapped, star_seq, star_qual, star_cigar;
    uint64_t read;
    fmgpu_position rec;                                     // (mapped)
    uint32_t m, flag, mapq, nh;
    const uint8_t *q, *qual, *rname, *sname;                // the read's symbols, its qualities, its name (nullptr: the number), the sequence's name
    uint32_t rn, sn;                                        // bytes of QNAME and of RNAME as written
    uint64_t length;
};

// [lo, hi): reads known to hold the line's (lstart[lo] <= line < lstart[hi])
__device__ __forceinline__ Line describe(const SamArgs& a, uint64_t line, uint64_t lo, uint64_t hi) {
    Line d;                                                 // the last read r with lstart[r] <= line: the one that has lines (lstart increases strictly over such reads)
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.lstart[mid] <= line) lo = mid; else hi = mid; }
    d.read = lo;
    d.bad = BAD_NONE; d.toolong = LONG_NONE;
    const uint32_t first = a.first[lo];
    d.mapped = first != kNoRecord32;
    const uint64_t q0 = a.qoff[lo], m64 = a.qoff[lo + 1] - q0;
    if (m64 >= kMaxSamBytes) d.toolong = LONG_READ;
    d.m = d.toolong ? 0u : (uint32_t)m64;
    d.q = a.qbuf + q0;
    uint32_t strand = 0;
    bool secondary = false;
    d.flag = 4; d.mapq = 0; d.nh = 0;
    d.rec = fmgpu_position{0, 0, 0, 0, 0};
    if (d.mapped) {
        const uint64_t i = first + (line - a.lstart[lo]);
        d.rec = load_record(a.pos, i, a.aligned16);
        strand = a.shift ? (uint32_t)(d.rec.qidx & 1u) : 0u;
        const unsigned long long key = a.key[lo];
        secondary = (uint32_t)key != (uint32_t)i;
        d.flag = (strand ? 16u : 0u) | (secondary ? 256u : 0u);
        d.mapq = !secondary && a.nmin[lo] == 1u ? a.mapq_unique : a.mapq_multi;
        d.nh = a.end[lo] - first;
    }
    name_of(a.read_names, a.use_read_names, d.read, BAD_RNAME_ROW, &d.rname, &d.rn, &d.bad, &d.toolong);
    d.qual = nullptr;
    uint32_t qn = 0;
    if (a.use_quals) qual_of(a.quals, d.read, d.m, &d.qual, &qn, &d.bad, &d.toolong);
    d.sname = nullptr; d.sn = 1;
    if (d.mapped) name_of(a.seq_names, a.use_seq_names, d.rec.seq_id, BAD_SNAME_ROW, &d.sname, &d.sn, &d.bad, &d.toolong);
    d.star_seq = d.m == 0 || (secondary && !a.secondary_seq);
    d.star_qual = d.star_seq || !a.use_quals || qn == 0;
    d.star_cigar = !d.mapped || !a.cigar || d.m == 0;
    // QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ QUAL [NM:i: NH:i:] and eleven or thirteen separators
    uint64_t len = (uint64_t)d.rn + digits10(d.flag) + d.sn + (d.mapped ? digits10(d.rec.pos + 1) : 1u) + digits10(d.mapq) + (d.star_cigar ? 1u : digits10(d.m) + 1u) + 3u +
                   (d.star_seq ? 1u : d.m) + (d.star_qual ? 1u : d.m) + 11u;
    if (d.mapped) len += 5u + digits10(d.rec.errors) + 5u + digits10(d.nh) + 2u;
    if (!d.toolong && (len >> 32)) d.toolong = LONG_LINE;
    d.length = len;
    return d;
}

__global__ __launch_bounds__(256) void k_sam_measure(SamArgs a, uint32_t* __restrict__ lens) {
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > a.bound) return;
    const bool dead = failed(a);
    const uint64_t lines = dead ? 0 : a.lstart[a.nq];
    if (l == a.bound) a.err[E_LINES] = lines;
    if (l >= lines) { lens[l] = 0; return; }
    const Line d = describe(a, l, 0, a.nq);
    if (d.bad) atomicMin(&a.err[E_LINE], (unsigned long long)((l << 8) | d.bad));
    if (d.toolong) atomicMin(&a.err[E_LONG], (unsigned long long)((l << 8) | d.toolong));
    lens[l] = d.bad || d.toolong ? 0u : (uint32_t)d.length;
}

// what a refused line was: out[0] = its read, out[1] = its record (kNone: the read has none)
__global__ void k_sam_explain(SamArgs a, uint64_t line, uint64_t* out) {
    uint64_t lo = 0, hi = a.nq;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (a.lstart[mid] <= line) lo = mid; else hi = mid; }
    out[0] = lo;
    out[1] = a.first[lo] != kNoRecord32 ? a.first[lo] + (line - a.lstart[lo]) : kNone;
}

__global__ __launch_bounds__(256) void k_sam_write(SamArgs a, const uint8_t* __restrict__ tables, const uint64_t* __restrict__ off, uint64_t lines, uint64_t total,
                                                   uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTextWindow];
    __shared__ uint8_t tab[512];                            // the SEQ byte of a symbol: [0, 256) strand 0, [256, 512) strand 1 (complemented)
    Frame f;
    if (!frame_open(tables, tab, off, lines, total, out, &f)) return;
    // r0, r1: the reads of lines l0 and l1 - 1 (lstart[0] = 0), found by every wave like the lines themselves
    const uint64_t r0 = wave_search(a.lstart, a.nq, f.l0, false), r1 = wave_search(a.lstart, a.nq, f.l1 - 1, false);
    __syncthreads();
    const Window w{lds, f.lo};
    const uint64_t hi = f.hi, n = f.l1 - f.l0;
    for (uint64_t base = 0; base < n; base += 256u) {
        const uint64_t j = base + 4u * (threadIdx.x & 63u) + (threadIdx.x >> 6);      // consecutive lines go to the four waves in turn
        Runs r = {nullptr, nullptr, 0, 0, 0, 0};
        uint32_t rev = 0;
        if (j < n) {
            const uint64_t l = f.l0 + j;
            const Line d = describe(a, l, r0, r1 + 1);
            uint64_t at = off[l] + f.shift;
            at = field_name(w, hi, at, d.rname, d.rn, !a.use_read_names, d.read);
            at = field_decimal(w, at, d.flag, '\t');
            if (d.mapped) { at = field_name(w, hi, at, d.sname, d.sn, !a.use_seq_names, d.rec.seq_id); at = field_decimal(w, at, d.rec.pos + 1, '\t'); }
            else at = field_text(w, at, "*\t0\t", 4);
            at = field_decimal(w, at, d.mapq, '\t');
            if (d.star_cigar) at = field_text(w, at, "*\t", 2);
            else { at = field_decimal(w, at, d.m, 'M'); w.put(at, '\t'); ++at; }
            at = field_text(w, at, "*\t0\t0\t", 6);
            rev = d.mapped && a.shift && (d.rec.qidx & 1u) ? 1u : 0u;
            field_tail(w, at, d.star_seq, d.star_qual, d.m, d.q, d.qual, d.mapped, d.rec.errors, d.nh, &r);
        }
        put_run(w, hi, r.seq, r.seq_len, r.seq_at, rev, tab);
        put_run(w, hi, r.qual, r.qual_len, r.qual_at, rev, nullptr);
    }
    __syncthreads();
    window_flush(lds, f.gbase, f.lo, f.from, f.hi);
}

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_positions_sam(const fmgpu_position* positions, uint64_t count, const fmgpu_sam_spec* spec, uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                        uint64_t* out_line_off, uint64_t* out_lines, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!spec) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: spec is null");
    if (!spec->char_of) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: char_of is null");
    if (!out_bytes) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: out_bytes is null");
    const uint64_t nq = spec->nq;
    if (nq && !spec->qbuf) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: qbuf is null while nq > 0");
    if (nq && !spec->qoff) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: qoff is null while nq > 0");
    if (count && !positions) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: positions is null while count > 0");
    if (!out && capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: out is null while capacity > 0");
    if (spec->cigar > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: cigar must be 0 or 1");
    if (spec->emit_unmapped > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: emit_unmapped must be 0 or 1");
    if (spec->secondary_seq > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: secondary_seq must be 0 or 1");
    if (spec->reserved[0] || spec->reserved[1] || spec->reserved[2]) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: reserved must be 0");
    int rc;
    uint8_t tables[512];
    if ((rc = seq_tables(spec->char_of, spec->strands, "fmgpu_sam_spec", tables))) return rc;
    if ((rc = check_name_table(spec->read_names, "fmgpu_sam_spec", "read_names")) || (rc = check_name_table(spec->quals, "fmgpu_sam_spec", "quals")) ||
        (rc = check_name_table(spec->seq_names, "fmgpu_sam_spec", "seq_names"))) return rc;
    *out_bytes = 0;
    if (out_lines) *out_lines = 0;
    const uint64_t bound = count + (spec->emit_unmapped ? nq : 0);
    if (count >= kMaxSamLines || nq >= kMaxSamLines || bound >= kMaxSamLines)
        return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_sam: count, nq and count + (emit_unmapped ? nq : 0), the bound on the lines, must each stay below 2^32 - 256");
    if (bound == 0) return first_offset_zero(out_line_off, stream); // no line

    SamArgs a;
    std::memset(&a, 0, sizeof a);
    a.count = count; a.nq = nq; a.bound = bound;
    a.shift = spec->strands ? 1 : 0;
    a.cigar = spec->cigar; a.emit_unmapped = spec->emit_unmapped; a.secondary_seq = spec->secondary_seq;
    a.mapq_unique = spec->mapq_unique; a.mapq_multi = spec->mapq_multi;

    Staged spos, soff, sq, sbytes[3], sspans[3], sout;
    if ((rc = spos.in(positions, count * sizeof(fmgpu_position), stream))) return rc;
    if (nq && (rc = soff.in(spec->qoff, (nq + 1) * 8, stream))) return rc;
    const fmgpu_name_table* tabs[3] = {spec->read_names, spec->quals, spec->seq_names};
    NameTable* dst[3] = {&a.read_names, &a.quals, &a.seq_names};
    for (int k = 0; k < 3; ++k) if (tabs[k] && (rc = stage_name_table(tabs[k], sbytes[k], sspans[k], stream, dst[k]))) return rc;
    a.use_read_names = spec->read_names != nullptr; a.use_quals = spec->quals != nullptr; a.use_seq_names = spec->seq_names != nullptr;
    a.pos = (const fmgpu_position*)spos.dev;
    a.aligned16 = (reinterpret_cast<uintptr_t>(a.pos) & 15u) == 0;
    a.qoff = (const uint64_t*)soff.dev;

    // per read: key, lstart (8 bytes each), first, end, nmin, lcount (4 bytes each), one entry more than reads; per line of the bound: the offset and the length
    DBuf reads, lens, off, tmp, small;
    if ((rc = reads.alloc((nq + 1) * 32)) || (rc = lens.alloc((bound + 1) * 4)) || (rc = off.alloc((bound + 1 + E_WORDS) * 8)) || (rc = small.alloc(512 + 16))) return rc;
    a.key = reads.as<unsigned long long>();
    a.lstart = reads.as<uint64_t>() + (nq + 1);
    a.first = reinterpret_cast<uint32_t*>(a.lstart + (nq + 1));
    a.end = a.first + (nq + 1); a.nmin = a.end + (nq + 1); a.lcount = a.nmin + (nq + 1);
    uint64_t* const doff = off.as<uint64_t>();
    a.err = reinterpret_cast<unsigned long long*>(doff + bound + 1);
    FM_HIP(hipMemcpyAsync(small.p, tables, 512, hipMemcpyHostToDevice, stream));
    FM_HIP(hipMemsetAsync(a.key, 0xff, (nq + 1) * 8, stream));
    FM_HIP(hipMemsetAsync(a.first, 0xff, (nq + 1) * 4, stream));
    FM_HIP(hipMemsetAsync(a.nmin, 0, (nq + 1) * 4, stream));
    FM_HIP(hipMemsetAsync(a.err, 0xff, E_WORDS * 8, stream));

    Widened lcounts(a.lcount, Widen{}), lengths(lens.as<uint32_t>(), Widen{});
    auto scan_lines = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, lcounts, a.lstart, (size_t)(nq + 1), stream); };
    auto scan_lengths = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, lengths, doff, (size_t)(bound + 1), stream); };
    size_t tb = 0;
    FM_HIP(cub_size(&tb, scan_lines, scan_lengths));
    if ((rc = tmp.alloc(tb))) return rc;
    if (count) {
        FM_GRID(rgrid, count);
        k_sam_records<<<rgrid, dim3(256), 0, stream>>>(a);
        FM_LAUNCHED("k_sam_records");
        k_sam_count<<<rgrid, dim3(256), 0, stream>>>(a);
        FM_LAUNCHED("k_sam_count");
    }
    FM_GRID(qgrid, nq + 1);
    k_sam_reads<<<qgrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_sam_reads");
    FM_HIP(cub_run(scan_lines, tmp));
    FM_GRID(mgrid, bound + 1);
    k_sam_measure<<<mgrid, dim3(256), 0, stream>>>(a, lens.as<uint32_t>());
    FM_LAUNCHED("k_sam_measure");
    FM_HIP(cub_run(scan_lengths, tmp));
    uint64_t back[1 + E_WORDS];                                     // the size of the text, the error words, the number of lines: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, doff + bound, sizeof back, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    const uint64_t* err = back + 1;
    if (err[E_RANGE] != kNone) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: record " + std::to_string(err[E_RANGE]) + " names a read >= nq");
    if (err[E_ORDER] != kNone) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: record " + std::to_string(err[E_ORDER]) + " names a read below its predecessor's");
    if (err[E_QOFF] != kNone) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam: read " + std::to_string(err[E_QOFF]) + " has a qoff above its successor's");
    if (err[E_LINE] != kNone || err[E_LONG] != kNone) {
        const bool invalid = err[E_LINE] != kNone;
        const uint64_t word = invalid ? err[E_LINE] : err[E_LONG];
        uint64_t* const where = reinterpret_cast<uint64_t*>(small.as<uint8_t>() + 512);
        uint64_t who[2] = {0, 0};
        k_sam_explain<<<dim3(1), dim3(1), 0, stream>>>(a, word >> 8, where);
        FM_LAUNCHED("k_sam_explain");
        FM_HIP(hipMemcpyAsync(who, where, 16, hipMemcpyDeviceToHost, stream));
        FM_HIP(hipStreamSynchronize(stream));
        const std::string name = who[1] != kNone ? "record " + std::to_string(who[1]) : "unmapped read " + std::to_string(who[0]);
        return fail(invalid ? FMGPU_ERR_INVALID : FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_sam: " + name + " " + line_defect(invalid, word, "the quals"));
    }
    const uint64_t total = back[0], lines = err[E_LINES];
    if (out_lines) *out_lines = lines;
    bool write;
    if ((rc = text_tail(total, doff, lines, out, capacity, out_bytes, out_line_off, sout, stream, &write)) || !write) return rc;
    if (!total) { FM_HIP(hipStreamSynchronize(stream)); return 0; }
    uint64_t symbols = 0;                                           // the offsets do not decrease: the batch ends at qoff[nq]
    FM_HIP(hipMemcpyAsync(&symbols, a.qoff + nq, 8, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if ((rc = sq.in(spec->qbuf, symbols, stream))) return rc;
    a.qbuf = sq.dev ? (const uint8_t*)sq.dev : spec->qbuf;          // (a batch without a symbol: the pointer is never read through)
    uint8_t* const dout = (uint8_t*)sout.dev;
    FM_GRID(wgrid, text_windows(dout, total) * 256);
    k_sam_write<<<wgrid, dim3(256), 0, stream>>>(a, small.as<uint8_t>(), doff, lines, total, dout);
    FM_LAUNCHED("k_sam_write");
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

int fmgpu_sam_header(const fmgpu_name_table* seq_names, const uint64_t* seq_lengths, uint64_t nseq, const char* program_id, uint8_t* out, uint64_t capacity,
                     uint64_t* out_bytes) {
    if (!out_bytes) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: out_bytes is null");
    if (!out && capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: out is null while capacity > 0");
    if (nseq && !seq_names) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: seq_names is null while nseq > 0");
    if (nseq && !seq_lengths) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: seq_lengths is null while nseq > 0");
    if (nseq && (seq_names->count < nseq || !seq_names->spans || (!seq_names->bytes && seq_names->n_bytes)))
        return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: seq_names holds fewer than nseq rows");
    std::string text = "@HD\tVN:1.6\tSO:unknown\n";
    for (uint64_t s = 0; s < nseq; ++s) {
        const uint64_t o = seq_names->spans[s].offset, n = seq_names->spans[s].len;
        if (n > seq_names->n_bytes || o > seq_names->n_bytes - n) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: sequence " + std::to_string(s) + " has a name span that leaves the table's bytes");
        uint64_t m = 0;
        while (m < n && seq_names->bytes[o + m] != ' ' && seq_names->bytes[o + m] != '\t') ++m;
        if (!m) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_header: sequence " + std::to_string(s) + " has an empty name");
        text += "@SQ\tSN:";
        text.append(reinterpret_cast<const char*>(seq_names->bytes + o), m);
        text += "\tLN:" + std::to_string(seq_lengths[s]) + "\n";
    }
    if (program_id) text += std::string("@PG\tID:") + program_id + "\n";
    *out_bytes = text.size();
    if (!out && !capacity) return 0;
    if (text.size() > capacity) return fail(FMGPU_ERR_CAPACITY, "the header takes " + std::to_string(text.size()) + " bytes: more than `capacity`");
    std::memcpy(out, text.data(), text.size());
    return 0;
}

}  // extern "C"
