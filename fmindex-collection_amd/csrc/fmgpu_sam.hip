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
// The record loads and run boundaries, digit counts, name tables, the LDS window and its stores are fmgpu_positions.h's, shared with fmgpu_format.hip and fmgpu_mates.hip;
// the field_* helpers and the copy of SEQ and QUAL (put_run) are fmgpu_sam_fields.h's, shared with fmgpu_sam_mates.hip; here: SAM's line (describe).
#include "fmgpu_sam_fields.h"

namespace fmgpu {
namespace {

constexpr uint64_t kNone = ~0ull;
constexpr uint32_t kNoRecord32 = 0xffffffffu;
constexpr uint64_t kMaxSamLines = (1ull << 32) - 256;
constexpr uint64_t kMaxSamBytes = kMaxRowBytes;             // a read of this many symbols is refused, as a name or quality string of this many bytes is (table_row)

// the error words behind the offsets: the lowest record whose read is >= nq; whose read lies below its predecessor's; the lowest read whose offsets decrease; the lowest
// (line << 8 | code) the measure pass refuses as invalid; ... as unsupported; and (no error) the number of lines
enum : int { E_RANGE = 0, E_ORDER = 1, E_QOFF = 2, E_LINE = 3, E_LONG = 4, E_LINES = 5, E_WORDS = 6 };
enum : uint32_t { BAD_NONE = 0, BAD_RNAME_ROW = 1, BAD_RNAME_SPAN = 2, BAD_QUAL_ROW = 3, BAD_QUAL_SPAN = 4, BAD_QUAL_LEN = 5, BAD_SNAME_ROW = 6, BAD_SNAME_SPAN = 7 };
enum : uint32_t { LONG_NONE = 0, LONG_READ = 1, LONG_NAME = 2, LONG_LINE = 3 };

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

// table_row for a line: a row that is too long is no invalid line, it makes the line unsupported (where nothing else has yet)
__device__ __forceinline__ uint32_t row_of(const NameTable& t, uint64_t row, bool stop, const uint8_t** src, uint32_t* len, uint32_t* toolong) {
    const uint32_t b = table_row(t, row, stop, src, len);
    if (b != ROW_LONG) return b;
    if (!*toolong) *toolong = LONG_NAME;
    return ROW_OK;
}

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
    uint32_t b, n = 0;
    d.rname = nullptr; d.rn = digits10(d.read);
    if (a.use_read_names) {
        if ((b = row_of(a.read_names, d.read, true, &d.rname, &n, &d.toolong))) d.bad = BAD_RNAME_ROW + b - 1;
        d.rn = n ? n : 1u;
        if (!n) d.rname = nullptr;
    }
    d.qual = nullptr;
    uint32_t qn = 0;
    if (a.use_quals) {
        if ((b = row_of(a.quals, d.read, false, &d.qual, &qn, &d.toolong)) && !d.bad) d.bad = BAD_QUAL_ROW + b - 1;
        else if (!b && !d.toolong && qn != 0 && qn != d.m && !d.bad) d.bad = BAD_QUAL_LEN;
    }
    d.sname = nullptr; d.sn = 1;
    if (d.mapped) {
        d.sn = digits10(d.rec.seq_id);
        if (a.use_seq_names) {
            if ((b = row_of(a.seq_names, d.rec.seq_id, true, &d.sname, &n, &d.toolong)) && !d.bad) d.bad = BAD_SNAME_ROW + b - 1;
            d.sn = n ? n : 1u;
            if (!n) d.sname = nullptr;
        }
    }
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
    tab[threadIdx.x] = tables[threadIdx.x];
    tab[256u + threadIdx.x] = tables[256u + threadIdx.x];
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
    uint8_t* const gbase = out - shift;                     // position 0: 16-byte aligned, never stored to below position `shift`
    const uint64_t lo = (uint64_t)blockIdx.x * kTextWindow, extent = shift + total;
    const uint64_t hi = lo + kTextWindow < extent ? lo + kTextWindow : extent;
    const uint64_t from = lo > shift ? lo : shift;          // the window holds positions [from, hi) of the text = bytes [from - shift, hi - shift)
    if (from >= hi) return;                                 // (uniform)
    const uint64_t o0 = from - shift, o1 = hi - shift;
    // l0: the last line that starts at or before o0; l1: the first line that starts at or behind o1 (off[0] = 0 < o1; a line has at least its '\n': the offsets
    // increase strictly); r0, r1: the reads of lines l0 and l1 - 1 (lstart[0] = 0): every wave finds the four by itself, 64 probes per step
    const uint64_t l0 = wave_search(off, lines, o0, false), l1 = wave_search(off, lines, o1, true) + 1;
    const uint64_t r0 = wave_search(a.lstart, a.nq, l0, false), r1 = wave_search(a.lstart, a.nq, l1 - 1, false);
    __syncthreads();
    const Window w{lds, lo};
    const uint64_t n = l1 - l0;
    for (uint64_t base = 0; base < n; base += 256u) {
        const uint64_t j = base + 4u * (threadIdx.x & 63u) + (threadIdx.x >> 6);      // consecutive lines go to the four waves in turn
        const bool mine = j < n;
        const uint8_t *seq = nullptr, *qual = nullptr;
        uint32_t seq_len = 0, qual_len = 0, rev = 0;
        uint64_t seq_at = 0, qual_at = 0;
        if (mine) {
            const uint64_t l = l0 + j;
            const Line d = describe(a, l, r0, r1 + 1);
            uint64_t at = off[l] + shift;
            at = field_name(w, hi, at, d.rname, d.rn, !a.use_read_names, d.read);
            at = field_decimal(w, at, d.flag, '\t');
            if (d.mapped) { at = field_name(w, hi, at, d.sname, d.sn, !a.use_seq_names, d.rec.seq_id); at = field_decimal(w, at, d.rec.pos + 1, '\t'); }
            else at = field_text(w, at, "*\t0\t", 4);
            at = field_decimal(w, at, d.mapq, '\t');
            if (d.star_cigar) at = field_text(w, at, "*\t", 2);
            else { at = field_decimal(w, at, d.m, 'M'); w.put(at, '\t'); ++at; }
            at = field_text(w, at, "*\t0\t0\t", 6);
            rev = d.mapped && a.shift && (d.rec.qidx & 1u) ? 1u : 0u;
            if (d.star_seq) { w.put(at, '*'); at += 1; } else { seq = d.q; seq_len = d.m; seq_at = at; at += d.m; }
            w.put(at, '\t'); ++at;
            if (d.star_qual) { w.put(at, '*'); at += 1; } else { qual = d.qual; qual_len = d.m; qual_at = at; at += d.m; }
            if (d.mapped) {
                at = field_text(w, at, "\tNM:i:", 6);
                at = field_decimal(w, at, d.rec.errors, '\t');
                at = field_text(w, at, "NH:i:", 5);
                at = field_decimal(w, at, d.nh, '\n');
            } else w.put(at, '\n');
        }
        put_run(w, hi, seq, seq_len, seq_at, rev, tab);
        put_run(w, hi, qual, qual_len, qual_at, rev, nullptr);
    }
    __syncthreads();
    window_flush(lds, gbase, lo, from, hi);
}

const char* const kBadText[] = {"", "names a row beyond the read_names table", "has a read name span that leaves the table's bytes", "names a row beyond the quals table",
                                "has a quality span that leaves the table's bytes", "has a quality span whose len is neither 0 nor the read's length",
                                "names a row beyond the seq_names table", "has a sequence name span that leaves the table's bytes"};
const char* const kLongText[] = {"", "is a read of 2^31 symbols or more", "has a name or quality span of 2^31 bytes or more", "makes a line of 2^32 bytes or more"};

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
    if (spec->strands && !spec->strands->complement) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: strands has a null complement");
    if (spec->strands && (spec->strands->n < 1 || spec->strands->n > 256)) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_spec: strands->n must be in [1, 256]");
    int rc;
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
    uint8_t tables[512], comp[256];
    for (int c = 0; c < 256; ++c) comp[c] = (uint8_t)c;
    if (spec->strands) strands_table(spec->strands->complement, spec->strands->n, comp);
    for (int c = 0; c < 256; ++c) { tables[c] = spec->char_of[c]; tables[256 + c] = spec->char_of[comp[c]]; }

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
    size_t tb1 = 0, tb2 = 0;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb1, lcounts, a.lstart, (size_t)(nq + 1), stream));
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, lengths, doff, (size_t)(bound + 1), stream));
    if ((rc = tmp.alloc(tb1 > tb2 ? tb1 : tb2))) return rc;
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
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb1, lcounts, a.lstart, (size_t)(nq + 1), stream));
    FM_GRID(mgrid, bound + 1);
    k_sam_measure<<<mgrid, dim3(256), 0, stream>>>(a, lens.as<uint32_t>());
    FM_LAUNCHED("k_sam_measure");
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb2, lengths, doff, (size_t)(bound + 1), stream));
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
        return fail(invalid ? FMGPU_ERR_INVALID : FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_sam: " + name + " " + (invalid ? kBadText : kLongText)[word & 255u]);
    }
    const uint64_t total = back[0], lines = err[E_LINES];
    *out_bytes = total;
    if (out_lines) *out_lines = lines;
    if (out_line_off) FM_HIP(hipMemcpyAsync(out_line_off, doff, (lines + 1) * 8, hipMemcpyDefault, stream));
    if (!out && !capacity) { FM_HIP(hipStreamSynchronize(stream)); return 0; }
    if (total > capacity) {
        FM_HIP(hipStreamSynchronize(stream));
        return fail(FMGPU_ERR_CAPACITY, "the text takes " + std::to_string(total) + " bytes: more than `capacity`");
    }
    if (!total) { FM_HIP(hipStreamSynchronize(stream)); return 0; }
    uint64_t symbols = 0;                                           // the offsets do not decrease: the batch ends at qoff[nq]
    FM_HIP(hipMemcpyAsync(&symbols, a.qoff + nq, 8, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if ((rc = sq.in(spec->qbuf, symbols, stream))) return rc;
    a.qbuf = sq.dev ? (const uint8_t*)sq.dev : spec->qbuf;          // (a batch without a symbol: the pointer is never read through)
    if ((rc = sout.out(out, total, stream))) { (void)hipStreamSynchronize(stream); return rc; }
    uint8_t* const dout = (uint8_t*)sout.dev;
    const uint64_t windows = ((reinterpret_cast<uintptr_t>(dout) & 15u) + total + kTextWindow - 1) / kTextWindow;
    FM_GRID(wgrid, windows * 256);
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
