// fmgpu_sam_mates.hip — fmgpu_positions_sam_mates (include/fmgpu.h): the two mates of every fragment as two SAM records with the mate fields filled in, on the device.
// Nothing here depends on the row width or on an index.  A fragment f owns two slots, 2f (mate A) and 2f + 1 (mate B), and slot l IS line l of the output: in separate
// mode record arrays A and B fill the even and the odd slots, in interleaved mode reads 2f and 2f + 1 of the one array are the slots (fmgpu_mates.hip's layout).  The
// number of lines is known on the host, so there is no scan for line starts and no search for a line's read.  The passes:
//  k_sm_records    one lane per record of each array: read number in range and not below its predecessor's, pos < 2^62 (an offending record atomicMin's its index into
//                  an error word), the first and the last record of each slot from the boundaries between neighbours, atomicMin of (errors, index) per slot = the
//                  primary record of its read
//  k_sm_count      one lane per record: how many records of the slot carry its minimal errors (MAPQ of a mate outside a proper fragment)
//  k_sm_pairs      one lane per pair record: fragment, a and b in range and a / b records of mates A / B of that fragment (an offender atomicMin's its index),
//                  atomicMin of (a.errors + b.errors, index) per fragment = its chosen pair
//  k_sm_pair_count one lane per pair record: how many pairs of the fragment carry the minimal sum (MAPQ of a proper fragment)
//  k_sm_fragments  one lane per fragment: the offsets of its two reads do not decrease; the record of each mate: the chosen pair's, else the slot's primary, else none
//  k_sm_measure    one lane per line: the line's length as one 32-bit word, names, quality spans and lengths checked
//  (hipcub exclusive scan of the lengths to 64-bit offsets; the size of the text, the error words and the symbols of the two batches are read back together, once)
//  k_sm_write      the OUTPUT is cut into windows of 16 KiB aligned to 16 bytes of the output address, one per workgroup: each wave finds the lines that touch the window
//                  by a search of 64 probes per step, a lane per line formats the short fields of its part inside the window into LDS, the waves copy SEQ and QUAL, eight
//                  lanes to a field (aligned 16-byte loads, strand 1 reversed in registers), and the window leaves as aligned 16-byte stores.
// No lane loops over the records or the pairs of a fragment: a fragment with thousands of either costs its share of the per-record and per-pair passes.
// Every pass behind the ones that look for an error reads the error words and does nothing once one is set.
// Scratch: 84 bytes per fragment (24 per slot, 12 for the chosen pair, 12 per line for its length and offset), nothing per record and nothing per pair, plus the
// scan's own; freed on return.
// The record loads, digit counts, name tables, the LDS window and the end of the call are fmgpu_positions.h's; the slots, their error words, the records pass, the staging of
// the two sides and the report of those words are fmgpu_mate_slots.h's, shared with fmgpu_mates.hip; a line's defects, names and quality string, the write kernel's frame, the
// field writers and the copy of SEQ and QUAL are fmgpu_sam_fields.h's, shared with fmgpu_sam.hip; here: the choice of each mate's record and the paired line (describe).
#include "fmgpu_sam_fields.h"
#include "fmgpu_mate_slots.h"

namespace fmgpu {
namespace {

// the error words behind the offsets, in the order they are reported: fmgpu_mate_slots.h's eight; the lowest pair that names what does not exist; the lowest
// (line << 8 | code) the measure pass refuses as invalid; ... as unsupported (the codes: fmgpu_sam_fields.h); and (no errors) the symbols of batch A and of batch B
enum : int { E_PAIR = E_MATE_WORDS, E_LINE, E_LONG, E_SYM, E_WORDS = E_SYM + 2 };
enum : uint32_t { NEXT_STAR = 0, NEXT_SAME = 1, NEXT_NAME = 2 };

struct SmArgs {
    const fmgpu_position* pos[2];                           // (interleaved: [1] = [0], and so for count, qbuf, qoff, quals)
    uint64_t count[2];
    const fmgpu_mate_pair* pairs; uint64_t n_pairs;
    const uint8_t* qbuf[2]; const uint64_t* qoff[2];
    uint64_t n, reads;                                      // fragments; reads of a batch (n, interleaved 2 n)
    NameTable read_names, quals[2], seq_names;
    uint8_t shift, interleaved, use_read_names, use_quals[2], use_seq_names, cigar, strip, mapq_unique, mapq_multi;
    int aligned16[2];                                       // the records may be loaded as 16-byte pieces
    unsigned long long* key;                                // per slot: (errors << 32 | record) of the primary record of its read
    uint32_t *first, *end, *nmin, *xrec;                    // per slot: its first record, one behind its last, its records with the minimal errors, the mate's record
    unsigned long long* pkey;                               // per fragment: (error sum << 32 | pair) of its chosen pair
    uint32_t* pcnt;                                         // per fragment: its pairs with the minimal sum
    unsigned long long* err;                                // E_WORDS words
};

__device__ __forceinline__ bool failed_order(const SmArgs& a) { return (a.err[E_RANGE] & a.err[E_RANGE + 1] & a.err[E_ORDER] & a.err[E_ORDER + 1]) != kNone; }
__device__ __forceinline__ bool failed(const SmArgs& a) {
    unsigned long long all = kNone;
#pragma unroll
    for (int k = 0; k <= E_PAIR; ++k) all &= a.err[k];
    return all != kNone;
}

__global__ __launch_bounds__(256) void k_sm_records(SmArgs a, int side) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const fmgpu_position* __restrict__ p = a.pos[side];
    if (i >= a.count[side]) return;
    const uint64_t slot = mate_record(p, a.count[side], i, side, a.shift, a.reads, a.interleaved, a.err, a.first, a.end);
    if (slot != kNone) atomicMin(&a.key[slot], ((unsigned long long)p[i].errors << 32) | (unsigned long long)i);
}

__global__ __launch_bounds__(256) void k_sm_count(SmArgs a, int side) {
    if (failed_order(a)) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count[side]) return;
    const uint64_t read = a.pos[side][i].qidx >> a.shift;
    const uint64_t slot = a.interleaved ? read : 2 * read + (uint64_t)side;
    if ((uint32_t)(a.key[slot] >> 32) == a.pos[side][i].errors) atomicAdd(&a.nmin[slot], 1u);
}

// pair i: its fragment and its error sum; false where it names a fragment or a record that does not exist, or a record of another read than the fragment's mate
__device__ __forceinline__ bool pair_of(const SmArgs& a, uint64_t i, uint64_t* fragment, uint32_t* sum) {
    const fmgpu_mate_pair p = a.pairs[i];
    *fragment = p.fragment; *sum = 0;
    if (p.fragment >= a.n || p.a >= a.count[0] || p.b >= a.count[1]) return false;
    const fmgpu_position ra = a.pos[0][p.a], rb = a.pos[1][p.b];
    const uint64_t want_a = a.interleaved ? 2 * p.fragment : p.fragment, want_b = a.interleaved ? 2 * p.fragment + 1 : p.fragment;
    if ((ra.qidx >> a.shift) != want_a || (rb.qidx >> a.shift) != want_b) return false;
    *sum = ra.errors + rb.errors;
    return true;
}

__global__ __launch_bounds__(256) void k_sm_pairs(SmArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_pairs) return;
    uint64_t f;
    uint32_t sum;
    if (!pair_of(a, i, &f, &sum)) { atomicMin(&a.err[E_PAIR], (unsigned long long)i); return; }
    atomicMin(&a.pkey[f], ((unsigned long long)sum << 32) | (unsigned long long)i);
}

__global__ __launch_bounds__(256) void k_sm_pair_count(SmArgs a) {
    if (a.err[E_PAIR] != kNone) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_pairs) return;
    uint64_t f;
    uint32_t sum;
    if (pair_of(a, i, &f, &sum) && (uint32_t)(a.pkey[f] >> 32) == sum) atomicAdd(&a.pcnt[f], 1u);
}

__global__ __launch_bounds__(256) void k_sm_fragments(SmArgs a) {
    if (failed_order(a)) return;
    const uint64_t f = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= a.n) return;
    for (uint32_t side = 0; side < 2; ++side) {
        const uint64_t r = a.interleaved ? 2 * f + side : f;
        if (a.qoff[side][r + 1] < a.qoff[side][r]) atomicMin(&a.err[E_QOFF + (a.interleaved ? 0 : side)], (unsigned long long)r);
    }
    const unsigned long long chosen = a.pkey[f];
    if (chosen != kNone) {
        const fmgpu_mate_pair p = a.pairs[(uint32_t)chosen];
        a.xrec[2 * f] = p.a; a.xrec[2 * f + 1] = p.b;
    } else {
        for (uint32_t side = 0; side < 2; ++side) a.xrec[2 * f + side] = a.first[2 * f + side] != kNoRecord32 ? (uint32_t)a.key[2 * f + side] : kNoRecord32;
    }
}

// one line of the output: where it comes from and how long its fields are
struct Line {
    uint32_t bad, toolong;
    bool has_x, has_y, star_seq, star_qual, star_cigar, tneg, rname_numbered, rnext_numbered;
    uint64_t f;
    uint32_t m, flag, mapq, nh, rev, errors, rnext_kind;
    uint64_t pos1, pnext1, t, rname_id, rnext_id;           // POS and PNEXT as written; |TLEN|; the seq_id behind RNAME and RNEXT
    const uint8_t *q, *qual, *qname, *rname, *rnext;        // the read's symbols, its qualities, its name (nullptr: the number, or '*'), the sequences' names
    uint32_t qn, sn, nn;                                    // bytes of QNAME, RNAME and RNEXT as written
    uint64_t length;
};

__device__ __forceinline__ Line describe(const SmArgs& a, uint64_t line) {
    Line d;
    const uint32_t side = (uint32_t)(line & 1u), other = side ^ 1u;
    const uint64_t f = line >> 1;
    d.f = f;
    d.bad = BAD_NONE; d.toolong = LONG_NONE;
    const uint64_t row = a.interleaved ? line : f, yrow = a.interleaved ? (line ^ 1u) : f;
    const uint64_t q0 = a.qoff[side][row], m64 = a.qoff[side][row + 1] - q0, my = a.qoff[other][yrow + 1] - a.qoff[other][yrow];
    if (m64 >= kMaxSamBytes) d.toolong = LONG_READ;
    d.m = d.toolong ? 0u : (uint32_t)m64;
    d.q = a.qbuf[side] + q0;
    const uint32_t xi = a.xrec[line], yi = a.xrec[line ^ 1u];
    d.has_x = xi != kNoRecord32; d.has_y = yi != kNoRecord32;
    const fmgpu_position none{0, 0, 0, 0, 0};
    const fmgpu_position x = d.has_x ? load_record(a.pos[side], xi, a.aligned16[side]) : none, y = d.has_y ? load_record(a.pos[other], yi, a.aligned16[other]) : none;
    const uint32_t sx = d.has_x && a.shift ? (uint32_t)(x.qidx & 1u) : 0u, sy = d.has_y && a.shift ? (uint32_t)(y.qidx & 1u) : 0u;
    const bool proper = a.pkey[f] != kNone;
    d.flag = 1u | (side ? 128u : 64u) | (proper ? 2u : 0u) | (d.has_x ? 0u : 4u) | (d.has_y ? 0u : 8u) | (sx ? 16u : 0u) | (sy ? 32u : 0u);
    d.rev = sx;
    d.errors = x.errors;
    d.mapq = !d.has_x ? 0u : (proper ? a.pcnt[f] : a.nmin[line]) == 1u ? a.mapq_unique : a.mapq_multi;
    d.nh = d.has_x ? a.end[line] - a.first[line] : 0u;
    d.qname = nullptr; d.qn = digits10(f);
    if (a.use_read_names) {                                 // (name_of's logic with the "/1" "/2" strip between the lookup and the length)
        uint32_t n = 0;
        if (const uint32_t b = row_of(a.read_names, a.interleaved ? 2 * f : f, true, &d.qname, &n, &d.toolong)) d.bad = BAD_RNAME_ROW + b - 1;
        if (a.strip && n >= 3u && d.qname[n - 2u] == '/' && (d.qname[n - 1u] == '1' || d.qname[n - 1u] == '2')) n -= 2u;
        d.qn = n ? n : 1u;
        if (!n) d.qname = nullptr;
    }
    d.qual = nullptr;
    uint32_t qn = 0;
    if (a.use_quals[side]) qual_of(a.quals[side], row, d.m, &d.qual, &qn, &d.bad, &d.toolong);
    // RNAME and POS: the mate's own, else its mate's; RNEXT and PNEXT: the other mate's, else its own
    d.rname = nullptr; d.sn = 1; d.rname_numbered = false; d.rname_id = 0; d.pos1 = 0;
    d.rnext = nullptr; d.nn = 1; d.rnext_numbered = false; d.rnext_id = 0; d.pnext1 = 0; d.rnext_kind = NEXT_STAR;
    if (d.has_x || d.has_y) {
        const fmgpu_position& at = d.has_x ? x : y;
        d.rname_id = at.seq_id; d.pos1 = at.pos + 1;
        d.rname_numbered = !a.use_seq_names;
        name_of(a.seq_names, a.use_seq_names, d.rname_id, BAD_SNAME_ROW, &d.rname, &d.sn, &d.bad, &d.toolong);
        d.pnext1 = (d.has_y ? y.pos : x.pos) + 1;
        d.rnext_kind = NEXT_SAME;
        if (d.has_x && d.has_y && x.seq_id != y.seq_id) {
            d.rnext_kind = NEXT_NAME; d.rnext_id = y.seq_id; d.rnext_numbered = !a.use_seq_names;
            name_of(a.seq_names, a.use_seq_names, d.rnext_id, BAD_SNAME_ROW, &d.rnext, &d.nn, &d.bad, &d.toolong);
        }
    }
    d.t = 0; d.tneg = false;
    if (d.has_x && d.has_y && x.seq_id == y.seq_id) {        // (pos < 2^62 and reads below 2^62 symbols: no wrap)
        const uint64_t ex = x.pos + m64, ey = y.pos + my;
        d.t = (ex > ey ? ex : ey) - (x.pos < y.pos ? x.pos : y.pos);
        d.tneg = d.t != 0 && (x.pos > y.pos || (x.pos == y.pos && side));
    }
    d.star_seq = d.m == 0;
    d.star_qual = d.star_seq || !a.use_quals[side] || qn == 0;
    d.star_cigar = !d.has_x || !a.cigar || d.m == 0;
    // QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL [NM:i: NH:i:] and eleven or thirteen separators
    uint64_t len = (uint64_t)d.qn + digits10(d.flag) + d.sn + digits10(d.pos1) + digits10(d.mapq) + (d.star_cigar ? 1u : digits10(d.m) + 1u) + d.nn + digits10(d.pnext1) +
                   (d.tneg ? 1u : 0u) + digits10(d.t) + (d.star_seq ? 1u : d.m) + (d.star_qual ? 1u : d.m) + 11u;
    if (d.has_x) len += 5u + digits10(d.errors) + 5u + digits10(d.nh) + 2u;
    if (!d.toolong && (len >> 32)) d.toolong = LONG_LINE;
    d.length = len;
    return d;
}

__global__ __launch_bounds__(256) void k_sm_measure(SmArgs a, uint32_t* __restrict__ lens) {
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l > 2 * a.n) return;
    if (l == 2 * a.n) {                                     // the entry behind the last line; and what the host stages of the two batches (read only if no error is set)
        lens[l] = 0;
        a.err[E_SYM] = a.qoff[0][a.reads]; a.err[E_SYM + 1] = a.qoff[1][a.reads];
        return;
    }
    if (failed(a)) { lens[l] = 0; return; }
    const Line d = describe(a, l);
    if (d.bad) atomicMin(&a.err[E_LINE], (unsigned long long)((l << 8) | d.bad));
    if (d.toolong) atomicMin(&a.err[E_LONG], (unsigned long long)((l << 8) | d.toolong));
    lens[l] = d.bad || d.toolong ? 0u : (uint32_t)d.length;
}

__global__ __launch_bounds__(256) void k_sm_write(SmArgs a, const uint8_t* __restrict__ tables, const uint64_t* __restrict__ off, uint64_t total, uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kTextWindow];
    __shared__ uint8_t tab[512];                            // the SEQ byte of a symbol: [0, 256) strand 0, [256, 512) strand 1 (complemented)
    Frame f;
    if (!frame_open(tables, tab, off, 2 * a.n, total, out, &f)) return;
    __syncthreads();
    const Window w{lds, f.lo};
    const uint64_t hi = f.hi, n = f.l1 - f.l0;
    for (uint64_t base = 0; base < n; base += 256u) {
        const uint64_t j = base + 4u * (threadIdx.x & 63u) + (threadIdx.x >> 6);      // consecutive lines go to the four waves in turn
        Runs r = {nullptr, nullptr, 0, 0, 0, 0};
        uint32_t rev = 0;
        if (j < n) {
            const uint64_t l = f.l0 + j;
            const Line d = describe(a, l);
            uint64_t at = off[l] + f.shift;
            at = field_name(w, hi, at, d.qname, d.qn, !a.use_read_names, d.f);
            at = field_decimal(w, at, d.flag, '\t');
            at = field_name(w, hi, at, d.rname, d.sn, d.rname_numbered, d.rname_id);
            at = field_decimal(w, at, d.pos1, '\t');
            at = field_decimal(w, at, d.mapq, '\t');
            if (d.star_cigar) at = field_text(w, at, "*\t", 2);
            else { at = field_decimal(w, at, d.m, 'M'); w.put(at, '\t'); ++at; }
            if (d.rnext_kind == NEXT_SAME) at = field_text(w, at, "=\t", 2);
            else at = field_name(w, hi, at, d.rnext, d.nn, d.rnext_numbered, d.rnext_id);
            at = field_decimal(w, at, d.pnext1, '\t');
            if (d.tneg) { w.put(at, '-'); ++at; }
            at = field_decimal(w, at, d.t, '\t');
            rev = d.rev;
            field_tail(w, at, d.star_seq, d.star_qual, d.m, d.q, d.qual, d.has_x, d.errors, d.nh, &r);
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

int fmgpu_positions_sam_mates(const fmgpu_position* positions_a, uint64_t count_a, const fmgpu_position* positions_b, uint64_t count_b, const fmgpu_mate_pair* pairs,
                              uint64_t n_pairs, const fmgpu_sam_mates_spec* spec, uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* out_line_off,
                              void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!spec) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: spec is null");
    if (!spec->char_of) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: char_of is null");
    if (!out_bytes) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: out_bytes is null");
    const uint64_t n = spec->n_fragments;
    if (n && !spec->qbuf_a) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: qbuf_a is null while n_fragments > 0");
    if (n && !spec->qoff_a) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: qoff_a is null while n_fragments > 0");
    if (spec->interleaved > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: interleaved must be 0 or 1");
    if (spec->interleaved) {
        if (spec->qbuf_b || spec->qoff_b) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: qbuf_b and qoff_b must be null in interleaved mode");
        if (spec->quals_b) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: quals_b must be null in interleaved mode");
        if (positions_b || count_b) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: positions_b must be null with count_b = 0 in interleaved mode");
    } else {
        if (n && !spec->qbuf_b) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: qbuf_b is null in separate mode while n_fragments > 0");
        if (n && !spec->qoff_b) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: qoff_b is null in separate mode while n_fragments > 0");
        if (count_b && !positions_b) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: positions_b is null while count_b > 0");
    }
    if (count_a && !positions_a) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: positions_a is null while count_a > 0");
    if (n_pairs && !pairs) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: pairs is null while n_pairs > 0");
    if (!out && capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_positions_sam_mates: out is null while capacity > 0");
    if (spec->cigar > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: cigar must be 0 or 1");
    if (spec->strip_mate_suffix > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: strip_mate_suffix must be 0 or 1");
    if (spec->reserved[0] || spec->reserved[1] || spec->reserved[2]) return fail(FMGPU_ERR_INVALID, "fmgpu_sam_mates_spec: reserved must be 0");
    int rc;
    uint8_t tables[512];
    if ((rc = seq_tables(spec->char_of, spec->strands, "fmgpu_sam_mates_spec", tables))) return rc;
    if ((rc = check_name_table(spec->read_names, "fmgpu_sam_mates_spec", "read_names")) || (rc = check_name_table(spec->quals_a, "fmgpu_sam_mates_spec", "quals_a")) ||
        (rc = check_name_table(spec->quals_b, "fmgpu_sam_mates_spec", "quals_b")) || (rc = check_name_table(spec->seq_names, "fmgpu_sam_mates_spec", "seq_names"))) return rc;
    *out_bytes = 0;
    if (count_a >= kMaxMateRecords || count_b >= kMaxMateRecords || n_pairs >= kMaxMateRecords)
        return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_sam_mates: count_a, count_b and n_pairs must each stay below 2^32 - 256");
    if (n >= kMaxFragments) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_positions_sam_mates: n_fragments must stay below 2^31 - 1");
    if (n == 0) return first_offset_zero(out_line_off, stream);    // no line

    const bool inter = spec->interleaved != 0;
    const uint64_t lines = 2 * n;
    SmArgs a;
    std::memset(&a, 0, sizeof a);
    a.n = n; a.reads = inter ? 2 * n : n;
    a.count[0] = count_a; a.count[1] = inter ? count_a : count_b;
    a.n_pairs = n_pairs;
    a.shift = spec->strands ? 1 : 0; a.interleaved = spec->interleaved;
    a.cigar = spec->cigar; a.strip = spec->strip_mate_suffix; a.mapq_unique = spec->mapq_unique; a.mapq_multi = spec->mapq_multi;

    Staged spos[2], spairs, soff[2], sq[2], sbytes[4], sspans[4], sout;
    if ((rc = stage_mate_sides(positions_a, count_a, positions_b, count_b, spec->qoff_a, spec->qoff_b, n, inter, spos, soff, a.pos, a.qoff, stream))) return rc;
    if ((rc = spairs.in(pairs, n_pairs * sizeof(fmgpu_mate_pair), stream))) return rc;
    a.pairs = (const fmgpu_mate_pair*)spairs.dev;
    for (int s = 0; s < 2; ++s) a.aligned16[s] = (reinterpret_cast<uintptr_t>(a.pos[s]) & 15u) == 0;
    const fmgpu_name_table* tabs[4] = {spec->read_names, spec->quals_a, spec->quals_b, spec->seq_names};
    NameTable* dst[4] = {&a.read_names, &a.quals[0], &a.quals[1], &a.seq_names};
    for (int k = 0; k < 4; ++k) if (tabs[k] && (rc = stage_name_table(tabs[k], sbytes[k], sspans[k], stream, dst[k]))) return rc;
    a.use_read_names = spec->read_names != nullptr; a.use_seq_names = spec->seq_names != nullptr;
    a.use_quals[0] = spec->quals_a != nullptr; a.use_quals[1] = spec->quals_b != nullptr;
    if (inter) { a.quals[1] = a.quals[0]; a.use_quals[1] = a.use_quals[0]; }

    // per slot: key (8 bytes), first, end, nmin, xrec (4 bytes each); per fragment: pkey (8), pcnt (4); per line and one more: the length and the offset
    DBuf slots, frags, lens, off, tmp, small;
    if ((rc = slots.alloc(lines * 24)) || (rc = frags.alloc(n * 12)) || (rc = lens.alloc((lines + 1) * 4)) || (rc = off.alloc((lines + 1 + E_WORDS) * 8)) ||
        (rc = small.alloc(512))) return rc;
    a.key = slots.as<unsigned long long>();
    a.first = reinterpret_cast<uint32_t*>(a.key + lines);
    a.end = a.first + lines; a.nmin = a.end + lines; a.xrec = a.nmin + lines;
    a.pkey = frags.as<unsigned long long>();
    a.pcnt = reinterpret_cast<uint32_t*>(a.pkey + n);
    uint64_t* const doff = off.as<uint64_t>();
    a.err = reinterpret_cast<unsigned long long*>(doff + lines + 1);
    FM_HIP(hipMemcpyAsync(small.p, tables, 512, hipMemcpyHostToDevice, stream));
    FM_HIP(hipMemsetAsync(a.key, 0xff, lines * 8, stream));
    FM_HIP(hipMemsetAsync(a.first, 0xff, lines * 4, stream));
    FM_HIP(hipMemsetAsync(a.nmin, 0, lines * 4, stream));
    FM_HIP(hipMemsetAsync(a.pkey, 0xff, n * 8, stream));
    FM_HIP(hipMemsetAsync(a.pcnt, 0, n * 4, stream));
    FM_HIP(hipMemsetAsync(a.err, 0xff, E_WORDS * 8, stream));

    Widened lengths(lens.as<uint32_t>(), Widen{});
    auto scan_lengths = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, lengths, doff, (size_t)(lines + 1), stream); };
    size_t tb = 0;
    FM_HIP(cub_size(&tb, scan_lengths));
    if ((rc = tmp.alloc(tb))) return rc;
    for (int s = 0; s < (inter ? 1 : 2); ++s) if (a.count[s]) {
        FM_GRID(rgrid, a.count[s]);
        k_sm_records<<<rgrid, dim3(256), 0, stream>>>(a, s);
        FM_LAUNCHED("k_sm_records");
    }
    for (int s = 0; s < (inter ? 1 : 2); ++s) if (a.count[s]) {
        FM_GRID(rgrid, a.count[s]);
        k_sm_count<<<rgrid, dim3(256), 0, stream>>>(a, s);
        FM_LAUNCHED("k_sm_count");
    }
    if (n_pairs) {
        FM_GRID(pgrid, n_pairs);
        k_sm_pairs<<<pgrid, dim3(256), 0, stream>>>(a);
        FM_LAUNCHED("k_sm_pairs");
        k_sm_pair_count<<<pgrid, dim3(256), 0, stream>>>(a);
        FM_LAUNCHED("k_sm_pair_count");
    }
    FM_GRID(fgrid, n);
    k_sm_fragments<<<fgrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_sm_fragments");
    FM_GRID(mgrid, lines + 1);
    k_sm_measure<<<mgrid, dim3(256), 0, stream>>>(a, lens.as<uint32_t>());
    FM_LAUNCHED("k_sm_measure");
    FM_HIP(cub_run(scan_lengths, tmp));
    uint64_t back[1 + E_WORDS];                                     // the size of the text, the error words, the symbols of the batches: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, doff + lines, sizeof back, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    const uint64_t* err = back + 1;
    const std::string me = "fmgpu_positions_sam_mates: ";
    if ((rc = mate_errors(err, "fmgpu_positions_sam_mates"))) return rc;
    if (err[E_PAIR] != kNone)
        return fail(FMGPU_ERR_INVALID, me + "pairs: pair " + std::to_string(err[E_PAIR]) + " names a fragment >= n_fragments, a record beyond its array or a record that is not its fragment's mate");
    if (err[E_LINE] != kNone || err[E_LONG] != kNone) {
        const bool invalid = err[E_LINE] != kNone;
        const uint64_t word = invalid ? err[E_LINE] : err[E_LONG], line = word >> 8;
        return fail(invalid ? FMGPU_ERR_INVALID : FMGPU_ERR_UNSUPPORTED,
                    me + "fragment " + std::to_string(line >> 1) + " mate " + (line & 1u ? "B " : "A ") + line_defect(invalid, word, "its quality"));
    }
    const uint64_t total = back[0];
    bool write;
    if ((rc = text_tail(total, doff, lines, out, capacity, out_bytes, out_line_off, sout, stream, &write)) || !write) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    const uint8_t* const qbufs[2] = {spec->qbuf_a, spec->qbuf_b};    // the offsets do not decrease: a batch ends at the last of them
    for (int s = 0; s < (inter ? 1 : 2); ++s) {
        if ((rc = sq[s].in(qbufs[s], err[E_SYM + s], stream))) return rc;
        a.qbuf[s] = sq[s].dev ? (const uint8_t*)sq[s].dev : qbufs[s];  // (a batch without a symbol: the pointer is never read through)
    }
    if (inter) a.qbuf[1] = a.qbuf[0];
    uint8_t* const dout = (uint8_t*)sout.dev;
    FM_GRID(wgrid, text_windows(dout, total) * 256);
    k_sm_write<<<wgrid, dim3(256), 0, stream>>>(a, small.as<uint8_t>(), doff, total, dout);
    FM_LAUNCHED("k_sm_write");
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
