// fmgpu_sam_fields.h — what the SAM writers share (fmgpu_sam.hip, fmgpu_sam_mates.hip): what can be wrong with a line and how it is told, a name and a quality string as
// a line takes them from their tables, the frame of the write kernel (its window and the window's lines, found by a whole wave), the fields of a line formatted into the
// LDS window of fmgpu_positions.h, the copy of SEQ and QUAL by whole waves (put_run), and on the host the symbol-to-character tables.  Everything on the device side is
// force-inlined into the kernels of the including unit.  What a line IS (describe) is each unit's own.
#pragma once
#include "fmgpu_positions.h"
#include "fmgpu_pieces.h"

namespace fmgpu {

constexpr uint64_t kMaxSamBytes = kMaxRowBytes;             // a read of this many symbols is refused, as a name or quality string of this many bytes is (table_row)

// why the measure pass refuses a line: as invalid (BAD_*), as unsupported (LONG_*)
enum : uint32_t { BAD_NONE = 0, BAD_RNAME_ROW = 1, BAD_RNAME_SPAN = 2, BAD_QUAL_ROW = 3, BAD_QUAL_SPAN = 4, BAD_QUAL_LEN = 5, BAD_SNAME_ROW = 6, BAD_SNAME_SPAN = 7 };
enum : uint32_t { LONG_NONE = 0, LONG_READ = 1, LONG_NAME = 2, LONG_LINE = 3 };

// table_row for a line: a row that is too long is no invalid line, it makes the line unsupported (where nothing else has yet)
__device__ __forceinline__ uint32_t row_of(const NameTable& t, uint64_t row, bool stop, const uint8_t** src, uint32_t* len, uint32_t* toolong) {
    const uint32_t b = table_row(t, row, stop, src, len);
    if (b != ROW_LONG) return b;
    if (!*toolong) *toolong = LONG_NAME;
    return ROW_OK;
}

// a name as the line writes it: row `id` of table t up to its first blank, or without a table (!use) the number `id` in decimal.  *src = nullptr for the number and for
// an empty name, which is written '*'; *len: the bytes written.  A row that is refused makes the line bad (bad0: BAD_RNAME_ROW or BAD_SNAME_ROW) where nothing has yet.
__device__ __forceinline__ void name_of(const NameTable& t, bool use, uint64_t id, uint32_t bad0, const uint8_t** src, uint32_t* len, uint32_t* bad, uint32_t* toolong) {
    *src = nullptr; *len = digits10(id);
    if (!use) return;
    uint32_t n = 0;
    const uint32_t b = row_of(t, id, true, src, &n, toolong);
    if (b && !*bad) *bad = bad0 + b - 1;
    *len = n ? n : 1u;
    if (!n) *src = nullptr;
}

// the quality string of a read of m symbols, row `row` of its table: *qn bytes at *src, none or m of them; anything else makes the line bad where nothing has yet
__device__ __forceinline__ void qual_of(const NameTable& t, uint64_t row, uint32_t m, const uint8_t** src, uint32_t* qn, uint32_t* bad, uint32_t* toolong) {
    const uint32_t b = row_of(t, row, false, src, qn, toolong);
    if (b && !*bad) *bad = BAD_QUAL_ROW + b - 1;
    else if (!b && !*toolong && *qn != 0 && *qn != m && !*bad) *bad = BAD_QUAL_LEN;
}

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

// the frame of a write kernel.  The OUTPUT is cut into windows of kTextWindow bytes aligned to 16 bytes of the output address, one per workgroup: positions count from
// the 16-byte piece that holds the text's first byte (gbase; the text starts at position `shift`), the window holds positions [from, hi) of [lo, lo + kTextWindow) = bytes
// [from - shift, hi - shift) of the text.  l0: the last line that starts at or before the window's first byte; l1: the first line that starts at or behind its end
// (off[0] = 0 lies in front of that; a line has at least its '\n': the offsets increase strictly).
struct Frame { uint8_t* gbase; uint32_t shift; uint64_t lo, hi, from, l0, l1; };
// the frame of workgroup blockIdx.x for `total` bytes in `lines` lines that start at off[], every wave finding l0 and l1 by itself, and the two symbol tables loaded into
// LDS (tab, 512 bytes; the caller synchronises before it reads them).  false: the window holds no byte of the text (uniform).
__device__ __forceinline__ bool frame_open(const uint8_t* __restrict__ tables, uint8_t* tab, const uint64_t* __restrict__ off, uint64_t lines, uint64_t total, uint8_t* out,
                                           Frame* f) {
    tab[threadIdx.x] = tables[threadIdx.x];
    tab[256u + threadIdx.x] = tables[256u + threadIdx.x];
    f->shift = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
    f->gbase = out - f->shift;                              // position 0: 16-byte aligned, never stored to below position `shift`
    f->lo = (uint64_t)blockIdx.x * kTextWindow;
    const uint64_t extent = f->shift + total;
    f->hi = f->lo + kTextWindow < extent ? f->lo + kTextWindow : extent;
    f->from = f->lo > f->shift ? f->lo : f->shift;
    if (f->from >= f->hi) return false;
    f->l0 = wave_search(off, lines, f->from - f->shift, false);
    f->l1 = wave_search(off, lines, f->hi - f->shift, true) + 1;
    return true;
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

// the runs of a line that its lane leaves to put_run: SEQ and QUAL, their bytes and where they go (len 0: none)
struct Runs { const uint8_t *seq, *qual; uint32_t seq_len, qual_len; uint64_t seq_at, qual_at; };

// a line from SEQ on: '*' or the m symbols at q (deferred), a tab, '*' or the m quality bytes at qual (deferred), then "\tNM:i:<errors>\tNH:i:<nh>\n" for a line with a
// record (tagged) and a bare '\n' for one without
__device__ __forceinline__ void field_tail(const Window& w, uint64_t at, bool star_seq, bool star_qual, uint32_t m, const uint8_t* q, const uint8_t* qual, bool tagged,
                                           uint32_t errors, uint32_t nh, Runs* r) {
    if (star_seq) { w.put(at, '*'); at += 1; } else { r->seq = q; r->seq_len = m; r->seq_at = at; at += m; }
    w.put(at, '\t'); ++at;
    if (star_qual) { w.put(at, '*'); at += 1; } else { r->qual = qual; r->qual_len = m; r->qual_at = at; at += m; }
    if (tagged) {
        at = field_text(w, at, "\tNM:i:", 6);
        at = field_decimal(w, at, errors, '\t');
        at = field_text(w, at, "NH:i:", 5);
        at = field_decimal(w, at, nh, '\n');
    } else w.put(at, '\n');
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

// ---- host side
// spec->strands as a SAM writer takes it (spec: the struct the message names), and with it the SEQ byte of a symbol: tables[0 .. 255] for strand 0, tables[256 .. 511] for
// strand 1 (the complemented symbol's; without strands: the same)
inline int seq_tables(const uint8_t* char_of, const fmgpu_strands* strands, const char* spec, uint8_t* tables) {
    if (strands && !strands->complement) return fail(FMGPU_ERR_INVALID, std::string(spec) + ": strands has a null complement");
    if (strands && (strands->n < 1 || strands->n > 256)) return fail(FMGPU_ERR_INVALID, std::string(spec) + ": strands->n must be in [1, 256]");
    uint8_t comp[256];
    for (int c = 0; c < 256; ++c) comp[c] = (uint8_t)c;
    if (strands) strands_table(strands->complement, strands->n, comp);
    for (int c = 0; c < 256; ++c) { tables[c] = char_of[c]; tables[256 + c] = char_of[comp[c]]; }
    return 0;
}
// what a refused line is told: word = line << 8 | its BAD_* (invalid) or LONG_* code; quals: how the caller names the table of BAD_QUAL_ROW ("the quals", "its quality")
inline std::string line_defect(bool invalid, uint64_t word, const char* quals) {
    static const char* const kBadText[] = {"", "names a row beyond the read_names table", "has a read name span that leaves the table's bytes", nullptr,
                                           "has a quality span that leaves the table's bytes", "has a quality span whose len is neither 0 nor the read's length",
                                           "names a row beyond the seq_names table", "has a sequence name span that leaves the table's bytes"};
    static const char* const kLongText[] = {"", "is a read of 2^31 symbols or more", "has a name or quality span of 2^31 bytes or more", "makes a line of 2^32 bytes or more"};
    const uint32_t code = (uint32_t)(word & 255u);
    if (invalid && code == BAD_QUAL_ROW) return std::string("names a row beyond ") + quals + " table";
    return (invalid ? kBadText : kLongText)[code];
}

}  // namespace fmgpu
