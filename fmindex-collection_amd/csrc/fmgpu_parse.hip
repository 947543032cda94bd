// fmgpu_parse.hip — fmgpu_queries_parse (include/fmgpu.h): LINES / FASTA / FASTQ text to a query batch (qbuf, qoff) on the device.  Nothing here depends on the row
// width or on an index.  The text is walked in chunks of 16 bytes, one per lane and pass (one aligned 16-byte load; the first and last chunk byte by byte):
//  k_count_newlines  '\n' per chunk                     -> hipcub exclusive scan = the line number of every chunk's first byte; the total is the call's first read-back
//  k_line_starts     one word per line: its first byte  (ls[l], and ls[lines] = bytes)
//  k_line_stats      per line (FASTA; FASTQ with `final` or as a feed's piece): lowest header / sequence line, highest header line, header count; highest non-empty line — block-reduced, one atomic per block
//  k_records         one thread: reads and consumed from those; k_validate_fastq per line of a complete record (atomicMin of the offending line); k_settle_error one thread
//  k_symbols<false>  per chunk: the symbols its bytes below `consumed` produce, FOREIGN among them, FASTA headers -> two scans = output position / read number of every chunk
//  (second read-back: counts, error; a text error, the counting call and FMGPU_ERR_CAPACITY return here, before anything is written)
//  k_symbols<true>   the same walk writes qbuf (a lane owns the consecutive output bytes of its chunk), qoff at every read start and the spans
// A byte's role follows from its line number (LINES, FASTQ) or its line's first byte (FASTA: known inside the chunk, or ls[] for the line the chunk starts in).
#include "fmgpu_common.h"

#include <hipcub/hipcub.hpp>

namespace fmgpu {

constexpr uint32_t kNoLine = 0xffffffffu;
constexpr uint64_t kParseMaxBytes = 0xfffffffeull;          // positions and line numbers are 32-bit words on the device

struct ParseAcc {                                           // the device words the passes of one call share
    uint32_t first_hdr, first_seq;                          // FASTA: the lowest header line / non-empty line that is no header (kNoLine: none)
    uint32_t last_hdr1, headers;                            //        the highest header line + 1, the header lines
    uint32_t last_nonempty1;                                // FASTQ with `final` or as a feed's piece: the highest non-empty line + 1
    uint32_t err_line;                                      // the lowest offending line (kNoLine: none)
    uint32_t reads, next_line;                              // next_line: the line number of the first unconsumed byte (a feed's next piece starts there)
    unsigned long long consumed, err_offset, foreign;
};

struct ParseText {
    const uint8_t* p; uint64_t n;
    uint32_t mis;                                           // p & 15: chunk c holds positions 16 c - mis .. 16 c - mis + 15, so every full chunk is one aligned load
    int32_t final, format;
    int32_t piece;                                          // a feed's piece in front of the last one (fmgpu_feed_map_text): what only the bytes behind it can settle is left unconsumed
};

struct Chunk {
    uint32_t w[4];
    int64_t p0;                                             // the position of byte 0 (below 0 in chunk 0 of an unaligned text)
    uint32_t prev, next;                                    // the bytes beside the chunk: '\n' in front of position 0; behind the last byte '\n' when `final`, else 0
    __device__ uint32_t at(int i) const { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }
};

template <bool NEIGHBOURS>
__device__ inline void load_chunk(const ParseText& t, uint64_t c, Chunk& k) {
    const int64_t p0 = (int64_t)(16 * c) - (int64_t)t.mis;
    k.p0 = p0;
    if (p0 >= 0 && (uint64_t)p0 + 16 <= t.n) {
        const uint4 v = *reinterpret_cast<const uint4*>(t.p + p0);
        k.w[0] = v.x; k.w[1] = v.y; k.w[2] = v.z; k.w[3] = v.w;
    } else {
        k.w[0] = k.w[1] = k.w[2] = k.w[3] = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t p = p0 + i;
            if (p >= 0 && (uint64_t)p < t.n) k.w[i >> 2] |= (uint32_t)t.p[p] << (8 * (i & 3));
        }
    }
    if (NEIGHBOURS) {
        k.prev = p0 > 0 ? t.p[p0 - 1] : (uint32_t)'\n';
        k.next = (uint64_t)(p0 + 16) < t.n ? t.p[p0 + 16] : (t.final ? (uint32_t)'\n' : 0u);
    }
}

__global__ __launch_bounds__(256) void k_count_newlines(ParseText t, uint64_t nchunks, uint32_t* __restrict__ cnt) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > nchunks) return;
    uint32_t lines = 0;
    if (c < nchunks) {
        Chunk k; load_chunk<false>(t, c, k);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t p = k.p0 + i;
            lines += (p >= 0 && (uint64_t)p < t.n && k.at(i) == '\n') ? 1u : 0u;
        }
    }
    cnt[c] = lines;                                         // entry nchunks: 0, the scan leaves the total there
}

// ls[l] = the first byte of line l for l = 0 .. nl (one behind every '\n'), ls[lines] = n (lines = nl, or nl + 1 when the text does not end in '\n')
__global__ __launch_bounds__(256) void k_line_starts(ParseText t, uint64_t nchunks, const uint32_t* __restrict__ lnbase, uint32_t nl, uint32_t lines, uint32_t* __restrict__ ls) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchunks) return;
    if (c == 0) { ls[0] = 0; if (lines > nl) ls[lines] = (uint32_t)t.n; }
    Chunk k; load_chunk<false>(t, c, k);
    uint32_t l = lnbase[c];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t p = k.p0 + i;
        if (p >= 0 && (uint64_t)p < t.n && k.at(i) == '\n') { ++l; if (l <= nl) ls[l] = (uint32_t)(p + 1); }
    }
}

// the end of line l without its terminator ('\n', and a '\r' in front of it or as the last byte of a `final` text)
__device__ inline uint32_t line_end(const ParseText& t, const uint32_t* __restrict__ ls, uint32_t l, uint32_t nl) {
    const uint32_t s = ls[l];
    uint32_t e = ls[l + 1] - (l < nl ? 1u : 0u);
    if (e > s && t.p[e - 1] == '\r' && (l < nl || t.final)) --e;
    return e;
}

struct OpMin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct OpMax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct OpSum { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
// over the 256 threads of a block (every thread calls it); `lds` holds four words
template <class Op>
__device__ inline uint32_t block_reduce(uint32_t v, Op op, uint32_t* lds) {
    for (int o = 32; o; o >>= 1) v = op(v, (uint32_t)__shfl_xor((int)v, o));
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(lds[0], lds[1]), op(lds[2], lds[3]));
}

__global__ __launch_bounds__(256) void k_line_stats(ParseText t, const uint32_t* __restrict__ ls, uint32_t nl, uint32_t lines, ParseAcc* acc) {
    __shared__ uint32_t lds[4];
    const uint64_t l64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = l64 < lines;
    const uint32_t l = (uint32_t)l64;
    bool nonempty = false, hdr = false;
    if (live) {
        const uint32_t s = ls[l];
        uint32_t e = line_end(t, ls, l, nl);
        if (t.piece && l >= nl && e > s && t.p[e - 1] == '\r') --e;                      // an unterminated "\r": the '\n' may follow in the next window
        nonempty = e > s;
        hdr = nonempty && t.p[s] == '>';
    }
    if (t.format == FMGPU_TEXT_FASTA) {
        const uint32_t fh = block_reduce(hdr ? l : kNoLine, OpMin(), lds);
        const uint32_t fs = block_reduce(nonempty && !hdr ? l : kNoLine, OpMin(), lds);
        const uint32_t lh = block_reduce(hdr ? l + 1 : 0u, OpMax(), lds);
        const uint32_t nh = block_reduce(hdr ? 1u : 0u, OpSum(), lds);
        if (threadIdx.x == 0) {
            if (fh != kNoLine) atomicMin(&acc->first_hdr, fh);
            if (fs != kNoLine) atomicMin(&acc->first_seq, fs);
            if (nh) { atomicMax(&acc->last_hdr1, lh); atomicAdd(&acc->headers, nh); }
        }
    } else {
        const uint32_t ln = block_reduce(nonempty ? l + 1 : 0u, OpMax(), lds);
        if (threadIdx.x == 0 && ln) atomicMax(&acc->last_nonempty1, ln);
    }
}

// the complete records and where they end (include/fmgpu.h has the rules)
__global__ void k_records(ParseText t, const uint32_t* __restrict__ ls, uint32_t nl, uint32_t lines, ParseAcc* acc) {
    uint32_t reads = 0, err = kNoLine;
    uint64_t consumed = 0;
    if (t.format == FMGPU_TEXT_LINES) {
        reads = t.final ? lines : nl;
        consumed = ls[reads];
    } else if (t.format == FMGPU_TEXT_FASTA) {
        if (acc->first_seq < acc->first_hdr) err = acc->first_seq;                      // text before the first header
        else if (t.final) { reads = acc->headers; consumed = t.n; }
        else if (acc->headers >= 2) { reads = acc->headers - 1; consumed = ls[acc->last_hdr1 - 1]; }
    } else {
        // `final`: empty lines at the very end are discarded first; a piece leaves them (and the record they may truncate) to the pieces behind it
        const uint32_t have = t.final ? acc->last_nonempty1 : (t.piece && acc->last_nonempty1 < nl ? acc->last_nonempty1 : nl);
        reads = have / 4;
        consumed = ls[4 * reads];
        if (t.final && (have & 3u)) err = 4 * reads;                                    // a truncated record
    }
    acc->reads = reads; acc->consumed = consumed; acc->err_line = err;
    acc->next_line = t.format == FMGPU_TEXT_LINES ? reads : t.format == FMGPU_TEXT_FASTQ ? 4 * reads : (consumed && !t.final ? acc->last_hdr1 - 1 : (consumed ? lines : 0u));
}

__global__ __launch_bounds__(256) void k_validate_fastq(ParseText t, const uint32_t* __restrict__ ls, uint32_t nl, ParseAcc* acc) {
    const uint64_t l64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l64 >= 4ull * acc->reads) return;
    const uint32_t l = (uint32_t)l64, role = l & 3u, s = ls[l];
    bool ok = true;
    if (role == 0 || role == 2) ok = line_end(t, ls, l, nl) > s && t.p[s] == (role == 0 ? '@' : '+');
    else if (role == 3) ok = line_end(t, ls, l, nl) - s == line_end(t, ls, l - 2, nl) - ls[l - 2];
    if (!ok) atomicMin(&acc->err_line, l);
}

// a text error: the counts describe the records in front of the offending one
__global__ void k_settle_error(ParseText t, const uint32_t* __restrict__ ls, ParseAcc* acc) {
    const uint32_t err = acc->err_line;
    if (err == kNoLine) return;
    acc->err_offset = ls[err];
    const uint32_t reads = t.format == FMGPU_TEXT_FASTQ ? err / 4 : 0u;
    acc->reads = reads;
    acc->consumed = t.format == FMGPU_TEXT_FASTQ ? ls[4 * reads] : 0u;
    acc->next_line = 4 * reads;
}

struct ParseOut { uint8_t* qbuf; uint64_t* qoff; fmgpu_text_span* names; fmgpu_text_span* quals; };

// WRITE = false: kcnt[c] = the symbols chunk c produces, hcnt[c] = the FASTA headers it holds (positions below `consumed` only), FOREIGN symbols added to acc->foreign.
// WRITE = true: kcnt / hcnt hold their exclusive scans; symbols, offsets and spans are written.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_symbols(ParseText t, uint64_t nchunks, const uint8_t* __restrict__ symbol_of, const uint32_t* __restrict__ lnbase,
                                                 const uint32_t* __restrict__ ls, uint32_t nl, ParseAcc* acc, uint32_t* __restrict__ kcnt, uint32_t* __restrict__ hcnt, ParseOut out) {
    __shared__ uint8_t table[256];
    __shared__ uint32_t lds[4];
    table[threadIdx.x] = symbol_of[threadIdx.x];
    __syncthreads();
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t consumed = acc->consumed;
    const int32_t format = t.format;
    uint32_t kept = 0, hdrs = 0, foreign = 0;
    if (c < nchunks) {
        Chunk k; load_chunk<true>(t, c, k);
        if (k.p0 < (int64_t)consumed) {
            uint32_t l = lnbase[c];
            bool seq = true;                                                            // FASTA: the current line is a sequence line
            if (format == FMGPU_TEXT_FASTA) seq = t.p[ls[l]] != '>';
            uint64_t o = WRITE ? kcnt[c] : 0;
            uint32_t r = WRITE && format == FMGPU_TEXT_FASTA ? hcnt[c] : 0;
            uint32_t pb = k.prev;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int64_t p = k.p0 + i;
                if (p < 0 || (uint64_t)p >= consumed) continue;
                const uint32_t b = k.at(i);
                const uint32_t nb = (uint64_t)(p + 1) < t.n ? (i < 15 ? k.at(i < 15 ? i + 1 : 15) : k.next) : (t.final ? (uint32_t)'\n' : 0u);
                if (pb == '\n') {                                                       // p starts line l
                    if (format == FMGPU_TEXT_FASTA) {
                        seq = b != '>';
                        if (!seq) {
                            if (WRITE) {
                                out.qoff[r] = o;
                                if (out.names) { out.names[r].offset = (uint64_t)p + 1; out.names[r].len = line_end(t, ls, l, nl) - (uint32_t)(p + 1); }
                                if (out.quals) { out.quals[r].offset = 0; out.quals[r].len = 0; }
                            }
                            ++r; ++hdrs;
                        }
                    } else if (WRITE) {
                        if (format == FMGPU_TEXT_LINES) {
                            out.qoff[l] = o;
                            if (out.names) { out.names[l].offset = 0; out.names[l].len = 0; }
                            if (out.quals) { out.quals[l].offset = 0; out.quals[l].len = 0; }
                        } else if ((l & 3u) == 0) {
                            out.qoff[l >> 2] = o;
                            if (out.names) { out.names[l >> 2].offset = (uint64_t)p + 1; out.names[l >> 2].len = line_end(t, ls, l, nl) - (uint32_t)(p + 1); }
                        } else if ((l & 3u) == 3 && out.quals) {
                            out.quals[l >> 2].offset = (uint64_t)p; out.quals[l >> 2].len = line_end(t, ls, l, nl) - (uint32_t)p;
                        }
                    }
                }
                const bool term = b == '\n' || (b == '\r' && nb == '\n');
                const bool in_seq = format == FMGPU_TEXT_FASTQ ? (l & 3u) == 1 : seq;
                if (in_seq && !term) {
                    const uint32_t v = table[b];
                    if (v != FMGPU_SYM_DROP) {
                        if (WRITE) out.qbuf[o] = (uint8_t)v;
                        ++o; ++kept;
                        foreign += v == FMGPU_SYM_FOREIGN ? 1u : 0u;
                    }
                }
                if (b == '\n') ++l;
                pb = b;
            }
        }
    }
    if (WRITE) {
        if (c == 0) out.qoff[acc->reads] = kcnt[nchunks];                               // the end of the last read = the symbols of the call
        return;
    }
    if (c <= nchunks) { kcnt[c] = kept; if (format == FMGPU_TEXT_FASTA) hcnt[c] = hdrs; }
    const uint32_t f = block_reduce(foreign, OpSum(), lds);
    if (threadIdx.x == 0 && f) atomicAdd(&acc->foreign, (unsigned long long)f);
}

// a feed's piece (fmgpu_feed_map_text): the spans of its reads become spans of the caller's text (offset += base, in 64 bits), lens[r] = the read's symbols.  A lane
// moves one span as one 16-byte word: consecutive lanes, consecutive words.
__global__ __launch_bounds__(256) void k_piece_spans(fmgpu_text_span* __restrict__ names, fmgpu_text_span* __restrict__ quals, uint64_t* __restrict__ lens,
                                                     const uint64_t* __restrict__ qoff, uint64_t reads, uint64_t base, int32_t shift_names, int32_t shift_quals) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < reads; r += (uint64_t)gridDim.x * blockDim.x) {
        if (names && shift_names) { ulonglong2 v = reinterpret_cast<ulonglong2*>(names)[r]; v.x += base; reinterpret_cast<ulonglong2*>(names)[r] = v; }
        if (quals && shift_quals) { ulonglong2 v = reinterpret_cast<ulonglong2*>(quals)[r]; v.x += base; reinterpret_cast<ulonglong2*>(quals)[r] = v; }
        if (lens) lens[r] = qoff[r + 1] - qoff[r];
    }
}

int parse_piece_spans(fmgpu_text_span* names, fmgpu_text_span* quals, uint64_t* lens, const uint64_t* qoff, uint64_t reads, uint64_t base, int32_t format, hipStream_t stream) {
    const bool shift_names = base && format != FMGPU_TEXT_LINES, shift_quals = base && format == FMGPU_TEXT_FASTQ;      // (the other spans are {0, 0})
    if (!reads || (!lens && !(names && shift_names) && !(quals && shift_quals))) return 0;
    dim3 grid; if (int rc = grid_of(reads, &grid, 1u << 16)) return rc;
    k_piece_spans<<<grid, dim3(256), 0, stream>>>(names, quals, lens, qoff, reads, base, shift_names ? 1 : 0, shift_quals ? 1 : 0);
    FM_LAUNCHED("k_piece_spans");
    return 0;
}

static int exclusive_sum(MapBuffer* tmp, size_t tmp_bytes, uint32_t* words, uint64_t count, hipStream_t stream) {
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp->p, tmp_bytes, words, words, (size_t)count, stream));
    return 0;
}

static const char* text_error(int32_t format, uint64_t line) {
    if (format == FMGPU_TEXT_FASTA) return "a non-empty line in front of the first '>' header";
    switch (line & 3u) {
        case 0: return "a FASTQ record must start with an '@' header line and have four lines";
        case 2: return "the third line of a FASTQ record must start with '+'";
        default: return "a FASTQ quality line must be as long as its sequence line";
    }
}

// The passes of fmgpu_queries_parse on device text and on the caller's growing buffers (fmgpu_common.h): the one-shot call below hands it per-call buffers, a feed the
// buffers of a slot.  bytes > 0.  Two read-backs synchronise `stream`.  *result describes this text alone; the message of a text error names line_base + the line and
// offset_base + the offset (a feed's piece: its place in the caller's text), and *text_error tells it from the other causes of FMGPU_ERR_INVALID.
int parse_device(const uint8_t* dtext, uint64_t bytes, int32_t format, int32_t final, int32_t piece, const uint8_t* dtable, ParseBuffers* b, bool counting,
                 uint64_t symbol_capacity, uint64_t read_capacity, uint64_t line_base, uint64_t offset_base, fmgpu_parse_result* result, uint64_t* next_line,
                 bool* is_text_error, hipStream_t stream) {
    std::memset(result, 0, sizeof *result);
    if (next_line) *next_line = 0;
    if (is_text_error) *is_text_error = false;
    if (bytes > kParseMaxBytes) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_queries_parse takes at most 2^32 - 2 bytes per call: parse the text in chunks, each starting at the previous call's `consumed`");
    int rc;
    ParseText t;
    t.p = dtext; t.n = bytes; t.mis = (uint32_t)((uintptr_t)dtext & 15u); t.final = final ? 1 : 0; t.format = format; t.piece = piece && !final ? 1 : 0;
    const uint64_t nchunks = (t.mis + bytes + 15) / 16;
    const bool fasta = format == FMGPU_TEXT_FASTA;

    if ((rc = b->acc->need(sizeof(ParseAcc))) || (rc = b->lnbase->need((nchunks + 1) * 4)) || (rc = b->kcnt->need((nchunks + 1) * 4))) return rc;
    if (fasta && (rc = b->hcnt->need((nchunks + 1) * 4))) return rc;
    uint32_t* const lnbase = reinterpret_cast<uint32_t*>(b->lnbase->p);
    uint32_t* const kcnt = reinterpret_cast<uint32_t*>(b->kcnt->p);
    uint32_t* const hcnt = reinterpret_cast<uint32_t*>(b->hcnt->p);
    size_t tb = 0;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, lnbase, lnbase, (size_t)(nchunks + 1), stream));
    if ((rc = b->tmp->need(tb ? tb : 8))) return rc;
    ParseAcc acc;
    std::memset(&acc, 0, sizeof acc);
    acc.first_hdr = acc.first_seq = acc.err_line = kNoLine;
    FM_HIP(hipMemcpyAsync(b->acc->p, &acc, sizeof acc, hipMemcpyHostToDevice, stream));
    ParseAcc* dacc = reinterpret_cast<ParseAcc*>(b->acc->p);

    FM_GRID(cgrid, nchunks + 1);
    k_count_newlines<<<cgrid, dim3(256), 0, stream>>>(t, nchunks, lnbase);
    FM_LAUNCHED("k_count_newlines");
    if ((rc = exclusive_sum(b->tmp, tb, lnbase, nchunks + 1, stream))) return rc;
    uint32_t nl = 0;
    uint8_t last = 0;
    FM_HIP(hipMemcpyAsync(&nl, lnbase + nchunks, 4, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipMemcpyAsync(&last, t.p + bytes - 1, 1, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    const uint32_t lines = nl + (last != '\n' ? 1u : 0u);                              // >= 1: the text is not empty

    if ((rc = b->ls->need(((size_t)lines + 1) * 4))) return rc;
    uint32_t* const ls = reinterpret_cast<uint32_t*>(b->ls->p);
    k_line_starts<<<cgrid, dim3(256), 0, stream>>>(t, nchunks, lnbase, nl, lines, ls);
    FM_LAUNCHED("k_line_starts");
    FM_GRID(lgrid, lines);
    if (fasta || (format == FMGPU_TEXT_FASTQ && (t.final || t.piece))) {
        k_line_stats<<<lgrid, dim3(256), 0, stream>>>(t, ls, nl, lines, dacc);
        FM_LAUNCHED("k_line_stats");
    }
    k_records<<<dim3(1), dim3(1), 0, stream>>>(t, ls, nl, lines, dacc);
    FM_LAUNCHED("k_records");
    if (format == FMGPU_TEXT_FASTQ) {
        k_validate_fastq<<<lgrid, dim3(256), 0, stream>>>(t, ls, nl, dacc);
        FM_LAUNCHED("k_validate_fastq");
    }
    if (format != FMGPU_TEXT_LINES) {
        k_settle_error<<<dim3(1), dim3(1), 0, stream>>>(t, ls, dacc);
        FM_LAUNCHED("k_settle_error");
    }
    ParseOut none = {nullptr, nullptr, nullptr, nullptr};
    k_symbols<false><<<cgrid, dim3(256), 0, stream>>>(t, nchunks, dtable, lnbase, ls, nl, dacc, kcnt, hcnt, none);
    FM_LAUNCHED("k_symbols<false>");
    if ((rc = exclusive_sum(b->tmp, tb, kcnt, nchunks + 1, stream))) return rc;
    if (fasta && (rc = exclusive_sum(b->tmp, tb, hcnt, nchunks + 1, stream))) return rc;
    uint32_t symbols = 0;
    FM_HIP(hipMemcpyAsync(&acc, dacc, sizeof acc, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipMemcpyAsync(&symbols, kcnt + nchunks, 4, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));

    result->reads = acc.reads; result->symbols = symbols; result->consumed = acc.consumed; result->foreign = acc.foreign;
    if (next_line) *next_line = acc.next_line;
    if (acc.err_line != kNoLine) {
        result->error_line = acc.err_line; result->error_offset = acc.err_offset;
        if (is_text_error) *is_text_error = true;
        return fail(FMGPU_ERR_INVALID, "text error in line " + std::to_string(line_base + acc.err_line) + " (0-based, byte offset " + std::to_string(offset_base + acc.err_offset) + "): " + text_error(format, acc.err_line));
    }
    if (counting) return 0;
    if (symbols > symbol_capacity || acc.reads > read_capacity)
        return fail(FMGPU_ERR_CAPACITY, "the text holds " + std::to_string(acc.reads) + " reads of " + std::to_string(symbols) + " symbols: more than the output buffers take");

    if ((rc = b->qbuf->need((size_t)symbols + b->qpad)) || (rc = b->qoff->need(((size_t)acc.reads + 1) * 8))) return rc;
    if (b->names && (rc = b->names->need((size_t)acc.reads * sizeof(fmgpu_text_span)))) return rc;
    if (b->quals && (rc = b->quals->need((size_t)acc.reads * sizeof(fmgpu_text_span)))) return rc;
    ParseOut out = {(uint8_t*)b->qbuf->p, (uint64_t*)b->qoff->p, b->names ? (fmgpu_text_span*)b->names->p : nullptr, b->quals ? (fmgpu_text_span*)b->quals->p : nullptr};
    k_symbols<true><<<cgrid, dim3(256), 0, stream>>>(t, nchunks, dtable, lnbase, ls, nl, dacc, kcnt, hcnt, out);
    FM_LAUNCHED("k_symbols<true>");
    return 0;
}

namespace {

struct OwnScratch : MapBuffer {                                     // the one-shot call's scratch: freed on return
    DBuf d;
    int need(size_t nbytes) override {
        if (nbytes <= bytes) return 0;
        const int rc = d.alloc(nbytes);
        p = d.p; bytes = d.p ? d.bytes : 0;
        return rc;
    }
};
struct CallerOutput : MapBuffer {                                   // an output of the one-shot call: device memory in place, host memory staged; sized once
    Staged s; void* target; hipStream_t stream;
    CallerOutput(void* target_, hipStream_t stream_) : target(target_), stream(stream_) {}
    int need(size_t nbytes) override {
        const int rc = s.out(target, nbytes, stream);
        p = s.dev; bytes = nbytes;
        return rc;
    }
};

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_queries_parse(const uint8_t* text, uint64_t bytes, int32_t format, int32_t final, const uint8_t* symbol_of, uint8_t* out_qbuf, uint64_t symbol_capacity,
                        uint64_t* out_qoff, uint64_t read_capacity, fmgpu_text_span* out_names, fmgpu_text_span* out_quals, fmgpu_parse_result* result, void* stream_) {
    if (!result || !symbol_of) return fail(FMGPU_ERR_INVALID, "result / symbol_of is null");
    if (format != FMGPU_TEXT_LINES && format != FMGPU_TEXT_FASTA && format != FMGPU_TEXT_FASTQ) return fail(FMGPU_ERR_INVALID, "unknown text format " + std::to_string(format));
    if (!text && bytes) return fail(FMGPU_ERR_INVALID, "text is null");
    if (!out_qbuf != !out_qoff) return fail(FMGPU_ERR_INVALID, "out_qbuf and out_qoff are both given or both null (the counting call)");
    const bool counting = !out_qbuf;
    if (counting && (out_names || out_quals)) return fail(FMGPU_ERR_INVALID, "the counting call takes no span arrays");
    std::memset(result, 0, sizeof *result);
    hipStream_t stream = (hipStream_t)stream_;
    if (bytes == 0) {
        if (out_qoff) {
            if (is_device_pointer(out_qoff)) { FM_HIP(hipMemsetAsync(out_qoff, 0, 8, stream)); FM_HIP(hipStreamSynchronize(stream)); }
            else out_qoff[0] = 0;
        }
        return 0;
    }
    if (bytes > kParseMaxBytes) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_queries_parse takes at most 2^32 - 2 bytes per call: parse the text in chunks, each starting at the previous call's `consumed`");

    int rc;
    Staged stext;
    if ((rc = stext.in(text, bytes, stream))) return rc;
    OwnScratch table, acc, lnbase, kcnt, hcnt, tmp, ls;
    if ((rc = table.need(256))) return rc;
    FM_HIP(hipMemcpyAsync(table.p, symbol_of, 256, hipMemcpyHostToDevice, stream));
    CallerOutput sq(out_qbuf, stream), so(out_qoff, stream), sn(out_names, stream), sl(out_quals, stream);
    ParseBuffers b;
    b.acc = &acc; b.lnbase = &lnbase; b.kcnt = &kcnt; b.hcnt = &hcnt; b.tmp = &tmp; b.ls = &ls;
    b.qbuf = &sq; b.qoff = &so; b.names = out_names ? &sn : nullptr; b.quals = out_quals ? &sl : nullptr;
    if ((rc = parse_device((const uint8_t*)stext.dev, bytes, format, final, 0, (const uint8_t*)table.p, &b, counting, symbol_capacity, read_capacity, 0, 0, result, nullptr,
                           nullptr, stream))) return rc;
    if (counting) return 0;
    if ((rc = sq.s.finish()) || (rc = so.s.finish()) || (rc = sn.s.finish()) || (rc = sl.s.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
