// fmgpu_align.hip — fmgpu_chains_align (include/fmgpu.h): the chains of fmgpu_seeds_chain to CIGAR alignments on the device.
// Nothing here depends on the row width or on an index.  An *element* is one (chain, anchor) pair; elements are numbered by a scan of the chains' n_anchors, so that
// chain c owns elements estart[c] .. estart[c] + n_anchors - 1.  Element e is piece k with the gap behind it; everything an element states about itself it takes from
// its own anchor and its successor.  No lane walks a chain.
//  k_align_chains     one lane per chain: n_anchors and first against n_anchor, qidx against nq, the read's length against qend and 2^28, the window against tend - tbeg
//  (hipcub exclusive scan of n_anchors) k_align_sum: the anchors of chains 0 .. c against n_anchor
//  k_align_pieces     one lane per element: its chain (a binary search in the scan), the anchor's checks, l', the piece against the text, gq and gt; a trivial gap is
//                     settled here, a chain with a gap beyond max_gap_len or max_cells is marked left out, every other gap becomes a GapTask in one of four lists by what
//                     its traceback needs: lane (up to kLaneGap x kLaneGap), LDS wave (up to kLdsNeed bytes), slice wave (up to kSliceNeed), the rest
//  k_align_lane<W>    one lane per listed gap: the whole matrix in plain loops, one row of values and 2 bits per cell in LDS, the traceback
//  k_align_wave<W, L> one wave per listed gap, taken by ticket: row by row, the lanes across 64 text columns; the left-to-right dependency of a row is a min-plus prefix
//                     scan over the lanes (six shuffles) with a carry between the chunks of a row, the previous row lies in the wave's scratch indexed by the text
//                     column, the directions leave as two ballots per chunk; then the traceback by the whole wave in step (wave-uniform loads)
//       W = false counts: runs, first and last operation, bases under =, X, I, D into the element's result.  W = true writes the operations to their slots.
//  k_align_count      one lane per element: the operations it adds once neighbours with the same operation are merged (pm: its piece joins the `=` in front of it,
//                     gm: its gap's first run joins its piece); the bases into the chain's record by atomic adds
//  (hipcub exclusive scan of those counts) k_align_records: first_op, n_ops, status; the operation count beside the error words; ONE read-back
//  k_align_emit       one lane per element: clips, the piece and a trivial gap to their slots; a slot several elements share (a merged `=`) is summed by atomic adds
//                     into zeroed memory, the first contributor in line order adds the code
//  then the gap kernels again with W = true.
// The gap kernels work on GapTask lists and element result slots only, so that another call can feed them with tasks of its own.
// Scratch: 116 bytes per anchor (32 the element results, 20 chain number and the two scan arrays, 64 the task lists), 49 per chain, hipcub's own, and the traceback
// scratch of the slice waves: nothing when band, max_gap_len and max_cells keep every gap within kLdsNeed, else min(256, n_anchor) slices of up to kSliceNeed bytes, and
// one slice of what the largest admissible gap needs where that is more.  Freed on return.
#include "fmgpu_positions.h"

namespace fmgpu {
namespace {

constexpr uint64_t kMaxAlignRecords = (1ull << 32) - 256;
constexpr uint64_t kMaxOpLen = 1ull << 28;                  // a read or a window of this many symbols is refused: an operation's length has 28 bits
constexpr uint64_t kMaxCells = 1ull << 30;
constexpr uint32_t kLaneGap = 15;                           // gaps of up to this many symbols on both sides go one per lane (not tuned)
constexpr uint32_t kLdsNeed = 16384;                        // bytes of LDS a wave of the LDS tier has for directions and one row
constexpr uint64_t kSliceNeed = 1ull << 19;                 // bytes of a slice of the traceback budget
constexpr uint32_t kSliceWaves = 256;                       // slices at most: the budget is kSliceWaves x kSliceNeed
constexpr uint32_t kLdsWaves = 4096;                        // waves of the LDS tier at most; each takes gaps until its list is empty
constexpr int32_t kInf = 0x3fffffff;
enum : uint32_t { OP_I = FMGPU_OP_I, OP_D = FMGPU_OP_D, OP_S = FMGPU_OP_S, OP_EQ = FMGPU_OP_EQ, OP_X = FMGPU_OP_X };

// the error words in the order they are reported (E_PIECE holds chain << 32 | anchor); E_LONG: a read or a window of 2^28 symbols; W_OPS carries the operation count
enum : int { E_ANCHORS = 0, E_INDEX = 1, E_HIT = 2, E_QUERY = 3, E_ORDER = 4, E_ENDS = 5, E_QEND = 6, E_WINDOW = 7, E_PIECE = 8, E_LONG = 9, E_WORDS = 10, W_OPS = 10 };
enum : int { L_LANE = 0, L_LDS = 1, L_SLICE = 2, L_REST = 3 };      // the task lists; words[L_*] their lengths, words[4 + L_*] the tickets of the wave kernels

struct GapTask { uint64_t q, t; uint32_t gq, gt, elem, pad; };      // Q = qbuf + q, T = tbuf + t; the result goes to res[elem]
static_assert(sizeof(GapTask) == 32, "one 32-byte task");
// what an element knows after the counting pass: l', the runs of its gap with the first and the last operation, the bases of its gap
struct ElemRes { uint32_t lp, runs, codes, nm, nx, ni, nd, trivial; };      // codes: first | last << 8; trivial: the gap is one I or D settled without a matrix
static_assert(sizeof(ElemRes) == 32, "one 32-byte result");
static_assert(sizeof(fmgpu_chain_alignment) == 32 && sizeof(fmgpu_align_spec) == 32, "the sizes include/fmgpu.h states");

struct AlignArgs {
    const fmgpu_chain* chains; uint64_t nc;
    const uint32_t* anchors; uint64_t n_anchor;
    const fmgpu_position* pos; uint64_t count;
    const fmgpu_seed_span* spans; uint64_t n_spans;
    const uint8_t* qbuf; const uint64_t* qoff; uint64_t nq;
    const uint8_t* tbuf; const uint64_t* toff;
    uint32_t band, max_gap_len; uint64_t max_cells;
    uint64_t *ncount, *estart;                              // nc + 1 each: n_anchors, its exclusive scan
    unsigned long long* err;                                // E_WORDS + 1 words
    uint8_t* cstatus;                                       // per chain: 1 left out
    fmgpu_chain_alignment* rec;                             // per chain (scratch: the caller's `out` is written behind the read-back)
    uint32_t* echain;                                       // per element
    ElemRes* res;                                           // per element
    uint64_t *ecnt, *eoff;                                  // n_anchor + 1 each: the operations an element adds, their exclusive scan
    GapTask *list_a, *list_b;                               // n_anchor each: lane tasks from the front of list_a, LDS tasks from its back; slice / rest in list_b
    uint32_t* words;                                        // 8
    uint32_t* ops;                                          // the writing pass: the (staged) out_ops
};

__device__ __forceinline__ bool failed(const AlignArgs& a) {
    unsigned long long all = kNone;
#pragma unroll
    for (int k = 0; k < E_WORDS; ++k) all &= a.err[k];
    return all != kNone;
}

// the band of a gap: lo <= b - a <= hi
__host__ __device__ __forceinline__ void band_of(uint32_t gq, uint32_t gt, uint32_t w, int32_t* lo, int32_t* hi) {
    const int32_t d = (int32_t)gt - (int32_t)gq;
    *lo = (d < 0 ? d : 0) - (int32_t)w; *hi = (d > 0 ? d : 0) + (int32_t)w;
}
// the 64-column chunks of a row of the wave tiers, and the bytes a wave needs for a gap: two 64-bit ballots per chunk and row, one row of values over the text columns
__host__ __device__ __forceinline__ uint32_t chunks_per_row(uint32_t gt, uint64_t width) { return (uint32_t)(((width < gt + 1ull ? width : gt + 1ull) + 63u) / 64u); }
__host__ __device__ __forceinline__ uint64_t wave_need(uint32_t gq, uint32_t gt, uint64_t width) { return (gq + 1ull) * chunks_per_row(gt, width) * 16ull + 4ull * (gt + 1ull); }

__global__ __launch_bounds__(256) void k_align_chains(AlignArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > a.nc) return;
    if (c == a.nc) { a.ncount[c] = 0; return; }
    const fmgpu_chain ch = a.chains[c];
    a.ncount[c] = ch.n_anchors;
    if (ch.n_anchors == 0 || (uint64_t)ch.first + ch.n_anchors > a.n_anchor) atomicMin(&a.err[E_ANCHORS], (unsigned long long)c);
    const uint64_t t0 = a.toff[c], t1 = a.toff[c + 1];
    if (t1 < t0 || ch.tend < ch.tbeg || t1 - t0 != ch.tend - ch.tbeg) atomicMin(&a.err[E_WINDOW], (unsigned long long)c);
    else if (t1 - t0 >= kMaxOpLen) atomicMin(&a.err[E_LONG], (unsigned long long)c);
    if (ch.qidx >= a.nq) { atomicMin(&a.err[E_QUERY], (unsigned long long)c); return; }
    const uint64_t m = a.qoff[ch.qidx + 1] - a.qoff[ch.qidx];
    if (m >= kMaxOpLen) atomicMin(&a.err[E_LONG], (unsigned long long)c);
    if (ch.qend > m) atomicMin(&a.err[E_QEND], (unsigned long long)c);
}

__global__ __launch_bounds__(256) void k_align_sum(AlignArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nc) return;
    if (a.estart[c] + a.ncount[c] > a.n_anchor) atomicMin(&a.err[E_ANCHORS], (unsigned long long)c);
}

__global__ __launch_bounds__(256) void k_align_pieces(AlignArgs a) {
    if (a.err[E_ANCHORS] != kNone) return;                  // (then the elements are not numbered; every other check still looks for its lowest offender)
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.estart[a.nc]) return;
    uint64_t lo = 0, hi = a.nc;                             // the last chain that starts at or in front of e (no chain is empty)
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) / 2; if (a.estart[mid] <= e) lo = mid; else hi = mid; }
    const uint64_t c = lo;
    const fmgpu_chain ch = a.chains[c];
    const uint32_t k = (uint32_t)(e - a.estart[c]), n = ch.n_anchors;
    a.echain[e] = (uint32_t)c;
    ElemRes r{0, 0, 0, 0, 0, 0, 0, 0};
    a.res[e] = r;
    const uint32_t ai = a.anchors[ch.first + k];
    if (ai >= a.count) { atomicMin(&a.err[E_INDEX], (unsigned long long)c); return; }
    const fmgpu_position p = a.pos[ai];
    if (p.hit >= a.n_spans || a.spans[p.hit].qlen == 0) { atomicMin(&a.err[E_HIT], (unsigned long long)c); return; }
    const fmgpu_seed_span s = a.spans[p.hit];
    if (p.qidx != ch.qidx || p.seq_id != ch.seq_id) atomicMin(&a.err[E_QUERY], (unsigned long long)c);
    const uint64_t q_k = s.qbeg, l_k = s.qlen, t_k = p.pos;
    uint64_t lp = l_k, gq = 0, gt = 0, q_n = 0, t_n = 0;
    bool next = false;
    if (k + 1 < n) {
        const uint32_t aj = a.anchors[ch.first + k + 1];
        if (aj < a.count) {
            const fmgpu_position pn = a.pos[aj];
            if (pn.hit < a.n_spans) {                       // (an anchor that is refused is its own element's to report)
                q_n = a.spans[pn.hit].qbeg; t_n = pn.pos;
                if (q_n <= q_k || t_n <= t_k) atomicMin(&a.err[E_ORDER], (unsigned long long)c);
                else {
                    const uint64_t dq = q_n - q_k, dt = t_n - t_k;
                    lp = lp < dq ? lp : dq; lp = lp < dt ? lp : dt;
                    gq = dq - lp; gt = dt - lp; next = true;
                }
            }
        }
    }
    if (k == 0 && (ch.tbeg != t_k || ch.qbeg != q_k)) atomicMin(&a.err[E_ENDS], (unsigned long long)c);
    if (k + 1 == n && (ch.tend != t_k + l_k || ch.qend != q_k + l_k)) atomicMin(&a.err[E_ENDS], (unsigned long long)c);
    r.lp = (uint32_t)lp;
    if (ch.qidx >= a.nq) { a.res[e] = r; return; }
    const uint64_t qb = a.qoff[ch.qidx], m = a.qoff[ch.qidx + 1] - qb, tb = a.toff[c], t1 = a.toff[c + 1], wl = t1 >= tb ? t1 - tb : 0;
    // a piece that leaves the read or the window belongs to a chain that an earlier check refuses: it is not compared
    if (t_k >= ch.tbeg && t_k - ch.tbeg <= wl && lp <= wl - (t_k - ch.tbeg) && q_k + lp <= m) {
        const uint8_t* Q = a.qbuf + qb + q_k;
        const uint8_t* T = a.tbuf + tb + (t_k - ch.tbeg);
        bool same = true;
        for (uint64_t i = 0; i < lp; ++i) same = same && Q[i] == T[i];
        if (!same) atomicMin(&a.err[E_PIECE], (unsigned long long)(c << 32 | k));
        if (next && gq == 0 && gt > 0) { r.runs = 1; r.codes = OP_D | OP_D << 8; r.nd = (uint32_t)gt; r.trivial = 1; }
        else if (next && gt == 0 && gq > 0) { r.runs = 1; r.codes = OP_I | OP_I << 8; r.ni = (uint32_t)gq; r.trivial = 1; }
        else if (next && gq > 0) {
            int32_t blo = 0, bhi = 0;
            const bool fits = gq <= a.max_gap_len && gt <= a.max_gap_len;
            if (fits) band_of((uint32_t)gq, (uint32_t)gt, a.band, &blo, &bhi);
            const uint64_t width = (uint64_t)((int64_t)bhi - blo + 1);
            if (!fits || (gq + 1) * width > a.max_cells) a.cstatus[c] = 1;
            else if (q_n <= m && t_n - ch.tbeg <= wl) {     // (else an earlier check refuses the chain)
                GapTask g{qb + q_k + lp, tb + (t_k - ch.tbeg) + lp, (uint32_t)gq, (uint32_t)gt, (uint32_t)e, 0u};
                const uint64_t need = wave_need(g.gq, g.gt, width);
                if (g.gq <= kLaneGap && g.gt <= kLaneGap) a.list_a[atomicAdd(&a.words[L_LANE], 1u)] = g;
                else if (need <= kLdsNeed) a.list_a[a.n_anchor - 1 - atomicAdd(&a.words[L_LDS], 1u)] = g;
                else if (need <= kSliceNeed) a.list_b[atomicAdd(&a.words[L_SLICE], 1u)] = g;
                else a.list_b[a.n_anchor - 1 - atomicAdd(&a.words[L_REST], 1u)] = g;
            }
        }
    }
    a.res[e] = r;
}

// element e of chain c: whether it carries the head clip / the tail clip, whether its piece joins the `=` in front of it (pm) and its gap's first run its piece (gm)
struct Slots { uint32_t head, tail, pm, gm, head_len, tail_len; };
__device__ __forceinline__ Slots slots_of(const AlignArgs& a, uint64_t e, uint64_t c, const ElemRes& r) {
    const fmgpu_chain& ch = a.chains[c];
    const uint64_t k = e - a.estart[c], m = a.qoff[ch.qidx + 1] - a.qoff[ch.qidx];
    Slots s{0, 0, 0, 0, 0, 0};
    if (k == 0 && ch.qbeg > 0) { s.head = 1; s.head_len = ch.qbeg; }
    if (k + 1 == ch.n_anchors && m > ch.qend) { s.tail = 1; s.tail_len = (uint32_t)(m - ch.qend); }
    if (k > 0) { const ElemRes& b = a.res[e - 1]; s.pm = b.runs == 0 || (b.codes >> 8) == OP_EQ; }
    s.gm = r.runs > 0 && (r.codes & 0xffu) == OP_EQ;
    return s;
}

// what a gap kernel does with the runs of a traceback, which come last run first
template <bool WRITE> struct RunSink {
    const AlignArgs& a; uint32_t elem; ElemRes r; uint64_t base; uint32_t total, seen;
    __device__ RunSink(const AlignArgs& a_, uint32_t elem_) : a(a_), elem(elem_), r(a_.res[elem_]), base(0), total(0), seen(0) {
        if (WRITE) {
            const Slots s = slots_of(a, elem, a.echain[elem], r);
            base = a.eoff[elem] + s.head - s.pm + 1 - s.gm; total = r.runs;
        } else { r.runs = 0; r.codes = 0; r.nm = r.nx = r.ni = r.nd = 0; }
    }
    __device__ void run(uint32_t code, uint32_t len, bool writer) {
        if (WRITE) {
            const uint32_t j = total - 1u - seen;           // the run's place in line order
            if (writer) {
                if (code == OP_EQ && j == 0) atomicAdd(&a.ops[base], len << 4);             // joins its piece, which adds the code
                else if (code == OP_EQ && j + 1 == total) atomicAdd(&a.ops[base + j], len << 4 | code);      // the piece behind it may join
                else a.ops[base + j] = len << 4 | code;
            }
        } else {
            if (seen == 0) r.codes = code << 8;
            r.codes = (r.codes & 0xff00u) | code;
            r.runs++;
            if (code == OP_EQ) r.nm += len; else if (code == OP_X) r.nx += len; else if (code == OP_I) r.ni += len; else r.nd += len;
        }
        seen++;
    }
    __device__ void done(bool writer) { if (!WRITE && writer) a.res[elem] = r; }
};

// One lane per gap of up to kLaneGap x kLaneGap: row a of the matrix is 16 cells of 2 bits, one word; the row of values and the words of all rows lie in LDS, a lane's
// entries 256 apart.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_align_lane(AlignArgs a) {
    __shared__ uint32_t dirs[kLaneGap + 1][256];
    __shared__ uint16_t vals[kLaneGap + 1][256];
    if (failed(a)) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.words[L_LANE]) return;
    const GapTask g = a.list_a[i];
    if (a.cstatus[a.echain[g.elem]]) return;
    const uint32_t x = threadIdx.x;
    const uint8_t *Q = a.qbuf + g.q, *T = a.tbuf + g.t;
    int32_t lo, hi;
    band_of(g.gq, g.gt, a.band, &lo, &hi);
    constexpr uint32_t INF = 0x3fff;
    uint64_t tsym = 0;                                      // the gap's text, 4 bits per symbol where it fits, else read again
    for (uint32_t b = 0; b < g.gt; ++b) tsym |= (uint64_t)(T[b] & 15u) << (4 * b);
    bool narrow = true;
    for (uint32_t b = 0; b < g.gt; ++b) narrow = narrow && T[b] < 16;
    for (uint32_t aa = 0; aa <= g.gq; ++aa) {
        const uint32_t qs = aa ? Q[aa - 1] : 0u;
        uint32_t word = 0, diag = INF, left = INF;
        for (uint32_t b = 0; b <= g.gt; ++b) {
            const int32_t off = (int32_t)b - (int32_t)aa;
            const uint32_t up = aa ? vals[b][x] : INF;
            uint32_t v = INF, dir = 2;
            if (off >= lo && off <= hi) {
                if (aa == 0 && b == 0) v = 0;
                else {
                    const uint32_t ts = b ? (narrow ? (uint32_t)(tsym >> (4 * (b - 1))) & 15u : T[b - 1]) : 0u;
                    const uint32_t vd = (aa && b && diag < INF) ? diag + (qs != ts ? 1u : 0u) : INF;
                    const uint32_t vl = left < INF ? left + 1u : INF, vu = up < INF ? up + 1u : INF;
                    v = vd < vl ? vd : vl; v = v < vu ? v : vu;
                    dir = vd == v ? 0u : vl == v ? 1u : 2u;
                }
            }
            word |= dir << (2 * b);
            diag = up; left = v;
            vals[b][x] = (uint16_t)v;
        }
        dirs[aa][x] = word;
    }
    RunSink<WRITE> sink(a, g.elem);
    uint32_t aa = g.gq, b = g.gt, cur = 0, len = 0;
    while (aa || b) {
        const uint32_t dir = aa == 0 ? 1u : b == 0 ? 2u : (dirs[aa][x] >> (2 * b)) & 3u;       // (row 0 and column 0 have one way back)
        uint32_t code;
        if (dir == 0) { code = Q[aa - 1] == T[b - 1] ? OP_EQ : OP_X; --aa; --b; }
        else if (dir == 1) { code = OP_D; --b; }
        else { code = OP_I; --aa; }
        if (code == cur) ++len;
        else { if (len) sink.run(cur, len, true); cur = code; len = 1; }
    }
    if (len) sink.run(cur, len, true);
    sink.done(true);
}

__device__ __forceinline__ int32_t shfl_up_i(int32_t v, uint32_t by) { return __shfl_up(v, by, 64); }

// One gap on one wave.  `mine`: wave_need bytes, LDS or global: the ballots of every (row, chunk) first, the row of values behind them.  Row aa covers the text columns
// blo .. bhi that the band leaves it; chunk ci holds columns blo + 64 ci + lane.  All 64 lanes run the traceback in step on the same words.
template <bool WRITE>
__device__ __forceinline__ void align_gap_wave(const AlignArgs& a, const GapTask& g, uint8_t* mine) {
    const uint32_t lane = threadIdx.x;
    int32_t lo, hi;
    band_of(g.gq, g.gt, a.band, &lo, &hi);
    const uint32_t cpr = chunks_per_row(g.gt, (uint64_t)((int64_t)hi - lo + 1));
    uint64_t* bits = reinterpret_cast<uint64_t*>(mine);
    int32_t* row = reinterpret_cast<int32_t*>(mine + (g.gq + 1ull) * cpr * 16ull);
    const uint8_t *Q = a.qbuf + g.q, *T = a.tbuf + g.t;
    const int32_t gt = (int32_t)g.gt;
    for (int32_t aa = 0; aa <= (int32_t)g.gq; ++aa) {
        const int32_t blo = aa + lo > 0 ? aa + lo : 0, bhi = aa + hi < gt ? aa + hi : gt;
        const int32_t pblo = aa - 1 + lo > 0 ? aa - 1 + lo : 0, pbhi = aa - 1 + hi < gt ? aa - 1 + hi : gt;      // the row in front (aa > 0)
        const uint32_t qs = aa ? Q[aa - 1] : 0u;
        int32_t carry_v = kInf;                              // the value left of the chunk's first column
        int32_t carry_old = (aa > 0 && blo >= 1 && blo - 1 >= pblo && blo - 1 <= pbhi) ? row[blo - 1] : kInf;     // the old value left of it
        uint32_t ci = 0;
        for (int32_t c0 = blo; c0 <= bhi; c0 += 64, ++ci) {
            const int32_t b = c0 + (int32_t)lane;
            const bool valid = b <= bhi;
            const int32_t oldv = (valid && aa > 0 && b >= pblo && b <= pbhi) ? row[b] : kInf;
            int32_t dv = shfl_up_i(oldv, 1);
            if (lane == 0) dv = carry_old;
            int32_t vd = kInf;
            if (valid && aa > 0 && b > 0 && dv < kInf) vd = dv + (qs != T[b - 1] ? 1 : 0);
            const int32_t vu = oldv < kInf ? oldv + 1 : kInf;
            int32_t xv = vd < vu ? vd : vu;
            if (aa == 0 && b == 0) xv = 0;
            if (!valid) xv = kInf;
            int32_t y = xv - (int32_t)lane;                 // v(b) = min over b' <= b of x(b') + (b - b')
#pragma unroll
            for (uint32_t o = 1; o < 64; o <<= 1) { const int32_t t = shfl_up_i(y, o); if (lane >= o) y = t < y ? t : y; }
            int32_t v = y + (int32_t)lane;
            const int32_t cv = carry_v + (int32_t)lane + 1;
            v = cv < v ? cv : v;
            int32_t left = shfl_up_i(v, 1);
            if (lane == 0) left = carry_v;
            const uint32_t dir = vd == v ? 0u : left + 1 == v ? 1u : 2u;
            const uint64_t b0 = __ballot(valid && (dir & 1u)), b1 = __ballot(valid && (dir & 2u));
            if (lane == 0) { bits[((uint64_t)aa * cpr + ci) * 2] = b0; bits[((uint64_t)aa * cpr + ci) * 2 + 1] = b1; }
            carry_old = __shfl(oldv, 63, 64); carry_v = __shfl(v, 63, 64);
            if (valid) row[b] = v;
        }
        __threadfence_block();
        __syncthreads();
    }
    RunSink<WRITE> sink(a, g.elem);
    int32_t aa = (int32_t)g.gq, b = gt;
    uint32_t cur = 0, len = 0;
    while (aa || b) {
        const int32_t blo = aa + lo > 0 ? aa + lo : 0;
        const uint32_t idx = (uint32_t)(b - blo);
        const uint64_t w = ((uint64_t)aa * cpr + idx / 64u) * 2;
        uint32_t dir = (uint32_t)((bits[w] >> (idx & 63u)) & 1u) | (uint32_t)((bits[w + 1] >> (idx & 63u)) & 1u) << 1;
        dir = aa == 0 ? 1u : b == 0 ? 2u : dir;             // (row 0 and column 0 have one way back)
        uint32_t code;
        if (dir == 0) { code = Q[aa - 1] == T[b - 1] ? OP_EQ : OP_X; --aa; --b; }
        else if (dir == 1) { code = OP_D; --b; }
        else { code = OP_I; --aa; }
        if (code == cur) ++len;
        else { if (len) sink.run(cur, len, lane == 0); cur = code; len = 1; }
    }
    if (len) sink.run(cur, len, lane == 0);
    sink.done(lane == 0);
    __syncthreads();                                        // the next gap overwrites the scratch
}

// LDS: the wave's scratch is LDS (list L_LDS); else slice `blockIdx.x` of `scratch`, `region` bytes each (list L_SLICE, or L_REST on one wave)
template <bool WRITE, bool LDS>
__global__ __launch_bounds__(64) void k_align_wave(AlignArgs a, int list, uint8_t* scratch, uint64_t region) {
    __shared__ uint64_t lds[LDS ? kLdsNeed / 8 : 1];
    if (failed(a)) return;
    uint8_t* mine = LDS ? reinterpret_cast<uint8_t*>(lds) : scratch + (uint64_t)blockIdx.x * region;
    for (;;) {
        uint32_t ticket = 0;
        if (threadIdx.x == 0) ticket = atomicAdd(&a.words[4 + list], 1u);
        ticket = __shfl(ticket, 0, 64);
        if (ticket >= a.words[list]) return;
        const GapTask g = list == L_LDS ? a.list_a[a.n_anchor - 1 - ticket] : list == L_SLICE ? a.list_b[ticket] : a.list_b[a.n_anchor - 1 - ticket];
        if (a.cstatus[a.echain[g.elem]]) continue;
        align_gap_wave<WRITE>(a, g, mine);
    }
}

__global__ __launch_bounds__(256) void k_align_count(AlignArgs a) {
    if (failed(a)) return;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.estart[a.nc]) return;
    const uint32_t c = a.echain[e];
    if (a.cstatus[c]) return;                               // (ecnt is zeroed)
    const ElemRes r = a.res[e];
    const Slots s = slots_of(a, e, c, r);
    a.ecnt[e] = (uint64_t)s.head + 1u + r.runs + s.tail - s.pm - s.gm;
    fmgpu_chain_alignment* rec = a.rec + c;
    atomicAdd(&rec->n_match, r.lp + r.nm);
    if (r.nx) atomicAdd(&rec->n_mismatch, r.nx);
    if (r.ni) atomicAdd(&rec->n_ins, r.ni);
    if (r.nd) atomicAdd(&rec->n_del, r.nd);
}

__global__ __launch_bounds__(256) void k_align_records(AlignArgs a) {
    if (failed(a)) return;
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > a.nc) return;
    if (c == a.nc) { a.err[W_OPS] = a.eoff[a.estart[c]]; return; }
    fmgpu_chain_alignment* rec = a.rec + c;
    rec->first_op = a.eoff[a.estart[c]];
    rec->n_ops = (uint32_t)(a.eoff[a.estart[c + 1]] - a.eoff[a.estart[c]]);
    rec->status = a.cstatus[c];
}

__global__ __launch_bounds__(256) void k_align_emit(AlignArgs a) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.estart[a.nc]) return;
    const uint32_t c = a.echain[e];
    if (a.cstatus[c]) return;
    const ElemRes r = a.res[e];
    const Slots s = slots_of(a, e, c, r);
    const uint64_t at = a.eoff[e], piece = at + s.head - s.pm;
    if (s.head) a.ops[at] = s.head_len << 4 | OP_S;
    atomicAdd(&a.ops[piece], r.lp << 4 | (s.pm ? 0u : OP_EQ));
    if (r.trivial) a.ops[piece + 1] = (r.ni + r.nd) << 4 | (r.codes & 0xffu);
    if (s.tail) a.ops[piece + 1 + r.runs - s.gm] = s.tail_len << 4 | OP_S;
}

// the most bytes a wave needs for a gap that the spec admits
uint64_t largest_need(const fmgpu_align_spec& s) {
    const uint64_t g = s.max_gap_len, width = g + 2ull * s.band + 1;
    if (g == 0) return 0;
    uint64_t cells = (g + 1) * width;
    cells = cells < s.max_cells ? cells : s.max_cells;
    return cells / 4 + 16 * (g + 1) + 16 + 4 * (g + 1);      // (rows x ceil(width / 64) x 16 <= cells / 4 + 16 rows)
}

// an input array: used in place where it is device memory, else `bytes` of it staged; the bytes of a symbol buffer are its last offset, read where the offsets are
int symbol_bytes(const uint64_t* off, uint64_t last, uint64_t* bytes, hipStream_t stream) {
    if (!is_device_pointer(off)) { *bytes = off[last]; return 0; }
    FM_HIP(hipMemcpyAsync(bytes, off + last, 8, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

template <bool WRITE>
int gap_kernels(const AlignArgs& a, dim3 egrid, uint32_t lds_waves, uint32_t slice_waves, uint8_t* scratch, uint64_t slice, uint64_t rest, hipStream_t stream) {
    FM_HIP(hipMemsetAsync(a.words + 4, 0, 16, stream));
    k_align_lane<WRITE><<<egrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_align_lane");
    k_align_wave<WRITE, true><<<dim3(lds_waves), dim3(64), 0, stream>>>(a, L_LDS, nullptr, 0);
    FM_LAUNCHED("k_align_wave");
    if (slice) {
        k_align_wave<WRITE, false><<<dim3(slice_waves), dim3(64), 0, stream>>>(a, L_SLICE, scratch, slice);
        FM_LAUNCHED("k_align_wave");
    }
    if (rest) {
        k_align_wave<WRITE, false><<<dim3(1), dim3(64), 0, stream>>>(a, L_REST, scratch, rest);
        FM_LAUNCHED("k_align_wave");
    }
    return 0;
}

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_chains_align(const fmgpu_chain* chains, uint64_t n_chains, const uint32_t* anchors, uint64_t n_anchor, const fmgpu_position* positions, uint64_t count,
                       const fmgpu_seed_span* spans, uint64_t n_spans, const uint8_t* qbuf, const uint64_t* qoff, const uint8_t* tbuf, const uint64_t* toff,
                       const fmgpu_align_spec* spec, fmgpu_chain_alignment* out, uint32_t* out_ops, uint64_t ops_capacity, uint64_t* out_ops_count, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!spec) return fail(FMGPU_ERR_INVALID, "fmgpu_chains_align: spec is null");
    if (!out_ops_count) return fail(FMGPU_ERR_INVALID, "fmgpu_chains_align: out_ops_count is null");
    if (spec->band > 65535u) return fail(FMGPU_ERR_INVALID, "fmgpu_align_spec: band must lie in 0 .. 65535");
    if (spec->max_gap_len > 65535u) return fail(FMGPU_ERR_INVALID, "fmgpu_align_spec: max_gap_len must lie in 0 .. 65535");
    if (spec->max_cells < 1 || spec->max_cells > kMaxCells) return fail(FMGPU_ERR_INVALID, "fmgpu_align_spec: max_cells must lie in 1 .. 2^30");
    for (int k = 0; k < 8; ++k) if (spec->reserved[k]) return fail(FMGPU_ERR_INVALID, "fmgpu_align_spec: reserved must be 0");
    if (n_chains) {
        const struct { const void* p; const char* name; } need[] = {{chains, "chains"}, {anchors, "anchors"}, {positions, "positions"}, {spans, "spans"}, {qbuf, "qbuf"},
                                                                    {qoff, "qoff"}, {tbuf, "tbuf"}, {toff, "toff"}, {out, "out"}};
        for (const auto& n : need) if (!n.p) return fail(FMGPU_ERR_INVALID, std::string("fmgpu_chains_align: ") + n.name + " is null while n_chains > 0");
    }
    if (!out_ops && ops_capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_chains_align: out_ops is null while ops_capacity > 0");
    *out_ops_count = 0;
    if (n_chains >= kMaxAlignRecords || n_anchor >= kMaxAlignRecords || count >= kMaxAlignRecords || n_spans >= kMaxAlignRecords)
        return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_chains_align: n_chains, n_anchor, count and n_spans must each stay below 2^32 - 256");
    if (n_chains == 0) return 0;

    AlignArgs a;
    std::memset(&a, 0, sizeof a);
    a.nc = n_chains; a.n_anchor = n_anchor; a.count = count; a.n_spans = n_spans; a.nq = spec->nq;
    a.band = spec->band; a.max_gap_len = spec->max_gap_len; a.max_cells = spec->max_cells;
    const uint64_t nc = n_chains, ne = n_anchor ? n_anchor : 1;

    int rc;
    Staged schains, sanchors, spos, sspans, sqoff, sqbuf, stoff, stbuf, sops;
    // (a symbol buffer in device memory is used in place, whatever its size; one in host memory is staged up to its last offset)
    const bool qdev = is_device_pointer(qbuf), tdev = is_device_pointer(tbuf);
    uint64_t qbytes = 0, tbytes = 0;
    if (!qdev && spec->nq && (rc = symbol_bytes(qoff, spec->nq, &qbytes, stream))) return rc;
    if (!tdev && (rc = symbol_bytes(toff, nc, &tbytes, stream))) return rc;
    if ((rc = schains.in(chains, nc * sizeof(fmgpu_chain), stream)) || (rc = sanchors.in(anchors, n_anchor * 4, stream)) ||
        (rc = spos.in(positions, count * sizeof(fmgpu_position), stream)) || (rc = sspans.in(spans, n_spans * sizeof(fmgpu_seed_span), stream)) ||
        (rc = sqoff.in(qoff, (spec->nq + 1) * 8, stream)) || (!qdev && (rc = sqbuf.in(qbuf, qbytes, stream))) || (rc = stoff.in(toff, (nc + 1) * 8, stream)) ||
        (!tdev && (rc = stbuf.in(tbuf, tbytes, stream))))
        return rc;
    a.chains = (const fmgpu_chain*)schains.dev; a.anchors = (const uint32_t*)sanchors.dev; a.pos = (const fmgpu_position*)spos.dev;
    a.spans = (const fmgpu_seed_span*)sspans.dev; a.qoff = (const uint64_t*)sqoff.dev; a.qbuf = qdev ? qbuf : (const uint8_t*)sqbuf.dev; a.toff = (const uint64_t*)stoff.dev;
    a.tbuf = tdev ? tbuf : (const uint8_t*)stbuf.dev;

    // the traceback scratch of the slice waves, by what the spec admits
    const uint64_t most = largest_need(*spec);
    const uint32_t slice_waves = (uint32_t)std::min<uint64_t>(kSliceWaves, ne), lds_waves = (uint32_t)std::min<uint64_t>(kLdsWaves, ne);
    const uint64_t slice = most > kLdsNeed ? std::min<uint64_t>(most, kSliceNeed) : 0, rest = most > kSliceNeed ? most : 0;
    DBuf perchain, records, elems, results, scans, lists, words, trace, tmp;
    if ((rc = perchain.alloc((2 * (nc + 1) + E_WORDS + 1) * 8 + nc)) || (rc = records.alloc(nc * sizeof(fmgpu_chain_alignment))) || (rc = elems.alloc(ne * 4)) ||
        (rc = results.alloc(ne * sizeof(ElemRes))) || (rc = scans.alloc(2 * (ne + 1) * 8)) || (rc = lists.alloc(2 * ne * sizeof(GapTask))) || (rc = words.alloc(32)) ||
        (rc = trace.alloc(std::max<uint64_t>(slice * slice_waves, rest))))
        return rc;
    a.ncount = perchain.as<uint64_t>(); a.estart = a.ncount + (nc + 1);
    a.err = reinterpret_cast<unsigned long long*>(a.estart + (nc + 1));
    a.cstatus = reinterpret_cast<uint8_t*>(a.err + (E_WORDS + 1));
    a.rec = records.as<fmgpu_chain_alignment>();
    a.echain = elems.as<uint32_t>(); a.res = results.as<ElemRes>();
    a.ecnt = scans.as<uint64_t>(); a.eoff = a.ecnt + (ne + 1);
    a.list_a = lists.as<GapTask>(); a.list_b = a.list_a + ne;
    a.n_anchor = ne;                                        // (the lists' ends; with n_anchor == 0 every chain fails the first check)
    a.words = words.as<uint32_t>();
    const uint64_t real_anchor = n_anchor;

    auto scan_chains = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, a.ncount, a.estart, (size_t)(nc + 1), stream); };
    auto scan_elems = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, a.ecnt, a.eoff, (size_t)(ne + 1), stream); };
    size_t tb = 0;
    FM_HIP(cub_size(&tb, scan_chains, scan_elems));
    if ((rc = tmp.alloc(tb))) return rc;

    FM_HIP(hipMemsetAsync(a.err, 0xff, (E_WORDS + 1) * 8, stream));
    FM_HIP(hipMemsetAsync(a.cstatus, 0, nc, stream));
    FM_HIP(hipMemsetAsync(a.rec, 0, nc * sizeof(fmgpu_chain_alignment), stream));
    FM_HIP(hipMemsetAsync(a.ecnt, 0, (ne + 1) * 8, stream));
    FM_HIP(hipMemsetAsync(a.words, 0, 32, stream));
    FM_GRID(cgrid, nc + 1);
    FM_GRID(egrid, ne);
    {
        AlignArgs first = a;
        first.n_anchor = real_anchor;
        k_align_chains<<<cgrid, dim3(256), 0, stream>>>(first);
        FM_LAUNCHED("k_align_chains");
        FM_HIP(cub_run(scan_chains, tmp));
        k_align_sum<<<cgrid, dim3(256), 0, stream>>>(first);
        FM_LAUNCHED("k_align_sum");
    }
    k_align_pieces<<<egrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_align_pieces");
    if ((rc = gap_kernels<false>(a, egrid, lds_waves, slice_waves, trace.as<uint8_t>(), slice, rest, stream))) return rc;
    k_align_count<<<egrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_align_count");
    FM_HIP(cub_run(scan_elems, tmp));
    k_align_records<<<cgrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_align_records");
    uint64_t back[E_WORDS + 1];                             // the error words and the operation count: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, a.err, sizeof back, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    static const char* const kWhat[E_PIECE] = {" has no anchors, or anchors beyond n_anchor", " has an anchor index beyond count", " has an anchor with a hit beyond the spans or a span with qlen == 0",
                                               " names a query beyond nq, or has an anchor of another query or sequence", " has two consecutive anchors that do not ascend in both q and t",
                                               " has tbeg, tend, qbeg or qend that its first and last anchor do not give", " has a qend beyond its read", " has a window whose length is not tend - tbeg"};
    for (int k = 0; k < E_PIECE; ++k) if (back[k] != kNone) return fail(FMGPU_ERR_INVALID, "fmgpu_chains_align: chain " + std::to_string(back[k]) + kWhat[k]);
    if (back[E_LONG] != kNone) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_chains_align: chain " + std::to_string(back[E_LONG]) + " has a read or a window of 2^28 symbols or more");
    if (back[E_PIECE] != kNone)
        return fail(FMGPU_ERR_INVALID, "fmgpu_chains_align: chain " + std::to_string(back[E_PIECE] >> 32) + ", anchor " + std::to_string(back[E_PIECE] & 0xffffffffull) + ": the text differs from the read");
    const uint64_t total = back[W_OPS];
    *out_ops_count = total;
    FM_HIP(hipMemcpyAsync(out, a.rec, nc * sizeof(fmgpu_chain_alignment), hipMemcpyDefault, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (!out_ops && !ops_capacity) return 0;
    if (total > ops_capacity) return fail(FMGPU_ERR_CAPACITY, std::to_string(total) + " operations: more than `ops_capacity`");
    if (!total) return 0;

    if ((rc = sops.out(out_ops, total * 4, stream))) return rc;
    a.ops = (uint32_t*)sops.dev;
    FM_HIP(hipMemsetAsync(a.ops, 0, total * 4, stream));
    k_align_emit<<<egrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_align_emit");
    if ((rc = gap_kernels<true>(a, egrid, lds_waves, slice_waves, trace.as<uint8_t>(), slice, rest, stream))) return rc;
    if ((rc = sops.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
