// fmgpu_chain.hip — fmgpu_seeds_chain (include/fmgpu.h): the located seeds of every query joined to collinear chains on the device.
// Nothing here depends on the row width or on an index.  Anchor i is (qidx, seq_id, t = pos, q = spans[hit].qbeg, l = spans[hit].qlen); inside a query the anchors are
// ordered by (seq_id, t, q, index), a run is a maximal stretch with one (qidx, seq_id), and a *place* is an anchor's index in that order over the whole batch.  A query's
// anchors stand at the same indices in the order as in `positions` (qidx does not decrease and the last sort is stable), so the first pass's run edges serve both.
//  k_chain_check      one lane per record: qidx in range and not below its predecessor's, hit < n_spans, pos < 2^62, the span's qlen and end (an offending record
//                     atomicMin's its index into an error word), the first and the last record of each query
//  (the order: four stable hipcub radix sorts of index values, by q, by t, by seq_id, by qidx, a key gather in front of each)
//  k_chain_gather     one lane per place: t, q, l as one 16-byte record, run start, the query left out by max_anchors; a run of one anchor is settled here (f = l, a
//                     chain of its own)
//  (hipcub exclusive scan of the run starts) k_chain_runs: each run's first place
//  k_chain_short      one lane per run of 2 .. kShortRun anchors: the three sweeps in plain loops; a longer run is appended to a list
//  k_chain_long       one wave per listed run, taken by ticket: the three sweeps, the last max_lookback anchors' fields in an LDS ring of 256 x 16 bytes; the 64 lanes take
//                     the candidates of one anchor, 64 at a time, and ONE cross-lane maximum of a packed key decides the step: value << 32 | place for a link (the best
//                     value, the nearest candidate), t << 32 | ~place for an heir (the largest t, the earliest child)
//       sweep 1, forward:  f and p        sweep 2, backward:  t, heir, chain length, leaf        sweep 3, forward:  each anchor's chain start and its rank in the chain
//  k_chain_keep       one lane per place: a chain start's score and length against the filters
//  (hipcub exclusive scan of the kept starts) k_chain_queries: per query its class and its chains, cut to max_chains; (scan to out_off); ONE read-back: the number of
//  chains, the error words, the kept starts
//  k_chain_compact    the kept starts with the key first place of the query << 32 | ~score; (ONE stable radix sort: queries ascending, scores descending, places ascending)
//  k_chain_emit       one lane per kept start in that order: its rank in its query against max_chains, the chain record without `first`, its slot
//  (hipcub exclusive scan of n_anchors) k_chain_first;  k_chain_scatter: EVERY anchor writes itself to first + rank of its chain.  No lane walks a chain.
// No lane loops over more than max_lookback candidates per anchor and nothing is quadratic in a run: a run of n anchors costs n x ceil(max_lookback / 64) wave steps in
// each of the first two sweeps and n in the third, one behind the other, so that ONE run of 10^5 anchors bounds the call however few the others are.  max_anchors is the
// caller's guard.  Every pass behind the first reads the error words and does nothing once one is set.
// Scratch: 85 bytes per anchor (24 the sorts' keys and index values, 16 the anchor record, 32 the sweeps' eight words, 13 flags, scan, run and slot words) and 0.25 for the
// list of long runs, 25 per query, 12 per kept chain, plus hipcub's own; freed on return.
// The run boundaries of the first pass (run_edges) and the hipcub calls written once (cub_size, cub_run) are fmgpu_positions.h's.
#include "fmgpu_positions.h"

namespace fmgpu {
namespace {

constexpr uint32_t kNo = 0xffffffffu;
constexpr uint64_t kMaxChainRecords = (1ull << 32) - 256;
constexpr uint64_t kPosLimit = 1ull << 62;
constexpr uint64_t kSpanLimit = 1ull << 31;
constexpr uint32_t kShortRun = 32;                          // runs of up to this many anchors go one per lane, longer ones one per wave
constexpr uint32_t kRing = 256;                             // the largest max_lookback: entries of the LDS ring
constexpr uint32_t kLongBlocks = 2048;                      // waves of k_chain_long at most; each takes runs until the list is empty

// the error words behind out_off's scratch, in the order they are reported; the word behind them carries the number of kept chain starts to the host
enum : int { E_RANGE = 0, E_ORDER = 1, E_HIT = 2, E_POS = 3, E_SPAN = 4, E_WORDS = 5, W_KEPT = 5 };
enum : uint8_t { F_START = 1, F_SKIPPED = 2, F_KEEP = 4 };
enum : uint8_t { CLS_NONE = 0, CLS_CHAINED = 1, CLS_FILTERED = 2, CLS_SKIPPED = 3 };

struct Anchor { uint64_t t; uint32_t q, l; };
static_assert(sizeof(Anchor) == 16, "one 16-byte piece");
static_assert(sizeof(fmgpu_chain) == 56 && sizeof(fmgpu_chain_spec) == 48, "the sizes include/fmgpu.h states");

struct ChainArgs {
    const fmgpu_position* pos; uint64_t count;
    const fmgpu_seed_span* spans; uint64_t n_spans;
    uint64_t nq;
    uint32_t max_gap, max_skew, gap_cost, lookback, min_score, min_anchors, max_chains, max_anchors;
    uint32_t *qfirst, *qend;                                // per query: its first record, one behind its last (the same in `positions` and in the order)
    uint64_t *qcount, *qoff;                                // nq + 1: the chains of each query, its first chain; qoff[nq] = the number of chains
    unsigned long long* err;                                // E_WORDS + 1 words, behind qoff
    uint8_t* cls;                                           // per query
    const uint32_t* order;                                  // per place: the anchor's index in `positions`
    Anchor* anc;                                            // per place
    uint8_t* flag;                                          // count + 1: F_*
    uint32_t *f, *p, *tt, *len, *leaf, *heir, *start, *rank;      // per place; p, leaf, heir and start are places (kNo: none)
    uint32_t* scan;                                         // count + 1: run starts in front of a place, later kept chain starts in front of it
    uint32_t* runstart;                                     // count + 1: the first place of each run
    uint32_t* words;                                        // [0] runs, [1] listed long runs, [2] the ticket of k_chain_long
    uint2* longruns;                                        // first place and anchors of each run of more than kShortRun anchors
    uint32_t* cslot;                                        // per place: the output slot of the chain that starts there (kNo: not reported)
};

struct BitOf {
    uint8_t mask;
    __host__ __device__ uint32_t operator()(uint8_t v) const { return v & mask ? 1u : 0u; }
};
using Bits = hipcub::TransformInputIterator<uint32_t, BitOf, const uint8_t*>;

__device__ __forceinline__ bool failed(const ChainArgs& a) {
    unsigned long long all = kNone;
#pragma unroll
    for (int k = 0; k < E_WORDS; ++k) all &= a.err[k];
    return all != kNone;
}

__global__ __launch_bounds__(256) void k_chain_check(ChainArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    uint64_t q;
    bool first, last;
    if (!run_edges(a.pos, a.count, i, 0u, a.nq, &a.err[E_RANGE], &a.err[E_ORDER], &q, &first, &last)) return;
    const uint32_t hit = a.pos[i].hit;
    if (hit >= a.n_spans) atomicMin(&a.err[E_HIT], (unsigned long long)i);
    else {
        const fmgpu_seed_span s = a.spans[hit];
        if (s.qlen == 0 || (uint64_t)s.qbeg + s.qlen >= kSpanLimit) atomicMin(&a.err[E_SPAN], (unsigned long long)i);
    }
    if (a.pos[i].pos >= kPosLimit) atomicMin(&a.err[E_POS], (unsigned long long)i);
    if (first) a.qfirst[q] = (uint32_t)i;
    if (last) a.qend[q] = (uint32_t)i + 1u;
}

// the keys of the four sorts: nothing here is indexed by a query number, and a hit beyond the spans reads none, so these run whatever the first pass found
__global__ __launch_bounds__(256) void k_chain_key_q(ChainArgs a, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.count) return;
    const uint32_t hit = a.pos[i].hit;
    keys[i] = hit < a.n_spans ? a.spans[hit].qbeg : 0u; vals[i] = (uint32_t)i;
}
template <int FIELD>                                        // 0: pos, 1: seq_id, 2: qidx
__global__ __launch_bounds__(256) void k_chain_key(ChainArgs a, const uint32_t* __restrict__ vals, uint64_t* __restrict__ keys) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.count) return;
    const fmgpu_position& r = a.pos[vals[j]];
    keys[j] = FIELD == 0 ? r.pos : FIELD == 1 ? r.seq_id : r.qidx;
}

__global__ __launch_bounds__(256) void k_chain_gather(ChainArgs a) {
    if (failed(a)) return;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.count) return;
    const fmgpu_position r = a.pos[a.order[g]];
    const fmgpu_seed_span s = a.spans[r.hit];
    *reinterpret_cast<ulonglong2*>(a.anc + g) = make_ulonglong2(r.pos, (unsigned long long)s.qbeg | ((unsigned long long)s.qlen << 32));
    bool first = g == 0, last = g + 1 == a.count;
    if (!first) { const fmgpu_position& b = a.pos[a.order[g - 1]]; first = b.qidx != r.qidx || b.seq_id != r.seq_id; }
    if (!last) { const fmgpu_position& b = a.pos[a.order[g + 1]]; last = b.qidx != r.qidx || b.seq_id != r.seq_id; }
    const bool skipped = a.max_anchors && a.qend[r.qidx] - a.qfirst[r.qidx] > a.max_anchors;
    a.flag[g] = (uint8_t)((first ? F_START : 0) | (skipped ? F_SKIPPED : 0));
    if (first && last && !skipped) {                        // a run of one anchor: nothing to sweep
        const uint32_t at = (uint32_t)g;
        a.f[g] = s.qlen; a.p[g] = kNo; a.tt[g] = s.qlen; a.len[g] = 1u; a.leaf[g] = at; a.heir[g] = kNo; a.start[g] = at; a.rank[g] = 0u;
    }
}

__global__ __launch_bounds__(256) void k_chain_runs(ChainArgs a) {
    if (failed(a)) return;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > a.count) return;
    if (g == a.count) { a.runstart[a.scan[g]] = (uint32_t)g; a.words[0] = a.scan[g]; }
    else if (a.flag[g] & F_START) a.runstart[a.scan[g]] = (uint32_t)g;
}

__device__ __forceinline__ Anchor load_anchor(const Anchor* __restrict__ anc, uint64_t g) {
    const ulonglong2 x = *reinterpret_cast<const ulonglong2*>(anc + g);
    return Anchor{x.x, (uint32_t)x.y, (uint32_t)(x.y >> 32)};
}

// anchor (t_i, q_i, l_i) behind candidate (t_j, q_j): may it link, and with what gain (>= 1)
__device__ __forceinline__ bool link_gain(const ChainArgs& a, uint64_t t_i, uint32_t q_i, uint32_t l_i, uint64_t t_j, uint32_t q_j, uint32_t* gain) {
    if (t_j >= t_i || q_j >= q_i) return false;
    const uint64_t dt = t_i - t_j, dq = q_i - q_j;
    if (dt > a.max_gap || dq > a.max_gap) return false;
    const uint64_t dd = dt > dq ? dt - dq : dq - dt;
    if (dd > a.max_skew) return false;
    uint64_t m = l_i < dq ? l_i : dq;
    m = m < dt ? m : dt;
    const uint64_t cost = ((uint64_t)a.gap_cost * dd) >> 8;
    if (m <= cost) return false;
    *gain = (uint32_t)(m - cost);
    return true;
}

__global__ __launch_bounds__(256) void k_chain_short(ChainArgs a) {
    if (failed(a)) return;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.words[0]) return;
    const uint32_t b = a.runstart[r], n = a.runstart[r + 1] - b;
    if (n == 1u || (a.flag[b] & F_SKIPPED)) return;
    if (n > kShortRun) { a.longruns[atomicAdd(&a.words[1], 1u)] = make_uint2(b, n); return; }
    const uint32_t L = a.lookback;
    for (uint32_t i = 0; i < n; ++i) {                      // f and p
        const Anchor x = load_anchor(a.anc, b + i);
        uint32_t best = x.l, from = kNo;
        for (uint32_t d = 1; d <= i && d <= L; ++d) {       // nearest first: a later equal value does not replace it
            const Anchor y = load_anchor(a.anc, b + i - d);
            uint32_t gain;
            if (!link_gain(a, x.t, x.q, x.l, y.t, y.q, &gain)) continue;
            const uint32_t v = a.f[b + i - d] + gain;
            if (v > best) { best = v; from = b + i - d; }
        }
        a.f[b + i] = best; a.p[b + i] = from;
    }
    for (uint32_t j = n; j-- > 0;) {                        // t, heir, chain length, leaf
        uint32_t t = 0, heir = kNo;
        for (uint32_t d = 1; j + d < n && d <= L; ++d)      // earliest first: a later equal t does not replace it
            if (a.p[b + j + d] == b + j && a.tt[b + j + d] > t) { t = a.tt[b + j + d]; heir = b + j + d; }
        a.heir[b + j] = heir;
        if (heir == kNo) { a.tt[b + j] = a.f[b + j]; a.len[b + j] = 1u; a.leaf[b + j] = b + j; }
        else { a.tt[b + j] = t; a.len[b + j] = a.len[heir] + 1u; a.leaf[b + j] = a.leaf[heir]; }
    }
    for (uint32_t i = 0; i < n; ++i) {                      // chain start and rank
        const uint32_t from = a.p[b + i];
        if (from != kNo && a.heir[from] == b + i) { a.start[b + i] = a.start[from]; a.rank[b + i] = a.rank[from] + 1u; }
        else { a.start[b + i] = b + i; a.rank[b + i] = 0u; }
    }
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) { const uint64_t w = (uint64_t)__shfl_xor((unsigned long long)v, o, 64); v = w > v ? w : v; }
    return v;
}

// One wave per run.  Places inside the run count from 0 here (b + place in the arrays).  Ring entry of place j, at j & 255, written once place j is decided and read by
// the at most max_lookback <= 256 places that follow it in the sweep's direction: sweep 1 {t low, t high, q, f}, sweep 2 {t, p, chain length, leaf}, sweep 3 {chain
// start, rank, heir}.  The slot of place j is that of j -+ 256, which the step reads (when max_lookback is 256) before lane 0 writes it.  The anchors of a step come from
// registers: the wave loads 64 at a time, one per lane, and each result goes back into its lane, so that global memory is read and written 64 places at a time.
__global__ __launch_bounds__(64) void k_chain_long(ChainArgs a) {
    __shared__ uint4 ring[kRing];
    if (failed(a)) return;
    const uint32_t lane = threadIdx.x, L = a.lookback;
    for (;;) {
        uint32_t ticket = 0;
        if (lane == 0) ticket = atomicAdd(&a.words[2], 1u);
        ticket = __shfl(ticket, 0, 64);
        if (ticket >= a.words[1]) return;
        const uint2 run = a.longruns[ticket];
        const uint32_t b = run.x, n = run.y;
        for (uint32_t c0 = 0; c0 < n; c0 += 64u) {          // sweep 1
            const uint32_t m = n - c0 < 64u ? n - c0 : 64u;
            Anchor x{0, 0, 0};
            if (lane < m) x = load_anchor(a.anc, b + c0 + lane);
            uint32_t my_f = 0, my_p = kNo;
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t i = c0 + k;
                const uint64_t t_i = (uint64_t)__shfl((unsigned long long)x.t, (int)k, 64);
                const uint32_t q_i = __shfl(x.q, (int)k, 64), l_i = __shfl(x.l, (int)k, 64);
                uint64_t key = 0;
                for (uint32_t d0 = 0; d0 < L && d0 < i; d0 += 64u) {
                    const uint32_t d = d0 + lane + 1u;
                    if (d > L || d > i) continue;
                    const uint4 e = ring[(i - d) & (kRing - 1u)];
                    uint32_t gain;
                    if (!link_gain(a, t_i, q_i, l_i, (uint64_t)e.x | ((uint64_t)e.y << 32), e.z, &gain)) continue;
                    const uint64_t cand = (((uint64_t)e.w + gain) << 32) | (i - d);
                    key = cand > key ? cand : key;
                }
                key = wave_max(key);
                uint32_t f_i = l_i, p_i = kNo;
                if ((uint32_t)(key >> 32) > l_i) { f_i = (uint32_t)(key >> 32); p_i = b + (uint32_t)key; }
                if (lane == k) { my_f = f_i; my_p = p_i; }
                if (lane == 0) ring[i & (kRing - 1u)] = make_uint4((uint32_t)t_i, (uint32_t)(t_i >> 32), q_i, f_i);
                __syncthreads();
            }
            if (lane < m) { a.f[b + c0 + lane] = my_f; a.p[b + c0 + lane] = my_p; }
        }
        __threadfence();
        for (uint32_t done = 0; done < n; done += 64u) {    // sweep 2: lane k holds place n - 1 - done - k
            const uint32_t m = n - done < 64u ? n - done : 64u, top = n - 1u - done;
            uint32_t x_f = 0, x_p = kNo;
            if (lane < m) { x_f = a.f[b + top - lane]; x_p = a.p[b + top - lane]; x_p = x_p == kNo ? kNo : x_p - b; }
            uint32_t my_t = 0, my_len = 0, my_leaf = 0, my_heir = kNo;
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t j = top - k;
                const uint32_t f_j = __shfl(x_f, (int)k, 64), p_j = __shfl(x_p, (int)k, 64);
                uint64_t key = 0;
                for (uint32_t d0 = 0; d0 < L && j + d0 + 1u < n; d0 += 64u) {
                    const uint32_t d = d0 + lane + 1u;
                    if (d > L || j + d >= n) continue;
                    const uint4 e = ring[(j + d) & (kRing - 1u)];
                    if (e.y != j) continue;
                    const uint64_t cand = ((uint64_t)e.x << 32) | (kNo - (j + d));
                    key = cand > key ? cand : key;
                }
                key = wave_max(key);
                uint32_t t_j = f_j, len_j = 1u, leaf_j = j, heir_j = kNo;
                if (key) {                                  // (a child's t is at least its f, which is above f_j)
                    heir_j = kNo - (uint32_t)key;
                    const uint4 e = ring[heir_j & (kRing - 1u)];
                    t_j = e.x; len_j = e.z + 1u; leaf_j = e.w;
                }
                if (lane == k) { my_t = t_j; my_len = len_j; my_leaf = leaf_j; my_heir = heir_j; }
                if (lane == 0) ring[j & (kRing - 1u)] = make_uint4(t_j, p_j, len_j, leaf_j);
                __syncthreads();
            }
            if (lane < m) {
                const uint32_t g = b + top - lane;
                a.tt[g] = my_t; a.len[g] = my_len; a.leaf[g] = b + my_leaf; a.heir[g] = my_heir == kNo ? kNo : b + my_heir;
            }
        }
        __threadfence();
        for (uint32_t c0 = 0; c0 < n; c0 += 64u) {          // sweep 3
            const uint32_t m = n - c0 < 64u ? n - c0 : 64u;
            uint32_t x_p = kNo, x_heir = kNo;
            if (lane < m) {
                x_p = a.p[b + c0 + lane]; x_p = x_p == kNo ? kNo : x_p - b;
                x_heir = a.heir[b + c0 + lane]; x_heir = x_heir == kNo ? kNo : x_heir - b;
            }
            uint32_t my_start = 0, my_rank = 0;
            for (uint32_t k = 0; k < m; ++k) {
                const uint32_t i = c0 + k;
                const uint32_t p_i = __shfl(x_p, (int)k, 64), heir_i = __shfl(x_heir, (int)k, 64);
                uint32_t start_i = i, rank_i = 0u;
                if (p_i != kNo) {
                    const uint4 e = ring[p_i & (kRing - 1u)];
                    if (e.z == i) { start_i = e.x; rank_i = e.y + 1u; }
                }
                if (lane == k) { my_start = start_i; my_rank = rank_i; }
                if (lane == 0) ring[i & (kRing - 1u)] = make_uint4(start_i, rank_i, heir_i, 0u);
                __syncthreads();
            }
            if (lane < m) { a.start[b + c0 + lane] = b + my_start; a.rank[b + c0 + lane] = my_rank; }
        }
    }
}

// the chain that starts at place s: its score; *branch: it hangs off a better chain
__device__ __forceinline__ uint32_t chain_score(const ChainArgs& a, uint64_t s, bool* branch) {
    const uint32_t from = a.p[s];
    *branch = from != kNo;
    return a.tt[s] - (from != kNo ? a.f[from] : 0u);
}

__global__ __launch_bounds__(256) void k_chain_keep(ChainArgs a) {
    if (failed(a)) return;
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.count) return;
    const uint8_t fl = a.flag[g];
    if ((fl & F_SKIPPED) || a.start[g] != (uint32_t)g) return;
    bool branch;
    if (chain_score(a, g, &branch) >= a.min_score && a.len[g] >= (a.min_anchors ? a.min_anchors : 1u)) a.flag[g] = fl | F_KEEP;
}

__global__ __launch_bounds__(256) void k_chain_queries(ChainArgs a) {
    if (failed(a)) return;
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > a.nq) return;
    if (q == a.nq) { a.err[W_KEPT] = a.scan[a.count]; return; }
    const uint32_t first = a.qfirst[q];
    uint64_t chains = 0;
    uint8_t c = CLS_NONE;
    if (first != kNo) {
        const uint32_t end = a.qend[q];
        if (a.max_anchors && end - first > a.max_anchors) c = CLS_SKIPPED;
        else {
            chains = a.scan[end] - a.scan[first];
            if (a.max_chains && chains > a.max_chains) chains = a.max_chains;
            c = chains ? CLS_CHAINED : CLS_FILTERED;
        }
    }
    a.qcount[q] = chains; a.cls[q] = c;
}

__global__ __launch_bounds__(256) void k_chain_compact(ChainArgs a, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.count || !(a.flag[g] & F_KEEP)) return;
    bool branch;
    const uint32_t score = chain_score(a, g, &branch), at = a.scan[g];
    keys[at] = ((uint64_t)a.qfirst[a.pos[a.order[g]].qidx] << 32) | (uint32_t)~score;
    vals[at] = (uint32_t)g;
}

__global__ __launch_bounds__(256) void k_chain_emit(ChainArgs a, const uint32_t* __restrict__ sorted, uint64_t kept, fmgpu_chain* __restrict__ out, uint32_t* __restrict__ out_n) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kept) return;
    const uint32_t s = sorted[k];
    const fmgpu_position r = a.pos[a.order[s]];
    const uint64_t place = k - a.scan[a.qfirst[r.qidx]];    // among the kept chains of its query, in output order
    if (a.max_chains && place >= a.max_chains) return;
    const uint64_t o = a.qoff[r.qidx] + place;
    const Anchor x = load_anchor(a.anc, s), y = load_anchor(a.anc, a.leaf[s]);
    bool branch;
    fmgpu_chain c;
    c.qidx = r.qidx; c.seq_id = r.seq_id; c.tbeg = x.t; c.tend = y.t + y.l; c.qbeg = x.q; c.qend = y.q + y.l;
    c.score = chain_score(a, s, &branch); c.n_anchors = a.len[s]; c.first = 0u; c.flags = branch ? 1u : 0u;
    out[o] = c;
    out_n[o] = c.n_anchors;
    a.cslot[s] = (uint32_t)o;
}

__global__ __launch_bounds__(256) void k_chain_first(fmgpu_chain* __restrict__ out, const uint32_t* __restrict__ first, uint64_t total) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o < total) out[o].first = first[o];
}

__global__ __launch_bounds__(256) void k_chain_scatter(ChainArgs a, const uint32_t* __restrict__ first, uint32_t* __restrict__ out_anchor) {
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.count || (a.flag[g] & F_SKIPPED)) return;
    const uint32_t o = a.cslot[a.start[g]];
    if (o != kNo) out_anchor[first[o] + a.rank[g]] = a.order[g];
}

// nothing to chain: zero offsets and classes, in host or device memory
int chain_nothing(uint64_t nq, uint64_t* out_off, uint8_t* out_class, hipStream_t stream) {
    bool waits = false;
    if (out_off) {
        if (is_device_pointer(out_off)) { FM_HIP(hipMemsetAsync(out_off, 0, (nq + 1) * 8, stream)); waits = true; }
        else std::memset(out_off, 0, (nq + 1) * 8);
    }
    if (out_class && nq) {
        if (is_device_pointer(out_class)) { FM_HIP(hipMemsetAsync(out_class, 0, nq, stream)); waits = true; }
        else std::memset(out_class, 0, nq);
    }
    if (waits) FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_seeds_chain(const fmgpu_position* positions, uint64_t count, const fmgpu_seed_span* spans, uint64_t n_spans, const fmgpu_chain_spec* spec,
                      fmgpu_chain* out, uint64_t capacity, uint64_t* out_count, uint32_t* out_anchor, uint64_t* out_off, uint8_t* out_class, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!spec) return fail(FMGPU_ERR_INVALID, "fmgpu_seeds_chain: spec is null");
    if (!out_count) return fail(FMGPU_ERR_INVALID, "fmgpu_seeds_chain: out_count is null");
    if (spec->max_gap < 1 || spec->max_gap > 0x7fffffffu) return fail(FMGPU_ERR_INVALID, "fmgpu_chain_spec: max_gap must lie in 1 .. 2^31 - 1");
    if (spec->max_skew < 1 || spec->max_skew > 0x7fffffffu) return fail(FMGPU_ERR_INVALID, "fmgpu_chain_spec: max_skew must lie in 1 .. 2^31 - 1");
    if (spec->gap_cost_q8 > 65536u) return fail(FMGPU_ERR_INVALID, "fmgpu_chain_spec: gap_cost_q8 must lie in 0 .. 65536");
    if (spec->max_lookback < 1 || spec->max_lookback > kRing) return fail(FMGPU_ERR_INVALID, "fmgpu_chain_spec: max_lookback must lie in 1 .. 256");
    for (int k = 0; k < 8; ++k) if (spec->reserved[k]) return fail(FMGPU_ERR_INVALID, "fmgpu_chain_spec: reserved must be 0");
    if (count && !positions) return fail(FMGPU_ERR_INVALID, "fmgpu_seeds_chain: positions is null while count > 0");
    if (count && !spans) return fail(FMGPU_ERR_INVALID, "fmgpu_seeds_chain: spans is null while count > 0");
    if (!out && capacity) return fail(FMGPU_ERR_INVALID, "fmgpu_seeds_chain: out is null while capacity > 0");
    *out_count = 0;
    if (count >= kMaxChainRecords || n_spans >= kMaxChainRecords) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_seeds_chain: count and n_spans must each stay below 2^32 - 256");
    const uint64_t nq = spec->nq;
    if (nq == 0 || count == 0) return chain_nothing(nq, out_off, out_class, stream);

    ChainArgs a;
    std::memset(&a, 0, sizeof a);
    a.count = count; a.n_spans = n_spans; a.nq = nq;
    a.max_gap = spec->max_gap; a.max_skew = spec->max_skew; a.gap_cost = spec->gap_cost_q8; a.lookback = spec->max_lookback;
    a.min_score = spec->min_score; a.min_anchors = spec->min_anchors; a.max_chains = spec->max_chains; a.max_anchors = spec->max_anchors;

    int rc;
    Staged spos, sspans, sout, sanchor;
    if ((rc = spos.in(positions, count * sizeof(fmgpu_position), stream)) || (rc = sspans.in(spans, n_spans * sizeof(fmgpu_seed_span), stream))) return rc;
    a.pos = (const fmgpu_position*)spos.dev; a.spans = (const fmgpu_seed_span*)sspans.dev;

    const uint64_t max_long = count / (kShortRun + 1u) + 1u;
    DBuf queries, offs, keys, vals, anchors, sweeps, flags, words, longs, tmp;
    if ((rc = queries.alloc(nq * 9)) || (rc = offs.alloc((2 * (nq + 1) + E_WORDS + 1) * 8)) || (rc = keys.alloc(count * 16)) || (rc = vals.alloc(count * 8)) ||
        (rc = anchors.alloc(count * sizeof(Anchor))) || (rc = sweeps.alloc((11 * count + 2) * 4)) || (rc = flags.alloc(count + 1)) || (rc = words.alloc(16)) ||
        (rc = longs.alloc(max_long * sizeof(uint2))))
        return rc;
    a.qfirst = queries.as<uint32_t>(); a.qend = a.qfirst + nq; a.cls = reinterpret_cast<uint8_t*>(a.qend + nq);
    a.qcount = offs.as<uint64_t>(); a.qoff = a.qcount + (nq + 1);
    a.err = reinterpret_cast<unsigned long long*>(a.qoff + (nq + 1));
    uint64_t *k0 = keys.as<uint64_t>(), *k1 = k0 + count;
    uint32_t *v0 = vals.as<uint32_t>(), *v1 = v0 + count;
    a.anc = anchors.as<Anchor>();
    a.f = sweeps.as<uint32_t>(); a.p = a.f + count; a.tt = a.p + count; a.len = a.tt + count; a.leaf = a.len + count; a.heir = a.leaf + count;
    a.start = a.heir + count; a.rank = a.start + count; a.cslot = a.rank + count; a.scan = a.cslot + count; a.runstart = a.scan + (count + 1);
    a.flag = flags.as<uint8_t>();
    a.words = words.as<uint32_t>();
    a.longruns = longs.as<uint2>();
    a.order = v0;                                           // where the fourth sort leaves the index values
    int q_bits = 1;
    while (q_bits < 64 && (nq - 1) >> q_bits) ++q_bits;

    Bits run_starts(a.flag, BitOf{F_START}), kept_starts(a.flag, BitOf{F_KEEP});
    auto scan_runs = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, run_starts, a.scan, (size_t)(count + 1), stream); };
    auto scan_kept = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, kept_starts, a.scan, (size_t)(count + 1), stream); };
    auto scan_queries = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, a.qcount, a.qoff, (size_t)(nq + 1), stream); };
    auto sort_q = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, (uint32_t*)k0, (uint32_t*)k1, v0, v1, (size_t)count, 0, 31, stream); };
    auto sort_t = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, v1, v0, (size_t)count, 0, 62, stream); };
    auto sort_seq = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, v0, v1, (size_t)count, 0, 64, stream); };
    auto sort_qidx = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, v1, v0, (size_t)count, 0, q_bits, stream); };
    size_t tb = 0;
    FM_HIP(cub_size(&tb, scan_runs, scan_kept, scan_queries, sort_q, sort_t, sort_seq, sort_qidx));
    if ((rc = tmp.alloc(tb))) return rc;

    FM_HIP(hipMemsetAsync(a.qfirst, 0xff, nq * 4, stream));
    FM_HIP(hipMemsetAsync(a.qcount, 0, (nq + 1) * 8, stream));
    FM_HIP(hipMemsetAsync(a.cls, 0, nq, stream));
    FM_HIP(hipMemsetAsync(a.err, 0xff, (E_WORDS + 1) * 8, stream));
    FM_HIP(hipMemsetAsync(a.flag, 0, count + 1, stream));
    FM_HIP(hipMemsetAsync(a.words, 0, 16, stream));
    FM_HIP(hipMemsetAsync(a.cslot, 0xff, count * 4, stream));
    FM_GRID(grid, count + 1);
    FM_GRID(qgrid, nq + 1);
    k_chain_check<<<grid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_check");
    k_chain_key_q<<<grid, dim3(256), 0, stream>>>(a, (uint32_t*)k0, v0);
    FM_LAUNCHED("k_chain_key_q");
    FM_HIP(cub_run(sort_q, tmp));                                   // v1: by q, then index
    k_chain_key<0><<<grid, dim3(256), 0, stream>>>(a, v1, k0);
    FM_LAUNCHED("k_chain_key");
    FM_HIP(cub_run(sort_t, tmp));                                   // v0: by t, stable
    k_chain_key<1><<<grid, dim3(256), 0, stream>>>(a, v0, k0);
    FM_LAUNCHED("k_chain_key");
    FM_HIP(cub_run(sort_seq, tmp));                                 // v1: by seq_id, stable
    k_chain_key<2><<<grid, dim3(256), 0, stream>>>(a, v1, k0);
    FM_LAUNCHED("k_chain_key");
    FM_HIP(cub_run(sort_qidx, tmp));                                // v0: by qidx, stable: the order
    k_chain_gather<<<grid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_gather");
    FM_HIP(cub_run(scan_runs, tmp));
    k_chain_runs<<<grid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_runs");
    k_chain_short<<<grid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_short");
    k_chain_long<<<dim3((unsigned)std::min<uint64_t>(max_long, kLongBlocks)), dim3(64), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_long");
    k_chain_keep<<<grid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_keep");
    FM_HIP(cub_run(scan_kept, tmp));
    k_chain_queries<<<qgrid, dim3(256), 0, stream>>>(a);
    FM_LAUNCHED("k_chain_queries");
    FM_HIP(cub_run(scan_queries, tmp));
    uint64_t back[2 + E_WORDS];                                     // the number of chains, the error words, the kept chain starts: the call's one read-back
    FM_HIP(hipMemcpyAsync(back, a.qoff + nq, sizeof back, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    const uint64_t* err = back + 1;
    static const char* const kWhat[E_WORDS] = {" names a query beyond nq", " names a query below its predecessor's", " has a hit beyond the spans", " has a pos of 2^62 or more",
                                               " has a span with qlen == 0 or qbeg + qlen of 2^31 or more"};
    for (int k = 0; k < E_WORDS; ++k) if (err[k] != kNone) return fail(FMGPU_ERR_INVALID, "fmgpu_seeds_chain: record " + std::to_string(err[k]) + kWhat[k]);
    const uint64_t total = back[0], kept = err[W_KEPT];
    *out_count = total;
    if (out_off) FM_HIP(hipMemcpyAsync(out_off, a.qoff, (nq + 1) * 8, hipMemcpyDefault, stream));
    if (out_class) FM_HIP(hipMemcpyAsync(out_class, a.cls, nq, hipMemcpyDefault, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (!out && !capacity) return 0;
    if (total > capacity) return fail(FMGPU_ERR_CAPACITY, std::to_string(total) + " chains: more than `capacity`");
    if (!total) return 0;

    // the order of the chains: the kept starts by (query, score descending, place), then each one's rank in its query against max_chains
    DBuf chains, tmp2;
    if ((rc = chains.alloc((kept + 2 * (total + 1)) * 4))) return rc;
    uint32_t *sorted = chains.as<uint32_t>(), *out_n = sorted + kept, *first = out_n + (total + 1);
    auto sort_kept = [&](void* t, size_t& b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, v1, sorted, (size_t)kept, 0, 64, stream); };
    auto scan_anchors = [&](void* t, size_t& b) { return hipcub::DeviceScan::ExclusiveSum(t, b, out_n, first, (size_t)(total + 1), stream); };
    size_t tb2 = 0;
    FM_HIP(cub_size(&tb2, sort_kept, scan_anchors));
    if ((rc = tmp2.alloc(tb2))) return rc;
    if ((rc = sout.out(out, total * sizeof(fmgpu_chain), stream))) return rc;
    k_chain_compact<<<grid, dim3(256), 0, stream>>>(a, k0, v1);
    FM_LAUNCHED("k_chain_compact");
    FM_HIP(cub_run(sort_kept, tmp2));
    FM_HIP(hipMemsetAsync(out_n, 0, (total + 1) * 4, stream));
    FM_GRID(kgrid, kept);
    k_chain_emit<<<kgrid, dim3(256), 0, stream>>>(a, sorted, kept, (fmgpu_chain*)sout.dev, out_n);
    FM_LAUNCHED("k_chain_emit");
    FM_HIP(cub_run(scan_anchors, tmp2));
    FM_GRID(ogrid, total);
    k_chain_first<<<ogrid, dim3(256), 0, stream>>>((fmgpu_chain*)sout.dev, first, total);
    FM_LAUNCHED("k_chain_first");
    if (out_anchor) {
        if ((rc = sanchor.out(out_anchor, count * 4, stream))) return rc;
        if (sanchor.owned) FM_HIP(hipMemsetAsync(sanchor.dev, 0, count * 4, stream));      // (a host array gets zeros behind the anchors of the reported chains)
        k_chain_scatter<<<grid, dim3(256), 0, stream>>>(a, first, (uint32_t*)sanchor.dev);
        FM_LAUNCHED("k_chain_scatter");
        if ((rc = sanchor.finish())) return rc;
    }
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

}  // extern "C"
