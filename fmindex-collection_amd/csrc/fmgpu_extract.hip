// fmgpu_extract.hip — text extraction from the index (the reference's reconstructText, utils.h:672-703, as parallel LF walks):
//  fmgpu_index_accelerate_extract  the text map (per seqId: length, end row, global start) and the sampled rows in text order
//  build_sample_chain              Format C (fmgpu_common.h) from that sample table: k_chain_fill walks `rate` LF steps back from every sampled row
//  k_range_pieces                  per range: the sequence, the bounds check, the sampled positions inside it (two binary searches) -> piece count
//  k_extract                       one piece per lane: an LF walk back from a sampled row (or the end row), symbols buffered into 8-byte stores
// In global coordinates (start[s] + pos) a range [g0, g1) is cut at every sampled position inside (g0, g1); its last piece starts at the first sample at
// or after g1 in the sequence, or at the sequence's end row, and walks past key - g1 symbols before it writes.  A piece walks from its key down to the
// previous cut (or g0): it applies LF only to rows of positions > g0 >= start[s], whose BWT symbol lies inside the sequence — it never crosses into the
// previous sequence, and a delimiter inside [0, len) is a symbol like any other.
#include "fmgpu_search_shared.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <numeric>

namespace FMGPU_NS {

struct ExtView {
    const uint64_t* seq_id; const uint64_t* len; const uint64_t* start; const idx_t* end_row;
    const uint64_t* key; const idx_t* row;
    uint64_t nseq, nsamp;
};
static ExtView ext_view(const ExtractTable& t) { return ExtView{t.seq_id, t.len, t.start, t.end_row, t.key, t.row, t.nseq, t.nsamp}; }

// the pieces of one range: [g0, g1) in global coordinates, samples a .. a + pieces - 2 inside it, the last piece's key and row
struct RangeInfo { uint64_t g0, g1, a, fkey; uint64_t frow; };

__device__ __forceinline__ uint64_t lower_bound_u64(const uint64_t* v, uint64_t n, uint64_t x) {     // first i with v[i] >= x
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2u; if (v[mid] < x) lo = mid + 1u; else hi = mid; }
    return lo;
}

// ------------------------------------------------------------------ table build
// the number of sampled rows: rank at the last word + its bits
__global__ void k_sample_count(ViewSA sa, uint64_t nwords, uint64_t n, unsigned long long* out) {
    const uint64_t j = nwords - 1u;
    uint64_t w = sa.bits[j];
    const uint64_t valid = n - j * 64u;
    if (valid < 64u) w &= lowmask((uint32_t)valid);
    out[0] = sa_rank(sa, (idx_t)(j * 64u)) + popc64(w);
}
// every sampled row k (rank order): its global coordinate and its row; a seqId outside the map or a pos beyond its length sets *bad
__global__ __launch_bounds__(256) void k_sample_keys(ViewSA sa, uint64_t nwords, uint64_t n, ExtView ev, uint64_t* __restrict__ keys, idx_t* __restrict__ rows,
                                                     unsigned long long* __restrict__ bad) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nwords) return;
    uint64_t w = sa.bits[j];
    const uint64_t valid = n - j * 64u;
    if (valid < 64u) w &= lowmask((uint32_t)valid);
    if (!w) return;
    uint64_t k = sa_rank(sa, (idx_t)(j * 64u));
    bool broken = false;
    while (w) {
        const uint32_t b = (uint32_t)__ffsll((unsigned long long)w) - 1u;
        w &= w - 1u;
        const uint64_t seq = dense_access(sa.f0, sa.bits0, sa.div0, k);
        const uint64_t pos = dense_access(sa.f1, sa.bits1, sa.div1, k);
        const uint64_t s = lower_bound_u64(ev.seq_id, ev.nseq, seq);
        if (s >= ev.nseq || ev.seq_id[s] != seq || pos > ev.len[s]) { broken = true; keys[k] = 0; }
        else keys[k] = ev.start[s] + pos;
        rows[k] = (idx_t)(j * 64u + b);
        ++k;
    }
    if (broken) atomicOr(bad, 1ull);
}
__global__ void k_iota_rows(uint64_t* __restrict__ out, uint64_t first, uint64_t count) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < count) out[t] = first + t;
}

// ------------------------------------------------------------------ Format C (fmgpu_common.h)
constexpr uint32_t kChainMaxListed = 512;            // unusable entries: more than these and the chain is not built
// entry t from the handle alone: `rate` LF steps back from the t-th sampled row in text order; usable if they pass symbols 1..4 only and arrive at the row of entry t - 1
template <class Occ>
__global__ __launch_bounds__(256) void k_chain_fill(Occ occ, ViewSA sa, const idx_t* __restrict__ srow, uint64_t nsamp, uint32_t rate, uint2* __restrict__ chain,
                                                    uint32_t* __restrict__ chain_of, uint32_t* __restrict__ ex, uint32_t* __restrict__ nex) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nsamp) return;
    const idx_t row = srow[t];
    bool usable = t > 0;
    uint32_t syms = 0;
    if (usable) {
        idx_t r = row;
        for (uint32_t j = 0; j < rate; ++j) {
            uint32_t c;
            r = occ.lf_symbol(r, c);
            if (c - 1u >= 4u) { usable = false; break; }
            syms |= (c - 1u) << (2u * j);
        }
        if (usable && r != srow[t - 1u]) usable = false;
    }
    chain[t] = make_uint2((uint32_t)row, usable ? syms : 0u);
    chain_of[sa_rank(sa, row)] = (uint32_t)t;
    if (!usable) { const uint32_t k = atomicAdd(nex, 1u); if (k < kChainMaxListed) ex[k] = (uint32_t)t; }
}

// ------------------------------------------------------------------ extraction
// pieces pass: len[t] and pieces[t] of every range (entry `count`: 0, so that the exclusive scans of count + 1 entries end in the totals); a bad range sets *bad
__global__ __launch_bounds__(256) void k_range_pieces(const fmgpu_text_range* __restrict__ ranges, uint64_t count, ExtView ev, RangeInfo* __restrict__ info,
                                                      uint64_t* __restrict__ len, uint64_t* __restrict__ pieces, unsigned long long* __restrict__ bad) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > count) return;
    uint64_t l = 0, p = 0;
    if (t < count) {
        const fmgpu_text_range r = ranges[t];
        const uint64_t s = lower_bound_u64(ev.seq_id, ev.nseq, r.seq_id);
        if (s >= ev.nseq || ev.seq_id[s] != r.seq_id || r.len > ev.len[s] || r.pos > ev.len[s] - r.len) atomicOr(bad, 1ull);
        else if (r.len) {
            const uint64_t g0 = ev.start[s] + r.pos, g1 = g0 + r.len, gend = ev.start[s] + ev.len[s];
            const uint64_t a = lower_bound_u64(ev.key, ev.nsamp, g0 + 1u);     // the first sample after g0
            const uint64_t b = lower_bound_u64(ev.key, ev.nsamp, g1);          // the first sample at or after g1
            RangeInfo in{g0, g1, a, gend, (uint64_t)ev.end_row[s]};
            if (b < ev.nsamp && ev.key[b] <= gend) { in.fkey = ev.key[b]; in.frow = (uint64_t)ev.row[b]; }
            info[t] = in;
            l = r.len; p = b - a + 1u;
        }
    }
    len[t] = l; pieces[t] = p;
}

// One piece per lane.  The piece's range h is the last one with poff[h] <= t (an empty range shares its offset with its successor: never chosen).  The walk
// emits T[q] for q = key - 1 down to `lower`; T[q] lands at out + ooff[h] + (q - g0).  Symbols are gathered into the aligned 8-byte word they belong to and
// written with one store when the lane owns the whole word (byte stores only at the piece's two edges, whose words other lanes share).
template <class Occ, bool kLF>
__global__ __launch_bounds__(256) void k_extract(Occ occ, const idx_t* __restrict__ lf_table, const idx_t* __restrict__ C, uint32_t sigma, const uint64_t* __restrict__ key,
                                                 const idx_t* __restrict__ srow, const RangeInfo* __restrict__ info, const uint64_t* __restrict__ poff,
                                                 const uint64_t* __restrict__ ooff, uint64_t nranges, uint64_t first, uint64_t cnt, uint8_t* __restrict__ out,
                                                 unsigned long long* __restrict__ steps_total) {
    __shared__ idx_t sC[kLF ? 257 : 1];
    if constexpr (kLF) {
        for (uint32_t c = threadIdx.x; c <= sigma; c += blockDim.x) sC[c] = C[c];
        __syncthreads();
    }
    const uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t steps = 0;
    if (u < cnt) {
        const uint64_t t = first + u;
        uint64_t lo = 0, hi = nranges - 1u;
        while (lo < hi) { const uint64_t mid = hi - (hi - lo) / 2u; if (poff[mid] <= t) lo = mid; else hi = mid - 1u; }
        const uint64_t h = lo, j = t - poff[h], npc = poff[h + 1u] - poff[h];
        const RangeInfo r = info[h];
        const uint64_t lower = j == 0 ? r.g0 : key[r.a + j - 1u];
        uint64_t top; idx_t row;
        if (j + 1u < npc) { top = key[r.a + j]; row = srow[r.a + j]; } else { top = r.fkey; row = (idx_t)r.frow; }
        const uint64_t end = top < r.g1 ? top : r.g1;                   // written: [lower, end)
        uint8_t* const base = out + (ooff[h] - r.g0);                   // (+ q: the address of T[q]; only formed for q in [g0, g1))
        uint64_t word = 0;
        uint32_t hib = 0;                                               // the highest byte of the current word written so far
        bool fresh = true;
        for (uint64_t q = top; q > lower;) {
            --q;
            uint32_t c;
            if constexpr (kLF) { row = lf_table[row]; c = symbol_of_lf_lds(sC, sigma, row); }
            else row = occ.lf_symbol(row, c);
            ++steps;
            if (q >= end) continue;
            uint8_t* const p = base + q;
            const uint32_t k = (uint32_t)((uintptr_t)p & 7u);
            if (fresh) { hib = k; fresh = false; }
            word |= (uint64_t)(c & 0xffu) << (8u * k);
            if (k == 0u || q == lower) {                                // the word is complete, or the piece ends inside it
                if (k == 0u && hib == 7u) *reinterpret_cast<uint64_t*>(p) = word;
                else for (uint32_t i = k; i <= hib; ++i) p[i - k] = (uint8_t)(word >> (8u * i));
                word = 0; fresh = true;
            }
        }
    }
    add_counters(steps_total, steps, 0u, 0u);
}

namespace api {
#include "fmgpu_api_decl.h"

static void drop_extract(Index* x) {
    if (x->ext.dev) { (void)hipFree(x->ext.dev); x->device_bytes -= x->ext.bytes; }
    x->ext = ExtractTable{};
}

int fmgpu_index_accelerate_extract(fmgpu_index_t h, int32_t enable) {
    Index* x = reinterpret_cast<Index*>(h);
    if (!x) return fail(FMGPU_ERR_INVALID, "index handle is null");
    if (int drc = on_handle_device(x)) return drc;
    drop_extract(x);
    if (!enable) return 0;
    if (!x->has_sa) return fail(FMGPU_ERR_INVALID, "index was created without an annotated (sampled suffix) array");
    const uint64_t n = x->bwt.n;
    const uint64_t r0 = x->hC[0], nsent = x->hC[1] - x->hC[0];
    if (n == 0 || nsent == 0) return fail(FMGPU_ERR_UNSUPPORTED, "the index has no delimiter rows: no sequence ends to extract from");
    int rc;
    // ---- text map: the sentinel rows located (host: a few values per sequence)
    std::vector<uint64_t> seq(nsent), pos(nsent), st(nsent);
    {
        DBuf buf;
        if ((rc = buf.alloc(nsent * 8 * 4))) return rc;
        uint64_t* b = buf.as<uint64_t>();
        k_iota_rows<<<dim3((unsigned)((nsent + 255) / 256)), 256>>>(b, r0, nsent);
        FM_LAUNCHED("k_iota_rows");
        if ((rc = api::fmgpu_locate(h, b, nsent, b + nsent, b + 2 * nsent, b + 3 * nsent, nullptr, nullptr))) return rc;
        FM_HIP(hipMemcpy(seq.data(), b + nsent, nsent * 8, hipMemcpyDeviceToHost));
        FM_HIP(hipMemcpy(pos.data(), b + 2 * nsent, nsent * 8, hipMemcpyDeviceToHost));
        FM_HIP(hipMemcpy(st.data(), b + 3 * nsent, nsent * 8, hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> order(nsent);
    for (uint64_t i = 0; i < nsent; ++i) {
        if (st[i] == ~0ull) return fail(FMGPU_ERR_UNSUPPORTED, "sentinel row " + std::to_string(r0 + i) + " does not locate");
        pos[i] += st[i];
    }
    std::iota(order.begin(), order.end(), 0ull);
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return seq[a] != seq[b] ? seq[a] < seq[b] : pos[a] < pos[b]; });
    ExtractTable t;
    std::vector<uint64_t> hstart;
    std::vector<idx_t> hend;
    for (uint64_t i = 0; i < nsent; ++i) {
        const uint64_t o = order[i];
        if (i + 1 < nsent && seq[order[i + 1]] == seq[o]) continue;     // the last delimiter of its seqId
        hstart.push_back(t.host_seq.empty() ? 0 : hstart.back() + t.host_len.back() + 1);
        t.host_seq.push_back(seq[o]); t.host_len.push_back(pos[o]); hend.push_back((idx_t)(r0 + o));
    }
    t.nseq = t.host_seq.size();
    const uint64_t gmax = hstart.back() + t.host_len.back();            // the largest global coordinate
    // ---- sample table: every sampled row with its global coordinate, sorted by it
    const uint64_t nwords = (n + 63) / 64;
    DBuf small;
    if ((rc = small.alloc(16))) return rc;
    k_sample_count<<<1, 1>>>(x->vsa, nwords, n, small.as<unsigned long long>());
    FM_LAUNCHED("k_sample_count");
    uint64_t m = 0;
    FM_HIP(hipMemcpy(&m, small.p, 8, hipMemcpyDeviceToHost));
    t.nsamp = m;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_len = al(t.nseq * 8), o_start = o_len + al(t.nseq * 8), o_end = o_start + al(t.nseq * 8), o_key = o_end + al(t.nseq * sizeof(idx_t));
    const size_t o_row = o_key + al(m * 8), total = o_row + al(m * sizeof(idx_t));
    DBuf tab;
    if ((rc = tab.alloc(total))) return rc;
    uint8_t* d = tab.as<uint8_t>();
    FM_HIP(hipMemcpy(d, t.host_seq.data(), t.nseq * 8, hipMemcpyHostToDevice));
    FM_HIP(hipMemcpy(d + o_len, t.host_len.data(), t.nseq * 8, hipMemcpyHostToDevice));
    FM_HIP(hipMemcpy(d + o_start, hstart.data(), t.nseq * 8, hipMemcpyHostToDevice));
    FM_HIP(hipMemcpy(d + o_end, hend.data(), t.nseq * sizeof(idx_t), hipMemcpyHostToDevice));
    t.seq_id = (const uint64_t*)d; t.len = (const uint64_t*)(d + o_len); t.start = (const uint64_t*)(d + o_start); t.end_row = (const idx_t*)(d + o_end);
    t.key = (const uint64_t*)(d + o_key); t.row = (const idx_t*)(d + o_row);
    if (m) {
        DBuf keys, rows, tmp;
        if ((rc = keys.alloc(m * 8)) || (rc = rows.alloc(m * sizeof(idx_t)))) return rc;
        FM_HIP(hipMemset(small.p, 0, 8));
        FM_GRID(grid, nwords);
        k_sample_keys<<<grid, 256>>>(x->vsa, nwords, n, ext_view(t), keys.as<uint64_t>(), rows.as<idx_t>(), small.as<unsigned long long>());
        FM_LAUNCHED("k_sample_keys");
        unsigned long long bad = 0;
        FM_HIP(hipMemcpy(&bad, small.p, 8, hipMemcpyDeviceToHost));
        if (bad) return fail(FMGPU_ERR_UNSUPPORTED, "a sampled entry names a seqId that no sentinel row gave, or a pos beyond that sequence's last delimiter");
        int end_bit = 1;
        while (end_bit < 64 && (gmax >> end_bit)) ++end_bit;
        size_t tb = 0;
        FM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys.as<uint64_t>(), (uint64_t*)(d + o_key), rows.as<idx_t>(), (idx_t*)(d + o_row), (size_t)m, 0, end_bit));
        if ((rc = tmp.alloc(tb))) return rc;
        FM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, keys.as<uint64_t>(), (uint64_t*)(d + o_key), rows.as<idx_t>(), (idx_t*)(d + o_row), (size_t)m, 0, end_bit));
        FM_HIP(hipDeviceSynchronize());
    }
    t.bytes = total;
    t.dev = tab.take();
    x->ext = std::move(t);
    x->device_bytes += total;
    return 0;
}

int fmgpu_sequence_lengths(fmgpu_index_t h, uint64_t* seq_ids, uint64_t* lengths, uint64_t capacity, uint64_t* out_count) {
    Index* x = reinterpret_cast<Index*>(h);
    if (!x) return fail(FMGPU_ERR_INVALID, "index handle is null");
    if (out_count) *out_count = 0;
    if (!x->ext.dev) return fail(FMGPU_ERR_UNSUPPORTED, "no text map: call fmgpu_index_accelerate_extract first");
    if (!out_count) return fail(FMGPU_ERR_INVALID, "out_count is null");
    const uint64_t k = x->ext.nseq;
    *out_count = k;
    if (k > capacity) return fail(FMGPU_ERR_CAPACITY, "seqId buffer too small: " + std::to_string(k) + " sequences, capacity " + std::to_string(capacity));
    if (!seq_ids || !lengths) return fail(FMGPU_ERR_INVALID, "seq_ids / lengths is null");
    std::copy(x->ext.host_seq.begin(), x->ext.host_seq.end(), seq_ids);
    std::copy(x->ext.host_len.begin(), x->ext.host_len.end(), lengths);
    return 0;
}

int fmgpu_extract(fmgpu_index_t h, const fmgpu_text_range* ranges, uint64_t count, uint8_t* out, uint64_t capacity, uint64_t* out_count,
                  fmgpu_stats* stats, void* stream_) {
    Index* x = reinterpret_cast<Index*>(h);
    if (!x) return fail(FMGPU_ERR_INVALID, "index handle is null");
    if (int drc = on_handle_device(x)) return drc;
    if (stats) *stats = fmgpu_stats{};
    if (out_count) *out_count = 0;
    if (count == 0) return 0;
    if (!ranges || !out || !out_count) return fail(FMGPU_ERR_INVALID, "ranges / out / out_count is null");
    if (!x->ext.dev) return fail(FMGPU_ERR_UNSUPPORTED, "no sample table: call fmgpu_index_accelerate_extract first");
    hipStream_t stream = (hipStream_t)stream_;
    const ExtView ev = ext_view(x->ext);
    Staged sr;
    int rc;
    if ((rc = sr.in(ranges, count * sizeof(fmgpu_text_range), stream))) return rc;
    // pieces pass: ooff = exclusive scan of len, poff = of the piece counts (count + 1 entries each: the last holds the total); ONE read-back of both and the flag
    DBuf info, len, pcs, ooff, poff, tmp;
    if ((rc = info.alloc(count * sizeof(RangeInfo))) || (rc = len.alloc((count + 1) * 8)) || (rc = pcs.alloc((count + 1) * 8)) ||
        (rc = ooff.alloc((count + 1) * 8)) || (rc = poff.alloc((count + 2) * 8)))
        return rc;
    unsigned long long* dbad = (unsigned long long*)(poff.as<uint64_t>() + count + 1);
    FM_HIP(hipMemsetAsync(dbad, 0, 8, stream));
    FM_GRID(lgrid, count + 1);
    k_range_pieces<<<lgrid, dim3(256), 0, stream>>>((const fmgpu_text_range*)sr.dev, count, ev, info.as<RangeInfo>(), len.as<uint64_t>(), pcs.as<uint64_t>(), dbad);
    FM_LAUNCHED("k_range_pieces");
    size_t tb = 0;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, len.as<uint64_t>(), ooff.as<uint64_t>(), (size_t)(count + 1), stream));
    if ((rc = tmp.alloc(tb))) return rc;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, len.as<uint64_t>(), ooff.as<uint64_t>(), (size_t)(count + 1), stream));
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, pcs.as<uint64_t>(), poff.as<uint64_t>(), (size_t)(count + 1), stream));
    CallScratch* sc = nullptr;
    if ((rc = call_scratch(&sc))) return rc;
    unsigned long long* hback = sc->pinned;
    FM_HIP(hipMemcpyAsync(hback, ooff.as<uint64_t>() + count, 8, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipMemcpyAsync(hback + 1, poff.as<uint64_t>() + count, 16, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    const uint64_t total = hback[0], npieces = hback[1];
    *out_count = total;
    if (hback[2]) return fail(FMGPU_ERR_INVALID, "a range names an unknown seq_id or reaches beyond its sequence's length");
    if (total > capacity) return fail(FMGPU_ERR_CAPACITY, "symbol buffer too small: " + std::to_string(total) + " symbols, capacity " + std::to_string(capacity));
    if (total == 0) return 0;
    Staged so;
    if ((rc = so.out(out, total, stream))) return rc;
    unsigned long long* dsteps = nullptr;
    if ((rc = step_counters(stats != nullptr, stream, &dsteps))) return rc;
    EventTimer timer(stream, stats != nullptr);
    const idx_t* lf = x->bwt.lf_table;
    // launches of at most 2^28 pieces (2^20 blocks): far below the grid limit (a grid of 2^32 threads is cut short without an error)
    constexpr uint64_t kChunk = 1ull << 28;
    timer.start();
    for (uint64_t first = 0; first < npieces; first += kChunk) {
        const uint64_t cnt = std::min(kChunk, npieces - first);
        FM_GRID(grid, cnt);
        if (lf)                                                     // one 4-byte load per step; the symbol from C
            k_extract<OccA<0>, true><<<grid, 256, 0, stream>>>(OccA<0>{x->bwt.va}, lf, x->dC, (uint32_t)x->bwt.sigma, ev.key, ev.row, info.as<RangeInfo>(),
                                                               poff.as<uint64_t>(), ooff.as<uint64_t>(), count, first, cnt, (uint8_t*)so.dev, dsteps);
        else
            rc = dispatch_occ(x->bwt, [&](auto occ, auto) {
                k_extract<decltype(occ), false><<<grid, 256, 0, stream>>>(occ, nullptr, x->dC, (uint32_t)x->bwt.sigma, ev.key, ev.row, info.as<RangeInfo>(),
                                                                        poff.as<uint64_t>(), ooff.as<uint64_t>(), count, first, cnt, (uint8_t*)so.dev, dsteps);
                return 0;
            });
        if (rc) return rc;
        FM_LAUNCHED("k_extract");
    }
    timer.stop();
    if (stats) {
        unsigned long long hs[kCounterKinds] = {0, 0, 0, 0};
        if ((rc = read_step_counters(dsteps, stream, hs))) return rc;
        stats->lf_steps = hs[0]; stats->hits = total; stats->kernel_ms = timer.ms();
    }
    rc = so.finish();
    (void)hipStreamSynchronize(stream);                             // (the call returns after completion; its scratch is freed on return)
    return rc;
}

}  // namespace api

// ---- Format C: lifecycle (the builder of the sample table above orders the samples)
void drop_sample_chain(Index* x) {
    if (!x->chain) return;
    (void)hipFree(x->chain); (void)hipFree(x->chain_of); (void)hipFree(x->chain_ex);
    x->device_bytes -= x->chain_bytes;
    x->chain = nullptr; x->chain_of = nullptr; x->chain_ex = nullptr; x->chain_nex = 0; x->chain_rate = 0; x->chain_n = 0; x->chain_bytes = 0;
}
int build_sample_chain(Index* x, hipStream_t stream) {
    if constexpr (kWide) return 0;
    DevString& s = x->bwt;
    const uint64_t rate = x->has_sa ? x->vsa.div1 : 0;               // the sampled positions are the multiples of the rate: their common divisor
    if (x->chain || !x->has_sa || s.sigma != 5 || !s.pairs || s.search_family() != FAM_A || s.va.bstride != 64u || rate < 1 || rate > 16 || !opt_on(FMGPU_OPT_SAMPLE_CHAIN)) return 0;
    FM_HIP(hipStreamSynchronize(stream));
    // the samples in text order: the extract table's (key, row) arrays — the handle's own, or a temporary
    const bool temp = !x->ext.dev;
    const fmgpu_index_t h = reinterpret_cast<fmgpu_index_t>(x);
    if (temp) {
        const int erc = api::fmgpu_index_accelerate_extract(h, 1);
        if (erc == FMGPU_ERR_UNSUPPORTED || erc == FMGPU_ERR_INVALID) { set_error(""); return 0; }      // (no delimiter rows, samples outside the text map: no chain, and no message left behind)
        if (erc) return erc;                                           // (out of memory, a HIP error: the caller's error)
    }
    struct Temp { fmgpu_index_t h; bool on; ~Temp() { if (on) (void)api::fmgpu_index_accelerate_extract(h, 0); } } guard{h, temp};
    const uint64_t m = x->ext.nsamp;
    if (m < 2 || m >= 0xffffffffull) return 0;
    DBuf chain, of, ex, cnt; int rc;
    if ((rc = chain.alloc(m * 8)) || (rc = of.alloc(m * 4)) || (rc = ex.alloc(kChainMaxListed * 4)) || (rc = cnt.alloc(8))) return rc;
    FM_HIP(hipMemsetAsync(cnt.p, 0, 8, stream));
    FM_HIP(hipMemsetAsync(ex.p, 0xff, kChainMaxListed * 4, stream));
    FM_GRID(grid, m);
    k_chain_fill<<<grid, dim3(256), 0, stream>>>(OccA<5>{s.va}, x->vsa, x->ext.row, m, (uint32_t)rate, chain.as<uint2>(), of.as<uint32_t>(), ex.as<uint32_t>(), cnt.as<uint32_t>());
    FM_LAUNCHED("k_chain_fill");
    uint32_t nex = 0;
    FM_HIP(hipMemcpyAsync(&nex, cnt.p, 4, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (nex > kChainMaxListed) return 0;                              // many sequences, or samples that are not `rate` apart: exact search stays on the pair table
    std::vector<uint32_t> list(nex);
    if (nex) FM_HIP(hipMemcpy(list.data(), ex.p, nex * 4, hipMemcpyDeviceToHost));
    std::sort(list.begin(), list.end());
    if (nex) FM_HIP(hipMemcpy(ex.p, list.data(), nex * 4, hipMemcpyHostToDevice));
    x->chain_bytes = chain.bytes + of.bytes + ex.bytes;
    x->chain = (uint2*)chain.take(); x->chain_of = (uint32_t*)of.take(); x->chain_ex = (uint32_t*)ex.take();
    x->chain_nex = nex; x->chain_rate = (uint32_t)rate; x->chain_n = m;
    x->device_bytes += x->chain_bytes;
    return 0;
}

}  // namespace FMGPU_NS
