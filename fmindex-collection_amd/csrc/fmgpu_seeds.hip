// fmgpu_seeds.hip — fmgpu_search_smems (include/fmgpu.h): the super-maximal exact matches of every read of a batch and the match length of every batch symbol.
//  k_smem_walk    one lane per batch symbol = one end e: backward search of q[e], q[e - 1], ... from [0, n) until the read's start, a break or an empty extension;
//                 writes L[e], the last non-empty interval and whether e is its read's last symbol
//  k_smem_select  a flag per symbol: an SMEM end (e is the read's last symbol or L[e + 1] <= L[e]) that passes the filters
//  (hipcub exclusive scan of the flags; the total is the one read-back of the call)
//  k_smem_emit    one record per flagged symbol at its scan value: fmgpu_hit + fmgpu_seed_span, in batch order
// The intervals of ALL ends are kept between the walk and the emit (8 bytes per symbol with 32-bit rows, a coalesced store per lane) instead of walking the selected
// ends a second time: the selected ends are the ones with the longest matches of their read, so a second walk would repeat most of the random lines of the first.
#include "fmgpu_search_shared.h"

namespace FMGPU_NS {

// the read of batch symbol `at`: the last r with qoff[r] <= at (qoff[0] <= at < qoff[nq]; empty reads share their offset with the read behind them and are stepped over)
__device__ __forceinline__ uint64_t read_of_symbol(const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t at) {
    uint64_t lo = 0, hi = nq;
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (qoff[mid] <= at) lo = mid; else hi = mid; }
    return lo;
}

// one extension of both interval ends by c (1 <= c < sigma: a delimiter is a break and never gets here).  Format A: an interval inside one 64-row block loads
// that block's entry once, as k_exact_a does, and counts its table accesses the same way; every other layout goes through its lf2.
template <class Occ> struct CountsTable { static constexpr bool value = false; };
template <int SIGMA> struct CountsTable<OccA<SIGMA>> { static constexpr bool value = true; };
template <class Occ>
__device__ __forceinline__ void extend_both(const Occ& occ, idx_t a, idx_t b, uint32_t c, idx_t& ra, idx_t& rb, uint32_t& acc) { occ.lf2(a, b, c, ra, rb); }
template <int SIGMA>
__device__ __forceinline__ void extend_both(const OccA<SIGMA>& occ, idx_t a, idx_t b, uint32_t c, idx_t& ra, idx_t& rb, uint32_t& acc) {
    EntryA ea = load_entry_a(occ.v, a, c);
    EntryA eb = ea;
    ++acc;
    if ((a >> 6) != (b >> 6)) { eb = load_entry_a(occ.v, b, c); ++acc; }
    ra = ea.cnt + popc64(ea.bits & lowmask((uint32_t)a & 63u));
    rb = eb.cnt + popc64(eb.bits & lowmask((uint32_t)b & 63u));
}

constexpr uint32_t kSeedLastOfRead = 2u;             // what the walk leaves in the flag word of a read's last symbol (k_smem_select replaces it)

// `first` = qoff[0], `total` = qoff[nq] - qoff[0] < 2^32 (FM_GRID); every read is shorter than 2^32 symbols.  Lane i serves batch symbol first + i; at step l the
// lanes of a wave read the bytes first + i - l: one sliding 64-byte window of the batch.  At most e + 1 passes per lane.
template <class Occ>
__global__ __launch_bounds__(256) void k_smem_walk(Occ occ, const uint8_t* __restrict__ qbuf, const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t first, uint64_t total,
                                                   idx_t n, uint32_t* __restrict__ out_len, idx_t* __restrict__ iv_lb, idx_t* __restrict__ iv_rows, uint32_t* __restrict__ flag,
                                                   unsigned long long* __restrict__ steps_total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t steps = 0, acc = 0;
    if (i < total) {
        const uint64_t at = first + i;
        const uint64_t r = read_of_symbol(qoff, nq, at);
        const uint64_t start = qoff[r];
        const uint32_t e = (uint32_t)(at - start);
        const uint32_t sigma = occ.sigma();
        idx_t lb = 0, rows = n;
        uint32_t L = 0;
        QueryReader<> qr; qr.init(qbuf, start, e + 1u);
        for (uint32_t left = e + 1u; left > 0; --left) {
            const uint32_t c = qr.next();
            if (c - 1u >= sigma - 1u) break;                       // a break: the delimiter or a byte outside the alphabet (no step)
            idx_t ra, rb;
            extend_both(occ, lb, (idx_t)(lb + rows), c, ra, rb, acc);
            ++steps;
            if (rb == ra) break;                                   // the extension came out empty: the interval before it stands
            lb = ra; rows = rb - ra; ++L;
        }
        out_len[i] = L;
        iv_lb[i] = lb; iv_rows[i] = rows;
        flag[i] = at + 1 == qoff[r + 1] ? kSeedLastOfRead : 0u;
    }
    add_counters(steps_total, steps, CountsTable<Occ>::value ? 12u * acc : 0u, CountsTable<Occ>::value ? acc : 0u);
}

// flag[i] = 1 for the ends that are reported; flag[total] = 0, so that the exclusive scan over total + 1 words ends in the count
__global__ __launch_bounds__(256) void k_smem_select(const uint32_t* __restrict__ len, const idx_t* __restrict__ iv_rows, uint64_t total, uint32_t min_len, uint64_t max_rows,
                                                     uint32_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > total) return;
    uint32_t sel = 0;
    if (i < total) {
        const uint32_t L = len[i];
        const bool last = flag[i] == kSeedLastOfRead;              // (a read's last symbol is never followed by a symbol of the same read)
        const bool smem = L >= 1u && (last || len[i + 1] <= L);
        sel = smem && L >= min_len && (max_rows == 0 || (uint64_t)iv_rows[i] <= max_rows) ? 1u : 0u;
    }
    flag[i] = sel;
}

// at[i] = exclusive scan of the flags: symbol i is reported iff at[i + 1] != at[i], as record at[i]; seq = at[i] - at[the read's first symbol]
__global__ __launch_bounds__(256) void k_smem_emit(const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t first, uint64_t total, const uint32_t* __restrict__ len,
                                                   const idx_t* __restrict__ iv_lb, const idx_t* __restrict__ iv_rows, const uint32_t* __restrict__ at,
                                                   fmgpu_hit* __restrict__ out, fmgpu_seed_span* __restrict__ out_span) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint32_t k = at[i];
    if (at[i + 1] == k) return;
    const uint64_t sym = first + i;
    const uint64_t r = read_of_symbol(qoff, nq, sym);
    const uint64_t start = qoff[r];
    const uint32_t L = len[i];
    fmgpu_hit h;
    h.qidx = r; h.lb = iv_lb[i]; h.lb_rev = 0; h.len = iv_rows[i]; h.errors = 0; h.seq = k - at[start - first];
    out[k] = h;
    fmgpu_seed_span s;
    s.qbeg = (uint32_t)(sym - start) + 1u - L; s.qlen = L;
    out_span[k] = s;
}

namespace api {
#include "fmgpu_api_decl.h"

// first and last offset and the longest read of a batch (an unsorted offset array shows up as a read of 2^64 - something symbols)
static int batch_shape(const uint64_t* qoff, const uint64_t* dqoff, uint64_t nq, hipStream_t stream, uint64_t* first, uint64_t* last, uint64_t* longest) {
    if (!is_device_pointer(qoff)) {
        uint64_t mx = 0;
        for (uint64_t q = 0; q < nq; ++q) mx = std::max(mx, qoff[q + 1] - qoff[q]);
        *first = qoff[0]; *last = qoff[nq]; *longest = mx;
        return 0;
    }
    CallScratch* sc = nullptr;
    int rc = call_scratch(&sc); if (rc) return rc;
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((nq + 255) / 256, kLenBlocks));
    k_len_range<<<dim3(blocks), dim3(256), 0, stream>>>(dqoff, nq, sc->len2);
    FM_LAUNCHED("k_len_range");
    unsigned long long* h = sc->pinned;
    FM_HIP(hipMemcpyAsync(h, sc->len2, ((size_t)2 * blocks + 1) * 8, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipMemcpyAsync(first, dqoff, 8, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    unsigned long long mx = 0;
    for (unsigned b = 0; b < blocks; ++b) mx = std::max(mx, h[2 * b]);
    *longest = mx; *last = h[2 * blocks];
    return 0;
}

static int search_smems(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, uint32_t min_len, uint64_t max_rows,
                        fmgpu_hit* out, fmgpu_seed_span* out_span, uint64_t capacity, uint64_t* out_count, uint32_t* out_match_len, fmgpu_stats* stats, void* stream_) {
    Index* x = reinterpret_cast<Index*>(h);
    if (!x) return fail(FMGPU_ERR_INVALID, "index handle is null");
    if (int drc = on_handle_device(x)) return drc;
    if (stats) *stats = fmgpu_stats{};
    if (out_count) *out_count = 0;
    if (nq == 0) return 0;
    if (!qbuf || !qoff || !out_count) return fail(FMGPU_ERR_INVALID, "qbuf / qoff / out_count is null");
    if (capacity && (!out || !out_span)) return fail(FMGPU_ERR_INVALID, "out / out_span is null while capacity > 0");
    hipStream_t stream = (hipStream_t)stream_;
    Staged soff, sbuf, slen;
    int rc;
    if ((rc = soff.in(qoff, (nq + 1) * 8, stream))) return rc;
    const uint64_t* dqoff = (const uint64_t*)soff.dev;
    uint64_t first = 0, last = 0, longest = 0;
    if ((rc = batch_shape(qoff, dqoff, nq, stream, &first, &last, &longest))) return rc;
    if (last < first) return fail(FMGPU_ERR_INVALID, "qoff is not non-decreasing");
    if (longest > 0xffffffffull) return fail(FMGPU_ERR_UNSUPPORTED, "a read of 2^32 symbols or more (or qoff is not non-decreasing)");
    const uint64_t total = last - first;
    if (total == 0) return 0;
    FM_GRID(grid, total + 1);                                       // (2^32 symbols and more: FMGPU_ERR_UNSUPPORTED, never a launch cut short)
    if ((rc = sbuf.in(qbuf, last, stream))) return rc;
    // scratch per symbol: L (4 bytes, unless out_match_len is device memory and serves), the interval (2 rows: 8 / 16 bytes), the flag that becomes the scan (4 bytes)
    DBuf own_len, ivl, ivr, flag, tmp;
    uint32_t* dlen = nullptr;
    if (out_match_len) { if ((rc = slen.out(out_match_len, total * 4, stream))) return rc; dlen = (uint32_t*)slen.dev; }
    else { if ((rc = own_len.alloc(total * 4))) return rc; dlen = own_len.as<uint32_t>(); }
    if ((rc = ivl.alloc(total * sizeof(idx_t))) || (rc = ivr.alloc(total * sizeof(idx_t))) || (rc = flag.alloc((total + 1) * 4))) return rc;
    size_t tb = 0;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag.as<uint32_t>(), flag.as<uint32_t>(), (size_t)(total + 1), stream));
    if ((rc = tmp.alloc(tb))) return rc;
    unsigned long long* dsteps = nullptr;
    if ((rc = step_counters(stats != nullptr, stream, &dsteps))) return rc;
    EventTimer timer(stream, stats != nullptr);
    const idx_t n = (idx_t)x->bwt.n;
    timer.start();
    rc = dispatch_occ(x->bwt, [&](auto occ, auto) {
        k_smem_walk<decltype(occ)><<<grid, dim3(256), 0, stream>>>(occ, (const uint8_t*)sbuf.dev, dqoff, nq, first, total, n, dlen, ivl.as<idx_t>(), ivr.as<idx_t>(),
                                                                   flag.as<uint32_t>(), dsteps);
        return 0;
    });
    timer.stop();
    if (rc) return rc;
    FM_LAUNCHED("k_smem_walk");
    k_smem_select<<<grid, dim3(256), 0, stream>>>(dlen, ivr.as<idx_t>(), total, min_len, max_rows, flag.as<uint32_t>());
    FM_LAUNCHED("k_smem_select");
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, flag.as<uint32_t>(), flag.as<uint32_t>(), (size_t)(total + 1), stream));
    CallScratch* sc = nullptr;
    if ((rc = call_scratch(&sc))) return rc;
    unsigned long long* hback = sc->pinned;
    hback[0] = 0;
    FM_HIP(hipMemcpyAsync(hback, flag.as<uint32_t>() + total, 4, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    const uint64_t count = (uint32_t)hback[0];
    *out_count = count;
    if (stats) {
        unsigned long long hs[kCounterKinds] = {0, 0, 0, 0};
        if ((rc = read_step_counters(dsteps, stream, hs))) return rc;
        stats->lf_steps = hs[0]; stats->hits = count; stats->kernel_ms = timer.ms();
        stats->table_bytes = hs[1]; stats->table_accesses = hs[2];
    }
    if ((rc = slen.finish())) return rc;                            // (the match lengths stand whatever the capacity)
    if (count > capacity) return fail(FMGPU_ERR_CAPACITY, "seed buffer too small: " + std::to_string(count) + " seeds, capacity " + std::to_string(capacity));
    if (count) {
        Staged so, sp;
        if ((rc = so.out(out, count * sizeof(fmgpu_hit), stream)) || (rc = sp.out(out_span, count * sizeof(fmgpu_seed_span), stream))) return rc;
        k_smem_emit<<<grid, dim3(256), 0, stream>>>(dqoff, nq, first, total, dlen, ivl.as<idx_t>(), ivr.as<idx_t>(), flag.as<uint32_t>(), (fmgpu_hit*)so.dev, (fmgpu_seed_span*)sp.dev);
        FM_LAUNCHED("k_smem_emit");
        if ((rc = so.finish()) || (rc = sp.finish())) return rc;
    }
    FM_HIP(hipStreamSynchronize(stream));
    return 0;                                                       // (the scratch is freed on return)
}

int fmgpu_search_smems(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, uint32_t min_len, uint64_t max_rows,
                       fmgpu_hit* out, fmgpu_seed_span* out_span, uint64_t capacity, uint64_t* out_count, uint32_t* out_match_len, fmgpu_stats* stats, void* stream) {
    return search_smems(h, qbuf, qoff, nq, min_len, max_rows, out, out_span, capacity, out_count, out_match_len, stats, stream);
}

// the batch is unpacked into a per-call byte scratch (freed on return), then the byte path runs: the results are those of the byte call on fmgpu_queries_unpack4(packed)
int fmgpu_search_smems_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq, uint32_t min_len, uint64_t max_rows,
                          fmgpu_hit* out, fmgpu_seed_span* out_span, uint64_t capacity, uint64_t* out_count, uint32_t* out_match_len, fmgpu_stats* stats, void* stream) {
    Index* x = reinterpret_cast<Index*>(h);
    if (!x) return fail(FMGPU_ERR_INVALID, "index handle is null");
    if (x->bwt.sigma > 15) return fail(FMGPU_ERR_UNSUPPORTED, "4-bit packed queries need sigma <= 15, this index has sigma = " + std::to_string(x->bwt.sigma));
    if (!nq || !packed || !qoff || !out_count || (capacity && (!out || !out_span)))
        return search_smems(h, packed, qoff, nq, min_len, max_rows, out, out_span, capacity, out_count, out_match_len, stats, stream);     // (the byte call's own answer)
    if (int drc = on_handle_device(x)) return drc;
    UnpackedQueries u;
    if (int rc = unpack_queries(packed, qoff, nq, (hipStream_t)stream, &u)) return rc;
    return search_smems(h, u.qbuf(), u.qoff(), nq, min_len, max_rows, out, out_span, capacity, out_count, out_match_len, stats, stream);
}

}  // namespace api
}  // namespace FMGPU_NS
