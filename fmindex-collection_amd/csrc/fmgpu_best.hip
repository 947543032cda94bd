// fmgpu_best.hip — best-stratum search (include/fmgpu.h: fmgpu_search_best*): a ladder of schemes walked over one batch, every stratum over the reads that no earlier
// stratum found.  Marking the found reads, selecting and compacting the others and renaming qidx happen here, on the device; the strata themselves are the routed
// fmgpu_search_scheme / fmgpu_search_ng21 calls on device pointers.  The `_pairs` forms treat reads 2j and 2j + 1 as the two strands of one read: once either is
// found, neither goes on (k_best_pairs).  Nothing here depends on the row width.
#include "fmgpu_common.h"

#include <hipcub/hipcub.hpp>

namespace fmgpu {

// ---- the records a stratum has just written: sub = the read's number in the stratum's sub-batch.  A record with rows marks its read found (many records of one read
// store the same byte: plain stores, no atomics) and names the stratum in out_stratum; every record gets the read's number in the caller's batch.
__global__ __launch_bounds__(256) void k_best_mark(fmgpu_hit* __restrict__ rec, uint64_t count, uint8_t* __restrict__ found, uint64_t nsub, const uint32_t* __restrict__ qmap,
                                                   uint8_t* __restrict__ out_stratum, uint32_t stratum) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t sub = rec[i].qidx;
        if (sub >= nsub) continue;                                  // (no search kernel writes one: nothing is stored through a number outside the sub-batch)
        const uint64_t q = qmap ? qmap[sub] : sub;
        if (rec[i].len > 0) {
            found[sub] = 1;
            if (out_stratum) out_stratum[q] = (uint8_t)stratum;
        }
        rec[i].qidx = q;
    }
}

// ---- the pair ladder: reads 2j and 2j + 1 of the sub-batch are the two strands of one read (selection keeps or drops both, so they stay adjacent).  A pair is found
// when either of its reads is: both flags are set, and both entries of out_stratum name the stratum.  One thread per pair, after k_best_mark.
__global__ __launch_bounds__(256) void k_best_pairs(uint8_t* __restrict__ found, uint64_t npairs, const uint32_t* __restrict__ qmap, uint8_t* __restrict__ out_stratum,
                                                    uint32_t stratum) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < npairs; j += (uint64_t)gridDim.x * blockDim.x) {
        if (!(found[2 * j] | found[2 * j + 1])) continue;
        found[2 * j] = 1; found[2 * j + 1] = 1;
        if (out_stratum) {
            out_stratum[qmap ? qmap[2 * j] : 2 * j] = (uint8_t)stratum;
            out_stratum[qmap ? qmap[2 * j + 1] : 2 * j + 1] = (uint8_t)stratum;
        }
    }
}

struct NotFound { __host__ __device__ __forceinline__ uint8_t operator()(const uint8_t& f) const { return f ? 0 : 1; } };
using UnfoundFlags = hipcub::TransformInputIterator<uint8_t, NotFound, const uint8_t*>;

// ---- lengths of the selected reads (original read numbers in qmap, *nsel of them) in `slots` slots, 0 behind the last one: their exclusive sum is the next sub-batch's qoff
__global__ __launch_bounds__(256) void k_best_lengths(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ qmap, const uint32_t* __restrict__ nsel, uint64_t slots,
                                                      uint64_t* __restrict__ len) {
    const uint64_t n = *nsel;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < slots; j += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t v = 0;
        if (j < n) { const uint64_t q = qmap[j]; v = qoff[q + 1] - qoff[q]; }
        len[j] = v;
    }
}
// the one read-back of a stratum: reads left, symbols left
__global__ void k_best_tally(const uint32_t* __restrict__ nsel, const uint64_t* __restrict__ sub_qoff, uint64_t* __restrict__ tally) {
    tally[0] = *nsel;
    tally[1] = sub_qoff[*nsel];
}

// ---- the symbols of the selected reads, from the caller's batch into the compact scratch.  A thread makes 16 output bytes: it finds the read of its first symbol by
// bisection of the new qoff and walks on from there over read boundaries (empty reads are stepped over); a full chunk leaves as one aligned 16-byte store.
__global__ __launch_bounds__(256) void k_best_gather(const uint8_t* __restrict__ qbuf, const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ qmap,
                                                     const uint64_t* __restrict__ sub_qoff, uint64_t nsel, uint64_t total, uint8_t* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t s0 = 16 * t;
    if (s0 >= total) return;
    uint64_t lo = 0, hi = nsel;                                     // the last read r with sub_qoff[r] <= s0 (sub_qoff[0] = 0; s0 < total = sub_qoff[nsel])
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (sub_qoff[mid] <= s0) lo = mid; else hi = mid; }
    uint64_t r = lo, begin = sub_qoff[r], end = sub_qoff[r + 1];
    const uint8_t* src = qbuf + qoff[qmap[r]];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint64_t s = s0 + k;
        if (s >= total) break;
        if (s >= end) {
            while (s >= end) { ++r; begin = end; end = sub_qoff[r + 1]; }
            src = qbuf + qoff[qmap[r]];
        }
        w[k >> 2] |= (uint32_t)src[s - begin] << (8u * (k & 3u));
    }
    if (s0 + 16 <= total) *reinterpret_cast<uint4*>(out + s0) = make_uint4(w[0], w[1], w[2], w[3]);
    else for (uint32_t k = 0; k < 16u && s0 + k < total; ++k) out[s0 + k] = (uint8_t)(w[k >> 2] >> (8u * (k & 3u)));
}

// ---- one stratum = the single-scheme call of the ladder's kind
static int check_one(fmgpu_index_t h, const fmgpu_scheme* s, uint64_t max_hits) { return check_scheme(h, s, max_hits); }
static int check_one(fmgpu_index_t h, const fmgpu_expanded_scheme* s, uint64_t) { return check_expanded_scheme(h, s); }
static int search_one(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* s, uint64_t max_hits, fmgpu_hit* out, uint64_t capacity,
                      uint64_t* out_count, fmgpu_stats* stats, void* stream) {
    return ::fmgpu_search_scheme(h, qbuf, qoff, nq, s, max_hits, out, capacity, out_count, stats, stream);
}
static int search_one(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_expanded_scheme* s, uint64_t max_hits, fmgpu_hit* out,
                      uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream) {
    return ::fmgpu_search_ng21(h, qbuf, qoff, nq, s, max_hits, out, capacity, out_count, stats, stream);
}

static int fill_unfound(uint8_t* out_stratum, uint64_t nq, hipStream_t stream) {
    if (!out_stratum || !nq) return 0;
    if (!is_device_pointer(out_stratum)) { std::memset(out_stratum, 255, nq); return 0; }
    FM_HIP(hipMemsetAsync(out_stratum, 255, nq, stream));
    FM_HIP(hipStreamSynchronize(stream));
    return 0;
}

template <class Scheme>
static int run_best(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const Scheme* schemes, int32_t n_schemes, uint64_t max_hits, fmgpu_hit* out,
                    uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, hipStream_t stream, bool packed, bool pairs = false) {
    if (n_schemes < 0 || n_schemes > 254) return fail(FMGPU_ERR_INVALID, "n_schemes must be in [0, 254] (out_stratum keeps 255 for an unfound read)");
    if (pairs && (nq & 1)) return fail(FMGPU_ERR_INVALID, "a pair ladder takes an even number of reads (reads 2j and 2j + 1 are a pair)");
    if (out_count) *out_count = 0;
    if (stats) for (int32_t i = 0; i < n_schemes; ++i) stats[i] = fmgpu_stats{};
    if (n_schemes == 0 || nq == 0) return fill_unfound(out_stratum, nq, stream);
    if (packed) {
        int32_t sigma = 0;
        if (int rc = ::fmgpu_index_info(h, nullptr, &sigma, nullptr, nullptr, nullptr)) return rc;
        if (sigma > 15) return fail(FMGPU_ERR_UNSUPPORTED, "4-bit packed queries need sigma <= 15, this index has sigma = " + std::to_string(sigma));
    }
    if (!schemes) return fail(FMGPU_ERR_INVALID, "schemes is null");
    for (int32_t i = 0; i < n_schemes; ++i) if (int rc = check_one(h, &schemes[i], max_hits)) return rc;
    if (!qbuf || !qoff || (!out && capacity) || !out_count) return fail(FMGPU_ERR_INVALID, "qbuf / qoff / out / out_count is null");
    if (nq > 0x7fffffffull) return fail(FMGPU_ERR_UNSUPPORTED, "a best-stratum batch holds at most 2^31 - 1 reads");

    // the caller's batch in HBM, as bytes
    int rc;
    UnpackedQueries unpacked;
    Staged soff, sbuf, sout, sstratum;
    const uint8_t* dq = nullptr;
    const uint64_t* doff = nullptr;
    if (packed) {
        if ((rc = unpack_queries(qbuf, qoff, nq, stream, &unpacked))) return rc;
        dq = unpacked.qbuf(); doff = unpacked.qoff();
    } else {
        if ((rc = soff.in(qoff, (nq + 1) * 8, stream))) return rc;
        uint64_t last = 0;
        if (is_device_pointer(qoff)) { FM_HIP(hipMemcpyAsync(&last, qoff + nq, 8, hipMemcpyDeviceToHost, stream)); FM_HIP(hipStreamSynchronize(stream)); }
        else last = qoff[nq];
        if ((rc = sbuf.in(qbuf, last, stream))) return rc;
        dq = (const uint8_t*)sbuf.dev; doff = (const uint64_t*)soff.dev;
        if (!dq) dq = qbuf;                                         // (a batch without a symbol: the pointer is never read through)
    }
    if ((rc = sout.out(out, capacity * sizeof(fmgpu_hit), stream))) return rc;
    if ((rc = sstratum.out(out_stratum, out_stratum ? nq : 0, stream))) return rc;
    fmgpu_hit* const dout = (fmgpu_hit*)sout.dev;
    uint8_t* const dstratum = out_stratum ? (uint8_t*)sstratum.dev : nullptr;
    if (dstratum) FM_HIP(hipMemsetAsync(dstratum, 255, nq, stream));

    // scratch of the ladder, one allocation: found flags of the current sub-batch; with a second stratum two read-number maps (the current one and the one being selected),
    // the lengths and offsets of the next sub-batch, hipcub's workspace and the tally
    DBuf work, symbols;
    size_t tmp_bytes = 0;
    const auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_maps = up(nq), o_lens = o_maps + up(2 * nq * 4), o_off = o_lens + up((nq + 1) * 8), o_small = o_off + up((nq + 1) * 8), o_tmp = o_small + 256;
    if (n_schemes > 1) {
        size_t b1 = 0, b2 = 0, b3 = 0;
        FM_HIP(hipcub::DeviceSelect::Flagged(nullptr, b1, hipcub::CountingInputIterator<uint32_t>(0u), UnfoundFlags((const uint8_t*)nullptr, NotFound{}), (uint32_t*)nullptr,
                                             (uint32_t*)nullptr, (int)nq, stream));
        FM_HIP(hipcub::DeviceSelect::Flagged(nullptr, b2, (const uint32_t*)nullptr, UnfoundFlags((const uint8_t*)nullptr, NotFound{}), (uint32_t*)nullptr, (uint32_t*)nullptr,
                                             (int)nq, stream));
        FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b3, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(nq + 1), stream));
        tmp_bytes = std::max<size_t>(std::max(b1, std::max(b2, b3)), 8);
    }
    if ((rc = work.alloc(n_schemes > 1 ? o_tmp + tmp_bytes : nq))) return rc;
    uint8_t* const base = work.as<uint8_t>();
    uint8_t* const found = base;
    uint32_t* const maps = reinterpret_cast<uint32_t*>(base + o_maps);
    uint64_t* const lens = reinterpret_cast<uint64_t*>(base + o_lens);
    uint64_t* const sub_off = reinterpret_cast<uint64_t*>(base + o_off);
    uint64_t* const d_tally = reinterpret_cast<uint64_t*>(base + o_small);          // [0] reads left, [1] symbols left; behind them the selection's own count
    uint32_t* const d_nsel = reinterpret_cast<uint32_t*>(base + o_small + 16);
    void* const tmp = base + o_tmp;

    uint64_t produced = 0, cur_n = nq;
    const uint8_t* cur_q = dq;
    const uint64_t* cur_off = doff;
    const uint32_t* cur_map = nullptr;                               // stratum 0: the sub-batch is the batch
    int next_slot = 0;
    for (int32_t i = 0; i < n_schemes; ++i) {
        FM_HIP(hipMemsetAsync(found, 0, cur_n, stream));
        uint64_t cnt = 0;
        fmgpu_stats st{};
        rc = search_one(h, cur_q, cur_off, cur_n, &schemes[i], max_hits, dout ? dout + produced : nullptr, capacity - produced, &cnt, stats ? &st : nullptr, stream);
        if (stats) stats[i] = st;
        if (rc == FMGPU_ERR_CAPACITY) {
            *out_count = produced + cnt;
            return fail(FMGPU_ERR_CAPACITY, "result buffer holds " + std::to_string(capacity) + " records, " + std::to_string(produced + cnt) + " produced up to stratum " + std::to_string(i));
        }
        if (rc) return rc;
        if (cnt) {
            dim3 grid; if ((rc = grid_of(cnt, &grid, 1u << 16))) return rc;
            k_best_mark<<<grid, dim3(256), 0, stream>>>(dout + produced, cnt, found, cur_n, cur_map, dstratum, (uint32_t)i);
            FM_LAUNCHED("k_best_mark");
            if (pairs) {
                dim3 pgrid; if ((rc = grid_of(cur_n / 2, &pgrid, 1u << 16))) return rc;
                k_best_pairs<<<pgrid, dim3(256), 0, stream>>>(found, cur_n / 2, cur_map, dstratum, (uint32_t)i);
                FM_LAUNCHED("k_best_pairs");
            }
        }
        produced += cnt;
        if (i + 1 == n_schemes) break;
        // the reads this stratum left unfound, in batch order, and the offsets of their sub-batch
        uint32_t* const next_map = maps + (size_t)next_slot * nq;
        size_t tb = tmp_bytes;
        const UnfoundFlags flags(found, NotFound{});
        if (cur_map) FM_HIP(hipcub::DeviceSelect::Flagged(tmp, tb, cur_map, flags, next_map, d_nsel, (int)cur_n, stream));
        else FM_HIP(hipcub::DeviceSelect::Flagged(tmp, tb, hipcub::CountingInputIterator<uint32_t>(0u), flags, next_map, d_nsel, (int)cur_n, stream));
        dim3 lgrid; if ((rc = grid_of(cur_n + 1, &lgrid, 1u << 16))) return rc;
        k_best_lengths<<<lgrid, dim3(256), 0, stream>>>(doff, next_map, d_nsel, cur_n + 1, lens);
        FM_LAUNCHED("k_best_lengths");
        tb = tmp_bytes;
        FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, (const uint64_t*)lens, sub_off, (int)(cur_n + 1), stream));
        k_best_tally<<<dim3(1), dim3(1), 0, stream>>>(d_nsel, sub_off, d_tally);
        FM_LAUNCHED("k_best_tally");
        uint64_t tally[2] = {0, 0};
        FM_HIP(hipMemcpyAsync(tally, d_tally, 16, hipMemcpyDeviceToHost, stream));
        FM_HIP(hipStreamSynchronize(stream));
        if (tally[0] == 0) break;                                   // every read has been found
        if (tally[0] > cur_n) return fail(FMGPU_ERR_HIP, "best-stratum selection returned more reads than it was given");
        if (pairs && (tally[0] & 1)) return fail(FMGPU_ERR_HIP, "pair ladder: the selection split a pair");
        // one scratch for every remainder: the later ones are subsets of the first, and stream order puts a gather behind the search that read the scratch before
        if (!symbols.p && (rc = symbols.alloc(tally[1] + 16))) return rc;
        if (tally[1] + 16 > symbols.bytes) return fail(FMGPU_ERR_HIP, "best-stratum remainder grew");
        if (tally[1]) {
            FM_GRID(ggrid, (tally[1] + 15) / 16);
            k_best_gather<<<ggrid, dim3(256), 0, stream>>>(dq, doff, next_map, sub_off, tally[0], tally[1], symbols.as<uint8_t>());
            FM_LAUNCHED("k_best_gather");
        }
        cur_q = symbols.as<uint8_t>(); cur_off = sub_off; cur_n = tally[0]; cur_map = next_map;
        next_slot ^= 1;
    }
    *out_count = produced;
    if (sout.writeback) sout.bytes = produced * sizeof(fmgpu_hit);
    if ((rc = sout.finish())) return rc;
    if ((rc = sstratum.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));                           // the scratch is freed on return
    return 0;
}

}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_search_best(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                      fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream) {
    return run_best(h, qbuf, qoff, nq, schemes, n_schemes, max_hits_per_query, out, capacity, out_count, out_stratum, stats, (hipStream_t)stream, false);
}
int fmgpu_search_best_ng21(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_expanded_scheme* schemes, int32_t n_schemes,
                           uint64_t max_hits_per_query, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream) {
    return run_best(h, qbuf, qoff, nq, schemes, n_schemes, max_hits_per_query, out, capacity, out_count, out_stratum, stats, (hipStream_t)stream, false);
}
int fmgpu_search_best_pairs(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                            fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream) {
    return run_best(h, qbuf, qoff, nq, schemes, n_schemes, max_hits_per_query, out, capacity, out_count, out_stratum, stats, (hipStream_t)stream, false, true);
}
int fmgpu_search_best_ng21_pairs(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_expanded_scheme* schemes, int32_t n_schemes,
                                 uint64_t max_hits_per_query, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream) {
    return run_best(h, qbuf, qoff, nq, schemes, n_schemes, max_hits_per_query, out, capacity, out_count, out_stratum, stats, (hipStream_t)stream, false, true);
}
int fmgpu_search_best_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                         fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream) {
    return run_best(h, packed, qoff, nq, schemes, n_schemes, max_hits_per_query, out, capacity, out_count, out_stratum, stats, (hipStream_t)stream, true);
}
int fmgpu_search_best_ng21_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq, const fmgpu_expanded_scheme* schemes, int32_t n_schemes,
                              uint64_t max_hits_per_query, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream) {
    return run_best(h, packed, qoff, nq, schemes, n_schemes, max_hits_per_query, out, capacity, out_count, out_stratum, stats, (hipStream_t)stream, true);
}

}  // extern "C"
