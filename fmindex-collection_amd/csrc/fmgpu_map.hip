// fmgpu_map.hip — fmgpu_map / fmgpu_map_q4 / fmgpu_map_strands (include/fmgpu.h): search, order and locate chained on the device.  The stages are the library's own calls on device
// pointers — fmgpu_search_best* or fmgpu_search_exact*, fmgpu_hits_sort or fmgpu_hits_from_intervals, fmgpu_locate_hits — and the capacity-retry loop around each of them
// lives here once: the hit and position lists are produced in scratch that grows until the stage fits, so the counts a caller gets are exact.  map_device is the chain on
// device buffers; the one-shot calls below stage a batch around it, the feeds (fmgpu_feed.hip) run it per chunk on their slots' buffers.  Nothing here depends on the
// row width.
#include "fmgpu_common.h"

#include <algorithm>

namespace fmgpu {

static_assert(sizeof(fmgpu_map_query) == 40, "fmgpu_map_query is 40 bytes");
static_assert(sizeof(fmgpu_hit) == 40 && sizeof(fmgpu_position) == 32, "record sizes of the ABI");

// a chunk's records renumbered for the caller's batch
__global__ __launch_bounds__(256) void k_map_rebase(fmgpu_hit* __restrict__ hits, uint64_t hit_count, fmgpu_position* __restrict__ positions, uint64_t pos_count,
                                                    uint64_t first, uint32_t hit_base) {
    const uint64_t most = hit_count > pos_count ? hit_count : pos_count;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < most; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i < hit_count) hits[i].qidx += first;
        if (i < pos_count) { positions[i].qidx += first; positions[i].hit += hit_base; }
    }
}

int map_rebase(fmgpu_hit* hits, uint64_t hit_count, fmgpu_position* positions, uint64_t pos_count, uint64_t first, uint64_t hit_base, hipStream_t stream) {
    if ((!hit_count && !pos_count) || (!first && !hit_base)) return 0;
    dim3 grid; if (int rc = grid_of(std::max(hit_count, pos_count), &grid, 1u << 16)) return rc;
    k_map_rebase<<<grid, dim3(256), 0, stream>>>(hits, hit_count, positions, pos_count, first, (uint32_t)hit_base);
    FM_LAUNCHED("k_map_rebase");
    return 0;
}

int check_map_query(const fmgpu_map_query* what) {
    if (!what) return fail(FMGPU_ERR_INVALID, "what is null");
    if (what->kind < FMGPU_MAP_EXACT || what->kind > FMGPU_MAP_NG21) return fail(FMGPU_ERR_INVALID, "fmgpu_map_query: kind must be FMGPU_MAP_EXACT, FMGPU_MAP_SCHEME or FMGPU_MAP_NG21");
    if (what->kind == FMGPU_MAP_EXACT ? what->n_schemes != 0 : (what->n_schemes < 1 || what->n_schemes > 254))
        return fail(FMGPU_ERR_INVALID, "fmgpu_map_query: n_schemes must be 0 for FMGPU_MAP_EXACT and in [1, 254] for a ladder");
    if (what->reserved != 0) return fail(FMGPU_ERR_INVALID, "fmgpu_map_query: reserved must be 0");
    return 0;
}

int check_map_schemes(fmgpu_index_t h, const fmgpu_map_query* what, bool packed) {
    int32_t sigma = 0;
    if (int rc = ::fmgpu_index_info(h, nullptr, &sigma, nullptr, nullptr, nullptr)) return rc;
    if (packed && sigma > 15) return fail(FMGPU_ERR_UNSUPPORTED, "4-bit packed queries need sigma <= 15, this index has sigma = " + std::to_string(sigma));
    if (what->kind != FMGPU_MAP_EXACT) {
        if (!what->schemes) return fail(FMGPU_ERR_INVALID, "schemes is null");
        for (int32_t i = 0; i < what->n_schemes; ++i) {
            const int rc = what->kind == FMGPU_MAP_SCHEME ? check_scheme(h, static_cast<const fmgpu_scheme*>(what->schemes) + i, what->max_hits_per_query)
                                                          : check_expanded_scheme(h, static_cast<const fmgpu_expanded_scheme*>(what->schemes) + i);
            if (rc) return rc;
        }
    }
    if (what->locate) if (int rc = ::fmgpu_locate_hits(h, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr)) return rc;      // (no record: the handle's own checks, the annotated array)
    return 0;
}

int map_device(fmgpu_index_t h, const uint8_t* dq, const uint64_t* doff, uint64_t nq, const fmgpu_map_query* what, bool packed, MapBuffer* hits, MapBuffer* positions,
               MapBuffer* intervals, uint8_t* dstratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats, hipStream_t stream, uint64_t* hit_count, uint64_t* pos_count,
               bool pairs) {
    *hit_count = *pos_count = 0;
    if (pairs && packed) return fail(FMGPU_ERR_UNSUPPORTED, "the pair ladder takes byte batches");
    const int32_t nstats = std::max(1, what->n_schemes);
    if (search_stats) for (int32_t i = 0; i < nstats; ++i) search_stats[i] = fmgpu_stats{};
    if (locate_stats) *locate_stats = fmgpu_stats{};
    const uint64_t first = what->first_records ? what->first_records : std::max<uint64_t>(1024, 4 * nq);
    const uint64_t max_hits = what->max_hits_per_query;
    int rc;
    if ((rc = hits->need((size_t)first * sizeof(fmgpu_hit)))) return rc;
    uint64_t cap = hits->bytes / sizeof(fmgpu_hit), cnt = 0;

    // ---- H: the search, then the ordering
    if (what->kind == FMGPU_MAP_EXACT) {
        if ((rc = intervals->need((size_t)nq * 16))) return rc;
        uint64_t* const dlb = reinterpret_cast<uint64_t*>(intervals->p);
        uint64_t* const dlen = dlb + nq;
        rc = packed ? ::fmgpu_search_exact_q4(h, dq, doff, nq, dlb, dlen, search_stats, stream) : ::fmgpu_search_exact(h, dq, doff, nq, dlb, dlen, search_stats, stream);
        if (rc) return rc;
        for (int attempt = 0;; ++attempt) {
            rc = hits_from_intervals_on(h, dlb, dlen, doff, nq, 0, max_hits, reinterpret_cast<fmgpu_hit*>(hits->p), cap, &cnt, dstratum, stream);
            if (rc != FMGPU_ERR_CAPACITY || attempt > 0) break;     // (the count is exact: the second run fits)
            if ((rc = hits->need((size_t)std::max(cnt, 2 * cap) * sizeof(fmgpu_hit)))) return rc;
            cap = hits->bytes / sizeof(fmgpu_hit);
        }
        if (rc) return rc;
    } else {
        // a stratum that overflows reports the records up to and including itself: growing to max(count, 2 x size) ends within n_schemes rounds
        for (int32_t attempt = 0;; ++attempt) {
            fmgpu_hit* const dh = reinterpret_cast<fmgpu_hit*>(hits->p);
            if (what->kind == FMGPU_MAP_SCHEME) {
                const fmgpu_scheme* s = static_cast<const fmgpu_scheme*>(what->schemes);
                rc = packed ? ::fmgpu_search_best_q4(h, dq, doff, nq, s, what->n_schemes, max_hits, dh, cap, &cnt, dstratum, search_stats, stream)
                     : pairs ? ::fmgpu_search_best_pairs(h, dq, doff, nq, s, what->n_schemes, max_hits, dh, cap, &cnt, dstratum, search_stats, stream)
                            : ::fmgpu_search_best(h, dq, doff, nq, s, what->n_schemes, max_hits, dh, cap, &cnt, dstratum, search_stats, stream);
            } else {
                const fmgpu_expanded_scheme* s = static_cast<const fmgpu_expanded_scheme*>(what->schemes);
                rc = packed ? ::fmgpu_search_best_ng21_q4(h, dq, doff, nq, s, what->n_schemes, max_hits, dh, cap, &cnt, dstratum, search_stats, stream)
                     : pairs ? ::fmgpu_search_best_ng21_pairs(h, dq, doff, nq, s, what->n_schemes, max_hits, dh, cap, &cnt, dstratum, search_stats, stream)
                            : ::fmgpu_search_best_ng21(h, dq, doff, nq, s, what->n_schemes, max_hits, dh, cap, &cnt, dstratum, search_stats, stream);
            }
            if (rc != FMGPU_ERR_CAPACITY || attempt > what->n_schemes) break;
            if ((rc = hits->need((size_t)std::max(cnt, 2 * cap) * sizeof(fmgpu_hit)))) return rc;
            cap = hits->bytes / sizeof(fmgpu_hit);
        }
        if (rc) return rc;
        if ((rc = ::fmgpu_hits_sort(reinterpret_cast<fmgpu_hit*>(hits->p), cnt, stream))) return rc;
    }
    *hit_count = cnt;
    if (!what->locate || cnt == 0) return 0;

    // ---- P
    if ((rc = positions->need((size_t)first * sizeof(fmgpu_position)))) return rc;
    uint64_t pcap = positions->bytes / sizeof(fmgpu_position), pcnt = 0;
    for (int attempt = 0;; ++attempt) {
        rc = ::fmgpu_locate_hits(h, reinterpret_cast<const fmgpu_hit*>(hits->p), cnt, reinterpret_cast<fmgpu_position*>(positions->p), pcap, &pcnt, locate_stats, stream);
        if (rc != FMGPU_ERR_CAPACITY || attempt > 0) break;         // (the count is exact: the second run fits)
        if ((rc = positions->need((size_t)std::max(pcnt, 2 * pcap) * sizeof(fmgpu_position)))) return rc;
        pcap = positions->bytes / sizeof(fmgpu_position);
    }
    if (rc) return rc;
    *pos_count = pcnt;
    return 0;
}

namespace {

struct OwnBuffer : MapBuffer {                                      // the one-shot call's scratch: freed on return
    DBuf d;
    int need(size_t nbytes) override {
        if (nbytes <= bytes) return 0;
        const int rc = d.alloc(nbytes);
        p = d.p; bytes = d.p ? d.bytes : 0;
        return rc;
    }
};

int run_map(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what, fmgpu_position* out, uint64_t capacity,
            uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_stats* search_stats,
            fmgpu_stats* locate_stats, hipStream_t stream, bool packed, bool both = false, const fmgpu_strands* strands = nullptr) {
    if (out_count) *out_count = 0;
    if (out_hit_count) *out_hit_count = 0;
    if (int rc = check_map_query(what)) return rc;
    if (both) if (int rc = check_strands(strands)) return rc;
    const int32_t nstats = std::max(1, what->n_schemes);
    if (search_stats) for (int32_t i = 0; i < nstats; ++i) search_stats[i] = fmgpu_stats{};
    if (locate_stats) *locate_stats = fmgpu_stats{};
    if (nq == 0) return 0;                                          // (before the handle is looked at; out_stratum untouched)
    if (both && nq > kMaxStrandReads) return fail(FMGPU_ERR_UNSUPPORTED, "a both-strand batch holds at most 2^30 - 1 reads");
    if (int rc = check_map_schemes(h, what, packed)) return rc;
    if (!qbuf || !qoff || !out_count || (!out && capacity) || (!out_hits && hits_capacity)) return fail(FMGPU_ERR_INVALID, "qbuf / qoff / out / out_count / out_hits is null");

    // the batch in HBM, once for every stage and every rerun
    int rc;
    Staged soff, sbuf, sstratum;
    if ((rc = soff.in(qoff, (nq + 1) * 8, stream))) return rc;
    uint64_t last = 0;
    if (is_device_pointer(qoff)) { FM_HIP(hipMemcpyAsync(&last, qoff + nq, 8, hipMemcpyDeviceToHost, stream)); FM_HIP(hipStreamSynchronize(stream)); }
    else last = qoff[nq];
    if ((rc = sbuf.in(qbuf, packed ? (last + 1) / 2 : last, stream))) return rc;
    const uint8_t* dq = sbuf.dev ? (const uint8_t*)sbuf.dev : qbuf;  // (a batch without a symbol: the pointer is never read through)
    const uint64_t* doff = (const uint64_t*)soff.dev;
    // both strands: only the forward strand was staged, the doubled batch is made in the call's scratch and the chain runs on it
    OwnBuffer q2, off2;
    DBuf dtable;
    if (both) {
        uint8_t table[256];
        strands_table(strands->complement, strands->n, table);
        if ((rc = dtable.alloc(256))) return rc;
        FM_HIP(hipMemcpyAsync(dtable.p, table, 256, hipMemcpyHostToDevice, stream));
        if ((rc = strands_device(dq, doff, nq, dtable.as<uint8_t>(), &q2, &off2, stream))) { (void)hipStreamSynchronize(stream); return rc; }      // (it synchronises: `table` is done with)
        dq = reinterpret_cast<const uint8_t*>(q2.p); doff = reinterpret_cast<const uint64_t*>(off2.p); nq *= 2;
    }
    if ((rc = sstratum.out(out_stratum, out_stratum ? nq : 0, stream))) return rc;

    OwnBuffer hits, positions, intervals;
    uint64_t cnt = 0, pcnt = 0;
    if ((rc = map_device(h, dq, doff, nq, what, packed, &hits, &positions, &intervals, out_stratum ? (uint8_t*)sstratum.dev : nullptr, search_stats,
                         locate_stats, stream, &cnt, &pcnt, both && strands->pair != 0))) return rc;
    *out_count = pcnt;
    if (out_hit_count) *out_hit_count = cnt;
    if ((rc = sstratum.finish())) return rc;
    if (pcnt > capacity) return fail(FMGPU_ERR_CAPACITY, "position buffer holds " + std::to_string(capacity) + " records, " + std::to_string(pcnt) + " produced");
    if (out_hits && cnt > hits_capacity) return fail(FMGPU_ERR_CAPACITY, "hit buffer holds " + std::to_string(hits_capacity) + " records, " + std::to_string(cnt) + " produced");
    if (pcnt) FM_HIP(hipMemcpyAsync(out, positions.p, (size_t)pcnt * sizeof(fmgpu_position), hipMemcpyDefault, stream));
    if (out_hits && cnt) FM_HIP(hipMemcpyAsync(out_hits, hits.p, (size_t)cnt * sizeof(fmgpu_hit), hipMemcpyDefault, stream));
    FM_HIP(hipStreamSynchronize(stream));                           // the scratch is freed on return
    return 0;
}

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_map(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what, fmgpu_position* out, uint64_t capacity,
              uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_stats* search_stats,
              fmgpu_stats* locate_stats, void* stream) {
    return run_map(h, qbuf, qoff, nq, what, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum, search_stats, locate_stats, (hipStream_t)stream, false);
}
int fmgpu_map_strands(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what, const fmgpu_strands* strands,
                      fmgpu_position* out, uint64_t capacity, uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                      uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats, void* stream) {
    return run_map(h, qbuf, qoff, nq, what, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum, search_stats, locate_stats, (hipStream_t)stream, false,
                   true, strands);
}
int fmgpu_map_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what, fmgpu_position* out, uint64_t capacity,
                 uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_stats* search_stats,
                 fmgpu_stats* locate_stats, void* stream) {
    return run_map(h, packed, qoff, nq, what, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum, search_stats, locate_stats, (hipStream_t)stream, true);
}

}  // extern "C"
