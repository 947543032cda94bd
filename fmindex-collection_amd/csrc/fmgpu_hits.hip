// fmgpu_hits.hip — fmgpu_hits_from_intervals (include/fmgpu.h): the intervals of an exact search turned into hit records in fmc::Search's report order, on the device:
//  k_interval_flags    one flag per read (does it produce a record), and its out_stratum byte
//  (hipcub exclusive scan of the flags: the record's place; the entry behind the last read is the count)
//  k_interval_records  every producing read writes its 40-byte record as five 8-byte vector stores
// Nothing here reads an index table; the file is built for both row widths like its neighbour fmgpu_locate.hip, and a call that comes with a handle (fmgpu_map) takes the
// build of that handle's width.
#include "fmgpu_common.h"

#include <hipcub/hipcub.hpp>

namespace FMGPU_NS {

// does read q produce a record: rows in its interval, rows allowed, and (with offsets) at least one symbol
__device__ __forceinline__ bool interval_produces(const uint64_t* __restrict__ len, const uint64_t* __restrict__ qoff, uint64_t q, uint64_t max_rows) {
    if (max_rows == 0 || len[q] == 0) return false;
    return !qoff || qoff[q + 1] > qoff[q];
}

// flag[q] for q < nq, flag[nq] = 0: the exclusive scan over nq + 1 entries ends in the count
__global__ __launch_bounds__(256) void k_interval_flags(const uint64_t* __restrict__ len, const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t max_rows,
                                                        uint32_t* __restrict__ flag, uint8_t* __restrict__ out_stratum) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= nq; q += (uint64_t)gridDim.x * blockDim.x) {
        const bool yes = q < nq && interval_produces(len, qoff, q, max_rows);
        flag[q] = yes ? 1u : 0u;
        if (out_stratum && q < nq) out_stratum[q] = yes ? (uint8_t)0 : (uint8_t)255;
    }
}

// place[q] = records before read q; place[nq] = the count (<= capacity: checked by the caller before this launch)
__global__ __launch_bounds__(256) void k_interval_records(const uint64_t* __restrict__ lb, const uint64_t* __restrict__ len, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ place, uint64_t nq, uint64_t qidx_base, uint64_t max_rows, uint64_t capacity,
                                                          fmgpu_hit* __restrict__ out) {
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * blockDim.x) {
        if (!flag[q]) continue;
        const uint64_t at = place[q];
        if (at >= capacity) continue;                               // (never: the count fits; nothing is stored beyond the caller's buffer)
        const uint64_t l = len[q];
        uint64_t* w = reinterpret_cast<uint64_t*>(out + at);        // a record is 8-byte aligned: five 8-byte stores
        w[0] = qidx_base + q;
        w[1] = lb[q];
        w[2] = 0;                                                   // lb_rev
        w[3] = l < max_rows ? l : max_rows;
        w[4] = 0;                                                   // errors = 0, seq = 0
    }
}

namespace api {
#include "fmgpu_api_decl.h"

int hits_from_intervals(const uint64_t* lb, const uint64_t* len, const uint64_t* qoff, uint64_t nq, uint64_t qidx_base, uint64_t max_rows, fmgpu_hit* out,
                        uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, void* stream_) {
    if (out_count) *out_count = 0;
    if (nq == 0) return 0;
    if (!lb || !len || !out_count || (!out && capacity)) return fail(FMGPU_ERR_INVALID, "lb / len / out / out_count is null");
    if (nq > 0x7ffffffeull) return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_hits_from_intervals takes at most 2^31 - 2 reads");
    hipStream_t stream = (hipStream_t)stream_;
    Staged slb, slen, soff, sstratum;
    int rc;
    if ((rc = slb.in(lb, nq * 8, stream)) || (rc = slen.in(len, nq * 8, stream)) || (rc = soff.in(qoff, qoff ? (nq + 1) * 8 : 0, stream))) return rc;
    if ((rc = sstratum.out(out_stratum, out_stratum ? nq : 0, stream))) return rc;
    const uint64_t* dlb = (const uint64_t*)slb.dev;
    const uint64_t* dlen = (const uint64_t*)slen.dev;
    const uint64_t* doff = qoff ? (const uint64_t*)soff.dev : nullptr;
    DBuf flag, place, tmp;
    if ((rc = flag.alloc((nq + 1) * 4)) || (rc = place.alloc((nq + 1) * 4))) return rc;
    size_t tb = 0;
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag.as<uint32_t>(), place.as<uint32_t>(), (int)(nq + 1), stream));
    if ((rc = tmp.alloc(tb))) return rc;
    dim3 grid; if ((rc = grid_of(nq + 1, &grid, 1u << 16))) return rc;
    k_interval_flags<<<grid, dim3(256), 0, stream>>>(dlen, doff, nq, max_rows, flag.as<uint32_t>(), out_stratum ? (uint8_t*)sstratum.dev : nullptr);
    FM_LAUNCHED("k_interval_flags");
    FM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb, flag.as<uint32_t>(), place.as<uint32_t>(), (int)(nq + 1), stream));
    CallScratch* sc = nullptr;
    if ((rc = call_scratch(&sc))) return rc;
    uint32_t* hback = reinterpret_cast<uint32_t*>(sc->pinned);
    FM_HIP(hipMemcpyAsync(hback, place.as<uint32_t>() + nq, 4, hipMemcpyDeviceToHost, stream));      // the one read-back: the count
    FM_HIP(hipStreamSynchronize(stream));
    const uint64_t total = hback[0];
    *out_count = total;
    if ((rc = sstratum.finish())) return rc;
    if (total > capacity) return fail(FMGPU_ERR_CAPACITY, "result buffer holds " + std::to_string(capacity) + " records, " + std::to_string(total) + " produced");
    if (total == 0) return 0;
    Staged sout;
    if ((rc = sout.out(out, total * sizeof(fmgpu_hit), stream))) return rc;
    k_interval_records<<<grid, dim3(256), 0, stream>>>(dlb, dlen, flag.as<uint32_t>(), place.as<uint32_t>(), nq, qidx_base, max_rows, total, (fmgpu_hit*)sout.dev);
    FM_LAUNCHED("k_interval_records");
    return sout.finish();                                           // (the scratch is freed on return: hipFree waits for the device)
}

}  // namespace api
}  // namespace FMGPU_NS
