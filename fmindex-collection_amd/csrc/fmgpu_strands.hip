// fmgpu_strands.hip — the both-strand batch (include/fmgpu.h: fmgpu_queries_strands): read 2q of the doubled batch is read q, read 2q + 1 is read q reversed and
// complemented, made on the device so that the second strand never crosses the bus.  strands_device is the pass on device buffers that grow; the one-shot call below,
// fmgpu_map_strands (fmgpu_map.hip) and the strands calls of the feeds (fmgpu_feed.hip) share it.  Nothing here depends on the row width.
#include "fmgpu_common.h"
#include "fmgpu_pieces.h"

namespace fmgpu {

// ---- the offsets of the doubled batch, closed-form: out_qoff[2q] = 2 (qoff[q] - qoff[0]), out_qoff[2q + 1] = out_qoff[2q] + len(q).  The same pass checks the
// caller's offsets: tail[0] = 1 where a pair of them decreases (every writer stores the same word: plain stores), tail[1] = the symbols of the batch.
__global__ __launch_bounds__(256) void k_strands_offsets(const uint64_t* __restrict__ qoff, uint64_t nq, uint64_t* __restrict__ out_qoff, uint64_t* __restrict__ tail) {
    const uint64_t base = qoff[0];
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q <= nq; q += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t at = qoff[q];
        if (q < nq) {
            const uint64_t next = qoff[q + 1];
            if (next < at || at < base) tail[0] = 1;
            out_qoff[2 * q] = 2 * (at - base);
            out_qoff[2 * q + 1] = 2 * (at - base) + (next - at);
        } else {
            if (at < base) tail[0] = 1;
            out_qoff[2 * q] = 2 * (at - base);
            tail[1] = at - base;
        }
    }
}

// ---- the symbols of the doubled batch.  A thread makes 16 output bytes: it finds the read of its first symbol by bisection of the caller's offsets (the closed form
// above) and walks on from there over strand and read boundaries (empty reads are stepped over).  What a chunk takes from one strand of one read is one run of source
// bytes: loaded as aligned 16-byte pieces and, for strand 1, reversed in registers and sent through the complement table in LDS (entries >= n are the identity).  A
// full chunk leaves as one aligned 16-byte store (byte by byte into a caller's device buffer that is not 16-byte aligned).
__global__ __launch_bounds__(256) void k_strands(const uint8_t* __restrict__ qbuf, const uint64_t* __restrict__ qoff, uint64_t nq, const uint8_t* __restrict__ table,
                                                 uint64_t total, uint8_t* __restrict__ out, int aligned) {
    __shared__ uint8_t comp[256];
    comp[threadIdx.x] = table[threadIdx.x];                         // (256 threads: one entry each)
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t s0 = 16 * t;
    if (s0 >= total) return;
    const uint64_t base = qoff[0];
    uint64_t lo = 0, hi = nq;                                       // the last read q with 2 (qoff[q] - base) <= s0: it is not empty, since s0 < total = 2 (qoff[nq] - base)
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (2 * (qoff[mid] - base) <= s0) lo = mid; else hi = mid; }
    uint64_t q = lo, src0 = qoff[q], src1 = qoff[q + 1];            // the read, its source bytes [src0, src1)
    uint64_t begin = 2 * (src0 - base);                             // where the current strand of the read starts in the output, `end` where it ends
    uint32_t strand = 0;
    if (s0 >= begin + (src1 - src0)) { strand = 1; begin += src1 - src0; }
    uint64_t end = begin + (src1 - src0);
    const uint64_t stop = s0 + 16 < total ? s0 + 16 : total;
    Piece acc{0, 0};
    for (uint64_t s = s0; s < stop;) {
        while (s >= end) {                                          // the next strand, or the next read's first one
            if (strand) { ++q; src0 = src1; src1 = qoff[q + 1]; }
            strand ^= 1u;
            begin = end; end = begin + (src1 - src0);
        }
        const uint32_t n = (uint32_t)((end < stop ? end : stop) - s);
        const uint64_t j = s - begin;                               // symbols j .. j + n - 1 of the strand
        Piece v;
        if (!strand) v = load_bytes(qbuf + src0 + j, n);
        else {                                                      // source bytes src1 - j - n .. src1 - j - 1, last one first
            const Piece f = load_bytes(qbuf + (src1 - j - n), n);
            Piece r{__builtin_bswap64(f.hi), __builtin_bswap64(f.lo)};
            r = piece_shr(r, 16u - n);
            uint64_t clo = 0, chi = 0;
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {
                if (k < n) clo |= (uint64_t)comp[(r.lo >> (8u * k)) & 255u] << (8u * k);
                if (k + 8u < n) chi |= (uint64_t)comp[(r.hi >> (8u * k)) & 255u] << (8u * k);
            }
            v = Piece{clo, chi};
        }
        v = piece_shl(v, (uint32_t)(s - s0));
        acc.lo |= v.lo; acc.hi |= v.hi;
        s += n;
    }
    if (aligned && s0 + 16 <= total) *reinterpret_cast<uint4*>(out + s0) = make_uint4((uint32_t)acc.lo, (uint32_t)(acc.lo >> 32), (uint32_t)acc.hi, (uint32_t)(acc.hi >> 32));
    else for (uint32_t k = 0; k < 16u && s0 + k < total; ++k) out[s0 + k] = (uint8_t)((k < 8u ? acc.lo >> (8u * k) : acc.hi >> (8u * (k - 8u))) & 255u);
}

int check_strands(const fmgpu_strands* strands) {
    if (!strands) return fail(FMGPU_ERR_INVALID, "strands is null");
    if (!strands->complement) return fail(FMGPU_ERR_INVALID, "fmgpu_strands: complement is null");
    if (strands->n < 1 || strands->n > 256) return fail(FMGPU_ERR_INVALID, "fmgpu_strands: n must be in [1, 256]");
    if (strands->pair < 0 || strands->pair > 1) return fail(FMGPU_ERR_INVALID, "fmgpu_strands: pair must be 0 or 1");
    return 0;
}

void strands_table(const uint8_t* complement, int32_t n, uint8_t* table) {
    for (int c = 0; c < 256; ++c) table[c] = c < n ? complement[c] : (uint8_t)c;
}

// the two passes on device memory: out_qoff (2 nq + 1 entries), out, tail = two words of scratch.  *symbols = the symbols of the
// caller's batch.  One read-back (the check of the offsets and the count) in front of the symbol pass, whose reads are bounded by those offsets.
static int strands_passes(const uint8_t* dq, const uint64_t* doff, uint64_t nq, const uint8_t* dtable, uint64_t* out_qoff, uint64_t* tail,
                          const std::function<int(uint64_t, uint8_t**)>& out_for, hipStream_t stream, uint64_t* symbols) {
    FM_HIP(hipMemsetAsync(tail, 0, 16, stream));
    dim3 ogrid; if (int rc = grid_of(nq + 1, &ogrid, 1u << 16)) return rc;
    k_strands_offsets<<<ogrid, dim3(256), 0, stream>>>(doff, nq, out_qoff, tail);
    FM_LAUNCHED("k_strands_offsets");
    uint64_t back[2] = {0, 0};
    FM_HIP(hipMemcpyAsync(back, tail, 16, hipMemcpyDeviceToHost, stream));
    FM_HIP(hipStreamSynchronize(stream));
    if (back[0]) return fail(FMGPU_ERR_INVALID, "qoff is not non-decreasing");
    *symbols = back[1];
    const uint64_t total = 2 * back[1];
    uint8_t* out = nullptr;
    if (int rc = out_for(total, &out)) return rc;
    if (!total) return 0;
    FM_GRID(grid, (total + 15) / 16);
    k_strands<<<grid, dim3(256), 0, stream>>>(dq, doff, nq, dtable, total, out, (reinterpret_cast<uintptr_t>(out) & 15u) == 0);
    FM_LAUNCHED("k_strands");
    return 0;
}

int strands_device(const uint8_t* dq, const uint64_t* doff, uint64_t nq, const uint8_t* dtable, MapBuffer* q2, MapBuffer* off2, hipStream_t stream) {
    if (nq > kMaxStrandReads) return fail(FMGPU_ERR_UNSUPPORTED, "a both-strand batch holds at most 2^30 - 1 reads");
    if (int rc = off2->need((size_t)(2 * nq + 1 + 2) * 8)) return rc;                // the offsets, and the two words of the check behind them
    uint64_t* const o = reinterpret_cast<uint64_t*>(off2->p);
    uint64_t symbols = 0;
    return strands_passes(dq, doff, nq, dtable, o, o + 2 * nq + 1, [&](uint64_t total, uint8_t** out) {
        if (int rc = q2->need((size_t)total + 16)) return rc;                         // (the search kernels load whole aligned 16-byte pieces)
        *out = reinterpret_cast<uint8_t*>(q2->p);
        return 0;
    }, stream, &symbols);
}

}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_queries_strands(const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const uint8_t* complement, int32_t n, uint8_t* out_qbuf, uint64_t* out_qoff,
                          void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 1 || n > 256) return fail(FMGPU_ERR_INVALID, "fmgpu_queries_strands: n must be in [1, 256]");
    if (nq > kMaxStrandReads) return fail(FMGPU_ERR_UNSUPPORTED, "a both-strand batch holds at most 2^30 - 1 reads");
    if (nq == 0) {
        if (!out_qoff) return 0;
        if (!is_device_pointer(out_qoff)) { out_qoff[0] = 0; return 0; }
        FM_HIP(hipMemsetAsync(out_qoff, 0, 8, stream));
        return 0;
    }
    if (!qbuf || !qoff || !complement || !out_qbuf || !out_qoff) return fail(FMGPU_ERR_INVALID, "qbuf / qoff / complement / out_qbuf / out_qoff is null");
    uint8_t table[256];
    strands_table(complement, n, table);
    int rc;
    Staged soff, sbuf, sooff, sout;
    DBuf small;                                                     // the table, and the two words of the check behind it
    if ((rc = small.alloc(256 + 16))) return rc;
    FM_HIP(hipMemcpyAsync(small.p, table, 256, hipMemcpyHostToDevice, stream));
    if ((rc = soff.in(qoff, (nq + 1) * 8, stream))) return rc;
    uint64_t last = 0;
    if (is_device_pointer(qoff)) { FM_HIP(hipMemcpyAsync(&last, qoff + nq, 8, hipMemcpyDeviceToHost, stream)); FM_HIP(hipStreamSynchronize(stream)); }
    else last = qoff[nq];
    if ((rc = sbuf.in(qbuf, last, stream))) return rc;
    if ((rc = sooff.out(out_qoff, (2 * nq + 1) * 8, stream))) return rc;
    const uint8_t* dq = sbuf.dev ? (const uint8_t*)sbuf.dev : qbuf;  // (a batch without a symbol: the pointer is never read through)
    uint64_t symbols = 0;
    rc = strands_passes(dq, (const uint64_t*)soff.dev, nq, small.as<uint8_t>(), (uint64_t*)sooff.dev, reinterpret_cast<uint64_t*>(small.as<uint8_t>() + 256),
                        [&](uint64_t total, uint8_t** out) {
                            if (int r = sout.out(out_qbuf, total, stream)) return r;
                            *out = (uint8_t*)sout.dev;
                            return 0;
                        }, stream, &symbols);
    if (rc) { (void)hipStreamSynchronize(stream); return rc; }
    if ((rc = sooff.finish())) return rc;
    if ((rc = sout.finish())) return rc;
    FM_HIP(hipStreamSynchronize(stream));                           // the table is freed on return
    return 0;
}

}  // extern "C"
