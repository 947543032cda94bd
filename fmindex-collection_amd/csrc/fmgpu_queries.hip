// fmgpu_queries.hip — the 4-bit packed query form (include/fmgpu.h): the device packer (with the reverse-complement strand), the unpacker, and the
// unpack route that serves every `_q4` search whose kernel reads bytes.  Nothing here depends on the row width.
#include "fmgpu_common.h"

namespace fmgpu {

// ---- unpack: symbols first .. first + count - 1 of `packed` as bytes out[0 ..], nibble 15 as 255.  A thread takes the two symbols of one packed byte; only the
// bytes that hold a symbol of the range are loaded.
__global__ __launch_bounds__(256) void k_unpack4(const uint8_t* __restrict__ packed, uint64_t first, uint64_t count, uint8_t* __restrict__ out) {
    const uint64_t b0 = first >> 1, nb = ((first + count + 1) >> 1) - b0;             // the packed bytes of the range
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nb; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t v = packed[b0 + t];
        const uint64_t s = 2 * (b0 + t);                                            // the byte's low symbol
        const uint32_t lo = v & 15u, hi = v >> 4;
        if (s >= first) out[s - first] = (uint8_t)(lo == 15u ? 255u : lo);
        if (s + 1 >= first && s + 1 < first + count) out[s + 1 - first] = (uint8_t)(hi == 15u ? 255u : hi);
    }
}

// ---- pack: the output offsets first (one strand: qoff - qoff[0]; both strands: read 2q at twice that, read 2q + 1 behind it), then the nibbles
__global__ __launch_bounds__(256) void k_pack4_offsets(const uint64_t* __restrict__ qoff, uint64_t nq, int both, uint64_t* __restrict__ out_qoff) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > nq) return;
    const uint64_t at = qoff[q] - qoff[0];
    if (!both) { out_qoff[q] = at; return; }
    out_qoff[2 * q] = 2 * at;
    if (q < nq) out_qoff[2 * q + 1] = 2 * at + (qoff[q + 1] - qoff[q]);
}
struct Complement { uint8_t c[16]; };
// A thread makes eight output bytes = sixteen output symbols, so every output byte has one writer although reads share bytes.  It finds the read of its first
// symbol by bisection of out_qoff and walks on from there (empty reads are stepped over).
__global__ __launch_bounds__(256) void k_pack4(const uint8_t* __restrict__ qbuf, const uint64_t* __restrict__ qoff, uint32_t sigma, Complement comp, int both,
                                               const uint64_t* __restrict__ out_qoff, uint64_t nreads, uint64_t total, uint8_t* __restrict__ out, int aligned) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t s0 = 16 * t, nbytes = (total + 1) >> 1;
    if (s0 >= total) return;
    uint64_t lo = 0, hi = nreads;                                   // the last read r with out_qoff[r] <= s0 (out_qoff[0] = 0; s0 < total = out_qoff[nreads])
    while (hi - lo > 1) { const uint64_t mid = (lo + hi) >> 1; if (out_qoff[mid] <= s0) lo = mid; else hi = mid; }
    uint64_t r = lo, begin = out_qoff[r], end = out_qoff[r + 1];
    uint64_t word = 0;
    for (uint32_t k = 0; k < 16u; ++k) {
        const uint64_t s = s0 + k;
        if (s >= total) break;
        while (s >= end) { ++r; begin = end; end = out_qoff[r + 1]; }
        const uint64_t q = both ? r >> 1 : r, j = s - begin;
        const bool rev = both && (r & 1u);
        const uint32_t b = qbuf[rev ? qoff[q + 1] - 1 - j : qoff[q] + j];
        uint32_t c = b < sigma ? (rev ? comp.c[b] : b) : 15u;
        if (c >= sigma) c = 15u;
        word |= (uint64_t)c << (4u * k);
    }
    if (aligned && 8 * t + 8 <= nbytes) *reinterpret_cast<uint64_t*>(out + 8 * t) = word;
    else for (uint32_t k = 0; k < 8u && 8 * t + k < nbytes; ++k) out[8 * t + k] = (uint8_t)(word >> (8u * k));
}

// first and last offset of a batch (a device array: one read-back of each)
static int offset_ends(const uint64_t* qoff, uint64_t nq, hipStream_t stream, uint64_t* first, uint64_t* last) {
    if (is_device_pointer(qoff)) {
        FM_HIP(hipMemcpyAsync(first, qoff, 8, hipMemcpyDeviceToHost, stream));
        FM_HIP(hipMemcpyAsync(last, qoff + nq, 8, hipMemcpyDeviceToHost, stream));
        FM_HIP(hipStreamSynchronize(stream));
    } else { *first = qoff[0]; *last = qoff[nq]; }
    if (*last < *first) return fail(FMGPU_ERR_INVALID, "qoff is not non-decreasing");
    return 0;
}
static int launch_unpack(const uint8_t* dpacked, uint64_t first, uint64_t count, uint8_t* dout, hipStream_t stream) {
    if (!count) return 0;
    dim3 grid; if (int rc = grid_of((count + 3) / 2, &grid, 1u << 20)) return rc;
    k_unpack4<<<grid, dim3(256), 0, stream>>>(dpacked, first, count, dout);
    FM_LAUNCHED("k_unpack4");
    return 0;
}

int unpack_queries(const uint8_t* packed, const uint64_t* qoff, uint64_t nq, hipStream_t stream, UnpackedQueries* u) {
    u->stream = stream;
    uint64_t first = 0, last = 0;
    int rc;
    if ((rc = u->off.in(qoff, (nq + 1) * 8, stream))) return rc;
    if ((rc = offset_ends(qoff, nq, stream, &first, &last))) return rc;
    if ((rc = u->packed.in(packed, (last + 1) / 2, stream))) return rc;
    if ((rc = u->bytes.alloc(last + 16))) return rc;                // byte i of the scratch is symbol i: the launcher takes the offsets as they are
    return launch_unpack((const uint8_t*)u->packed.dev, first, last - first, u->bytes.as<uint8_t>() + first, stream);
}

}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_queries_pack4(const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, int32_t sigma, const uint8_t* complement,
                        uint8_t* out_packed, uint64_t* out_qoff, void* stream_) {
    if (sigma < 2 || sigma > 15) return fail(FMGPU_ERR_UNSUPPORTED, "4-bit packed queries need 2 <= sigma <= 15");
    if (nq == 0) return 0;
    if (!qbuf || !qoff || !out_packed || !out_qoff) return fail(FMGPU_ERR_INVALID, "qbuf / qoff / out_packed / out_qoff is null");
    hipStream_t stream = (hipStream_t)stream_;
    const int both = complement ? 1 : 0;
    Complement comp;
    std::memset(comp.c, 15, sizeof comp.c);
    if (complement) {
        if (is_device_pointer(complement)) FM_HIP(hipMemcpy(comp.c, complement, (size_t)sigma, hipMemcpyDeviceToHost));
        else std::memcpy(comp.c, complement, (size_t)sigma);
    }
    uint64_t first = 0, last = 0;
    Staged soff, sbuf, spacked, sooff;
    int rc;
    if ((rc = soff.in(qoff, (nq + 1) * 8, stream))) return rc;
    if ((rc = offset_ends(qoff, nq, stream, &first, &last))) return rc;
    const uint64_t nreads = both ? 2 * nq : nq, total = (last - first) * (both ? 2u : 1u);
    if ((rc = sbuf.in(qbuf, last, stream))) return rc;
    if ((rc = sooff.out(out_qoff, (nreads + 1) * 8, stream))) return rc;
    if ((rc = spacked.out(out_packed, (total + 1) / 2, stream))) return rc;
    FM_GRID(ogrid, nq + 1);
    k_pack4_offsets<<<ogrid, dim3(256), 0, stream>>>((const uint64_t*)soff.dev, nq, both, (uint64_t*)sooff.dev);
    FM_LAUNCHED("k_pack4_offsets");
    if (total) {
        FM_GRID(grid, (total + 15) / 16);
        k_pack4<<<grid, dim3(256), 0, stream>>>((const uint8_t*)sbuf.dev, (const uint64_t*)soff.dev, (uint32_t)sigma, comp, both, (const uint64_t*)sooff.dev,
                                                nreads, total, (uint8_t*)spacked.dev, ((uintptr_t)spacked.dev & 7u) == 0);
        FM_LAUNCHED("k_pack4");
    }
    if ((rc = sooff.finish())) return rc;
    return spacked.finish();
}

int fmgpu_queries_unpack4(const uint8_t* packed, const uint64_t* qoff, uint64_t nq, uint8_t* out_bytes, void* stream_) {
    if (nq == 0) return 0;
    if (!packed || !qoff || !out_bytes) return fail(FMGPU_ERR_INVALID, "packed / qoff / out_bytes is null");
    hipStream_t stream = (hipStream_t)stream_;
    uint64_t first = 0, last = 0;
    Staged spacked, sout;
    int rc;
    if ((rc = offset_ends(qoff, nq, stream, &first, &last))) return rc;
    if ((rc = spacked.in(packed, (last + 1) / 2, stream))) return rc;
    if ((rc = sout.out(out_bytes, last - first, stream))) return rc;
    if ((rc = launch_unpack((const uint8_t*)spacked.dev, first, last - first, (uint8_t*)sout.dev, stream))) return rc;
    return sout.finish();
}

}  // extern "C"
