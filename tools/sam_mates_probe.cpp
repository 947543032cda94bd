// tools/sam_mates_probe.cpp — the measurement of DESIGN.md 4.20: fmgpu_positions_sam_mates device to device between two hipEvents, against fmgpu_positions_sam on the
// same primary records and against a single-threaded host loop behind one download of the records and pairs, whose text is compared byte for byte with the device's.
// One interleaved batch of 2 F reads of 101 symbols with names and qualities, everything resident on the device.  Build and run (F fragments, repeats):
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/sam_mates_probe.cpp -o tools/sam_mates_probe -Lfmindex-collection_amd -lfmgpu -Wl,-rpath,'$ORIGIN/../fmindex-collection_amd'
//   tools/sam_mates_probe 4000000 7
#include <hip/hip_runtime.h>
#include "../include/fmgpu.h"

#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define OK(call) do { int rc_ = (call); if (rc_ != 0) { std::printf("FAILED %s: %d %s\n", #call, rc_, fmgpu_last_error()); return 1; } } while (0)
#define HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { std::printf("FAILED %s: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

static uint64_t state = 88172645463325252ull;
static inline uint64_t rnd() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state; }

template <class T> static T* up(std::vector<T> const& v) {
    void* p = nullptr;
    if (fmgpu_malloc(&p, v.size() * sizeof(T) + 16) != 0 || fmgpu_memcpy_h2d(p, v.data(), v.size() * sizeof(T)) != 0) { std::printf("FAILED upload: %s\n", fmgpu_last_error()); std::exit(1); }
    return static_cast<T*>(p);
}
static char* dec(char* p, uint64_t v) { char t[24]; int n = 0; do { t[n++] = char('0' + v % 10); v /= 10; } while (v); while (n) *p++ = t[--n]; return p; }

int main(int argc, char** argv) {
    uint64_t const F = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4000000, R = 2 * F, M = 101;
    int const repeats = argc > 2 ? std::atoi(argv[2]) : 7;
    std::vector<uint8_t> qbuf(R * M), qual(R * M), names;
    std::vector<uint64_t> qoff(R + 1);
    std::vector<fmgpu_text_span> nspan(R), qspan(R);
    for (auto& c : qbuf) c = uint8_t(1 + (rnd() & 3));
    for (auto& c : qual) c = uint8_t(33 + rnd() % 41);
    for (uint64_t r = 0; r <= R; ++r) qoff[r] = r * M;
    for (uint64_t r = 0; r < R; ++r) {
        std::string const n = "SRR000001." + std::to_string(r / 2 + 1) + "/" + std::to_string(r % 2 + 1) + " length=101";
        nspan[r] = fmgpu_text_span{names.size(), n.size()};
        names.insert(names.end(), n.begin(), n.end());
        qspan[r] = fmgpu_text_span{r * M, M};
    }
    // one record per read for 95 % of the reads; 90 % of the fragments with both mates get a pair: B sits 150 .. 400 behind A on the other strand
    std::vector<fmgpu_position> pos;
    std::vector<fmgpu_mate_pair> pairs;
    for (uint64_t f = 0; f < F; ++f) {
        bool const hasA = rnd() % 100 < 95, hasB = rnd() % 100 < 95, joined = hasA && hasB && rnd() % 100 < 90;
        uint64_t const seq = rnd() % 24, p = rnd() % 240000000, s = rnd() & 1;
        uint32_t ia = 0, ib = 0;
        if (hasA) { ia = uint32_t(pos.size()); pos.push_back(fmgpu_position{2 * (2 * f) + s, seq, p, uint32_t(rnd() % 3), 0}); }
        if (hasB) { ib = uint32_t(pos.size()); pos.push_back(fmgpu_position{2 * (2 * f + 1) + (joined ? 1 - s : (rnd() & 1)), joined ? seq : rnd() % 24, joined ? p + 150 + rnd() % 250 : rnd() % 240000000, uint32_t(rnd() % 3), 0}); }
        if (joined) pairs.push_back(fmgpu_mate_pair{f, 0, ia, ib, 0, 0});
    }
    std::vector<std::string> seqs;
    std::vector<uint8_t> sbytes;
    std::vector<fmgpu_text_span> sspan;
    for (int k = 0; k < 24; ++k) { std::string const n = "chr" + std::to_string(k + 1); sspan.push_back(fmgpu_text_span{sbytes.size(), n.size()}); sbytes.insert(sbytes.end(), n.begin(), n.end()); seqs.push_back(n); }
    uint8_t char_of[256], comp[5] = {0, 4, 3, 2, 1};
    std::memset(char_of, 'N', 256);
    std::memcpy(char_of, "$ACGT", 5);
    fmgpu_strands st{comp, 5, 0};

    auto* dq = up(qbuf); auto* dqual = up(qual); auto* dnames = up(names); auto* doff = up(qoff); auto* dns = up(nspan); auto* dqs = up(qspan);
    auto* dpos = up(pos); auto* dpairs = up(pairs); auto* dsb = up(sbytes); auto* dss = up(sspan);
    fmgpu_name_table rt{dnames, names.size(), dns, R}, qt{dqual, qual.size(), dqs, R}, nt{dsb, sbytes.size(), dss, 24};
    fmgpu_sam_mates_spec ms{};
    ms.qbuf_a = dq; ms.qoff_a = doff; ms.n_fragments = F; ms.char_of = char_of; ms.strands = &st; ms.read_names = &rt; ms.quals_a = &qt; ms.seq_names = &nt;
    ms.interleaved = 1; ms.cigar = 1; ms.strip_mate_suffix = 1; ms.mapq_unique = 60;
    fmgpu_sam_spec ss{};
    ss.qbuf = dq; ss.qoff = doff; ss.nq = R; ss.char_of = char_of; ss.strands = &st; ss.read_names = &rt; ss.quals = &qt; ss.seq_names = &nt; ss.cigar = 1; ss.emit_unmapped = 1; ss.mapq_unique = 60;

    uint64_t mbytes = 0, sbytes_out = 0, slines = 0;
    OK(fmgpu_positions_sam_mates(dpos, pos.size(), nullptr, 0, dpairs, pairs.size(), &ms, nullptr, 0, &mbytes, nullptr, nullptr));
    OK(fmgpu_positions_sam(dpos, pos.size(), &ss, nullptr, 0, &sbytes_out, nullptr, &slines, nullptr));
    void* dout = nullptr;
    OK(fmgpu_malloc(&dout, std::max(mbytes, sbytes_out) + 16));
    hipEvent_t e0, e1;
    HIP(hipEventCreate(&e0)); HIP(hipEventCreate(&e1));
    std::vector<float> tm, ts;
    for (int it = 0; it < 2 + repeats; ++it) {                        // two warm-up rounds; the two calls alternate
        float ms_ = 0;
        uint64_t got = 0;
        HIP(hipEventRecord(e0, nullptr));
        OK(fmgpu_positions_sam_mates(dpos, pos.size(), nullptr, 0, dpairs, pairs.size(), &ms, static_cast<uint8_t*>(dout), mbytes, &got, nullptr, nullptr));
        HIP(hipEventRecord(e1, nullptr)); HIP(hipEventSynchronize(e1)); HIP(hipEventElapsedTime(&ms_, e0, e1));
        if (it >= 2) tm.push_back(ms_);
        HIP(hipEventRecord(e0, nullptr));
        OK(fmgpu_positions_sam(dpos, pos.size(), &ss, static_cast<uint8_t*>(dout), sbytes_out, &got, nullptr, &slines, nullptr));
        HIP(hipEventRecord(e1, nullptr)); HIP(hipEventSynchronize(e1)); HIP(hipEventElapsedTime(&ms_, e0, e1));
        if (it >= 2) ts.push_back(ms_);
    }
    std::sort(tm.begin(), tm.end()); std::sort(ts.begin(), ts.end());
    auto report = [&](char const* what, std::vector<float> const& t, uint64_t bytes, uint64_t lines) {
        float const med = t[t.size() / 2];
        std::printf("%s: %" PRIu64 " lines, %" PRIu64 " bytes; ms min %.2f median %.2f max %.2f over %zu runs; %.2f GB/s, %.1f M lines/s at the median\n", what, lines, bytes,
                    t.front(), med, t.back(), t.size(), bytes / (med * 1e6), lines / (med * 1e3));
    };
    report("fmgpu_positions_sam_mates (device to device)", tm, mbytes, R);
    report("fmgpu_positions_sam (device to device, same records)", ts, sbytes_out, slines);

    // the device's paired text, for the comparison below
    std::vector<uint8_t> text(mbytes);
    uint64_t got = 0;
    OK(fmgpu_positions_sam_mates(dpos, pos.size(), nullptr, 0, dpairs, pairs.size(), &ms, static_cast<uint8_t*>(dout), mbytes, &got, nullptr, nullptr));
    OK(fmgpu_memcpy_d2h(text.data(), dout, mbytes));

    // the host loop: one download of the records and the pairs, then one thread
    std::vector<double> th;
    std::vector<char> host(mbytes + 4096);
    uint64_t hbytes = 0;
    for (int it = 0; it < 3; ++it) {
        auto const t0 = std::chrono::steady_clock::now();
        std::vector<fmgpu_position> hp(pos.size());
        std::vector<fmgpu_mate_pair> hpr(pairs.size());
        OK(fmgpu_memcpy_d2h(hp.data(), dpos, hp.size() * sizeof hp[0]));
        OK(fmgpu_memcpy_d2h(hpr.data(), dpairs, hpr.size() * sizeof hpr[0]));
        std::vector<uint32_t> first(R, UINT32_MAX), end(R, 0), prim(R, UINT32_MAX), nmin(R, 0), pcnt(F, 0);
        std::vector<uint64_t> pkey(F, UINT64_MAX);
        for (uint32_t i = 0; i < hp.size(); ++i) {
            uint64_t const r = hp[i].qidx >> 1;
            if (first[r] == UINT32_MAX) first[r] = i;
            end[r] = i + 1;
            if (prim[r] == UINT32_MAX || hp[i].errors < hp[prim[r]].errors) { prim[r] = i; nmin[r] = 1; } else if (hp[i].errors == hp[prim[r]].errors) ++nmin[r];
        }
        for (uint32_t i = 0; i < hpr.size(); ++i) {
            uint64_t const key = uint64_t(hp[hpr[i].a].errors + hp[hpr[i].b].errors) << 32 | i, f = hpr[i].fragment;
            if ((key >> 32) < (pkey[f] >> 32) || pkey[f] == UINT64_MAX) { pkey[f] = key; pcnt[f] = 1; } else if ((key >> 32) == (pkey[f] >> 32)) ++pcnt[f];
        }
        char* o = host.data();
        for (uint64_t l = 0; l < R; ++l) {
            uint64_t const f = l >> 1;
            bool const proper = pkey[f] != UINT64_MAX;
            uint32_t const xi = proper ? (l & 1 ? hpr[uint32_t(pkey[f])].b : hpr[uint32_t(pkey[f])].a) : prim[l];
            uint32_t const yi = proper ? (l & 1 ? hpr[uint32_t(pkey[f])].a : hpr[uint32_t(pkey[f])].b) : prim[l ^ 1];
            bool const hx = xi != UINT32_MAX, hy = yi != UINT32_MAX;
            fmgpu_position const x = hx ? hp[xi] : fmgpu_position{}, y = hy ? hp[yi] : fmgpu_position{};
            uint32_t const sx = hx ? uint32_t(x.qidx & 1) : 0, sy = hy ? uint32_t(y.qidx & 1) : 0;
            auto const& sp = nspan[2 * f];
            uint64_t n = 0;
            while (n < sp.len && names[sp.offset + n] != ' ' && names[sp.offset + n] != '\t') ++n;
            if (n >= 3 && names[sp.offset + n - 2] == '/' && (names[sp.offset + n - 1] == '1' || names[sp.offset + n - 1] == '2')) n -= 2;
            std::memcpy(o, names.data() + sp.offset, n); o += n; *o++ = '\t';
            o = dec(o, 1u | (l & 1 ? 128u : 64u) | (proper ? 2u : 0u) | (hx ? 0u : 4u) | (hy ? 0u : 8u) | (sx ? 16u : 0u) | (sy ? 32u : 0u)); *o++ = '\t';
            if (hx || hy) { auto const& at = hx ? x : y; std::memcpy(o, seqs[at.seq_id].data(), seqs[at.seq_id].size()); o += seqs[at.seq_id].size(); *o++ = '\t'; o = dec(o, at.pos + 1); }
            else { *o++ = '*'; *o++ = '\t'; *o++ = '0'; }
            *o++ = '\t';
            o = dec(o, !hx ? 0u : ((proper ? pcnt[f] : nmin[l]) == 1 ? 60u : 0u)); *o++ = '\t';
            if (hx) { o = dec(o, M); *o++ = 'M'; } else *o++ = '*';
            *o++ = '\t';
            if (!hx && !hy) *o++ = '*'; else if (hx && hy && x.seq_id != y.seq_id) { std::memcpy(o, seqs[y.seq_id].data(), seqs[y.seq_id].size()); o += seqs[y.seq_id].size(); } else *o++ = '=';
            *o++ = '\t';
            o = dec(o, hy ? y.pos + 1 : hx ? x.pos + 1 : 0); *o++ = '\t';
            if (hx && hy && x.seq_id == y.seq_id) {
                uint64_t const t = std::max(x.pos + M, y.pos + M) - std::min(x.pos, y.pos);
                if (t && (x.pos > y.pos || (x.pos == y.pos && (l & 1)))) *o++ = '-';
                o = dec(o, t);
            } else *o++ = '0';
            *o++ = '\t';
            uint8_t const* q = qbuf.data() + l * M;
            if (sx) for (uint64_t j = 0; j < M; ++j) { uint8_t c = q[M - 1 - j]; *o++ = char(char_of[c < 5 ? comp[c] : c]); }
            else for (uint64_t j = 0; j < M; ++j) *o++ = char(char_of[q[j]]);
            *o++ = '\t';
            uint8_t const* ql = qual.data() + l * M;
            if (sx) for (uint64_t j = 0; j < M; ++j) *o++ = char(ql[M - 1 - j]); else { std::memcpy(o, ql, M); o += M; }
            if (hx) { std::memcpy(o, "\tNM:i:", 6); o += 6; o = dec(o, x.errors); std::memcpy(o, "\tNH:i:", 6); o += 6; o = dec(o, end[l] - first[l]); }
            *o++ = '\n';
        }
        hbytes = uint64_t(o - host.data());
        th.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(th.begin(), th.end());
    std::printf("host loop (one thread, behind the download of %zu records and %zu pairs): %" PRIu64 " bytes; ms min %.1f median %.1f max %.1f over %zu runs; %.3f GB/s at the median\n",
                pos.size(), pairs.size(), hbytes, th.front(), th[th.size() / 2], th.back(), th.size(), hbytes / (th[th.size() / 2] * 1e6));
    bool const same = hbytes == mbytes && std::memcmp(host.data(), text.data(), mbytes) == 0;
    std::printf("the host loop and the device wrote %s text\n", same ? "the same" : "DIFFERENT");
    return same ? 0 : 1;
}
