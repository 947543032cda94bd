// tools/sam_probe.py, the baseline leg: the SAM lines of include/fmgpu.h (fmgpu_positions_sam: both strands, all three tables given, names up to their first blank, no empty
// read or name) written by a snprintf loop into a memory buffer, on one core.  Built by the probe with g++ -O2 -shared; returns the bytes written (0: out of room).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

struct Position { uint64_t qidx, seq_id, pos; uint32_t errors, hit; };
struct Span { uint64_t offset, len; };

static uint64_t upToBlank(uint8_t const* s, uint64_t n) {
    uint64_t m = 0;
    while (m < n && s[m] != ' ' && s[m] != '\t') ++m;
    return m;
}

extern "C" uint64_t sam_loop(Position const* positions, uint64_t count, uint8_t const* qbuf, uint64_t const* qoff, uint64_t nq, uint8_t const* charOf, uint8_t const* charOfComp,
                             uint8_t const* nameBytes, Span const* names, uint8_t const* qualBytes, Span const* quals, uint8_t const* seqBytes, Span const* seqs,
                             unsigned mapqUnique, unsigned mapqMulti, char* out, uint64_t capacity) {
    uint64_t at = 0, i = 0;
    for (uint64_t r = 0; r < nq; ++r) {
        uint64_t const first = i;
        while (i < count && (positions[i].qidx >> 1) == r) ++i;
        uint64_t const m = qoff[r + 1] - qoff[r], qn = upToBlank(nameBytes + names[r].offset, names[r].len);
        uint8_t const* q = qbuf + qoff[r];
        uint8_t const* ql = qualBytes + quals[r].offset;
        if (at + qn + 2 * m + 256 > capacity) return 0;
        if (first == i) {                                              // the unmapped line
            std::memcpy(out + at, nameBytes + names[r].offset, qn); at += qn;
            at += static_cast<uint64_t>(std::snprintf(out + at, capacity - at, "\t4\t*\t0\t0\t*\t*\t0\t0\t"));
            for (uint64_t j = 0; j < m; ++j) out[at + j] = static_cast<char>(charOf[q[j]]);
            at += m; out[at++] = '\t';
            std::memcpy(out + at, ql, m); at += m; out[at++] = '\n';
            continue;
        }
        uint32_t least = UINT32_MAX;
        uint64_t primary = first, atLeast = 0;
        for (uint64_t k = first; k < i; ++k) if (positions[k].errors < least) { least = positions[k].errors; primary = k; }
        for (uint64_t k = first; k < i; ++k) atLeast += positions[k].errors == least;
        for (uint64_t k = first; k < i; ++k) {
            auto const& p = positions[k];
            bool const reverse = p.qidx & 1, secondary = k != primary;
            uint64_t const sn = upToBlank(seqBytes + seqs[p.seq_id].offset, seqs[p.seq_id].len);
            if (at + qn + sn + 2 * m + 256 > capacity) return 0;
            std::memcpy(out + at, nameBytes + names[r].offset, qn); at += qn;
            at += static_cast<uint64_t>(std::snprintf(out + at, capacity - at, "\t%u\t", (reverse ? 16u : 0u) | (secondary ? 256u : 0u)));
            std::memcpy(out + at, seqBytes + seqs[p.seq_id].offset, sn); at += sn;
            at += static_cast<uint64_t>(std::snprintf(out + at, capacity - at, "\t%zu\t%u\t%zuM\t*\t0\t0\t", static_cast<size_t>(p.pos + 1), !secondary && atLeast == 1 ? mapqUnique : mapqMulti,
                                                      static_cast<size_t>(m)));
            if (secondary) { out[at++] = '*'; out[at++] = '\t'; out[at++] = '*'; }
            else {
                if (reverse) for (uint64_t j = 0; j < m; ++j) out[at + j] = static_cast<char>(charOfComp[q[m - 1 - j]]);
                else for (uint64_t j = 0; j < m; ++j) out[at + j] = static_cast<char>(charOf[q[j]]);
                at += m; out[at++] = '\t';
                if (reverse) for (uint64_t j = 0; j < m; ++j) out[at + j] = static_cast<char>(ql[m - 1 - j]);
                else std::memcpy(out + at, ql, m);
                at += m;
            }
            at += static_cast<uint64_t>(std::snprintf(out + at, capacity - at, "\tNM:i:%u\tNH:i:%zu\n", p.errors, static_cast<size_t>(i - first)));
        }
    }
    return at;
}
