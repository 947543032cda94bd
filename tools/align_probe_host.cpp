// The rule of fmgpu_chains_align (include/fmgpu.h) on ONE host thread: the baseline of tools/align_probe.py (g++ -O2 -shared).  Inputs as the call takes them, in host
// memory and already checked (the probe makes them); out and ops as the call writes them.  Returns the number of operations; *cells receives the cells of all matrices.
#include <cstdint>
#include <cstring>
#include <vector>

namespace {
struct Chain { uint64_t qidx, seq_id, tbeg, tend; uint32_t qbeg, qend, score, n_anchors, first, flags; };
struct Position { uint64_t qidx, seq_id, pos; uint32_t errors, hit; };
struct Span { uint32_t qbeg, qlen; };
struct Record { uint64_t first_op; uint32_t n_ops, status, n_match, n_mismatch, n_ins, n_del; };
enum : uint32_t { OP_I = 1, OP_D = 2, OP_S = 4, OP_EQ = 7, OP_X = 8 };

struct Line {
    std::vector<uint32_t> ops;
    void add(uint32_t len, uint32_t code) {
        if (!len) return;
        if (!ops.empty() && (ops.back() & 15u) == code) ops.back() += len << 4;
        else ops.push_back(len << 4 | code);
    }
};

// one gap: the banded matrix row by row, directions 2 bits per cell, the traceback's operations in line order behind `line`
uint64_t gap(const uint8_t* Q, uint32_t gq, const uint8_t* T, uint32_t gt, uint32_t w, Line& line, std::vector<int32_t>& rows, std::vector<uint8_t>& dirs, std::vector<uint32_t>& back) {
    const int32_t d = (int32_t)gt - (int32_t)gq, lo = (d < 0 ? d : 0) - (int32_t)w, hi = (d > 0 ? d : 0) + (int32_t)w, width = hi - lo + 1;
    const int32_t INF = 0x3fffffff;
    rows.assign(2 * (size_t)width, INF);
    dirs.assign(((size_t)(gq + 1) * width + 3) / 4, 0);
    auto set = [&](uint32_t a, int32_t j, uint32_t dir) { const size_t i = (size_t)a * width + j; dirs[i / 4] |= dir << (2 * (i % 4)); };
    auto get = [&](uint32_t a, int32_t j) { const size_t i = (size_t)a * width + j; return (dirs[i / 4] >> (2 * (i % 4))) & 3u; };
    for (uint32_t a = 0; a <= gq; ++a) {
        int32_t* cur = rows.data() + (a & 1) * width;
        const int32_t* old = rows.data() + ((a & 1) ^ 1) * width;           // old[j]: the diagonal cell, old[j + 1]: the cell above
        for (int32_t j = 0; j < width; ++j) {
            const int32_t b = (int32_t)a + lo + j;
            int32_t v = INF;
            uint32_t dir = 2;
            if (b >= 0 && b <= (int32_t)gt) {
                if (a == 0 && b == 0) v = 0;
                else {
                    const int32_t vd = (a && b && old[j] < INF) ? old[j] + (Q[a - 1] != T[b - 1]) : INF;
                    const int32_t vl = (j && cur[j - 1] < INF) ? cur[j - 1] + 1 : INF;
                    const int32_t vu = (a && j + 1 < width && old[j + 1] < INF) ? old[j + 1] + 1 : INF;
                    v = vd < vl ? vd : vl; v = v < vu ? v : vu;
                    dir = vd == v ? 0u : vl == v ? 1u : 2u;
                }
            }
            cur[j] = v;
            set(a, j, dir);
        }
    }
    back.clear();
    uint32_t a = gq, b = gt;
    while (a || b) {
        const uint32_t dir = a == 0 ? 1u : b == 0 ? 2u : get(a, (int32_t)b - (int32_t)a - lo);
        if (dir == 0) { back.push_back(Q[a - 1] == T[b - 1] ? OP_EQ : OP_X); --a; --b; }
        else if (dir == 1) { back.push_back(OP_D); --b; }
        else { back.push_back(OP_I); --a; }
    }
    for (size_t i = back.size(); i-- > 0;) line.add(1, back[i]);
    return (uint64_t)(gq + 1) * width;
}
}  // namespace

extern "C" uint64_t align_host(const Chain* chains, uint64_t n_chains, const uint32_t* anchors, const Position* pos, const Span* spans, const uint8_t* qbuf, const uint64_t* qoff,
                               const uint8_t* tbuf, const uint64_t* toff, uint32_t band, uint32_t max_gap_len, uint64_t max_cells, Record* out, uint32_t* ops, uint64_t* cells) {
    uint64_t total = 0;
    *cells = 0;
    std::vector<int32_t> rows;
    std::vector<uint8_t> dirs;
    std::vector<uint32_t> back;
    Line line;
    for (uint64_t c = 0; c < n_chains; ++c) {
        const Chain& ch = chains[c];
        const uint8_t* Q = qbuf + qoff[ch.qidx];
        const uint8_t* T = tbuf + toff[c];
        const uint64_t m = qoff[ch.qidx + 1] - qoff[ch.qidx];
        Record r{total, 0, 0, 0, 0, 0, 0};
        line.ops.clear();
        line.add(ch.qbeg, OP_S);
        uint64_t chain_cells = 0;
        for (uint32_t k = 0; k < ch.n_anchors && !r.status; ++k) {
            const Position& p = pos[anchors[ch.first + k]];
            const uint64_t q = spans[p.hit].qbeg, t = p.pos - ch.tbeg;
            uint64_t lp = spans[p.hit].qlen;
            if (k + 1 < ch.n_anchors) {
                const Position& pn = pos[anchors[ch.first + k + 1]];
                const uint64_t dq = spans[pn.hit].qbeg - q, dt = pn.pos - ch.tbeg - t;
                lp = lp < dq ? lp : dq; lp = lp < dt ? lp : dt;
                const uint64_t gq = dq - lp, gt = dt - lp;
                line.add((uint32_t)lp, OP_EQ);
                if (gq == 0 || gt == 0) { line.add((uint32_t)gt, OP_D); line.add((uint32_t)gq, OP_I); }
                else {
                    const uint64_t width = (gt > gq ? gt - gq : gq - gt) + 2ull * band + 1;
                    if (gq > max_gap_len || gt > max_gap_len || (gq + 1) * width > max_cells) r.status = 1;
                    else chain_cells += gap(Q + q + lp, (uint32_t)gq, T + t + lp, (uint32_t)gt, band, line, rows, dirs, back);
                }
            } else line.add((uint32_t)lp, OP_EQ);
        }
        if (!r.status) {
            line.add((uint32_t)(m - ch.qend), OP_S);
            r.n_ops = (uint32_t)line.ops.size();
            for (uint32_t w : line.ops) {
                const uint32_t n = w >> 4, code = w & 15u;
                if (code == OP_EQ) r.n_match += n; else if (code == OP_X) r.n_mismatch += n; else if (code == OP_I) r.n_ins += n; else if (code == OP_D) r.n_del += n;
            }
            std::memcpy(ops + total, line.ops.data(), line.ops.size() * 4);
            total += line.ops.size();
            *cells += chain_cells;
        }
        out[c] = r;
    }
    return total;
}
