// tools/chain_probe.py's baseline: the rule of fmgpu_seeds_chain (include/fmgpu.h) on ONE host thread, behind one download of the records.  Per query a std::sort of
// its anchors by (seq_id, t, q, index), per run the three sweeps as plain loops (f and p; t, heir, chain length and leaf; chain start), then the query's chains sorted
// by (score descending, first place).  Built by the probe with g++ -O2 as a shared object of its own; nothing of the library is linked.
#include <algorithm>
#include <cstdint>
#include <vector>

namespace {
struct Position { uint64_t qidx, seq_id, pos; uint32_t errors, hit; };
struct Span { uint32_t qbeg, qlen; };
struct Chain { uint64_t qidx, seq_id, tbeg, tend; uint32_t qbeg, qend, score, n_anchors, first, flags; };
struct Anchor { uint64_t seq, t; uint32_t q, l, idx; };
constexpr uint32_t kNo = 0xffffffffu;
}  // namespace

extern "C" uint64_t chain_host(const Position* pos, uint64_t count, const Span* spans, uint64_t nq, uint32_t max_gap, uint32_t max_skew, uint32_t gap_cost_q8, uint32_t lookback,
                               uint32_t min_score, uint32_t min_anchors, uint32_t max_chains, uint32_t max_anchors, Chain* out, uint64_t capacity, uint32_t* out_anchor,
                               uint64_t* out_off) {
    std::vector<Anchor> a;
    std::vector<uint32_t> f, p, t, heir, len, leaf;
    std::vector<Chain> found;
    std::vector<uint32_t> found_start;
    uint64_t total = 0, anchors_out = 0, i0 = 0;
    for (uint64_t q = 0; q < nq; ++q) {
        out_off[q] = total;
        uint64_t i1 = i0;
        while (i1 < count && pos[i1].qidx == q) ++i1;
        const uint64_t n = i1 - i0;
        if (n == 0 || (max_anchors && n > max_anchors)) { i0 = i1; continue; }
        a.resize(n);
        for (uint64_t k = 0; k < n; ++k) { const Position& r = pos[i0 + k]; a[k] = Anchor{r.seq_id, r.pos, spans[r.hit].qbeg, spans[r.hit].qlen, (uint32_t)(i0 + k)}; }
        std::sort(a.begin(), a.end(), [](const Anchor& x, const Anchor& y) {
            if (x.seq != y.seq) return x.seq < y.seq;
            if (x.t != y.t) return x.t < y.t;
            if (x.q != y.q) return x.q < y.q;
            return x.idx < y.idx;
        });
        f.assign(n, 0); p.assign(n, kNo); t.assign(n, 0); heir.assign(n, kNo); len.assign(n, 1); leaf.assign(n, 0);
        found.clear(); found_start.clear();
        for (uint64_t b = 0; b < n;) {
            uint64_t e = b;
            while (e < n && a[e].seq == a[b].seq) ++e;
            for (uint64_t i = b; i < e; ++i) {
                uint32_t best = a[i].l, from = kNo;
                for (uint64_t d = 1; d <= i - b && d <= lookback; ++d) {
                    const Anchor& y = a[i - d];
                    if (y.t >= a[i].t || y.q >= a[i].q) continue;
                    const uint64_t dt = a[i].t - y.t, dq = a[i].q - y.q;
                    if (dt > max_gap || dq > max_gap) continue;
                    const uint64_t dd = dt > dq ? dt - dq : dq - dt;
                    if (dd > max_skew) continue;
                    const uint64_t m = std::min<uint64_t>(std::min<uint64_t>(a[i].l, dq), dt), cost = ((uint64_t)gap_cost_q8 * dd) >> 8;
                    if (m <= cost) continue;
                    const uint32_t v = f[i - d] + (uint32_t)(m - cost);
                    if (v > best) { best = v; from = (uint32_t)(i - d); }
                }
                f[i] = best; p[i] = from;
            }
            for (uint64_t j = e; j-- > b;) {
                uint32_t top = 0;
                for (uint64_t d = 1; j + d < e && d <= lookback; ++d)
                    if (p[j + d] == j && t[j + d] > top) { top = t[j + d]; heir[j] = (uint32_t)(j + d); }
                if (heir[j] == kNo) { t[j] = f[j]; len[j] = 1; leaf[j] = (uint32_t)j; }
                else { t[j] = top; len[j] = len[heir[j]] + 1; leaf[j] = leaf[heir[j]]; }
            }
            for (uint64_t s = b; s < e; ++s) {
                if (p[s] != kNo && heir[p[s]] == s) continue;
                const uint32_t score = t[s] - (p[s] != kNo ? f[p[s]] : 0u);
                if (score < min_score || len[s] < std::max(min_anchors, 1u)) continue;
                const Anchor& last = a[leaf[s]];
                found.push_back(Chain{q, a[s].seq, a[s].t, last.t + last.l, a[s].q, last.q + last.l, score, len[s], 0u, p[s] != kNo ? 1u : 0u});
                found_start.push_back((uint32_t)s);
            }
            b = e;
        }
        std::vector<uint32_t> order(found.size());
        for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return found[x].score > found[y].score; });      // (found is in the order of the first places)
        if (max_chains && order.size() > max_chains) order.resize(max_chains);
        for (uint32_t k : order) {
            if (total < capacity) {
                out[total] = found[k];
                out[total].first = (uint32_t)anchors_out;
                if (out_anchor) for (uint32_t s = found_start[k]; s != kNo; s = heir[s]) out_anchor[anchors_out++] = a[s].idx;
                else anchors_out += found[k].n_anchors;
            }
            ++total;
        }
        i0 = i1;
    }
    out_off[nq] = total;
    return total;
}
