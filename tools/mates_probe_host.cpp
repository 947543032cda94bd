// tools/mates_probe.py, the baseline leg: the pairs of include/fmgpu.h (fmgpu_positions_mates: separate batches, both strands, FR, every concordant pair) joined on one
// core: per fragment the records of mate B ordered by (seq_id, pos, index) with std::sort, per record of mate A a bisection to its window and a walk over it.  Built by
// the probe with g++ -O2 -shared; returns the number of pairs (written while they fit `capacity`), off[f] = the fragment's first pair.
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct Position { uint64_t qidx, seq_id, pos; uint32_t errors, hit; };
struct Pair { uint64_t fragment, tlen; uint32_t a, b, errors, flags; };

extern "C" uint64_t mates_join(Position const* a, uint64_t countA, Position const* b, uint64_t countB, uint64_t const* qoffA, uint64_t const* qoffB, uint64_t fragments,
                               uint64_t minTlen, uint64_t maxTlen, Pair* out, uint64_t capacity, uint64_t* off) {
    uint64_t pairs = 0, ia = 0, ib = 0;
    std::vector<uint32_t> order;
    for (uint64_t f = 0; f < fragments; ++f) {
        off[f] = pairs;
        uint64_t const a0 = ia, b0 = ib;
        while (ia < countA && (a[ia].qidx >> 1) == f) ++ia;
        while (ib < countB && (b[ib].qidx >> 1) == f) ++ib;
        if (a0 == ia || b0 == ib) continue;
        order.resize(ib - b0);
        for (uint64_t j = b0; j < ib; ++j) order[j - b0] = static_cast<uint32_t>(j);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            if (b[x].seq_id != b[y].seq_id) return b[x].seq_id < b[y].seq_id;
            if (b[x].pos != b[y].pos) return b[x].pos < b[y].pos;
            return x < y;
        });
        uint64_t const ma = qoffA[f + 1] - qoffA[f], mb = qoffB[f + 1] - qoffB[f];
        for (uint64_t i = a0; i < ia; ++i) {
            uint64_t const pa = a[i].pos, ea = pa + ma, sa = a[i].qidx & 1, lo = pa > maxTlen ? pa - maxTlen : 0, hi = pa + maxTlen;
            auto at = std::partition_point(order.begin(), order.end(), [&](uint32_t x) { return b[x].seq_id < a[i].seq_id || (b[x].seq_id == a[i].seq_id && b[x].pos < lo); });
            for (; at != order.end() && b[*at].seq_id == a[i].seq_id && b[*at].pos <= hi; ++at) {
                Position const& r = b[*at];
                uint64_t const pb = r.pos, eb = pb + mb, sb = r.qidx & 1, tlen = std::max(ea, eb) - std::min(pa, pb);
                if (tlen < minTlen || tlen > maxTlen || sa == sb) continue;
                uint64_t const pf = sa ? pb : pa, ef = sa ? eb : ea, pr = sa ? pa : pb, er = sa ? ea : eb;
                if (pf > pr || ef > er) continue;
                if (pairs < capacity) out[pairs] = Pair{f, tlen, static_cast<uint32_t>(i), *at, a[i].errors + r.errors, pa <= pb ? 1u : 0u};
                ++pairs;
            }
        }
    }
    off[fragments] = pairs;
    return pairs;
}
