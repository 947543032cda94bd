// fmgpu_search_sm.hip — search_hamming_sm::search (search/SearchHammingSM.h): the search-scheme Hamming walk in which a scoring matrix decides, per
// (query symbol, text symbol) pair, whether the pair is a free match, a mismatch that costs one error, or not pairable.  The query alphabet may be larger
// than the index's (IUPAC codes on a DNA index, a 28-letter protein query alphabet on 21 ranks).
//
//  k_scheme_sm   one read per lane, the flat loop over (read, search, node) of k_scheme (fmgpu_search.hip), reads handed out and hit records written by whole
//                waves, the lane-interleaved frame stack in HBM; run_sm is its launcher
//
// What differs from k_scheme: a node owns a SET of children — the members of the query symbol's free mask, then (while an error is left in the part) those of
// its cost mask, each in ascending symbol order and restricted to the symbols that occur in the cursor's interval — so there is no exact tail, no one-row fast
// path and no path key: a lane walks its read alone and `seq` is the callback position itself.  The two mask tables (2 x 256 words) live in LDS; the read is
// staged as whole bytes unless nibbles lose nothing (see run_sm).
#include "fmgpu_search_shared.h"

namespace FMGPU_NS {

constexpr uint32_t kSmRows = 256;            // rows of a mask table as the kernel holds it (rows >= query_sigma are empty: such a byte pairs with nothing)
constexpr uint32_t kSmCostPhase = 32;        // a frame's next child: the symbol (< 32) | this bit if the child is taken from the cost mask

template <class Occ, int MAXSIG>
// (the residency of k_scheme: its LDS allows no more, and the frame here is the same three words)
__global__ __launch_bounds__(256, MAXSIG <= 5 ? (kWide ? 4 : 5) : 1) void k_scheme_sm(Occ fw, Occ rv, SchemeDev sch, const uint32_t* __restrict__ masks,
                                                const uint8_t* __restrict__ qbuf, const uint64_t* __restrict__ qoff, uint64_t nq, idx_t n, uint64_t max_hits,
                                                fmgpu_hit* __restrict__ out, uint64_t cap, Counters* ctr, StackView stk, uint32_t qwords, uint32_t qnib,
                                                const uint32_t* __restrict__ order) {   // masks: free[256] | cost[256]; order (or null): the hand-out order (heavy reads first)
    static_assert(MAXSIG <= 32, "the masks are one word");
    extern __shared__ uint32_t s_query[];
    const QStage qst{s_query, qwords, qnib};
    __shared__ uint8_t s_pi[kMaxSearches * kMaxParts], s_l[kMaxSearches * kMaxParts], s_u[kMaxSearches * kMaxParts];
    __shared__ uint32_t s_part[kMaxParts];
    __shared__ uint32_t s_free[kSmRows], s_cost[kSmRows];
    for (int i = threadIdx.x; i < kMaxSearches * kMaxParts; i += blockDim.x) { s_pi[i] = sch.pi[i]; s_l[i] = sch.l[i]; s_u[i] = sch.u[i]; }
    if (threadIdx.x < kMaxParts) s_part[threadIdx.x] = sch.partition[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < kSmRows; i += blockDim.x) { s_free[i] = masks[i]; s_cost[i] = masks[kSmRows + i]; }
    __syncthreads();

    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t sigma = fw.sigma();
    const uint32_t P = (uint32_t)sch.P, S = (uint32_t)sch.S;
    uint32_t nodes = 0;
    uint64_t tbytes = 0; uint32_t tacc = 0;                         // counted as k_scheme counts them: the blocks of an extend-all, 24 bytes per frame written or read

    const uint32_t lane = threadIdx.x & 63u;
    __shared__ uint32_t s_hb[kWaveHitWords];
    uint32_t nh = 0;
    wave_ring_init(s_hb);
    uint64_t q = 0;
    uint32_t si = 0;                        // current search
    bool idle = false, have_query = false, fresh = false;
    const uint8_t* qs = qbuf; uint32_t m = 0, pbase = 0, prem = 0;
    uint64_t quota = 0; uint32_t seq = 0;
    Cur cur{0, 0, 0};
    uint32_t e = 0, part = 0, qL = 0, qR = 0, pev = 0, sp = 0, resume = kNoResume;      // pev: symbols left in the part; resume: the next child of a frame taken from the stack
    bool right = true;
    const uint8_t *pi = s_pi, *L = s_l, *U = s_u;
    auto part_len = [&](uint32_t p) -> uint32_t {                  // createUniformPartition, expand.h:324-335
        return sch.uniform ? pbase + (p < prem ? 1u : 0u) : s_part[p];
    };
    bool need_search = true;
    auto frame_words = [&](uint64_t& w0, uint64_t& w1, uint64_t& w2, uint32_t nxt) {      // the node the lane stands on as a frame (k_scheme's packing; nxt = phase | symbol in its `nxt` byte)
        if constexpr (kWide) {
            w0 = (uint64_t)cur.lb | ((uint64_t)(pev & 0xffffu) << 40) | ((uint64_t)(e & 0xffu) << 56);
            w1 = (uint64_t)cur.lbRev | ((uint64_t)(qR & 0xffffu) << 40) | ((uint64_t)(nxt & 0xffu) << 56);
            w2 = (uint64_t)cur.len | ((uint64_t)((qL + 1u) & 0xffffu) << 40) | ((uint64_t)(part & 0x7fu) << 56) | ((uint64_t)(right ? 1u : 0u) << 63);
        } else {
            w0 = (uint64_t)cur.lb | ((uint64_t)cur.lbRev << 32);
            w1 = (uint64_t)cur.len | ((uint64_t)(pev & 0xffffu) << 32) | ((uint64_t)(qR & 0xffffu) << 48);
            w2 = (uint64_t)(nxt & 0xffu) | ((uint64_t)(e & 0xffu) << 32) | ((uint64_t)(part & 0x7fu) << 40) |
                 ((uint64_t)(right ? 1u : 0u) << 47) | ((uint64_t)((qL + 1u) & 0xffffu) << 48);
        }
    };
    auto frame_take = [&](uint64_t w0, uint64_t w1, uint64_t w2) {  // stand on a frame's node again
        if constexpr (kWide) {
            const uint64_t m40 = (1ull << 40) - 1ull;
            cur.lb = (idx_t)(w0 & m40); pev = (uint32_t)(w0 >> 40) & 0xffffu; e = (uint32_t)(w0 >> 56) & 0xffu;
            cur.lbRev = (idx_t)(w1 & m40); qR = (uint32_t)(w1 >> 40) & 0xffffu; resume = (uint32_t)(w1 >> 56) & 0xffu;
            cur.len = (idx_t)(w2 & m40); qL = ((uint32_t)(w2 >> 40) & 0xffffu) - 1u; part = (uint32_t)(w2 >> 56) & 0x7fu; right = (w2 >> 63) & 1u;
        } else {
            cur.lb = (idx_t)w0; cur.lbRev = (idx_t)(w0 >> 32);
            cur.len = (idx_t)w1; pev = (uint32_t)(w1 >> 32) & 0xffffu; qR = (uint32_t)(w1 >> 48) & 0xffffu;
            resume = (uint32_t)w2 & 0xffu; e = (uint32_t)(w2 >> 32) & 0xffu; part = (uint32_t)(w2 >> 40) & 0x7fu;
            right = (w2 >> 47) & 1u;
            qL = ((uint32_t)(w2 >> 48) & 0xffffu) - 1u;
        }
    };
    for (;;) {
        // ---- wave-synchronous part: all 64 lanes pass here in every iteration
        const bool want_q = !idle && need_search && !(have_query && si + 1 < S && quota != 0);   // the next search of the read, unless it has its n records
        const uint64_t got = wave_hand_out(want_q, ctr, lane);
        if (want_q) {
            q = got;
            have_query = false;
            if (q >= nq) idle = true;
            else {
                if (order) q = order[q];
                const uint64_t qo = qoff[q];
                m = (uint32_t)(qoff[q + 1] - qo);
                qs = qbuf + qo;
                // a read shorter than the scheme has parts produces nothing (the rule of k_scheme); an explicit partition must cover the read exactly;
                // m <= stk.depth: one frame per consumed symbol at most
                if (m >= P && m <= stk.depth && (sch.uniform || m == sch.psum) && n != 0) { have_query = true; fresh = true; }
            }
        }
        const bool full = wave_ring_fill(s_hb) >= kWaveRingFlush; const uint64_t busy = __ballot(!idle);
        if (full || !busy) wave_flush_hits(s_hb, nh, lane, out, cap, ctr);
        if (!busy) break;
        if (idle) continue;
        if (need_search) {
            if (!have_query) continue;                             // the read fetched was unusable: the next iteration fetches another
            if (fresh) {
                fresh = false; si = 0; quota = max_hits; seq = 0;
                pbase = m / P; prem = m - pbase * P;
                qstage_load(qst, qbuf, qoff[q], m, sigma);
            } else ++si;
            pi = s_pi + si * kMaxParts; L = s_l + si * kMaxParts; U = s_u + si * kMaxParts;
            // Search(): SearchHammingSM.h:65-78 (part 0 is entered with e = 0 <= u[0])
            cur = Cur{0, 0, n};
            e = 0; part = 0; qL = 0; qR = 0; sp = 0; resume = kNoResume;
            for (uint32_t i = 0; i < pi[0]; ++i) { uint32_t pl = part_len(i); qL += pl; qR += pl; }
            qL -= 1;                                               // may wrap; not read until it is valid again
            pev = part_len(pi[0]);
            right = true;                                          // part == 0 -> Right
            need_search = false;
        }
        // invariant here: cur.len > 0, part < P, pev >= 1, `right` set; possibly a frame taken from the stack (resume)
        const Occ& occ = right ? rv : fw;
        const idx_t a = right ? cur.lbRev : cur.lb;
        idx_t lfa[MAXSIG], lfb[MAXSIG];
        occ.template all2<MAXSIG>(a, a + cur.len, lfa, lfb);        // the memory phase
        {
            const bool same = (a >> 6) == ((a + cur.len) >> 6);
            tbytes += (MAXSIG <= 5 ? 64u : 12u * sigma) * (same ? 1u : 2u); tacc += same ? 1u : 2u;
        }
        const uint32_t c = qstage_get(qst, qs, right ? qR : qL) & 255u;
        const uint32_t alive = alive_set<MAXSIG>(lfa, lfb, sigma).w[0];
        const uint32_t Fm = s_free[c], Km = s_cost[c];              // (a byte without a row: both empty)

        // ---- the node's child set: F first, then K, ascending symbols; what is left of it after the child taken now stays on the stack
        const bool resuming = resume != kNoResume;
        const uint32_t Lp = L[part], Up = U[part];
        const bool xOK = e + 1 <= Up;                              // searchPartRightDir (:117-129) vs ...NoErrors (:132-142)
        const bool last = pev == 1;                                // children that would fail l[p] <= e at the part's end (:106) are not made (k_scheme's mOK / sOK)
        // the reference's work: one extend-all, or one extension per free symbol (empty results included)
        if (!resuming) nodes += xOK ? 1u : (uint32_t)__popc(Fm);
        uint32_t Fs = (!last || Lp <= e) ? (Fm & alive) : 0u;
        uint32_t Ks = (xOK && (!last || Lp <= e + 1)) ? (Km & alive) : 0u;
        if (resuming) {
            const uint32_t below = (1u << (resume & 31u)) - 1u;
            if (resume & kSmCostPhase) { Fs = 0u; Ks &= ~below; } else Fs &= ~below;
        }
        const bool ok = (Fs | Ks) != 0u;
        const bool is_cost = Fs == 0u;
        const uint32_t take = (uint32_t)__ffs((int)(is_cost ? Ks : Fs)) - 1u;
        if (is_cost) Ks &= Ks - 1u; else Fs &= Fs - 1u;
        if (ok && (Fs | Ks)) {                                     // (re-)push the node: its remaining children start at nxt
            const uint32_t nxt = Fs ? (uint32_t)__ffs((int)Fs) - 1u : (kSmCostPhase | ((uint32_t)__ffs((int)Ks) - 1u));
            uint64_t w0, w1, w2;
            frame_words(w0, w1, w2, nxt);
            const uint64_t o = (uint64_t)sp * stk.nlanes + gid;     // sp < m <= stk.depth: a node has consumed fewer than m symbols
            stk.p0[o] = w0; stk.p1[o] = w1; stk.p2[o] = w2;
            ++sp; tbytes += 24u; ++tacc;
        }
        resume = kNoResume;
        bool back = !ok, to_next = false;
        if (ok) {
            cur = kid_of<MAXSIG>(lfa, lfb, cur, take, right, sigma);
            if (is_cost) e += 1;
            if (right) ++qR; else --qL;                            // one query symbol consumed
            to_next = --pev == 0;
        }
        if (to_next) {                                             // searchPart, :80-101
            ++part;
            if (part == P) {
                if (L[P - 1] <= e && e <= U[P - 1]) {              // delegate, with the clipping of search_n (SearchNg26.h:412-420)
                    Cur r = cur;
                    if ((uint64_t)r.len > quota) r.len = (idx_t)quota;
                    quota -= r.len;
                    wave_keep_hit(s_hb, nh, out, cap, ctr, q, r, e, seq++);
                    if (quota == 0) { need_search = true; continue; }     // n records: the read's remaining searches are skipped
                }
                back = true;
            } else if (e > U[part]) {
                back = true;
            } else {
                right = pi[part - 1] < pi[part];
                pev = part_len(pi[part]);
            }
        }
        if (back) {
            if (sp == 0) { need_search = true; continue; }
            --sp;
            const uint64_t o = (uint64_t)sp * stk.nlanes + gid;
            const uint64_t w0 = stk.p0[o], w1 = stk.p1[o], w2 = stk.p2[o];
            tbytes += 24u; ++tacc;
            frame_take(w0, w1, w2);
        }
    }
    uint32_t tot = wave_sum(nodes);
    const unsigned long long tb = wave_sum64(tbytes); const uint32_t ta = wave_sum(tacc);
    if ((threadIdx.x & 63u) == 0 && (tot || ta)) {
        atomicAdd(&ctr->nodes, (unsigned long long)tot);
        atomicAdd(&ctr->table_bytes, tb); atomicAdd(&ctr->table_accesses, (unsigned long long)ta);
    }
}

namespace api {
#include "fmgpu_api_decl.h"

// the caller's matrix checked and laid out as the kernel reads it: free[256] | cost[256], rows >= query_sigma empty
static int parse_matrix(const Index* x, const fmgpu_scoring_matrix* matrix, std::vector<uint32_t>& rows) {
    if (!matrix) return fail(FMGPU_ERR_INVALID, "scoring matrix is null");
    if (matrix->query_sigma < 1 || matrix->query_sigma > (int32_t)kSmRows) return fail(FMGPU_ERR_INVALID, "scoring matrix: query_sigma must be in [1, 256]");
    if (!matrix->free_mask || !matrix->cost_mask) return fail(FMGPU_ERR_INVALID, "scoring matrix: free_mask / cost_mask is null");
    const uint32_t valid = x->bwt.sigma >= 32 ? ~0u : (1u << x->bwt.sigma) - 1u;
    rows.assign(2 * kSmRows, 0u);
    for (int32_t c = 0; c < matrix->query_sigma; ++c) {
        const uint32_t f = matrix->free_mask[c], k = matrix->cost_mask[c];
        if ((f | k) & ~valid) return fail(FMGPU_ERR_INVALID, "scoring matrix: query symbol " + std::to_string(c) + " pairs with a text symbol >= sigma = " + std::to_string(x->bwt.sigma));
        if (f & k) return fail(FMGPU_ERR_INVALID, "scoring matrix: the free and the cost mask of query symbol " + std::to_string(c) + " overlap");
        rows[c] = f; rows[kSmRows + c] = k;
    }
    return 0;
}

static int run_sm(Index* x, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* scheme, const fmgpu_scoring_matrix* matrix,
                  uint64_t max_hits, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, hipStream_t stream) {
    if (stats) *stats = fmgpu_stats{};
    if (out_count) *out_count = 0;
    if (nq == 0) return 0;
    if (!qbuf || !qoff || (!out && capacity) || !out_count) return fail(FMGPU_ERR_INVALID, "qbuf / qoff / out / out_count is null");
    const int flags = kernel_flags();                              // the call's options, read once
    const bool heavy_first = opt_on(FMGPU_OPT_HEAVY_FIRST);
    SchemeDev sd{};
    uint32_t max_u = 0;
    bool nothing = false;
    if (int prc = parse_scheme(x, scheme, max_hits, flags, sd, max_u, nothing)) return prc;
    if (scheme->edit != 0) return fail(FMGPU_ERR_INVALID, "search_hamming_sm is a Hamming search: scheme->edit must be 0");
    if (x->bwt.sigma > 32) return fail(FMGPU_ERR_UNSUPPORTED, "search_hamming_sm needs sigma <= 32 (the masks are one word), this index has sigma = " + std::to_string(x->bwt.sigma));
    std::vector<uint32_t> rows;
    if (int mrc = parse_matrix(x, matrix, rows)) return mrc;
    if (nothing) return 0;
    StagedBatch batch;
    int rc;
    if ((rc = batch.stage(qbuf, qoff, nq, out, capacity, stream))) return rc;
    const uint32_t maxlen = batch.maxlen;
    DBuf dmasks;
    if ((rc = dmasks.alloc(rows.size() * 4))) return rc;
    FM_HIP(hipMemcpyAsync(dmasks.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, stream));
    // Read staging.  Nibbles (8 symbols per LDS word, a byte >= sigma as 15 = "pairs with nothing") only where that loses no row of the matrix: sigma <= 15 and no query
    // symbol beyond the index's alphabet has a row.  Otherwise whole bytes, 4 symbols per word: IUPAC code 5..15 on a sigma = 5 index must reach its row.
    // The budget is k_scheme's (64 KB less the static tables and the hit rings: 17 KB, 24 KB with 64-bit rows — the masks' 2 KB fit where k_scheme keeps C);
    // a batch whose longest read does not fit reads global memory.
    const uint32_t qnib = x->bwt.sigma <= 15 && matrix->query_sigma <= x->bwt.sigma ? 1u : 0u;
    uint32_t qwords = qnib ? (maxlen + 7) / 8 : (maxlen + 3) / 4;
    const size_t stage_budget = (size_t)64 * 1024 - (size_t)(kWide ? 24 : 17) * 1024;
    if ((size_t)qwords * 1024 > stage_budget) qwords = 0;
    const size_t lds_bytes = (size_t)qwords * 1024;
    const int bpc = resident_blocks({DfsKernel::scheme_sm, x->bwt.search_family(), x->bwt.sigma, lds_bytes}, 8, [&] {
        int nb = 0;
        dispatch_occ(x->bwt, [&](auto occ, auto ms) {
            if constexpr (decltype(ms)::value <= 32) nb = max_resident_blocks(k_scheme_sm<decltype(occ), decltype(ms)::value>, lds_bytes);
            return 0;
        });
        return nb;
    });
    DfsWorkspace ws;
    EventTimer timer(stream, stats != nullptr);
    const idx_t n = (idx_t)x->bwt.n;
    if ((rc = ws.init(maxlen, nq, bpc, stream))) return rc;
    // the reads of high-copy repeats are handed out first, as for the general kernel of run_dfs (a read whose last 16 symbols hold a code >= sigma is not flagged)
    uint32_t* order = nullptr;
    float prepass_ms = 0.f;
    if (nq >= (1u << 16) && nq < 0x7fffffffull && batch.minlen >= 1 && heavy_first) {
        rc = dispatch_occ(x->bwt, [&](auto occ, auto) { return heavy_first_on_blocks(occ, n, 0u, batch, nq, stream, &order, &prepass_ms); });
        if (rc) return rc;
    }
    FM_HIP(hipMemsetAsync(&ws.ctr->next, 0, 8, stream));           // reads are handed out from 0, one reservation per wave
    timer.start();                                                  // kernel_ms = the search kernel alone
    rc = dispatch_occ(x->bwt, [&](auto occ, auto ms) {
        using O = decltype(occ);
        if constexpr (decltype(ms)::value <= 32)
            k_scheme_sm<O, decltype(ms)::value><<<dim3(ws.grid), dim3(256), lds_bytes, stream>>>(occ, rev_occ<O>(x->rev), sd, dmasks.as<uint32_t>(), batch.q(), batch.off(), nq, n,
                                                                                            max_hits, batch.hits(), capacity, ws.ctr, ws.view, qwords, qnib, order);
        return 0;
    });
    timer.stop();
    return finish_dfs("k_scheme_sm", rc, ws, timer, prepass_ms, batch, capacity, out_count, stats, stream);
}

int fmgpu_search_hamming_sm(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* scheme, const fmgpu_scoring_matrix* matrix,
                            uint64_t max_hits_per_query, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream) {
    Index* x = reinterpret_cast<Index*>(h);
    if (!x) return fail(FMGPU_ERR_INVALID, "index handle is null");
    if (int drc = on_handle_device(x)) return drc;
    return run_sm(x, qbuf, qoff, nq, scheme, matrix, max_hits_per_query, out, capacity, out_count, stats, (hipStream_t)stream);
}

}  // namespace api
}  // namespace FMGPU_NS
