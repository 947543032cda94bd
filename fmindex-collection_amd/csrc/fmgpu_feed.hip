// fmgpu_feed.hip — feeds (include/fmgpu.h: fmgpu_feed_*): a session object bound to one index handle that searches a HOST batch chunk by chunk, with the upload of
// chunk i + 1 and the download of chunk i - 1 running beside the search of chunk i.  A feed owns pinned staging slots, device slots and three streams (upload, compute,
// download); the searches themselves are the routed single-handle calls on device pointers (exact search in the form that takes the chunk's shape from the host
// offsets: no read-back between chunks).  Everything that touches caller memory is host code in fmgpu_feed_host.h.  Nothing here depends on the row width.
//
// One chunk, on the calling thread:   wait for the slot (its previous chunk's download) -> scatter that chunk's results -> stage this chunk into the pinned slot (workers)
//   -> upload stream: H2D offsets + symbols, event U -> compute stream: wait U, search, event C -> download stream: wait C, D2H results, event D.
// Slot s serves chunks s, s + slots, ...: nothing is uploaded into it before event D of its previous chunk has been waited for on the host, which orders every reuse
// of its device and pinned buffers; the only stream-to-stream waits are U -> compute and C -> download.
#include "fmgpu_common.h"
#include "fmgpu_feed_host.h"

#include <memory>

namespace fmgpu {
namespace {

namespace fh = fmgpu_feed_host;

constexpr uint64_t kDefaultChunkReads = 1024 * 1024;         // defaults of fmgpu_feed_config (the sweep of tools/feed_probe.py)
constexpr uint64_t kDefaultChunkSymbols = 128ull << 20;
constexpr int kMaxSlots = 4;

// 0: pageable (or unknown to the runtime), 1: pinned host memory, 2: device / managed memory
int pointer_kind(const void* p) {
    if (!p) return 0;
    hipPointerAttribute_t a;
    std::memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged) return 2;
    return a.type == hipMemoryTypeHost ? 1 : 0;
}

struct Grown {            // a buffer that only ever grows: device memory or pinned host memory
    void* p = nullptr; size_t bytes = 0; bool pinned = false;
    int need(size_t b, uint64_t* tally) {
        if (b <= bytes) return 0;
        release(tally);
        b = (b + 255) & ~(size_t)255;
        hipError_t e = pinned ? hipHostMalloc(&p, b, hipHostMallocDefault) : hipMalloc(&p, b);
        if (e != hipSuccess) { p = nullptr; return hip_fail(e, pinned ? "hipHostMalloc(feed slot)" : "hipMalloc(feed slot)"); }
        bytes = b; *tally += b;
        return 0;
    }
    void release(uint64_t* tally) {
        if (!p) return;
        if (pinned) (void)hipHostFree(p); else (void)hipFree(p);
        if (tally) *tally -= bytes;
        p = nullptr; bytes = 0;
    }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct Slot {
    Grown d_q, d_off, d_lb, d_len, d_hits, d_pos, d_str;     // device (d_pos, d_str: the positions and strata of fmgpu_feed_map)
    Grown p_q, p_off, p_lb, p_len, p_hits, p_pos, p_str;     // pinned
    hipEvent_t ev_up = nullptr, ev_comp = nullptr, ev_down = nullptr;
    bool busy = false;                                       // a chunk is in flight: ev_down has been recorded
    uint64_t first = 0, reads = 0;                           // ... its reads
    uint64_t hits = 0, produced = 0;                         // ... scheme search: its records and the records of the chunks before it
    uint64_t positions = 0, located = 0;                     // ... map: its positions and the positions of the chunks before it
    bool hits_in_place = false, results_in_place = false;
    bool hits_down = false, pos_down = false, pos_in_place = false, str_down = false, str_in_place = false;      // ... map: what its download carries, and where to
    // fmgpu_feed_map_text: the slot's text (the window from byte `headroom` on, the carry in front of it), the parse scratch, the spans and lengths of its reads
    Grown d_text, d_acc, d_lnbase, d_kcnt, d_hcnt, d_tmp, d_ls, d_names, d_quals, d_rlen;
    Grown p_text, p_names, p_quals, p_rlen;
    hipEvent_t ev_text = nullptr;                            // the slot's text has been read: its piece is parsed and what it did not consume is copied out
    uint64_t headroom = 0, unconsumed = 0;                   // ... and where in d_text the unconsumed bytes start
    bool reads_down = false, names_in_place = false, quals_in_place = false, rlen_in_place = false;
    // the strands calls: the slot's doubled batch (fmgpu_strands.hip), made on the device behind the upload or the parse
    Grown d_q2, d_off2;
    uint64_t str_first = 0, str_reads = 0;                   // the chunk's slice of out_stratum (the doubled numbering where both strands are mapped)
    Slot() { p_q.pinned = p_off.pinned = p_lb.pinned = p_len.pinned = p_hits.pinned = p_pos.pinned = p_str.pinned = p_text.pinned = p_names.pinned = p_quals.pinned = p_rlen.pinned = true; }
    std::vector<Grown*> buffers() {
        return {&d_q, &d_off, &d_lb, &d_len, &d_hits, &d_pos, &d_str, &p_q, &p_off, &p_lb, &p_len, &p_hits, &p_pos, &p_str,
                &d_text, &d_acc, &d_lnbase, &d_kcnt, &d_hcnt, &d_tmp, &d_ls, &d_names, &d_quals, &d_rlen, &p_text, &p_names, &p_quals, &p_rlen,
                &d_q2, &d_off2};
    }
};

}  // namespace
}  // namespace fmgpu

struct fmgpu_feed {
    uint32_t magic = 0x46454544u;                            // "FEED"
    fmgpu_index_t h = nullptr;
    int32_t device = 0, sigma = 0, nibbles = 0;              // nibbles: exact search reads the 4-bit packed form itself on this handle
    uint64_t chunk_reads = 0, chunk_symbols = 0;
    int32_t slots = 2, pack4 = 0;
    std::unique_ptr<fmgpu_feed_host::Workers> workers;
    hipStream_t up = nullptr, comp = nullptr, down = nullptr;
    fmgpu::Slot slot[fmgpu::kMaxSlots];
    std::vector<uint64_t> plan;                              // first read of every chunk of the current call, and nq behind them
    uint64_t hit_hint = 0;                                   // records the largest chunk so far produced: what a slot's hit buffer is sized for before it runs
    fmgpu::Grown d_table;                                    // fmgpu_feed_map_text: the call's symbol table
    fmgpu::Grown d_comp;                                     // the strands calls: the call's complement table (256 entries), and its host side (it outlives the copy)
    uint8_t comp_host[256] = {};
    uint64_t pinned_bytes = 0, device_bytes = 0, last_chunks = 0, last_staged = 0, last_uploaded = 0;
};

namespace fmgpu {
namespace {

using Feed = ::fmgpu_feed;

void drain(Feed* f) {
    for (hipStream_t s : {f->up, f->comp, f->down}) if (s && hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
    for (int s = 0; s < f->slots; ++s) f->slot[s].busy = false;
}

int check_feed(Feed* f) {
    if (!f || f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return fail(FMGPU_ERR_NO_DEVICE, "no HIP device visible — the product path has no CPU fallback"); }
    if (dev != f->device) return fail(FMGPU_ERR_INVALID, "the handle lives on device " + std::to_string(f->device) + ", the calling thread's current device is " + std::to_string(dev));
    return 0;
}

// what one call searches: a flat byte batch, a flat packed batch or scattered reads
struct Batch {
    const uint8_t* qbuf = nullptr; const uint64_t* qoff = nullptr;       // flat
    const uint8_t* const* reads = nullptr; const uint64_t* lens = nullptr; // scattered
    uint64_t nq = 0;
    bool q4 = false;                                                     // the caller's batch is packed
    bool in_pinned = false;                                              // flat: qbuf is pinned memory (copied from where it lies)
};

// the plan of a call and the largest chunk: every offset is checked (non-decreasing) by the workers, the chunks are then cut by bisection
int make_plan(Feed* f, const Batch& b, uint64_t* max_reads, uint64_t* max_symbols) {
    f->plan.clear();
    uint64_t mr = 0, ms = 0;
    if (b.qoff) {
        std::vector<fh::Shape> part(f->workers->parts());
        f->workers->run([&](uint32_t t, uint32_t parts) { part[t] = fh::shape_of_offsets(b.qoff, fh::slice_cut(b.nq, parts, t), fh::slice_cut(b.nq, parts, t + 1)); });
        for (const fh::Shape& s : part) if (!s.ok) return fail(FMGPU_ERR_INVALID, "qoff is not non-decreasing");
        for (uint64_t first = 0; first < b.nq;) {
            const uint64_t end = fh::chunk_end(b.qoff, b.nq, first, f->chunk_reads, f->chunk_symbols);
            f->plan.push_back(first);
            mr = std::max(mr, end - first); ms = std::max(ms, b.qoff[end] - b.qoff[first]);
            first = end;
        }
    } else {                                                             // scattered reads: the same rule over the lengths
        for (uint64_t first = 0; first < b.nq;) {
            uint64_t end = first, sym = 0;
            while (end < b.nq && end - first < f->chunk_reads) {
                const uint64_t len = b.lens[end];
                if (end > first && len > f->chunk_symbols - sym) break;  // (sym <= chunk_symbols here: only a chunk's first read may be longer)
                if (len && !b.reads[end]) return fail(FMGPU_ERR_INVALID, "reads[" + std::to_string(end) + "] is null");
                sym += len; ++end;
                if (sym > f->chunk_symbols) break;                       // one over-long read: a chunk of its own
            }
            f->plan.push_back(first);
            mr = std::max(mr, end - first); ms = std::max(ms, sym);
            first = end;
        }
    }
    f->plan.push_back(b.nq);
    *max_reads = mr; *max_symbols = ms;
    return 0;
}

// every slot sized for the largest chunk of this call (buffers only ever grow)
int size_slots(Feed* f, uint64_t max_reads, uint64_t max_symbols, bool exact, bool out_pinned, bool in_pinned) {
    const size_t qbytes = (size_t)max_symbols + 64, obytes = ((size_t)max_reads + 1) * 8, rbytes = (size_t)max_reads * 8;
    const int used = (int)std::min<uint64_t>((uint64_t)f->slots, f->plan.size() - 1);
    for (int s = 0; s < used; ++s) {
        Slot& sl = f->slot[s];
        int rc;
        if ((rc = sl.d_q.need(qbytes, &f->device_bytes)) || (rc = sl.d_off.need(obytes, &f->device_bytes)) || (rc = sl.p_off.need(obytes, &f->pinned_bytes))) return rc;
        if (!in_pinned && (rc = sl.p_q.need(qbytes, &f->pinned_bytes))) return rc;
        if (exact) {
            if ((rc = sl.d_lb.need(rbytes, &f->device_bytes)) || (rc = sl.d_len.need(rbytes, &f->device_bytes))) return rc;
            if (!out_pinned && ((rc = sl.p_lb.need(rbytes, &f->pinned_bytes)) || (rc = sl.p_len.need(rbytes, &f->pinned_bytes)))) return rc;
        }
        for (hipEvent_t* ev : {&sl.ev_up, &sl.ev_comp, &sl.ev_down}) if (!*ev) FM_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    return 0;
}

// what staging a chunk leaves behind for its search
struct Staged1 {
    uint64_t reads = 0, total = 0;
    uint32_t longest = 0, shortest = 0;
    const uint8_t* dq = nullptr;          // what the search is handed as qbuf
    bool nibbles = false;                 // the slot holds nibbles
};

// stage chunk c into slot sl and enqueue its upload; the slot is free
int upload_chunk(Feed* f, const Batch& b, Slot& sl, uint64_t c, bool want_nibbles, Staged1* out) {
    const uint64_t first = f->plan[c], end = f->plan[c + 1], n = end - first;
    uint64_t* poff = sl.p_off.as<uint64_t>();
    uint8_t* pq = sl.p_q.as<uint8_t>();
    uint8_t* dq = sl.d_q.as<uint8_t>();
    fh::Workers& w = *f->workers;
    std::vector<fh::Shape> part(w.parts());
    size_t qbytes = 0, qskip = 0;          // bytes of the slot that travel, from byte qskip on
    const void* qsrc = nullptr;            // ... and where they lie
    Staged1 st;
    st.reads = n;
    if (b.qoff) {
        const uint64_t s0 = b.qoff[first], s1 = b.qoff[end], origin = fh::slot_origin(s0), sym = s1 - s0;
        const bool pack = want_nibbles && !b.q4;
        st.nibbles = b.q4 || pack;
        if (b.q4) { qskip = (size_t)((s0 >> 1) - (origin >> 1)); qbytes = (size_t)fh::packed_bytes(s0, s1); }
        else if (pack) { qskip = (size_t)((s0 - origin) >> 1); qbytes = (size_t)fh::packed_bytes(s0 - origin, s1 - origin); }
        else { qskip = (size_t)(s0 - origin); qbytes = (size_t)sym; }
        const bool in_place = b.in_pinned && !pack;
        w.run([&](uint32_t t, uint32_t parts) {
            const uint64_t r0 = fh::slice_cut(n, parts, t), r1 = fh::slice_cut(n, parts, t + 1);
            part[t] = fh::shape_of_offsets(b.qoff, first + r0, first + r1);
            fh::stage_offsets(b.qoff, first, origin, r0, t + 1 == parts ? n + 1 : r1, poff);
            if (in_place) return;
            if (b.q4) fh::stage_packed(b.qbuf, s0, origin, fh::slice_cut(qbytes, parts, t), fh::slice_cut(qbytes, parts, t + 1), pq);
            else if (pack) fh::pack_nibbles(b.qbuf + s0, fh::slice_cut(sym, parts, t, s0 - origin, 2), fh::slice_cut(sym, parts, t + 1, s0 - origin, 2), (uint32_t)f->sigma, s0 - origin, pq);
            else fh::stage_bytes(b.qbuf, s0, origin, fh::slice_cut(sym, parts, t), fh::slice_cut(sym, parts, t + 1), pq);
        });
        qsrc = in_place ? (const void*)(b.qbuf + (b.q4 ? (s0 >> 1) : s0)) : (const void*)(pq + qskip);
        if (!in_place) f->last_staged += qbytes;
    } else {
        st.nibbles = want_nibbles;
        fh::stage_lengths(b.lens, first, n, poff);
        const uint64_t sym = poff[n];
        const uint64_t align = want_nibbles ? 2 : 1;
        w.run([&](uint32_t t, uint32_t parts) {
            part[t] = fh::shape_of_lengths(b.lens, first + fh::slice_cut(n, parts, t), first + fh::slice_cut(n, parts, t + 1));
            fh::gather_reads(b.reads, first, poff, n, fh::slice_cut(sym, parts, t, 0, align), fh::slice_cut(sym, parts, t + 1, 0, align), want_nibbles ? (uint32_t)f->sigma : 0u, pq);
        });
        qbytes = (size_t)(want_nibbles ? (sym + 1) / 2 : sym);
        qsrc = pq;
        f->last_staged += qbytes;
    }
    fh::Shape shape;
    for (const fh::Shape& s : part) shape.merge(s);
    if (shape.longest > 0xffffffffull) return fail(FMGPU_ERR_UNSUPPORTED, "a read of 2^32 symbols or more");
    st.total = poff[n];                    // the slot's last offset: what the kernels' qoff[nq] is
    st.longest = (uint32_t)shape.longest; st.shortest = n ? (uint32_t)shape.shortest : 0u;
    st.dq = dq;
    if (qskip + qbytes + 32 > sl.d_q.bytes) return fail(FMGPU_ERR_HIP, "feed: a chunk outgrew its slot");
    FM_HIP(hipMemcpyAsync(sl.d_off.p, poff, (n + 1) * 8, hipMemcpyHostToDevice, f->up));
    if (qbytes) FM_HIP(hipMemcpyAsync(dq + qskip, qsrc, qbytes, hipMemcpyHostToDevice, f->up));
    FM_HIP(hipEventRecord(sl.ev_up, f->up));
    f->last_uploaded += (n + 1) * 8 + qbytes;
    *out = st;
    return 0;
}

// wait for the chunk a slot holds and hand its results to the caller
int retire_exact(Feed* f, Slot& sl, uint64_t* out_lb, uint64_t* out_len) {
    if (!sl.busy) return 0;
    FM_HIP(hipEventSynchronize(sl.ev_down));
    sl.busy = false;
    if (sl.results_in_place) return 0;
    const uint64_t* plb = sl.p_lb.as<uint64_t>(); const uint64_t* pln = sl.p_len.as<uint64_t>();
    const uint64_t first = sl.first, n = sl.reads;
    f->workers->run([&](uint32_t t, uint32_t parts) { fh::scatter_intervals(plb, pln, first, fh::slice_cut(n, parts, t), fh::slice_cut(n, parts, t + 1), out_lb, out_len); });
    f->last_staged += n * 16;
    return 0;
}
int retire_hits(Feed* f, Slot& sl, fmgpu_hit* out, uint64_t capacity) {
    if (!sl.busy) return 0;
    FM_HIP(hipEventSynchronize(sl.ev_down));
    sl.busy = false;
    if (!sl.hits || sl.produced + sl.hits > capacity) return 0;          // (records beyond the caller's capacity are counted, not written)
    const fmgpu_hit* src = sl.hits_in_place ? out + sl.produced : sl.p_hits.as<fmgpu_hit>();
    const uint64_t first = sl.first, n = sl.hits, produced = sl.produced;
    f->workers->run([&](uint32_t t, uint32_t parts) { fh::scatter_hits(src, fh::slice_cut(n, parts, t), fh::slice_cut(n, parts, t + 1), first, out, produced); });
    if (!sl.hits_in_place) f->last_staged += n * sizeof(fmgpu_hit);
    return 0;
}

void add_stats(fmgpu_stats* sum, const fmgpu_stats& st) {
    sum->lf_steps += st.lf_steps; sum->hits += st.hits; sum->kernel_ms += st.kernel_ms; sum->prepass_ms += st.prepass_ms;
    sum->table_bytes += st.table_bytes; sum->table_accesses += st.table_accesses; sum->table_steps += st.table_steps;
}

int begin_call(Feed* f) {
    f->last_chunks = f->last_staged = f->last_uploaded = 0;
    return 0;
}

int run_exact(Feed* f, const Batch& b, uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats) {
    if (stats) *stats = fmgpu_stats{};
    begin_call(f);
    const bool out_pinned = pointer_kind(out_lb) == 1 && pointer_kind(out_len) == 1;
    const bool want_nibbles = !b.q4 && f->pack4 && f->sigma <= 15 && f->nibbles;
    uint64_t max_reads = 0, max_symbols = 0;
    int rc;
    if ((rc = make_plan(f, b, &max_reads, &max_symbols))) return rc;
    if ((rc = size_slots(f, max_reads, max_symbols, true, out_pinned, b.in_pinned && !want_nibbles))) return rc;
    const uint64_t chunks = f->plan.size() - 1;
    f->last_chunks = chunks;
    auto body = [&]() -> int {
        for (uint64_t c = 0; c < chunks; ++c) {
            Slot& sl = f->slot[c % (uint64_t)f->slots];
            int r;
            if ((r = retire_exact(f, sl, out_lb, out_len))) return r;
            Staged1 st;
            if ((r = upload_chunk(f, b, sl, c, want_nibbles, &st))) return r;
            FM_HIP(hipStreamWaitEvent(f->comp, sl.ev_up, 0));
            fmgpu_stats cs{};
            if ((r = search_exact_shaped(f->h, st.dq, sl.d_off.as<uint64_t>(), st.reads, sl.d_lb.as<uint64_t>(), sl.d_len.as<uint64_t>(), stats ? &cs : nullptr, f->comp,
                                         st.nibbles ? 1 : 0, st.total, st.longest, st.shortest))) return r;
            if (stats) add_stats(stats, cs);
            FM_HIP(hipEventRecord(sl.ev_comp, f->comp));
            FM_HIP(hipStreamWaitEvent(f->down, sl.ev_comp, 0));
            sl.first = f->plan[c]; sl.reads = st.reads; sl.results_in_place = out_pinned;
            uint64_t* tlb = out_pinned ? out_lb + sl.first : sl.p_lb.as<uint64_t>();
            uint64_t* tln = out_pinned ? out_len + sl.first : sl.p_len.as<uint64_t>();
            FM_HIP(hipMemcpyAsync(tlb, sl.d_lb.p, st.reads * 8, hipMemcpyDeviceToHost, f->down));
            FM_HIP(hipMemcpyAsync(tln, sl.d_len.p, st.reads * 8, hipMemcpyDeviceToHost, f->down));
            FM_HIP(hipEventRecord(sl.ev_down, f->down));
            sl.busy = true;
        }
        for (uint64_t k = 0; k < (uint64_t)f->slots; ++k) {              // the chunks still in flight, oldest first
            Slot& sl = f->slot[(chunks + k) % (uint64_t)f->slots];
            if (int r = retire_exact(f, sl, out_lb, out_len)) return r;
        }
        return 0;
    };
    rc = body();
    if (rc) drain(f);
    return rc;
}

int run_scheme(Feed* f, const Batch& b, const fmgpu_scheme* scheme, uint64_t max_hits, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats) {
    if (stats) *stats = fmgpu_stats{};
    *out_count = 0;
    begin_call(f);
    const bool out_pinned = capacity && pointer_kind(out) == 1;
    uint64_t max_reads = 0, max_symbols = 0;
    int rc;
    if ((rc = make_plan(f, b, &max_reads, &max_symbols))) return rc;
    if ((rc = size_slots(f, max_reads, max_symbols, false, out_pinned, b.in_pinned))) return rc;
    const uint64_t chunks = f->plan.size() - 1;
    f->last_chunks = chunks;
    uint64_t produced = 0;
    auto body = [&]() -> int {
        for (uint64_t c = 0; c < chunks; ++c) {
            Slot& sl = f->slot[c % (uint64_t)f->slots];
            int r;
            if ((r = retire_hits(f, sl, out, capacity))) return r;
            Staged1 st;
            if ((r = upload_chunk(f, b, sl, c, false, &st))) return r;
            FM_HIP(hipStreamWaitEvent(f->comp, sl.ev_up, 0));
            // the slot's hit buffer: two records per read to begin with, what the largest chunk so far produced once one is known; too small for this chunk, it is
            // grown to the count the search reported and the chunk runs again
            uint64_t cnt = 0;
            fmgpu_stats cs{};
            for (int attempt = 0;; ++attempt) {
                const uint64_t want = std::max<uint64_t>(std::max<uint64_t>(16, 2 * st.reads), std::max(f->hit_hint, cnt));
                if ((r = sl.d_hits.need((size_t)want * sizeof(fmgpu_hit), &f->device_bytes))) return r;
                const uint64_t cap = sl.d_hits.bytes / sizeof(fmgpu_hit);
                r = ::fmgpu_search_scheme(f->h, st.dq, sl.d_off.as<uint64_t>(), st.reads, scheme, max_hits, sl.d_hits.as<fmgpu_hit>(), cap, &cnt, stats ? &cs : nullptr, f->comp);
                if (r == FMGPU_ERR_CAPACITY && attempt == 0 && cnt > cap) continue;
                if (r) return r;
                break;
            }
            f->hit_hint = std::max(f->hit_hint, cnt + cnt / 4);
            if (stats) add_stats(stats, cs);
            FM_HIP(hipEventRecord(sl.ev_comp, f->comp));
            FM_HIP(hipStreamWaitEvent(f->down, sl.ev_comp, 0));
            sl.first = f->plan[c]; sl.reads = st.reads; sl.hits = cnt; sl.produced = produced;
            const bool fits = produced + cnt <= capacity;
            sl.hits_in_place = out_pinned && fits;
            if (cnt && fits) {
                fmgpu_hit* target = out + produced;
                if (!sl.hits_in_place) {
                    if ((r = sl.p_hits.need((size_t)cnt * sizeof(fmgpu_hit), &f->pinned_bytes))) return r;
                    target = sl.p_hits.as<fmgpu_hit>();
                }
                FM_HIP(hipMemcpyAsync(target, sl.d_hits.p, (size_t)cnt * sizeof(fmgpu_hit), hipMemcpyDeviceToHost, f->down));
            }
            FM_HIP(hipEventRecord(sl.ev_down, f->down));
            sl.busy = true;
            produced += cnt;
        }
        for (uint64_t k = 0; k < (uint64_t)f->slots; ++k) {
            Slot& sl = f->slot[(chunks + k) % (uint64_t)f->slots];
            if (int r = retire_hits(f, sl, out, capacity)) return r;
        }
        return 0;
    };
    rc = body();
    if (rc) { drain(f); return rc; }
    *out_count = produced;
    if (produced > capacity) return fail(FMGPU_ERR_CAPACITY, "result buffer holds " + std::to_string(capacity) + " records, " + std::to_string(produced) + " produced");
    return 0;
}

int no_device_memory(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs) if (pointer_kind(p) == 2) return fail(FMGPU_ERR_INVALID, "a feed takes host memory only: an argument is device memory");
    return 0;
}

// ---- fmgpu_feed_map: fmgpu_map's chain (map_device, fmgpu_map.hip) per chunk on the slot's buffers
struct SlotBuffer : MapBuffer {                                          // a slot's device buffer as the chain's growing scratch
    Grown* g; uint64_t* tally;
    SlotBuffer(Grown* g_, uint64_t* tally_) : g(g_), tally(tally_) { p = g->p; bytes = g->bytes; }
    int need(size_t nbytes) override {
        const int rc = g->need(nbytes, tally);
        p = g->p; bytes = g->bytes;
        return rc;
    }
};

struct MapOut {                                                          // the caller's arrays
    fmgpu_position* out; uint64_t capacity;
    fmgpu_hit* out_hits; uint64_t hits_capacity;
    uint8_t* out_stratum;
};

// wait for the chunk a slot holds and hand what came through the pinned slot to the caller
int retire_map(Feed* f, Slot& sl, const MapOut& o) {
    if (!sl.busy) return 0;
    FM_HIP(hipEventSynchronize(sl.ev_down));
    sl.busy = false;
    fh::Workers& w = *f->workers;
    const auto copy = [&](void* dst, const void* src, size_t bytes) {
        w.run([&](uint32_t t, uint32_t parts) {
            const size_t a = (size_t)fh::slice_cut(bytes, parts, t), b = (size_t)fh::slice_cut(bytes, parts, t + 1);
            if (b > a) std::memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, b - a);
        });
        f->last_staged += bytes;
    };
    if (sl.hits_down && !sl.hits_in_place) copy(o.out_hits + sl.produced, sl.p_hits.p, (size_t)sl.hits * sizeof(fmgpu_hit));
    if (sl.pos_down && !sl.pos_in_place) copy(o.out + sl.located, sl.p_pos.p, (size_t)sl.positions * sizeof(fmgpu_position));
    if (sl.str_down && !sl.str_in_place) copy(o.out_stratum + sl.str_first, sl.p_str.p, (size_t)sl.str_reads);
    return 0;
}

// the call's complement table on the device, in front of the first chunk on the compute stream
int upload_complement(Feed* f, const fmgpu_strands* strands) {
    strands_table(strands->complement, strands->n, f->comp_host);
    if (int rc = f->d_comp.need(256, &f->device_bytes)) return rc;
    FM_HIP(hipMemcpyAsync(f->d_comp.p, f->comp_host, 256, hipMemcpyHostToDevice, f->comp));
    return 0;
}

// strands != null: every chunk is doubled on the device (strands_device) behind its upload and mapped as 2 x reads; records and strata count in the doubled numbering
int run_map(Feed* f, const Batch& b, const fmgpu_map_query* what, const fmgpu_strands* strands, const MapOut& o, uint64_t* out_count, uint64_t* out_hit_count,
            fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    begin_call(f);
    const uint64_t mult = strands ? 2 : 1;
    const bool pos_pinned = o.capacity && pointer_kind(o.out) == 1, hits_pinned = o.hits_capacity && pointer_kind(o.out_hits) == 1;
    const bool str_pinned = o.out_stratum && pointer_kind(o.out_stratum) == 1;
    const int32_t nstats = std::max(1, what->n_schemes);
    uint64_t max_reads = 0, max_symbols = 0;
    int rc;
    if ((rc = make_plan(f, b, &max_reads, &max_symbols))) return rc;
    if ((rc = size_slots(f, max_reads, max_symbols, false, true, b.in_pinned))) return rc;
    const uint64_t chunks = f->plan.size() - 1;
    f->last_chunks = chunks;
    if (strands && (rc = upload_complement(f, strands))) return rc;
    uint64_t produced = 0, located = 0;
    std::vector<fmgpu_stats> cs((size_t)nstats);
    auto body = [&]() -> int {
        for (uint64_t c = 0; c < chunks; ++c) {
            Slot& sl = f->slot[c % (uint64_t)f->slots];
            int r;
            if ((r = retire_map(f, sl, o))) return r;
            Staged1 st;
            if ((r = upload_chunk(f, b, sl, c, false, &st))) return r;
            const uint64_t nreads = mult * st.reads;
            if (o.out_stratum && (r = sl.d_str.need((size_t)nreads, &f->device_bytes))) return r;
            FM_HIP(hipStreamWaitEvent(f->comp, sl.ev_up, 0));
            const uint8_t* mq = st.dq;
            const uint64_t* moff = sl.d_off.as<uint64_t>();
            if (strands) {
                SlotBuffer bq2(&sl.d_q2, &f->device_bytes), boff2(&sl.d_off2, &f->device_bytes);
                if ((r = strands_device(st.dq, sl.d_off.as<uint64_t>(), st.reads, f->d_comp.as<uint8_t>(), &bq2, &boff2, f->comp))) return r;
                mq = sl.d_q2.as<uint8_t>(); moff = sl.d_off2.as<uint64_t>();
            }
            // the chain on the slot's buffers (they only ever grow; a stage that overflows one grows it and runs again), then the chunk's records renumbered for the batch
            SlotBuffer bh(&sl.d_hits, &f->device_bytes), bp(&sl.d_pos, &f->device_bytes), bi(&sl.d_lb, &f->device_bytes);
            uint64_t cnt = 0, pcnt = 0;
            fmgpu_stats ls{};
            if ((r = map_device(f->h, mq, moff, nreads, what, false, &bh, &bp, &bi, o.out_stratum ? sl.d_str.as<uint8_t>() : nullptr,
                                search_stats ? cs.data() : nullptr, locate_stats ? &ls : nullptr, f->comp, &cnt, &pcnt, strands && strands->pair != 0))) return r;
            if ((r = map_rebase(sl.d_hits.as<fmgpu_hit>(), cnt, sl.d_pos.as<fmgpu_position>(), pcnt, mult * f->plan[c], produced, f->comp))) return r;
            if (search_stats) for (int32_t i = 0; i < nstats; ++i) add_stats(&search_stats[i], cs[(size_t)i]);
            if (locate_stats) add_stats(locate_stats, ls);
            FM_HIP(hipEventRecord(sl.ev_comp, f->comp));
            FM_HIP(hipStreamWaitEvent(f->down, sl.ev_comp, 0));
            sl.first = f->plan[c]; sl.reads = st.reads; sl.hits = cnt; sl.produced = produced; sl.positions = pcnt; sl.located = located;
            sl.str_first = mult * sl.first; sl.str_reads = nreads;
            // records beyond the caller's capacity are counted, not written
            sl.hits_down = o.out_hits && cnt && produced + cnt <= o.hits_capacity; sl.hits_in_place = hits_pinned;
            sl.pos_down = pcnt && located + pcnt <= o.capacity; sl.pos_in_place = pos_pinned;
            sl.str_down = o.out_stratum != nullptr; sl.str_in_place = str_pinned;
            if (sl.hits_down) {
                void* target = o.out_hits + produced;
                if (!hits_pinned) { if ((r = sl.p_hits.need((size_t)cnt * sizeof(fmgpu_hit), &f->pinned_bytes))) return r; target = sl.p_hits.p; }
                FM_HIP(hipMemcpyAsync(target, sl.d_hits.p, (size_t)cnt * sizeof(fmgpu_hit), hipMemcpyDeviceToHost, f->down));
            }
            if (sl.pos_down) {
                void* target = o.out + located;
                if (!pos_pinned) { if ((r = sl.p_pos.need((size_t)pcnt * sizeof(fmgpu_position), &f->pinned_bytes))) return r; target = sl.p_pos.p; }
                FM_HIP(hipMemcpyAsync(target, sl.d_pos.p, (size_t)pcnt * sizeof(fmgpu_position), hipMemcpyDeviceToHost, f->down));
            }
            if (sl.str_down) {
                void* target = o.out_stratum + sl.str_first;
                if (!str_pinned) { if ((r = sl.p_str.need((size_t)nreads, &f->pinned_bytes))) return r; target = sl.p_str.p; }
                FM_HIP(hipMemcpyAsync(target, sl.d_str.p, (size_t)nreads, hipMemcpyDeviceToHost, f->down));
            }
            FM_HIP(hipEventRecord(sl.ev_down, f->down));
            sl.busy = true;
            produced += cnt; located += pcnt;
        }
        for (uint64_t k = 0; k < (uint64_t)f->slots; ++k) {
            Slot& sl = f->slot[(chunks + k) % (uint64_t)f->slots];
            if (int r = retire_map(f, sl, o)) return r;
        }
        return 0;
    };
    rc = body();
    if (rc) { drain(f); return rc; }
    *out_count = located;
    if (out_hit_count) *out_hit_count = produced;
    if (located > o.capacity) return fail(FMGPU_ERR_CAPACITY, "position buffer holds " + std::to_string(o.capacity) + " records, " + std::to_string(located) + " produced");
    if (o.out_hits && produced > o.hits_capacity) return fail(FMGPU_ERR_CAPACITY, "hit buffer holds " + std::to_string(o.hits_capacity) + " records, " + std::to_string(produced) + " produced");
    return 0;
}

// ---- fmgpu_feed_map_text: the raw text travels, piece by piece; every piece is parsed (parse_device, fmgpu_parse.hip) and mapped (map_device) on the compute stream
// One piece c in slot s = c % slots, on the calling thread:
//   compute: D2D the carry (what piece c - 1 left) from slot s - 1 into [H - carry, H) of slot s, event T(s - 1)           -> slot s - 1 may take its next window
//   upload : window c + 1 into slot s + 1 at byte H (after that slot's download D has been waited for and behind its T), event U(s + 1)
//   compute: wait U(s), parse [H - carry, H + window), event T(s), map, rebase of records and spans, event C -> download: wait C, D2H, event D
// A window's place does not depend on a parse result: its upload runs beside the parse and the search of the piece before it.
struct TextOut {
    MapOut m;
    fmgpu_text_span* names; fmgpu_text_span* quals; uint64_t* lens;
    uint64_t read_capacity;
    bool read_arrays() const { return m.out_stratum || names || quals || lens; }
};

int retire_text(Feed* f, Slot& sl, const TextOut& o) {
    if (!sl.busy) return 0;
    const bool reads_down = sl.reads_down;
    const uint64_t first = sl.first, reads = sl.reads;
    if (int rc = retire_map(f, sl, o.m)) return rc;
    if (!reads_down || !reads) return 0;
    fh::Workers& w = *f->workers;
    const auto copy = [&](void* dst, const void* src, size_t bytes) {
        w.run([&](uint32_t t, uint32_t parts) {
            const size_t a = (size_t)fh::slice_cut(bytes, parts, t), b = (size_t)fh::slice_cut(bytes, parts, t + 1);
            if (b > a) std::memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, b - a);
        });
        f->last_staged += bytes;
    };
    if (o.names && !sl.names_in_place) copy(o.names + first, sl.p_names.p, (size_t)reads * sizeof(fmgpu_text_span));
    if (o.quals && !sl.quals_in_place) copy(o.quals + first, sl.p_quals.p, (size_t)reads * sizeof(fmgpu_text_span));
    if (o.lens && !sl.rlen_in_place) copy(o.lens + first, sl.p_rlen.p, (size_t)reads * 8);
    return 0;
}

// a carry longer than the slot's headroom: a larger text buffer with the window (already uploaded) moved to its new place.  Rare, and synchronised.
int regrow_text(Feed* f, Slot& sl, uint64_t carry, uint64_t window) {
    const uint64_t H = fh::text_headroom_for(sl.headroom, carry);
    FM_HIP(hipStreamSynchronize(f->up));
    FM_HIP(hipStreamSynchronize(f->comp));
    Grown fresh;
    if (int rc = fresh.need((size_t)(H + std::max<uint64_t>(window, sl.d_text.bytes - std::min<uint64_t>(sl.d_text.bytes, sl.headroom)) + 32), &f->device_bytes)) return rc;
    if (window) {
        const hipError_t e = hipMemcpy(fresh.as<uint8_t>() + H, sl.d_text.as<uint8_t>() + sl.headroom, (size_t)window, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { fresh.release(&f->device_bytes); return hip_fail(e, "hipMemcpy(feed text regrow)"); }
    }
    sl.d_text.release(&f->device_bytes);
    sl.d_text = fresh;
    sl.headroom = H;
    return 0;
}

int run_map_text(Feed* f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final, const uint8_t* symbol_of, uint64_t B, const fmgpu_map_query* what,
                 const fmgpu_strands* strands, const TextOut& o, uint64_t* out_count, uint64_t* out_hit_count, fmgpu_parse_result* result, fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    begin_call(f);
    const bool in_pinned = pointer_kind(text) == 1;
    const bool pos_pinned = o.m.capacity && pointer_kind(o.m.out) == 1, hits_pinned = o.m.hits_capacity && pointer_kind(o.m.out_hits) == 1;
    const bool str_pinned = o.m.out_stratum && pointer_kind(o.m.out_stratum) == 1;
    const bool names_pinned = o.names && pointer_kind(o.names) == 1, quals_pinned = o.quals && pointer_kind(o.quals) == 1, lens_pinned = o.lens && pointer_kind(o.lens) == 1;
    const int32_t nstats = std::max(1, what->n_schemes);
    const uint64_t windows = fh::text_windows(bytes, B), slots = (uint64_t)f->slots;
    f->last_chunks = windows;
    const uint64_t widest = std::min(B, bytes);
    int rc;
    for (uint64_t s = 0; s < std::min(slots, windows); ++s) {
        Slot& sl = f->slot[s];
        sl.headroom = std::max(sl.headroom, fh::text_headroom(B));
        if ((rc = sl.d_text.need((size_t)(sl.headroom + widest + 32), &f->device_bytes))) return rc;
        if (!in_pinned && (rc = sl.p_text.need((size_t)widest, &f->pinned_bytes))) return rc;
        for (hipEvent_t* ev : {&sl.ev_up, &sl.ev_comp, &sl.ev_down, &sl.ev_text}) if (!*ev) FM_HIP(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    }
    if ((rc = f->d_table.need(256, &f->device_bytes))) return rc;
    FM_HIP(hipMemcpyAsync(f->d_table.p, symbol_of, 256, hipMemcpyHostToDevice, f->comp));
    if (strands && (rc = upload_complement(f, strands))) return rc;
    const uint64_t mult = strands ? 2 : 1;

    fmgpu_parse_result total;
    std::memset(&total, 0, sizeof total);
    uint64_t produced = 0, located = 0, carry = 0, line_base = 0;         // total.consumed: the offset of the current piece in `text`
    std::vector<fmgpu_stats> cs((size_t)nstats);
    bool text_error = false;

    const auto upload = [&](uint64_t c) -> int {                          // window c into its slot, once the slot is free
        Slot& sl = f->slot[c % slots];
        if (int r = retire_text(f, sl, o)) return r;
        const uint64_t w0 = fh::text_window_begin(c, B), len = fh::text_window_end(bytes, c, B) - w0;
        const uint8_t* src = text + w0;
        if (!in_pinned) {
            uint8_t* pt = sl.p_text.as<uint8_t>();
            f->workers->run([&](uint32_t t, uint32_t parts) {
                const size_t a = (size_t)fh::slice_cut(len, parts, t), b = (size_t)fh::slice_cut(len, parts, t + 1);
                if (b > a) std::memcpy(pt + a, src + a, b - a);
            });
            src = pt;
            f->last_staged += len;
        }
        if (sl.headroom + len + 16 > sl.d_text.bytes) return fail(FMGPU_ERR_HIP, "feed: a window outgrew its slot");
        FM_HIP(hipStreamWaitEvent(f->up, sl.ev_text, 0));
        FM_HIP(hipMemcpyAsync(sl.d_text.as<uint8_t>() + sl.headroom, src, (size_t)len, hipMemcpyHostToDevice, f->up));
        FM_HIP(hipEventRecord(sl.ev_up, f->up));
        f->last_uploaded += len;
        return 0;
    };

    auto body = [&]() -> int {
        int r;
        if ((r = upload(0))) return r;
        for (uint64_t c = 0; c < windows; ++c) {
            Slot& sl = f->slot[c % slots];
            const uint64_t len = fh::text_window_end(bytes, c, B) - fh::text_window_begin(c, B);
            if (!fh::text_piece_fits(carry, len))
                return fail(FMGPU_ERR_UNSUPPORTED, "fmgpu_feed_map_text: a piece (the unconsumed bytes and the next window) may hold at most 2^32 - 2 bytes: no record ends within " + std::to_string(carry) + " bytes");
            if (carry) {
                Slot& prev = f->slot[(c - 1) % slots];
                if (carry > sl.headroom && (r = regrow_text(f, sl, carry, len))) return r;
                FM_HIP(hipMemcpyAsync(sl.d_text.as<uint8_t>() + sl.headroom - carry, prev.d_text.as<uint8_t>() + prev.unconsumed, (size_t)carry, hipMemcpyDeviceToDevice, f->comp));
                FM_HIP(hipEventRecord(prev.ev_text, f->comp));
            }
            if (c + 1 < windows && (r = upload(c + 1))) return r;
            FM_HIP(hipStreamWaitEvent(f->comp, sl.ev_up, 0));

            // the piece, parsed on the slot's buffers
            SlotBuffer bacc(&sl.d_acc, &f->device_bytes), bln(&sl.d_lnbase, &f->device_bytes), bk(&sl.d_kcnt, &f->device_bytes), bhc(&sl.d_hcnt, &f->device_bytes),
                btmp(&sl.d_tmp, &f->device_bytes), bls(&sl.d_ls, &f->device_bytes), bq(&sl.d_q, &f->device_bytes), boff(&sl.d_off, &f->device_bytes),
                bn(&sl.d_names, &f->device_bytes), bql(&sl.d_quals, &f->device_bytes);
            ParseBuffers pb;
            pb.acc = &bacc; pb.lnbase = &bln; pb.kcnt = &bk; pb.hcnt = &bhc; pb.tmp = &btmp; pb.ls = &bls; pb.qbuf = &bq; pb.qoff = &boff;
            pb.names = o.names ? &bn : nullptr; pb.quals = o.quals ? &bql : nullptr; pb.qpad = 64;
            const uint64_t start = sl.headroom - carry, n = carry + len;
            fmgpu_parse_result pr;
            uint64_t next_line = 0;
            r = parse_device(sl.d_text.as<uint8_t>() + start, n, format, fh::text_piece_final(c, windows, final) ? 1 : 0, c + 1 < windows ? 1 : 0, f->d_table.as<uint8_t>(), &pb, false, ~0ull, ~0ull,
                             line_base, total.consumed, &pr, &next_line, &text_error, f->comp);
            if (text_error) {                                             // the counts of the records in front of the offending one, in the caller's text
                total.reads += pr.reads; total.symbols += pr.symbols; total.foreign += pr.foreign;
                total.error_line = line_base + pr.error_line; total.error_offset = total.consumed + pr.error_offset;
                total.consumed += pr.consumed;
                return r;
            }
            if (r) return r;
            FM_HIP(hipEventRecord(sl.ev_text, f->comp));
            sl.unconsumed = start + pr.consumed;
            const uint64_t reads = pr.reads, first = total.reads;

            // its reads, mapped: run_map's chain and rebase, and the spans rebased to the caller's text
            uint64_t cnt = 0, pcnt = 0;
            if (reads) {
                if (o.m.out_stratum && (r = sl.d_str.need((size_t)(mult * reads), &f->device_bytes))) return r;
                if (o.lens && (r = sl.d_rlen.need((size_t)reads * 8, &f->device_bytes))) return r;
                SlotBuffer bh(&sl.d_hits, &f->device_bytes), bp(&sl.d_pos, &f->device_bytes), bi(&sl.d_lb, &f->device_bytes);
                fmgpu_stats ls{};
                const uint8_t* mq = sl.d_q.as<uint8_t>();
                const uint64_t* moff = sl.d_off.as<uint64_t>();
                if (strands) {                                            // the piece's reads doubled on the device: the second strand never crosses the bus
                    SlotBuffer bq2(&sl.d_q2, &f->device_bytes), boff2(&sl.d_off2, &f->device_bytes);
                    if ((r = strands_device(mq, moff, reads, f->d_comp.as<uint8_t>(), &bq2, &boff2, f->comp))) return r;
                    mq = sl.d_q2.as<uint8_t>(); moff = sl.d_off2.as<uint64_t>();
                }
                if ((r = map_device(f->h, mq, moff, mult * reads, what, false, &bh, &bp, &bi, o.m.out_stratum ? sl.d_str.as<uint8_t>() : nullptr,
                                    search_stats ? cs.data() : nullptr, locate_stats ? &ls : nullptr, f->comp, &cnt, &pcnt, strands && strands->pair != 0))) return r;
                if ((r = map_rebase(sl.d_hits.as<fmgpu_hit>(), cnt, sl.d_pos.as<fmgpu_position>(), pcnt, mult * first, produced, f->comp))) return r;
                if ((r = parse_piece_spans(o.names ? sl.d_names.as<fmgpu_text_span>() : nullptr, o.quals ? sl.d_quals.as<fmgpu_text_span>() : nullptr,
                                           o.lens ? sl.d_rlen.as<uint64_t>() : nullptr, sl.d_off.as<uint64_t>(), reads, total.consumed, format, f->comp))) return r;
                if (search_stats) for (int32_t i = 0; i < nstats; ++i) add_stats(&search_stats[i], cs[(size_t)i]);
                if (locate_stats) add_stats(locate_stats, ls);
            }
            FM_HIP(hipEventRecord(sl.ev_comp, f->comp));
            FM_HIP(hipStreamWaitEvent(f->down, sl.ev_comp, 0));
            sl.first = first; sl.reads = reads; sl.hits = cnt; sl.produced = produced; sl.positions = pcnt; sl.located = located;
            sl.str_first = mult * first; sl.str_reads = mult * reads;
            // records and reads beyond the caller's capacity are counted, not written
            sl.hits_down = o.m.out_hits && cnt && produced + cnt <= o.m.hits_capacity; sl.hits_in_place = hits_pinned;
            sl.pos_down = pcnt && located + pcnt <= o.m.capacity; sl.pos_in_place = pos_pinned;
            sl.reads_down = reads && o.read_arrays() && first + reads <= o.read_capacity;
            sl.str_down = sl.reads_down && o.m.out_stratum; sl.str_in_place = str_pinned;
            sl.names_in_place = names_pinned; sl.quals_in_place = quals_pinned; sl.rlen_in_place = lens_pinned;
            const auto download = [&](bool wanted, bool in_place, void* target, Grown& pinned, const Grown& dev, size_t nbytes) -> int {
                if (!wanted || !nbytes) return 0;
                if (!in_place) { if (int e = pinned.need(nbytes, &f->pinned_bytes)) return e; target = pinned.p; }
                FM_HIP(hipMemcpyAsync(target, dev.p, nbytes, hipMemcpyDeviceToHost, f->down));
                return 0;
            };
            if ((r = download(sl.hits_down, hits_pinned, o.m.out_hits + produced, sl.p_hits, sl.d_hits, (size_t)cnt * sizeof(fmgpu_hit)))) return r;
            if ((r = download(sl.pos_down, pos_pinned, o.m.out + located, sl.p_pos, sl.d_pos, (size_t)pcnt * sizeof(fmgpu_position)))) return r;
            if ((r = download(sl.str_down, str_pinned, o.m.out_stratum + mult * first, sl.p_str, sl.d_str, (size_t)(mult * reads)))) return r;
            if ((r = download(sl.reads_down && o.names, names_pinned, o.names + first, sl.p_names, sl.d_names, (size_t)reads * sizeof(fmgpu_text_span)))) return r;
            if ((r = download(sl.reads_down && o.quals, quals_pinned, o.quals + first, sl.p_quals, sl.d_quals, (size_t)reads * sizeof(fmgpu_text_span)))) return r;
            if ((r = download(sl.reads_down && o.lens, lens_pinned, o.lens + first, sl.p_rlen, sl.d_rlen, (size_t)reads * 8))) return r;
            FM_HIP(hipEventRecord(sl.ev_down, f->down));
            sl.busy = true;
            produced += cnt; located += pcnt;
            total.reads += reads; total.symbols += pr.symbols; total.foreign += pr.foreign; total.consumed += pr.consumed;
            line_base += next_line;
            carry = n - pr.consumed;
        }
        for (uint64_t k = 0; k < slots; ++k) {
            Slot& sl = f->slot[(windows + k) % slots];
            if (int r2 = retire_text(f, sl, o)) return r2;
        }
        return 0;
    };
    rc = body();
    *result = total;
    *out_count = located;
    if (out_hit_count) *out_hit_count = produced;
    if (rc) { drain(f); return rc; }
    if (located > o.m.capacity) return fail(FMGPU_ERR_CAPACITY, "position buffer holds " + std::to_string(o.m.capacity) + " records, " + std::to_string(located) + " produced");
    if (o.m.out_hits && produced > o.m.hits_capacity) return fail(FMGPU_ERR_CAPACITY, "hit buffer holds " + std::to_string(o.m.hits_capacity) + " records, " + std::to_string(produced) + " produced");
    if (o.read_arrays() && total.reads > o.read_capacity) return fail(FMGPU_ERR_CAPACITY, "the read arrays hold " + std::to_string(o.read_capacity) + " entries, the text has " + std::to_string(total.reads) + " reads");
    return 0;
}

}  // namespace
}  // namespace fmgpu

using namespace fmgpu;

extern "C" {

int fmgpu_feed_plan(const uint64_t* qoff, uint64_t nq, uint64_t chunk_reads, uint64_t chunk_symbols, uint64_t* out_first, uint64_t capacity, uint64_t* out_chunks) {
    const int rc = fmgpu_feed_host::plan(qoff, nq, chunk_reads, chunk_symbols, out_first, capacity, out_chunks);
    if (rc == FMGPU_ERR_INVALID) return fail(rc, !out_chunks || (nq && !qoff) || (capacity && !out_first) ? "qoff / out_first / out_chunks is null"
                                                 : (!chunk_reads || !chunk_symbols) ? "chunk_reads and chunk_symbols must be at least 1" : "qoff is not non-decreasing");
    if (rc == FMGPU_ERR_CAPACITY) return fail(rc, "out_first holds " + std::to_string(capacity) + " chunks, the batch has " + std::to_string(*out_chunks));
    return rc;
}

int fmgpu_feed_create(fmgpu_index_t h, const fmgpu_feed_config* cfg, fmgpu_feed_t* out) {
    if (!out) return fail(FMGPU_ERR_INVALID, "out is null");
    *out = nullptr;
    int32_t device = 0;
    if (int rc = handle_device(h, &device)) return rc;
    fmgpu_feed_config c{};
    if (cfg) c = *cfg;
    if (c.slots == 0) c.slots = 2;
    if (c.host_threads == 0) c.host_threads = 4;
    if (c.slots < 2 || c.slots > kMaxSlots) return fail(FMGPU_ERR_INVALID, "fmgpu_feed_config: slots must be 0 or 2 .. 4");
    if (c.host_threads < 1 || c.host_threads > 16) return fail(FMGPU_ERR_INVALID, "fmgpu_feed_config: host_threads must be 0 or 1 .. 16");
    if (c.reserved != 0) return fail(FMGPU_ERR_INVALID, "fmgpu_feed_config: reserved must be 0");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return fail(FMGPU_ERR_NO_DEVICE, "no HIP device visible — the product path has no CPU fallback"); }
    if (dev != device) return fail(FMGPU_ERR_INVALID, "the handle lives on device " + std::to_string(device) + ", the calling thread's current device is " + std::to_string(dev));
    std::unique_ptr<fmgpu_feed> f(new (std::nothrow) fmgpu_feed);
    if (!f) return fail(FMGPU_ERR_NOMEM, "out of host memory");
    f->h = h; f->device = device;
    f->chunk_reads = c.chunk_reads ? c.chunk_reads : kDefaultChunkReads;
    f->chunk_symbols = c.chunk_symbols ? c.chunk_symbols : kDefaultChunkSymbols;
    if (f->chunk_reads > 0x7fffffffull) f->chunk_reads = 0x7fffffffull;                  // (a launch covers fewer than 2^32 threads)
    f->slots = c.slots; f->pack4 = c.pack4 != 0;
    if (int rc = ::fmgpu_index_info(h, nullptr, &f->sigma, nullptr, nullptr, nullptr)) return rc;
    if (int rc = exact_reads_nibbles_on(h, &f->nibbles)) return rc;
    try { f->workers.reset(new fmgpu_feed_host::Workers((uint32_t)c.host_threads)); }
    catch (const std::exception& e) { return fail(FMGPU_ERR_NOMEM, std::string("feed: cannot start the host threads: ") + e.what()); }
    for (hipStream_t* s : {&f->up, &f->comp, &f->down}) {
        hipError_t e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
        if (e != hipSuccess) { *s = nullptr; const int rc = hip_fail(e, "hipStreamCreateWithFlags(feed)"); fmgpu_feed_destroy(f.release()); return rc; }
    }
    *out = f.release();
    return 0;
}

int fmgpu_feed_destroy(fmgpu_feed_t f) {
    if (!f) return 0;
    if (f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is not a feed of this library");
    drain(f);
    for (Slot& sl : f->slot) {
        for (Grown* g : sl.buffers()) g->release(nullptr);
        for (hipEvent_t ev : {sl.ev_up, sl.ev_comp, sl.ev_down, sl.ev_text}) if (ev) (void)hipEventDestroy(ev);
    }
    f->d_table.release(nullptr);
    f->d_comp.release(nullptr);
    for (hipStream_t s : {f->up, f->comp, f->down}) if (s) (void)hipStreamDestroy(s);
    f->magic = 0;
    delete f;
    return 0;
}

int fmgpu_feed_info(fmgpu_feed_t f, uint64_t* pinned_bytes, uint64_t* device_bytes, uint64_t* last_chunks, uint64_t* last_staged_bytes, uint64_t* last_uploaded_bytes) {
    if (!f || f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    if (pinned_bytes) *pinned_bytes = f->pinned_bytes;
    if (device_bytes) *device_bytes = f->device_bytes;
    if (last_chunks) *last_chunks = f->last_chunks;
    if (last_staged_bytes) *last_staged_bytes = f->last_staged;
    if (last_uploaded_bytes) *last_uploaded_bytes = f->last_uploaded;
    return 0;
}

static int feed_exact(fmgpu_feed_t f, Batch b, uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats) {
    if (stats) *stats = fmgpu_stats{};
    if (b.nq == 0) return 0;                                                              // (before the feed is looked at)
    if (!f || f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    if (b.q4 && f->sigma > 15) return fail(FMGPU_ERR_UNSUPPORTED, "4-bit packed queries need sigma <= 15, this index has sigma = " + std::to_string(f->sigma));
    if (b.reads ? (!b.lens || !out_lb || !out_len) : (!b.qbuf || !b.qoff || !out_lb || !out_len))
        return fail(FMGPU_ERR_INVALID, b.reads || b.lens ? "reads / lens / out_lb / out_len is null" : "qbuf / qoff / out_lb / out_len is null");
    if (int rc = check_feed(f)) return rc;
    if (int rc = no_device_memory({b.qbuf, b.qoff, b.reads, b.lens, out_lb, out_len})) return rc;
    if (b.reads) if (int rc = no_device_memory({b.reads[0]})) return rc;                  // (looked at only once the array itself is known to be host memory)
    b.in_pinned = b.qbuf && pointer_kind(b.qbuf) == 1;
    return run_exact(f, b, out_lb, out_len, stats);
}

int fmgpu_feed_search_exact(fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats) {
    Batch b; b.qbuf = qbuf; b.qoff = qoff; b.nq = nq;
    return feed_exact(f, b, out_lb, out_len, stats);
}
int fmgpu_feed_search_exact_q4(fmgpu_feed_t f, const uint8_t* packed, const uint64_t* qoff, uint64_t nq, uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats) {
    Batch b; b.qbuf = packed; b.qoff = qoff; b.nq = nq; b.q4 = true;
    return feed_exact(f, b, out_lb, out_len, stats);
}
int fmgpu_feed_search_exact_v(fmgpu_feed_t f, const uint8_t* const* reads, const uint64_t* lens, uint64_t nq, uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats) {
    if (nq && !reads) return (f && f->magic == 0x46454544u) ? fail(FMGPU_ERR_INVALID, "reads / lens / out_lb / out_len is null") : fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    Batch b; b.reads = reads; b.lens = lens; b.nq = nq;
    return feed_exact(f, b, out_lb, out_len, stats);
}

static int feed_scheme(fmgpu_feed_t f, Batch b, const fmgpu_scheme* scheme, uint64_t max_hits, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats) {
    if (stats) *stats = fmgpu_stats{};
    if (out_count) *out_count = 0;
    if (b.nq == 0) return 0;
    if (!f || f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    if ((b.reads ? !b.lens : (!b.qbuf || !b.qoff)) || (!out && capacity) || !out_count)
        return fail(FMGPU_ERR_INVALID, b.reads || b.lens ? "reads / lens / out / out_count is null" : "qbuf / qoff / out / out_count is null");
    if (int rc = check_feed(f)) return rc;
    if (int rc = check_scheme(f->h, scheme, max_hits)) return rc;
    if (max_hits == 0 || scheme->n_searches == 0) return 0;                               // (the one-shot call's own answer: nothing to search)
    if (int rc = no_device_memory({b.qbuf, b.qoff, b.reads, b.lens, out, out_count})) return rc;
    if (b.reads) if (int rc = no_device_memory({b.reads[0]})) return rc;
    b.in_pinned = b.qbuf && pointer_kind(b.qbuf) == 1;
    return run_scheme(f, b, scheme, max_hits, out, capacity, out_count, stats);
}

int fmgpu_feed_search_scheme(fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                             fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats) {
    Batch b; b.qbuf = qbuf; b.qoff = qoff; b.nq = nq;
    return feed_scheme(f, b, scheme, max_hits_per_query, out, capacity, out_count, stats);
}
int fmgpu_feed_search_scheme_v(fmgpu_feed_t f, const uint8_t* const* reads, const uint64_t* lens, uint64_t nq, const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                               fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats) {
    if (nq && !reads) return (f && f->magic == 0x46454544u) ? fail(FMGPU_ERR_INVALID, "reads / lens / out / out_count is null") : fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    Batch b; b.reads = reads; b.lens = lens; b.nq = nq;
    return feed_scheme(f, b, scheme, max_hits_per_query, out, capacity, out_count, stats);
}

static int feed_map(fmgpu_feed_t f, Batch b, const fmgpu_map_query* what, bool both, const fmgpu_strands* strands, fmgpu_position* out, uint64_t capacity, uint64_t* out_count, fmgpu_hit* out_hits,
                    uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    if (out_count) *out_count = 0;
    if (out_hit_count) *out_hit_count = 0;
    if (int rc = check_map_query(what)) return rc;
    if (both) if (int rc = check_strands(strands)) return rc;
    if (search_stats) for (int32_t i = 0; i < std::max(1, what->n_schemes); ++i) search_stats[i] = fmgpu_stats{};
    if (locate_stats) *locate_stats = fmgpu_stats{};
    if (b.nq == 0) return 0;                                                              // (before the feed is looked at; out_stratum untouched)
    if (both && b.nq > kMaxStrandReads) return fail(FMGPU_ERR_UNSUPPORTED, "a both-strand batch holds at most 2^30 - 1 reads");
    if (!f || f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    if (int rc = check_feed(f)) return rc;
    if (int rc = check_map_schemes(f->h, what, false)) return rc;
    if ((b.reads ? !b.lens : (!b.qbuf || !b.qoff)) || !out_count || (!out && capacity) || (!out_hits && hits_capacity))
        return fail(FMGPU_ERR_INVALID, b.reads || b.lens ? "reads / lens / out / out_count / out_hits is null" : "qbuf / qoff / out / out_count / out_hits is null");
    if (int rc = no_device_memory({b.qbuf, b.qoff, b.reads, b.lens, out, out_count, out_hits, out_hit_count, out_stratum, both ? strands->complement : nullptr})) return rc;
    if (b.reads) if (int rc = no_device_memory({b.reads[0]})) return rc;
    b.in_pinned = b.qbuf && pointer_kind(b.qbuf) == 1;
    const MapOut o{out, capacity, out_hits, hits_capacity, out_stratum};
    return run_map(f, b, what, both ? strands : nullptr, o, out_count, out_hit_count, search_stats, locate_stats);
}

int fmgpu_feed_map(fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what, fmgpu_position* out, uint64_t capacity,
                   uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_stats* search_stats,
                   fmgpu_stats* locate_stats) {
    Batch b; b.qbuf = qbuf; b.qoff = qoff; b.nq = nq;
    return feed_map(f, b, what, false, nullptr, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum, search_stats, locate_stats);
}
int fmgpu_feed_map_strands(fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what, const fmgpu_strands* strands,
                           fmgpu_position* out, uint64_t capacity, uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                           uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    Batch b; b.qbuf = qbuf; b.qoff = qoff; b.nq = nq;
    return feed_map(f, b, what, true, strands, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum, search_stats, locate_stats);
}
int fmgpu_feed_map_v(fmgpu_feed_t f, const uint8_t* const* reads, const uint64_t* lens, uint64_t nq, const fmgpu_map_query* what, fmgpu_position* out, uint64_t capacity,
                     uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_stats* search_stats,
                     fmgpu_stats* locate_stats) {
    if (nq && !reads && !check_map_query(what))
        return (f && f->magic == 0x46454544u) ? fail(FMGPU_ERR_INVALID, "reads / lens / out / out_count / out_hits is null") : fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    Batch b; b.reads = reads; b.lens = lens; b.nq = nq;
    return feed_map(f, b, what, false, nullptr, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum, search_stats, locate_stats);
}

static int feed_map_text(fmgpu_feed_t f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final, const uint8_t* symbol_of, uint64_t chunk_bytes,
                         const fmgpu_map_query* what, bool both, const fmgpu_strands* strands, fmgpu_position* out, uint64_t capacity, uint64_t* out_count, fmgpu_hit* out_hits,
                         uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_text_span* out_names, fmgpu_text_span* out_quals, uint64_t* out_lens,
                         uint64_t read_capacity, fmgpu_parse_result* result, fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    if (out_count) *out_count = 0;
    if (out_hit_count) *out_hit_count = 0;
    if (result) std::memset(result, 0, sizeof *result);
    if (!result || !symbol_of) return fail(FMGPU_ERR_INVALID, "result / symbol_of is null");
    if (int rc = check_map_query(what)) return rc;
    if (both) if (int rc = check_strands(strands)) return rc;
    if (!out_count || (!out && capacity) || (!out_hits && hits_capacity)) return fail(FMGPU_ERR_INVALID, "out / out_count / out_hits is null");
    if (format != FMGPU_TEXT_LINES && format != FMGPU_TEXT_FASTA && format != FMGPU_TEXT_FASTQ) return fail(FMGPU_ERR_INVALID, "unknown text format " + std::to_string(format));
    if (!text && bytes) return fail(FMGPU_ERR_INVALID, "text is null");
    if (chunk_bytes && chunk_bytes < fmgpu_feed_host::kTextMinWindow) return fail(FMGPU_ERR_INVALID, "chunk_bytes must be 0 or at least 16");
    if (search_stats) for (int32_t i = 0; i < std::max(1, what->n_schemes); ++i) search_stats[i] = fmgpu_stats{};
    if (locate_stats) *locate_stats = fmgpu_stats{};
    if (!f || f->magic != 0x46454544u) return fail(FMGPU_ERR_INVALID, "feed is null or not a feed of this library");
    if (bytes == 0) return 0;
    if (int rc = check_feed(f)) return rc;
    if (int rc = check_map_schemes(f->h, what, false)) return rc;
    if (int rc = no_device_memory({text, symbol_of, out, out_count, out_hits, out_hit_count, out_stratum, out_names, out_quals, out_lens, result, both ? strands->complement : nullptr})) return rc;
    const TextOut o{MapOut{out, capacity, out_hits, hits_capacity, out_stratum}, out_names, out_quals, out_lens, read_capacity};
    return run_map_text(f, text, bytes, format, final, symbol_of, fmgpu_feed_host::text_window_bytes(chunk_bytes), what, both ? strands : nullptr, o, out_count, out_hit_count, result,
                        search_stats, locate_stats);
}

int fmgpu_feed_map_text(fmgpu_feed_t f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final, const uint8_t* symbol_of, uint64_t chunk_bytes,
                        const fmgpu_map_query* what, fmgpu_position* out, uint64_t capacity, uint64_t* out_count, fmgpu_hit* out_hits, uint64_t hits_capacity,
                        uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_text_span* out_names, fmgpu_text_span* out_quals, uint64_t* out_lens, uint64_t read_capacity,
                        fmgpu_parse_result* result, fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    return feed_map_text(f, text, bytes, format, final, symbol_of, chunk_bytes, what, false, nullptr, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum,
                         out_names, out_quals, out_lens, read_capacity, result, search_stats, locate_stats);
}
int fmgpu_feed_map_text_strands(fmgpu_feed_t f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final, const uint8_t* symbol_of, uint64_t chunk_bytes,
                                const fmgpu_map_query* what, const fmgpu_strands* strands, fmgpu_position* out, uint64_t capacity, uint64_t* out_count, fmgpu_hit* out_hits,
                                uint64_t hits_capacity, uint64_t* out_hit_count, uint8_t* out_stratum, fmgpu_text_span* out_names, fmgpu_text_span* out_quals, uint64_t* out_lens,
                                uint64_t read_capacity, fmgpu_parse_result* result, fmgpu_stats* search_stats, fmgpu_stats* locate_stats) {
    return feed_map_text(f, text, bytes, format, final, symbol_of, chunk_bytes, what, true, strands, out, capacity, out_count, out_hits, hits_capacity, out_hit_count, out_stratum,
                         out_names, out_quals, out_lens, read_capacity, result, search_stats, locate_stats);
}

}  // extern "C"
