// fmgpu_feed_host.h — the host-only half of a feed (include/fmgpu.h: fmgpu_feed_*): the chunk planner, the stagers that move one chunk between caller memory and a
// pinned slot (copy, gather of scattered reads, nibble packer), the scatter of results and hit records, and the small worker pool that runs them slice by slice.
// No HIP header is included and nothing here touches a device: fmgpu_feed.hip makes every HIP call, on the calling thread; tests/cpp/test_feed_host.cpp compiles this
// file alone under the host sanitizers.
//
// Chunk-relative symbols.  A chunk of reads first .. end - 1 of a flat batch sits in its slot from symbol A = qoff[first] & ~31 on: batch symbol s is slot symbol s - A,
// so byte s - A of a byte slot and nibble (s - A) & 1 of byte (s - A) >> 1 of a nibble slot.  A is a multiple of 32: the parity of a symbol, and its place inside an
// aligned 16-byte piece of either form, are those of the caller's batch.  The slot's offsets are qoff[i] - A.
#pragma once

#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/fmgpu.h"

namespace fmgpu_feed_host {

// ---- the planner: a chunk is the longest run of consecutive reads with at most chunk_reads reads and at most chunk_symbols symbols, and never less than one read
// the end of the chunk that starts at read `first` (first < nq), by bisection: qoff must be non-decreasing over first .. nq
inline uint64_t chunk_end(const uint64_t* qoff, uint64_t nq, uint64_t first, uint64_t chunk_reads, uint64_t chunk_symbols) {
    const uint64_t hi_reads = chunk_reads < nq - first ? first + chunk_reads : nq;
    const uint64_t base = qoff[first];
    const uint64_t limit = chunk_symbols > ~0ull - base ? ~0ull : base + chunk_symbols;
    // the last e in (first, hi_reads] with qoff[e] <= limit; first + 1 where none is (one over-long read)
    const uint64_t* p = std::upper_bound(qoff + first + 1, qoff + hi_reads + 1, limit);
    const uint64_t e = (uint64_t)(p - qoff) - 1;
    return e > first ? e : first + 1;
}

// fmgpu_feed_plan itself (the status codes of include/fmgpu.h): out_first gets chunks + 1 entries where capacity >= chunks, may be null where capacity == 0
inline int plan(const uint64_t* qoff, uint64_t nq, uint64_t chunk_reads, uint64_t chunk_symbols, uint64_t* out_first, uint64_t capacity, uint64_t* out_chunks) {
    if (!out_chunks || (nq && !qoff) || (capacity && !out_first)) return FMGPU_ERR_INVALID;
    *out_chunks = 0;
    if (chunk_reads == 0 || chunk_symbols == 0) return FMGPU_ERR_INVALID;
    for (uint64_t i = 0; i < nq; ++i) if (qoff[i + 1] < qoff[i]) return FMGPU_ERR_INVALID;
    uint64_t chunks = 0;
    for (uint64_t first = 0; first < nq; ++chunks) {
        if (chunks < capacity) out_first[chunks] = first;
        first = chunk_end(qoff, nq, first, chunk_reads, chunk_symbols);
    }
    *out_chunks = chunks;
    if (chunks > capacity) return FMGPU_ERR_CAPACITY;
    if (out_first) out_first[chunks] = nq;
    return 0;
}

// ---- the shape of a run of reads: symbols in all, the longest and the shortest read; ok = false where an offset decreases
struct Shape {
    uint64_t total = 0, longest = 0, shortest = ~0ull;
    bool ok = true;
    void add(uint64_t len) { total += len; longest = std::max(longest, len); shortest = std::min(shortest, len); }
    void merge(const Shape& o) { total += o.total; longest = std::max(longest, o.longest); shortest = std::min(shortest, o.shortest); ok = ok && o.ok; }
};
inline Shape shape_of_offsets(const uint64_t* qoff, uint64_t first, uint64_t end) {
    Shape s;
    for (uint64_t i = first; i < end; ++i) {
        if (qoff[i + 1] < qoff[i]) { s.ok = false; return s; }
        s.add(qoff[i + 1] - qoff[i]);
    }
    return s;
}
inline Shape shape_of_lengths(const uint64_t* lens, uint64_t first, uint64_t end) {
    Shape s;
    for (uint64_t i = first; i < end; ++i) s.add(lens[i]);
    return s;
}

// the first symbol a chunk's slot holds (see above)
inline uint64_t slot_origin(uint64_t first_symbol) { return first_symbol & ~(uint64_t)31; }

// ---- slices: part t of `parts` of the items 0 .. n, cut so that origin + cut is a multiple of `align` (a power of two) except at 0 and n — two workers never share a byte of nibbles
inline uint64_t slice_cut(uint64_t n, uint32_t parts, uint32_t t, uint64_t origin = 0, uint64_t align = 1) {
    if (t == 0) return 0;
    if (t >= parts) return n;
    uint64_t c = n / parts * t + std::min<uint64_t>(t, n % parts);
    c = ((origin + c) & ~(align - 1));
    c = c > origin ? c - origin : 0;
    return std::min(c, n);
}

// ---- the copy stager of a flat batch: the slot's offsets for reads first .. end (end - first + 1 entries, slice [a, b) of them)
inline void stage_offsets(const uint64_t* qoff, uint64_t first, uint64_t origin, uint64_t a, uint64_t b, uint64_t* slot_off) {
    for (uint64_t i = a; i < b; ++i) slot_off[i] = qoff[first + i] - origin;
}
// ... and its symbols: batch symbols s0 + a .. s0 + b of a byte batch into the byte slot (s0 = the chunk's first symbol)
inline void stage_bytes(const uint8_t* qbuf, uint64_t s0, uint64_t origin, uint64_t a, uint64_t b, uint8_t* slot) {
    if (b > a) std::memcpy(slot + (s0 - origin) + a, qbuf + s0 + a, b - a);
}
// ... or of a packed batch: the bytes that hold nibbles s0 .. s1 - 1 are bytes s0 >> 1 .. (s1 + 1) >> 1; slice [a, b) of those bytes
inline uint64_t packed_bytes(uint64_t s0, uint64_t s1) { return s1 > s0 ? ((s1 + 1) >> 1) - (s0 >> 1) : 0; }
inline void stage_packed(const uint8_t* packed, uint64_t s0, uint64_t origin, uint64_t a, uint64_t b, uint8_t* slot) {
    if (b > a) std::memcpy(slot + ((s0 >> 1) - (origin >> 1)) + a, packed + (s0 >> 1) + a, b - a);
}

// ---- the nibble packer: symbols a .. b - 1 of `src` (the chunk's own symbols, 0 = its first) become slot nibbles shift + a .. shift + b - 1, a byte >= sigma becomes 15.
// shift = the chunk's first symbol minus the slot's origin: an odd shift puts the first symbol into a HIGH nibble, as it lies in the caller's batch.  shift + a must be even
// unless a == 0 (slice_cut with align 2): the byte of an odd first nibble gets a 0 low nibble, the byte of an odd last one a 0 high nibble — every byte has one writer.
inline uint8_t nibble_of(uint8_t c, uint32_t sigma) { return c < sigma ? c : 15; }
// eight symbols at once, in one 64-bit word (little-endian, 1 <= sigma <= 16): the high bit of every byte >= sigma is raised without a carry between bytes and widened
// to a byte mask, the masked bytes become 15, and three shift-and-mask steps move the eight low nibbles together
inline uint32_t pack8(const uint8_t* src, uint32_t sigma) {
    const uint64_t k01 = 0x0101010101010101ull, k7f = 0x7f7f7f7f7f7f7f7full, k80 = 0x8080808080808080ull, k0f = 0x0f0f0f0f0f0f0f0full;
    uint64_t x;
    std::memcpy(&x, src, 8);
    const uint64_t m = (((((x & k7f) + (uint64_t)(0x80u - sigma) * k01) | x) & k80) >> 7) * 0xffull;
    uint64_t y = (x & ~m) | (m & k0f);
    y = (y | (y >> 4)) & 0x00ff00ff00ff00ffull;
    y = (y | (y >> 8)) & 0x0000ffff0000ffffull;
    y = (y | (y >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)y;
}
inline void pack_nibbles(const uint8_t* src, uint64_t a, uint64_t b, uint32_t sigma, uint64_t shift, uint8_t* slot) {
    uint64_t i = a;
    if (i < b && ((shift + i) & 1)) { slot[(shift + i) >> 1] = (uint8_t)(nibble_of(src[i], sigma) << 4); ++i; }
    if (sigma >= 1 && sigma <= 16) for (; i + 8 <= b; i += 8) { const uint32_t v = pack8(src + i, sigma); std::memcpy(slot + ((shift + i) >> 1), &v, 4); }
    for (; i + 1 < b; i += 2) slot[(shift + i) >> 1] = (uint8_t)(nibble_of(src[i], sigma) | (nibble_of(src[i + 1], sigma) << 4));
    if (i < b) slot[(shift + i) >> 1] = nibble_of(src[i], sigma);
}

// ---- the gather stager of scattered reads (the `_v` calls): the chunk's reads are reads[first + r], r = 0 .. n - 1, with slot offsets off[0 .. n] (off[0] = 0: the
// slot starts at the chunk's first symbol).  Symbols a .. b - 1 of the chunk go to the slot, as bytes or (sigma_pack != 0) as nibbles with the packer's rules, shift = 0: a must then be even.
inline void stage_lengths(const uint64_t* lens, uint64_t first, uint64_t n, uint64_t* slot_off) {
    uint64_t at = 0;
    for (uint64_t r = 0; r < n; ++r) { slot_off[r] = at; at += lens[first + r]; }
    slot_off[n] = at;
}
inline void gather_reads(const uint8_t* const* reads, uint64_t first, const uint64_t* off, uint64_t n, uint64_t a, uint64_t b, uint32_t sigma_pack, uint8_t* slot) {
    if (b <= a || n == 0) return;
    uint64_t r = (uint64_t)(std::upper_bound(off, off + n + 1, a) - off) - 1;      // the last read that starts at or before symbol a (empty reads before it are stepped over below)
    for (uint64_t s = a; s < b;) {
        while (off[r + 1] <= s) ++r;
        const uint64_t stop = std::min(b, off[r + 1]);
        const uint8_t* src = reads[first + r] - off[r];                            // src[s] = the chunk's symbol s while s is inside read r
        if (!sigma_pack) { std::memcpy(slot + s, src + s, stop - s); s = stop; continue; }
        for (; s < stop; ++s) {
            const uint8_t nib = nibble_of(src[s], sigma_pack);
            if (s & 1) slot[s >> 1] = (uint8_t)((s == a ? 0 : slot[s >> 1]) | (nib << 4));      // (the low nibble is this slice's own, written one symbol earlier: a is even)
            else slot[s >> 1] = nib;
        }
    }
}

// ---- results back: the chunk's intervals into the caller's arrays (slice [a, b) of the chunk's reads) ...
inline void scatter_intervals(const uint64_t* slot_lb, const uint64_t* slot_len, uint64_t first, uint64_t a, uint64_t b, uint64_t* out_lb, uint64_t* out_len) {
    if (b <= a) return;
    std::memcpy(out_lb + first + a, slot_lb + a, (b - a) * 8);
    std::memcpy(out_len + first + a, slot_len + a, (b - a) * 8);
}
// ... and its hit records (slice [a, b) of them) behind the `produced` records of the earlier chunks, qidx = the read's number in the caller's batch.  src == dst + produced
// (records that were copied into the caller's pinned memory directly) only renumbers.
inline void scatter_hits(const fmgpu_hit* src, uint64_t a, uint64_t b, uint64_t first, fmgpu_hit* dst, uint64_t produced) {
    fmgpu_hit* out = dst + produced;
    if (src != out && b > a) std::memcpy(out + a, src + a, (b - a) * sizeof(fmgpu_hit));
    for (uint64_t i = a; i < b; ++i) out[i].qidx += first;
}

// ---- text feeds (fmgpu_feed_map_text): the text is cut into windows of B bytes; piece c is what piece c - 1 left unconsumed (the carry) followed by window c.  A
// slot's device text buffer holds the window from byte H (the headroom) on and the carry in the H bytes in front of it.
constexpr uint64_t kTextDefaultWindow = 64ull << 20, kTextMinWindow = 16, kTextMaxHeadroom = 1ull << 20, kTextMaxPiece = 0xfffffffeull;
inline uint64_t text_window_bytes(uint64_t chunk_bytes) { return chunk_bytes ? chunk_bytes : kTextDefaultWindow; }      // (values below kTextMinWindow are refused by the caller)
inline uint64_t text_windows(uint64_t bytes, uint64_t B) { return bytes / B + (bytes % B ? 1 : 0); }
inline uint64_t text_window_begin(uint64_t c, uint64_t B) { return c * B; }                                            // c < text_windows(bytes, B): no overflow
inline uint64_t text_window_end(uint64_t bytes, uint64_t c, uint64_t B) { const uint64_t a = c * B; return bytes - a < B ? bytes : a + B; }
inline bool text_piece_final(uint64_t c, uint64_t windows, int32_t final) { return final != 0 && c + 1 == windows; }
inline uint64_t text_round16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }
// the headroom a slot starts with: a window's worth, at most 1 MiB, a multiple of 16 ...
inline uint64_t text_headroom(uint64_t B) { return text_round16(B < kTextMaxHeadroom ? B : kTextMaxHeadroom); }
// ... and the headroom it has once a carry has arrived: unchanged while the carry fits, else twice the carry
inline uint64_t text_headroom_for(uint64_t H, uint64_t carry) { return carry <= H ? H : text_round16(2 * carry); }
// a piece may hold 2^32 - 2 bytes (positions and line numbers are 32-bit words on the device)
inline bool text_piece_fits(uint64_t carry, uint64_t window) { return carry <= kTextMaxPiece && window <= kTextMaxPiece - carry; }

// ---- the workers: host_threads - 1 threads beside the calling one, which takes slice 0 itself.  run(fn) calls fn(t, parts) once for every t and returns when all have.
// They copy and pack, each on its own slice, and never make a HIP call.
class Workers {
  public:
    explicit Workers(uint32_t parts) : parts_(parts ? parts : 1) {
        for (uint32_t t = 1; t < parts_; ++t) threads_.emplace_back([this, t] { loop(t); });
    }
    ~Workers() {
        { std::lock_guard<std::mutex> g(mu_); stop_ = true; ++epoch_; }
        wake_.notify_all();
        for (auto& th : threads_) th.join();
    }
    Workers(const Workers&) = delete;
    Workers& operator=(const Workers&) = delete;
    uint32_t parts() const { return parts_; }
    void run(const std::function<void(uint32_t, uint32_t)>& fn) {
        if (parts_ == 1) { fn(0, 1); return; }
        { std::lock_guard<std::mutex> g(mu_); job_ = &fn; left_ = parts_ - 1; ++epoch_; }
        wake_.notify_all();
        fn(0, parts_);
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return left_ == 0; });
        job_ = nullptr;
    }

  private:
    void loop(uint32_t t) {
        uint64_t seen = 0;
        for (;;) {
            const std::function<void(uint32_t, uint32_t)>* job;
            {
                std::unique_lock<std::mutex> g(mu_);
                wake_.wait(g, [&] { return epoch_ != seen; });
                seen = epoch_;
                if (stop_) return;
                job = job_;
            }
            (*job)(t, parts_);
            { std::lock_guard<std::mutex> g(mu_); --left_; }
            done_.notify_one();
        }
    }
    uint32_t parts_;
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable wake_, done_;
    const std::function<void(uint32_t, uint32_t)>* job_ = nullptr;
    uint32_t left_ = 0;
    uint64_t epoch_ = 0;
    bool stop_ = false;
};

}  // namespace fmgpu_feed_host
