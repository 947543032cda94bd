/* fmgpu.h — C-ABI of libfmgpu.so, the MI355X (gfx950) backward-search engine.
 *
 * This is the drop-in boundary for the reference's batched search path.  The reference
 * (SGSSGene/fmindex-collection, header-only C++23) has no FFI; the interface this ABI replaces is
 * the set of free function templates and member functions cited at each entry point below
 * (paths relative to src/fmindex-collection/ in the reference).  The C++ mirror of the reference's
 * template API that calls this ABI lives in include/fmc_gpu.hpp; INTEGRATION.md shows the binding
 * a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative fmgpu_status; fmgpu_last_error() returns a
 *     thread-local message for the last failure on the calling thread; no C++ exception crosses
 *     the ABI.
 *   - data pointers may be host or device pointers (detected per pointer with
 *     hipPointerGetAttributes); host buffers are staged through HBM by the library, device buffers
 *     are used in place.  `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     Calls that receive host output buffers return after the results have landed; calls that
 *     only touch device buffers are asynchronous on `stream`.
 *   - an index handle is immutable after creation and may be used concurrently from several host
 *     threads (each call brings its own stream / buffers).
 *   - symbols are ranks in [0, sigma) exactly as in the reference (0 = sequence delimiter);
 *     row indices, interval bounds and counts are uint64_t like the reference's size_t.
 *   - row width: an index of fewer than 2^32 - 64 rows is held in 32-bit device tables and may use every optional accelerator table below;
 *     a larger one (up to 2^40 rows; the reference switches to a 64-bit suffix array at 2^31 rows, utils.h:243-247) is held in 64-bit-row
 *     tables: construction, exact search (with the interval and walk tables of fmgpu_index_accelerate_exact, 16-byte entries), search_ng26
 *     (Hamming and edit distance; equal-length Hamming batches on the lean kernel like 32-bit rows), search_ng21, search_backtracking, locate,
 *     cursor steps, String_c queries and the index file work on it; the multi-symbol-step table, the k-mismatch tables (LF^1..3, walk, prefix),
 *     the locate answer table and the one-word transport forms return FMGPU_ERR_UNSUPPORTED (fmgpu_index_row_bits tells which).
 *   - derived occurrence tables: beside the layout it is handed, an index keeps what its kernels read fastest, built on the device at creation,
 *     construction and load and counted in device_bytes — sigma = 5: a symbol-pair table (1 byte per row; exact search takes two symbols per
 *     step; both row widths) and, for a BiFMIndex with 32-bit rows, dense DNA blocks (0.5 byte per row and direction; the equal-length k-mismatch kernel); a Wavelet
 *     or EPR / EPRV2 bwt with 6 <= sigma <= 29: a symbol-plane table (2 bytes per row; exact search takes one memory line per step and interval end instead of
 *     one per tree level); a sigma = 5 string handed over as InterleavedEPR* / InterleavedEPRV2* blocks or as a Wavelet: the one-symbol block table every
 *     other DNA layout is held in (1 byte per row), and with it the two tables above — every layout searches at the same speed.
 *     A sigma = 5 index with 32-bit rows, the pair table and a sampled suffix array of rate <= 16 also gets a sample chain (12 bytes per sample: exact search moves a one-row read
 *     `rate` symbols per entry along the sampled rows in text order; FMGPU_OPT_SAMPLE_CHAIN = 0 keeps it out).
 *     Results do not depend on them (fmgpu_set_option: FMGPU_OPT_PAIR_TABLE / _DENSE_DNA / _SYMBOL_PLANES / _EXPAND_DNA = 0 keep them out).
 *   - the library reads no environment variable: what used to be FMGPU_* switches are options set through fmgpu_set_option.
 */
#ifndef FMGPU_H
#define FMGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMGPU_ABI_VERSION 6

typedef enum fmgpu_status {
    FMGPU_OK = 0,
    FMGPU_ERR_INVALID = -1,      /* bad argument (null pointer, sigma out of range, sizes that do not match the layout) */
    FMGPU_ERR_UNSUPPORTED = -2,  /* valid request this build cannot serve (e.g. an accelerator table on a 64-bit-row index, n >= 2^40 rows) */
    FMGPU_ERR_HIP = -3,          /* a HIP runtime call failed; message holds hipGetErrorString */
    FMGPU_ERR_NO_DEVICE = -4,    /* no gfx950 device visible */
    FMGPU_ERR_CAPACITY = -5,     /* result buffer too small; *out_count holds the required record count */
    FMGPU_ERR_NOMEM = -6
} fmgpu_status;

/* occurrence-table ("string with rank support") layouts of the reference, string/<file>.h */
typedef enum fmgpu_layout {
    FMGPU_IB8 = 0, FMGPU_IB16 = 1, FMGPU_IB32 = 2, FMGPU_IB16A = 3, /* InterleavedBitvector.h:168-173 */
    FMGPU_IBP16 = 4,                                                 /* InterleavedBitvectorPrefix.h:204-209 */
    FMGPU_EPR8 = 5, FMGPU_EPR16 = 6, FMGPU_EPR32 = 7,                /* InterleavedEPR.h:222-227 */
    FMGPU_EPRV2_8 = 8, FMGPU_EPRV2_16 = 9, FMGPU_EPRV2_32 = 10,      /* InterleavedEPRV2.h:289-309 */
    FMGPU_WAVELET = 11,                                              /* Wavelet.h:27-28 over bitvector::Bitvector */
    FMGPU_EPRV3_8 = 12, FMGPU_EPRV3_16 = 13, FMGPU_EPRV3_32 = 14,    /* EPRV3.h:263-272 */
    FMGPU_EPRV4 = 15,                                                /* EPRV4.h:14 */
    FMGPU_EPRV5 = 16,                                                /* EPRV5.h:14 */
    FMGPU_IEPRV7 = 17,                                               /* InterleavedEPRV7.h:15 */
    FMGPU_FBV_64_64K = 18, FMGPU_FBV_512_64K = 19, FMGPU_FBV_2048_64K = 20   /* FlattenedBitvectors2L.h:274-279; _512_64k is FMIndex's default String (fmindex/FMIndex.h:14) */
} fmgpu_layout;

/* One reference String object, described by the arrays it already holds in host memory.
 * Blocked layouts: `blocks` = String::blocks.data() (sizeof(Block) stride),
 *                  `super_blocks` = String::superBlocks.data() ([k][sigma] uint64).
 * Wavelet:         `nodes` = bit_ceil(sigma) node descriptors = Wavelet::bitvector[i].{superblocks,blocks,bits,totalLength}.
 * EPRV3/4/5/7:     `blocks` = String::bits.data() (one InBits per 64 rows; V7: the packed {bits, level0} structs),
 *                  `super_blocks` = String::superBlocks.data(), `levels[]` = the counter arrays bottom-up:
 *                  EPRV3 {blocks_}, EPRV4 {level0, level1, level2}, EPRV5 {level0, level1}, InterleavedEPRV7 {NULL, level1}.
 * FlattenedBitvectors2L: `blocks` = String::bits.data() (bitct bitsets of l1_bits per block), `super_blocks` = String::l0.data()
 *                  ([k][sigma+1] uint64, n_super_blocks = k), `levels[0]` = String::l1.data() ([k][sigma+1] uint16). */
typedef struct fmgpu_wavelet_node {
    const uint64_t* superblocks; uint64_t n_superblocks;   /* bitvector/Bitvector.h:31 */
    const uint8_t*  blocks;      uint64_t n_blocks;        /* :32 */
    const uint64_t* bits;        uint64_t n_bits;          /* :33 */
    uint64_t total_length;                                 /* :34 */
} fmgpu_wavelet_node;

typedef struct fmgpu_string_desc {
    int32_t  layout;              /* fmgpu_layout */
    int32_t  sigma;               /* String::Sigma, 2..256 */
    uint64_t n;                   /* String::size() */
    const void*     blocks;       uint64_t blocks_bytes;
    const uint64_t* super_blocks; uint64_t n_super_blocks;
    const fmgpu_wavelet_node* nodes; uint64_t n_nodes;
    const void* levels[3];        uint64_t level_bytes[3];
} fmgpu_string_desc;

/* suffixarray::SparseArray<std::tuple<uint32_t,uint32_t>, Bitvector2L<512,65536>> (suffixarray/SparseArray.h:31-76):
 * presence bitvector (bitvector/Bitvector2L.h:30-33) + two bit-packed DenseVectors (DenseVector.h:26-34). */
typedef struct fmgpu_dense_vector_desc {
    const uint64_t* data; uint64_t n_words;
    uint64_t bit_count; uint32_t bits; uint64_t largest_value; uint64_t common_divisor;
} fmgpu_dense_vector_desc;

typedef struct fmgpu_sparse_array_desc {
    uint64_t n;                                   /* rows (== string n) */
    const uint64_t* l0;   uint64_t n_l0;
    const uint16_t* l1;   uint64_t n_l1;
    const uint64_t* bits; uint64_t n_bit_words;   /* 8 words per 512-bit block */
    fmgpu_dense_vector_desc field[2];             /* documents.data[0] = seqId, data[1] = pos */
} fmgpu_sparse_array_desc;

/* FMIndex (fmindex/FMIndex.h:21-23) or BiFMIndex (fmindex/BiFMIndex.h:31-35).  BiFMIndex<String> holds both strings in one String type: bwt_rev must
 * have bwt's n, sigma and layout, or fmgpu_index_create returns FMGPU_ERR_INVALID (the kernels choose their reader by bwt's layout for both). */
typedef struct fmgpu_index_desc {
    fmgpu_string_desc bwt;
    const fmgpu_string_desc* bwt_rev;             /* NULL => unidirectional FMIndex */
    const uint64_t* C;                            /* sigma+1 entries */
    const fmgpu_sparse_array_desc* annotated_array; /* NULL => locate unavailable */
} fmgpu_index_desc;

typedef struct fmgpu_index* fmgpu_index_t;

/* one reported cursor: search/SearchNg26.h:398-403 delegate(qidx, cursor, errors).  Order: the search kernels emit records in no particular
 * order; inside a read, ascending (errors >> 8, seq) is the reference's callback order — `seq` is either the position of the report within its
 * read, or (search_ng26 with <= 2 substitutions / <= 3 edit errors and search_ng21, where idle lanes take over subtrees of a large read) the
 * low 32 bits of a path key whose upper bits sit in errors[8..31].  fmgpu_hits_sort orders the records and leaves seq = the dense callback
 * position, errors = the error count; a caller that reads raw records takes the error count from errors & 0xff. */
typedef struct fmgpu_hit {
    uint64_t qidx, lb, lb_rev, len;
    uint32_t errors, seq;
} fmgpu_hit;

/* search_scheme::Scheme flattened [search][part] (search_scheme/Search.h:19-27) */
typedef struct fmgpu_scheme {
    int32_t n_searches, n_parts;
    const uint64_t* pi; const uint64_t* l; const uint64_t* u;
    const uint64_t* partition;   /* n_parts entries, or NULL = createUniformPartition per query length (expand.h:324-343) */
    int32_t edit;                /* 0: Hamming distance (search_ng26::search<false>); != 0: edit distance (search<true>, the reference's default) */
    int32_t reserved;
} fmgpu_scheme;

/* an EXPANDED scheme, one {pi, l, u} entry per query symbol (search_scheme/expand.h:146-165), flattened [search][length]:
 * what search_ng21 walks (search/SearchNg21.h:184-200 prepare_reorder) */
typedef struct fmgpu_expanded_scheme {
    int32_t  n_searches, reserved;
    uint64_t length;             /* entries per search = symbols of a query that are searched */
    const uint64_t* pi; const uint64_t* l; const uint64_t* u;
} fmgpu_expanded_scheme;

typedef struct fmgpu_stats {
    uint64_t lf_steps;       /* exact search: executed extensions;  k-mismatch: visited nodes (cursor extensions) */
    uint64_t hits;           /* records produced */
    float    kernel_ms;      /* duration of the dominant kernel alone, measured with hipEvents on `stream` (0 if not requested) */
    float    prepass_ms;     /* k-mismatch searches: host-measured duration of the pass that orders the batch's hand-out (reads of high-copy repeats first: a flag
                                kernel, a sample read-back, a partition) when it ran, else 0 — part of a call's wall time, never of kernel_ms (same size and
                                offset as the `reserved` word of ABI 4) */
    /* what the dominant kernel actually asked of the memory system on the index tables, counted by the kernel itself (0 for kernels that do
     * not count): table_bytes = sum over issued table loads of the entry bytes consumed (a 12-byte block entry, an 8-byte walk entry, a
     * 64-byte block of an extend-all, a 16-byte frame ...), table_accesses = number of such accesses that can each touch a different
     * memory line (two loads into the same 64-byte block count once).  Query and result traffic is coalesced and not included.
     * The exact-search family (fmgpu_search_exact and its _packed / _q4 forms, the walk of fmgpu_search_smems) counts by the rule below. */
    uint64_t table_bytes;
    uint64_t table_accesses;
    uint64_t table_steps;    /* exact search from an interval table in front of the pair table or the symbol planes, or along the sample chain: LF steps that the entries stood for (entries used x their symbols); else 0 */
} fmgpu_stats;

/* ---- What fmgpu_stats.table_bytes / table_accesses / table_steps hold after an exact search ------------------------------------------------
 * The three fields are sums over the reads of a batch: a read's share depends on the read, the text and the tables of the handle, not on the reads
 * it shares a wave or a call with (a batch split into two calls adds up to the whole batch's).  tests/exact_traffic_model.py restates this text
 * on the CPU and tests/test_gpu_exact_traffic.py compares every kernel with it, exactly.
 *
 * The walk.  A read of m symbols is consumed from its LAST symbol to its first.  A step starts from an interval [a, b) of rows (the first from
 * [0, n)) and consumes one symbol c: a = C[c] + rank(a, c), b likewise; the walk ends after the step that leaves a == b, or with the read.  lf_steps
 * counts these steps whatever table served them.  A symbol c >= sigma is a step that empties the interval and is NO access.  An access counts
 * when it is issued, also when the step then comes out empty (a pair that finds nothing, a chain entry that does not match).
 * "One per end, one if shared" below means: one access for end a and one for end b, but one in all when a >> k == b >> k for blocks of 2^k rows.
 *
 *   what serves the call                                   one access                                                  bytes per access
 *   one-symbol blocks (k_exact_a; the single steps of      one block entry per end, one if shared (k = 6)              12
 *     every kernel below; the walk of fmgpu_search_smems)
 *     ... the delimiter (c == 0) on a handle with          always 2                                                    12
 *         FMGPU_FMT_FUSED
 *   pair table (k_exact_p)                                  two symbols y, x, both in 1 .. 4: one 128-row line per      68
 *                                                          end, one if shared (k = 7)
 *     ... the odd symbol of a read of odd length,          the FIRST step, taken from C when in 1 .. 4: none; a         0
 *         no interval table in front                       delimiter or foreign byte there is a single step
 *   symbol planes (k_exact_s)                              one 64-row line per end, one if shared (k = 6)              44
 *   multi-ary tree (k_exact_m)                             per step, per level and end one block of 64 node-local      4 + 8 d for a level of d digit bits
 *                                                          positions, one if shared (k = 6)
 *   EPR / EPRV2 blocks read in place (k_exact)             none                                                        0
 *   interval-table entry                                   the entry                                                   8 (16 with 64-bit rows)
 *   k-step table (k_exact_kstep)                           one context entry per end for K symbols, one if shared      12
 *                                                          (k = 6)
 *   walk tables (k_exact_kstep)                            one entry                                                   LF^J: 8 (16); LF^2J: 12 (16)
 *   sample chain (k_exact_chain)                           each block of the seek; the rank -> position word; each     64; 4; 8
 *                                                          chain entry read
 *   fmgpu_search_smems on any other layout                 none                                                        0
 *
 * Pair table.  Without an interval table a read of odd length takes its odd symbol first (above), then pairs.  A pair that holds a delimiter or a
 * foreign byte reads no line; it, and a pair whose line(s) were read and that came out empty, is taken as two single steps on the one-symbol blocks
 * (the second only if the first left rows).  A symbol left over behind the last pair is a single step.
 * Tree.  The levels take digits of 3 / 3 / 2 bits from the top for 8-bit symbols (bit_width(sigma - 1) bits: 1, 2, 3, 2+2, 3+2, 3+3, 3+2+2, 3+3+2).  At a
 * level the position of row i inside its node is the number of rows < i whose symbols share the higher digits of c; every level of a step is
 * read, also when an upper level already left a == b.
 * Interval table of L symbols (in front of the pair table, the symbol planes or inside k_exact_kstep; n > 1).  A read with m >= L whose last L symbols are
 * all in 1 .. sigma - 1 reads its entry: one access.  If the entry is not empty the read starts behind those L symbols, which cost nothing else; otherwise, and
 * for every other read, the walk starts from [0, n) as if there were no table — on the pair table in pairs from the last symbol, so that an odd symbol is
 * left over at the END and is a single step, never a step from C.  table_steps += L per entry that was used, in front of the pair table and the symbol
 * planes; k_exact_kstep leaves table_steps 0.
 * k_exact_kstep (any k-step / walk table, or an interval table that k_exact_p / k_exact_s do not serve).  After the interval entry, the main phase takes one
 * table load per pass: with one row left and 2J symbols remaining (LF^2J table) or J (LF^J table), J = 32 / bit_width(sigma - 2), one walk entry; else with
 * a k-step table one context entry per end for the next K symbols; else one single step.  The phase ends, without an access, at a stretch that is too short
 * or holds a symbol outside 1 .. sigma - 1; and, with the access counted, at a walk entry that met a delimiter and at a context or single step that comes out
 * empty.  A walk entry whose symbols differ from the read's: the symbols before the first differing one still go K at a time through the context table,
 * then the phase ends.  The tail phase takes single steps to the read's end or the empty interval; a step that came out empty in the main phase is issued
 * again there and counts again.  On an occurrence table other than the one-symbol blocks a single step of this kernel counts 2 accesses of 12 bytes.
 * Sample chain (32-bit rows, sigma 5, a batch whose longest read has >= 48 symbols).  The pair-table walk as above, but at the first pass of the pair loop (so
 * behind the odd symbol, then behind every pair or couple of single steps) at which the interval is one row and >= 32 symbols remain, the read is parked.
 * Seek: the 64-byte block of the row is read (one access); if the row is not sampled, fewer than rate - 1 steps were sought, the next symbol is in 1 .. 4
 * and the row holds it, the read steps to the next row and repeats.  Jump, only from a sampled row: the 4-byte rank -> position word and the row's 8-byte
 * chain entry; then, while >= rate symbols remain and the entry is usable (not the first sample of its sequence, no delimiter among the rate symbols in front
 * of it), the entry in front of it is read (8 bytes) and the rate symbols compared: equal moves there (rate steps, table_steps += rate), unequal ends the jump.
 * The rest is the pair-table walk again, in pairs from where the read stands (a symbol left over is a single step at the end).
 *
 * By hand, "x y z" (z consumed first) on a 32-bit-row sigma = 5 handle with FMGPU_FMT_PAIRS, no other table, a short batch: z in 1 .. 4 comes from C, no access;
 * the pair (y, x) starts from [C[z], C[z + 1]): 68 bytes if both ends share a 128-row line, else 136; if it comes out empty, y is read again as a single step
 * (12 or 24 bytes from the same interval) and x, if y left rows, as another.  With FMGPU_SEL_EXACT_ONE_SYMBOL: three steps of 12 or 24 bytes each, as long as rows are left.
 *
 * Other kernels.  k_scheme_lean (k-mismatch search on dense DNA blocks or one-symbol blocks) uses the fields as plain counters: table_accesses = blocks it
 * fetched (a node whose ends lie in two blocks counts two, a node re-visited for its next sibling fetches again), table_bytes = visited nodes of SEVERAL rows — a
 * count, not bytes (the other visited nodes stood on one row) — and table_steps = nodes that prefix-table entries stood for.  The other depth-first kernels and
 * locate follow the one-line description at the fields; no test pins them yet. */

/* Library options: process-wide, read when a handle is created / a call starts (set them before, not during, the calls they concern).
 * The first seven, FMGPU_OPT_BUCKET_ROWS and FMGPU_OPT_SAMPLE_CHAIN choose what a handle holds or how a batch / a construction is prepared — results never depend on them; FORCE_WIDE, KERNEL_SELECT and FAIL_SCRATCH are test hooks. */
typedef enum fmgpu_option {
    FMGPU_OPT_PAIR_TABLE = 0,      /* 1 (default): a sigma = 5 bwt gets the symbol-pair table (exact search takes two symbols per step) */
    FMGPU_OPT_DENSE_DNA = 1,       /* 1: both strings of a sigma = 5 BiFMIndex with 32-bit rows get dense DNA blocks (equal-length k-mismatch kernel) */
    FMGPU_OPT_SYMBOL_PLANES = 2,   /* 1: a Wavelet / EPR / EPRV2 bwt with 6 <= sigma <= 29 gets the symbol-plane table (one line per LF step and end) */
    FMGPU_OPT_EXPAND_DNA = 3,      /* 1: sigma = 5 strings handed over as EPR / EPRV2 blocks or as a Wavelet are expanded into the one-symbol block table at creation */
    FMGPU_OPT_LF_TABLE = 4,        /* 1: the explicit LF mapping is built at creation (fmgpu_index_accelerate_lf adds / drops it later) */
    FMGPU_OPT_FUSED_LOCATE = 5,    /* 1: the sampled suffix array's presence bits are fused into the sigma <= 5 blocks (one line per locate step) */
    FMGPU_OPT_HEAVY_FIRST = 6,     /* 1: k-mismatch batches are handed out with the reads of high-copy repeats first */
    FMGPU_OPT_FORCE_WIDE = 7,      /* test hook, 0: 1 = every new handle is held in 64-bit-row tables whatever its size */
    FMGPU_OPT_KERNEL_SELECT = 8,   /* test / A-B hook, 0: FMGPU_SEL_* bits — which of several result-identical kernels serves a call */
    FMGPU_OPT_FAIL_SCRATCH = 9,    /* test hook, 0: k = the k-th allocation of the next per-thread call scratch fails */
    FMGPU_OPT_BUCKET_ROWS = 10,    /* 0 (default): the bucketed suffix sorters cut their buckets as large as the free device memory allows; k > 0: k rows per bucket at most */
    FMGPU_OPT_SUFFIX_SORTER = 11,  /* which suffix sorter fmgpu_build_index uses (results do not depend on it).  0 (default): by the memory each needs —
                                    * 1: all suffixes at once: suffix array + rank array + keys of all rows (30 / 42 bytes per row with 32- / 64-bit rows beside the text);
                                    * 2: bucket by bucket with the inverse suffix array as rank array (6 / 10 bytes per row beside the text + one bucket + ~60 bytes per row that shares
                                    *    its first 12-21 symbols with another): prefix doubling on the ties, the suffix array itself is never held;
                                    * 3: bucket by bucket without any array of n entries (2 bytes per row + one bucket): ties are broken by reading further symbols, a text with
                                    *    very long exact repeats is refused (FMGPU_ERR_UNSUPPORTED) */
    FMGPU_OPT_SAMPLE_CHAIN = 12,   /* 1 (default): a sigma = 5 index with 32-bit rows, the pair table and a sampled suffix array of rate <= 16 gets the sample chain (12 bytes per sample:
                                    * exact search moves a one-row read `rate` symbols per 8-byte entry along the sampled rows in text order) */
    FMGPU_OPT_COUNT_ = 13
} fmgpu_option;
/* bits of FMGPU_OPT_KERNEL_SELECT: each takes a call off the kernel the library would pick (the parity tests run every kernel through them) */
#define FMGPU_SEL_GENERAL_DFS      (1 << 1)   /* search_ng26 / ng21: the general kernels (k_scheme, k_scheme_edit, k_ng21) */
#define FMGPU_SEL_NO_PREFIX_TABLE  (1 << 2)
#define FMGPU_SEL_NO_LF3           (1 << 3)   /* no LF^1..3 walk table */
#define FMGPU_SEL_NO_LF_GENERAL    (1 << 4)   /* no LF table in the general kernels */
#define FMGPU_SEL_NO_WALK_TABLE    (1 << 5)
#define FMGPU_SEL_NO_LENGTH_BUCKETS (1 << 6)
#define FMGPU_SEL_EXACT_ON_TREE    (1 << 21)  /* exact search on the wavelet levels although the symbol-plane table exists (k_exact_m) */
#define FMGPU_SEL_EXACT_ONE_SYMBOL (1 << 22)  /* exact search in one-symbol steps although the pair table exists (k_exact_a) */
#define FMGPU_SEL_LOCATE_PER_LANE  (1 << 23)  /* locate with one row per lane (k_locate_fused) instead of the quad-cooperative kernel */
#define FMGPU_SEL_NO_SHARING       (1 << 24)  /* no work sharing between the lanes of a wave */
#define FMGPU_SEL_NO_EXACT_LUT     (1 << 25)  /* exact search does not start from the interval table in front of the pair table */
#define FMGPU_SEL_NO_BOARD         (1 << 26)  /* no work sharing between the waves of a launch (the lanes of a wave still share) */
#define FMGPU_SEL_UNPACK_QUERIES   (1 << 27)  /* every `_q4` call unpacks its batch into a byte scratch and runs the byte kernels, also where a kernel reads the packed form itself */
#define FMGPU_SEL_NO_SAMPLE_CHAIN  (1 << 28)  /* exact search stays on the pair table for one-row reads although the sample chain exists */
#define FMGPU_SEL_LEAN_FORMAT_A    (1 << 29)  /* k_scheme_lean on the one-symbol blocks although dense DNA blocks exist */
#define FMGPU_SEL_NO_LEAN          (1 << 30)  /* k_scheme_fast<PLAIN> instead of k_scheme_lean */
#define FMGPU_SEL_ALL (FMGPU_SEL_GENERAL_DFS | FMGPU_SEL_NO_PREFIX_TABLE | FMGPU_SEL_NO_LF3 | FMGPU_SEL_NO_LF_GENERAL | FMGPU_SEL_NO_WALK_TABLE | FMGPU_SEL_NO_LENGTH_BUCKETS | \
                       FMGPU_SEL_EXACT_ON_TREE | FMGPU_SEL_EXACT_ONE_SYMBOL | FMGPU_SEL_LOCATE_PER_LANE | FMGPU_SEL_NO_SHARING | FMGPU_SEL_NO_EXACT_LUT | FMGPU_SEL_NO_BOARD | FMGPU_SEL_UNPACK_QUERIES | FMGPU_SEL_NO_SAMPLE_CHAIN | FMGPU_SEL_LEAN_FORMAT_A | FMGPU_SEL_NO_LEAN)
int         fmgpu_set_option(int32_t option, int64_t value);
int         fmgpu_get_option(int32_t option, int64_t* value);

int         fmgpu_abi_version(void);
const char* fmgpu_last_error(void);
int         fmgpu_device_count(int* count);
int         fmgpu_set_device(int device);   /* hipSetDevice for the calling thread.  A handle lives on the device that was current when it was created;
                                               calls on it must be made with that device current (one process per GPU needs a single call at start-up) */

/* index upload: copies (and re-lays out for HBM) the arrays; the caller keeps ownership of host memory.
 * replaces: FMIndex(span bwt, SparseArray) fmindex/FMIndex.h:30-34, BiFMIndex(...) fmindex/BiFMIndex.h:40-51 */
int fmgpu_index_create(const fmgpu_index_desc* desc, fmgpu_index_t* out);
int fmgpu_index_destroy(fmgpu_index_t h);
int fmgpu_index_info(fmgpu_index_t h, uint64_t* n, int32_t* sigma, int32_t* layout, int32_t* bidirectional, uint64_t* device_bytes);
int fmgpu_index_row_bits(fmgpu_index_t h, int32_t* bits);   /* 32 or 64: the width of the device tables this index is held in */
/* what the handle's bwt is held in at this moment (FMGPU_FMT_* bits): tells which kernel serves a search — e.g. exact search takes the pair table when
 * FMGPU_FMT_PAIRS is set, the symbol planes when FMGPU_FMT_PLANES is set and the handle has no one-symbol blocks, the interval / k-step / walk tables when any exists */
#define FMGPU_FMT_BLOCKS     (1u << 0)   /* one-symbol block table (the InterleavedBitvector* layouts, or the expansion of another layout) */
#define FMGPU_FMT_PAIRS      (1u << 1)   /* symbol-pair table */
#define FMGPU_FMT_DENSE      (1u << 2)   /* dense DNA blocks */
#define FMGPU_FMT_PLANES     (1u << 3)   /* symbol-plane table */
#define FMGPU_FMT_TREE       (1u << 4)   /* multi-ary wavelet tree (a Wavelet string) */
#define FMGPU_FMT_REFERENCE  (1u << 5)   /* EPR / EPRV2 blocks read in place */
#define FMGPU_FMT_LF         (1u << 6)   /* explicit LF mapping */
#define FMGPU_FMT_KSTEP      (1u << 7)   /* multi-symbol-step table */
#define FMGPU_FMT_INTERVALS  (1u << 8)   /* interval table of fmgpu_index_accelerate_exact */
#define FMGPU_FMT_WALK       (1u << 9)   /* walk tables */
#define FMGPU_FMT_PREFIX     (1u << 10)  /* prefix table of fmgpu_index_accelerate_search */
#define FMGPU_FMT_LOCATE     (1u << 11)  /* locate answer table */
#define FMGPU_FMT_FUSED      (1u << 12)  /* presence bits of the sampled suffix array fused into the blocks */
#define FMGPU_FMT_EXTRACT    (1u << 13)  /* text map and sample table of fmgpu_index_accelerate_extract */
#define FMGPU_FMT_CHAIN      (1u << 14)  /* sample chain: the sampled rows in text order with the symbols between them */
int fmgpu_index_formats(fmgpu_index_t h, uint32_t* mask);

/* The library's own index file — replaces saveIndex / loadIndex (fmindex/diskStorage.h:12-27) for a handle of this library: a header, a description of
 * the handle and every device array as it sits in HBM, each with a checksum; include_tables != 0 also stores whatever optional tables the handle
 * holds at that moment (LF, k-step, interval, walk, prefix, locate tables, Format A expansion), so that a process start costs one read and one copy per
 * array instead of a suffix sort and the table construction.  fmgpu_index_load creates the handle on the calling thread's current device; a file
 * that is truncated, damaged (checksums), of another format / ABI version or byte order, or whose description does not fit its own n / sigma / layouts (every
 * array size is checked against what creation would allocate, before anything is allocated) is refused with an error code and nothing is created.
 * NOT the reference's cereal format: its byte layout for the mmser members cannot be pinned without a reference-written file. */
int fmgpu_index_save(fmgpu_index_t h, const char* path, int32_t include_tables);
int fmgpu_index_load(const char* path, fmgpu_index_t* out);
/* A copy of the handle on the calling thread's CURRENT device: every array the handle holds (optional tables included) travels device to device (hipMemcpyPeer: over
 * xGMI, no host copy), the derived tables are rebuilt there.  SURVEY 8e: "upload once to GPU0 then hipMemcpyPeer rather than 8 PCIe uploads"; fmgpu_replicas_load uses it. */
int fmgpu_index_clone(fmgpu_index_t h, fmgpu_index_t* out);

/* The explicit LF mapping (one word per row and direction: LF(row) = C[s] + rank(row, s) of the row's own symbol s): one-load one-row
 * search nodes and locate steps, and what the walk tables are built from.  Built at creation unless FMGPU_OPT_LF_TABLE is 0; enable = 0 drops it (the walk tables must have been dropped before), enable != 0 builds it.  Without it the index is the
 * bit-packed occurrence table alone (GRCh38: 3.1 GB per direction).  Results are unchanged. */
int fmgpu_index_accelerate_lf(fmgpu_index_t h, int32_t enable);

/* Optional accelerator for fmgpu_search_exact: a k-symbol-step occurrence table (one table entry advances a cursor by `kstep`
 * symbols, so a query touches 1/kstep as many HBM lines).  Built on the device from the index itself; needs
 * (sigma-1)^kstep <= 255 contexts and 16 * (sigma-1)^kstep / 64 bytes per row of HBM (DNA, kstep 3: 16 B/row).  Results of every search
 * stay identical; kstep = 1 removes the k-step table.  Same idea as the reference's BiFMIndexKStep (fmindex/BiFMIndexKStep.h).
 * For InterleavedEPR* / InterleavedEPRV2* / Wavelet indices any kstep >= 1 first expands the occurrence table on the device into the
 * one-line-per-LF-step block format the InterleavedBitvector* layouts are held in (12 * sigma / 64 bytes per row and direction; a
 * Wavelet step otherwise touches bit_width(sigma-1) lines); every search kernel then reads that table, fmgpu_string_query keeps
 * answering from the native layout.  kstep = 0 removes the k-step table and the expansion. */
int fmgpu_index_accelerate(fmgpu_index_t h, int32_t kstep);   /* (all fmgpu_index_accelerate* calls modify the handle: not concurrently with searches on it) */

/* fmgpu_index_accelerate plus two more optional tables for fmgpu_search_exact (results unchanged):
 *   lut_len > 0: the interval of every string of `lut_len` symbols ((sigma-1)^lut_len entries of 8 bytes; DNA, 12 symbols: 134 MB) — a query
 *                starts from the entry of its last lut_len symbols instead of lut_len wide-interval steps;
 *   walk != 0:   per row LF^J and the J symbols met on the way, J = 32 / bit_width(sigma-2) (DNA: 16 symbols, protein: 6; 8 bytes per row):
 *                once the interval is one row, J query symbols are checked and consumed with one load;
 *   walk >= 2:   additionally LF^(2J) and the 2J symbols (12 bytes per row): 32 bp / 12 aa per load while that many symbols remain.
 * 64-bit-row indices: kstep <= 1 (the multi-symbol-step table holds 32-bit counts), every entry of the interval and walk tables is 16 bytes. */
int fmgpu_index_accelerate_exact(fmgpu_index_t h, int32_t kstep, int32_t lut_len, int32_t walk);

/* Optional accelerators for fmgpu_search_scheme on a BiFMIndex (results unchanged):
 *   prefix_len > 0: table of the bidirectional SA interval of every string of `prefix_len` symbols ((sigma-1)^prefix_len entries of 16 bytes; DNA,
 *                   11 symbols: 67 MB; 16 symbols: 69 GB, at most 2^32 entries) — the always-exact first part of a search (u[0] = 0, search_scheme/generator/h2.h) starts from its entry;
 *   walk & 1:       per row and direction LF, LF^2, LF^3 (12 bytes): a cursor of one row advances up to three symbols per load;
 *   walk & 2:       per row and direction LF^J and the J symbols met (8 bytes, J = 32 / bit_width(sigma-2)): with 2-bit symbols (sigma <= 5) a
 *                   one-row cursor advances 16 symbols per load wherever 16 steps of a search go in one direction. */
int fmgpu_index_accelerate_search(fmgpu_index_t h, int32_t prefix_len, int32_t walk);

/* Optional accelerator for fmgpu_locate (results unchanged): every row is located once and its (seqId, pos, steps) answer kept,
 * 12 bytes per row — one load per located row instead of ~samplingRate/2 LF steps with a presence-bit probe each.  enable = 0 drops it. */
int fmgpu_index_accelerate_locate(fmgpu_index_t h, int32_t enable);

/* Optional table for fmgpu_extract and fmgpu_sequence_lengths, built on the device from what the handle holds; enable = 0 drops it.
 *   - Text map: the sentinel rows 0 .. C[1]-1 are located; per seqId (ascending) its length = the pos of its LAST delimiter, its end row = that
 *     delimiter's sentinel row.  An earlier delimiter of the same seqId is an ordinary symbol 0 of the text.
 *   - Sample table: every sampled row, ordered by (seqId, pos).  Sampling may be irregular.  About 12 bytes per sample with 32-bit rows.
 * Returns FMGPU_ERR_UNSUPPORTED, and keeps nothing, if a sampled entry names a seqId no sentinel row gave (e.g. an index built without delimiters) or a
 * pos beyond that seqId's length.  The table counts in device_bytes and sets FMGPU_FMT_EXTRACT.  fmgpu_index_save does not store it and
 * fmgpu_index_clone does not carry it: call this again after a load or a clone.  Like the other accelerate calls it modifies the handle: not
 * concurrently with other calls on the same handle. */
int fmgpu_index_accelerate_extract(fmgpu_index_t h, int32_t enable);

/* The text map of fmgpu_index_accelerate_extract: seqIds in ascending order and each one's length (without its last delimiter).  *out_count = the
 * number of seqIds; FMGPU_ERR_CAPACITY (nothing written) if it exceeds `capacity`.  FMGPU_ERR_UNSUPPORTED without the table.  Host buffers. */
int fmgpu_sequence_lengths(fmgpu_index_t h, uint64_t* seq_ids, uint64_t* lengths, uint64_t capacity, uint64_t* out_count);

/* one text range of fmgpu_extract: symbols pos .. pos + len - 1 of sequence seq_id */
typedef struct fmgpu_text_range {
    uint64_t seq_id, pos, len;
} fmgpu_text_range;     /* 24 bytes */

/* Text symbols (ranks 0 .. sigma-1) of every range, concatenated in the given order, read from the index by LF walks on the device (the range is cut
 * into pieces at the sampled positions inside it; each piece walks back from a sampled row or from the sequence's end row).  What the reference's
 * reconstructText (utils.h:672-703) walks serially from each sequence's end.
 *   - *out_count = the sum of len, on success and on FMGPU_ERR_CAPACITY alike; above `capacity` the call returns FMGPU_ERR_CAPACITY and writes nothing.
 *   - FMGPU_ERR_INVALID: an unknown seq_id or pos + len beyond the sequence's length (checked on the device), a null ranges / out / out_count while
 *     count > 0.  count == 0 returns 0.  FMGPU_ERR_UNSUPPORTED without fmgpu_index_accelerate_extract's table.
 *   - ranges and out may be host or device memory; the call returns after completion (its scratch is freed).
 *   - stats: lf_steps = LF steps walked (the symbols of every piece, including those a range's last piece walks past beyond its end), hits = symbols
 *     written, kernel_ms = the walk kernel alone. */
int fmgpu_extract(fmgpu_index_t h, const fmgpu_text_range* ranges, uint64_t count, uint8_t* out, uint64_t capacity, uint64_t* out_count,
                  fmgpu_stats* stats, void* stream);

/* String_c batch evaluation (string/concepts.h:25-87): what[i] selects 0 = rank(idx,symb), 1 = prefix_rank(idx,symb),
 * 2 = symbol(idx); which = 0 -> bwt, 1 -> bwtRev */
int fmgpu_string_query(fmgpu_index_t h, int which, const uint64_t* idx, const uint8_t* symb, const uint8_t* what,
                       uint64_t count, uint64_t* out, void* stream);

/* search_no_errors::search (search/SearchNoErrors.h:12-26 per query / :28-86 batched): out_lb/out_len = cursor after the
 * last executed extension (len == 0: no occurrence) */
int fmgpu_search_exact(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                       uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats, void* stream);

/* the same search, each cursor as ONE word  lb << 32 | len  (32-bit-row indices only): the 8-byte-per-read form in which a rank's
 * intervals travel to the gathering rank ("only an RCCL gather of the resulting SA intervals") */
int fmgpu_search_exact_packed(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                              uint64_t* out_interval, fmgpu_stats* stats, void* stream);

/* ---- 4-bit packed query batches ------------------------------------------------------------------------------------------------------
 * The packed form of a batch holds one symbol per nibble instead of one per byte:
 *   - symbol i of the batch (i = qoff[q] + j for symbol j of read q) is nibble i & 1 of byte i >> 1 of the packed buffer; the EVEN index is the LOW nibble;
 *   - qoff is the array of the byte form: nq + 1 entries, counted in symbols, non-decreasing; qoff[0] need not be 0 and may be odd, so two reads may share a byte;
 *   - nibble 15 means "not a symbol"; any nibble >= sigma behaves like a byte >= sigma does in the byte form;
 *   - only indices with sigma <= 15 take packed queries (FMGPU_ERR_UNSUPPORTED otherwise, nothing written);
 *   - a kernel loads only the aligned 16-byte chunks that hold nibbles of the read it serves; a host buffer is staged with half the bytes of the byte form.
 * Calls that take this form end in `_q4` (fmgpu_search_exact_packed means packed OUTPUT and is not one of them).
 *
 * fmgpu_queries_pack4 packs a byte batch on the device; qbuf / qoff and out_packed / out_qoff may each be host or device memory.
 *   - a byte >= sigma becomes 15; the output batch starts at symbol 0 (out_qoff[0] = 0, nq + 1 entries); it takes (out_qoff[last] + 1) / 2 bytes, and a
 *     nibble left over in the last byte is 0;
 *   - complement != NULL (sigma entries, host or device): the output holds 2 nq reads and out_qoff 2 nq + 1 entries.  Read 2q is read q; read 2q + 1 is read q
 *     reversed, with complement[c] for c < sigma and 15 for the rest — a read followed by its reverse complement, the batch a both-strand search takes;
 *   - sigma outside 2 .. 15: FMGPU_ERR_UNSUPPORTED; a null pointer while nq > 0: FMGPU_ERR_INVALID; nq == 0 returns 0.
 * fmgpu_queries_unpack4 writes symbols qoff[0] .. qoff[nq] - 1 of a packed batch as bytes out_bytes[0 ..] (nibble 15 -> 255); the same errors. */
int fmgpu_queries_pack4(const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, int32_t sigma, const uint8_t* complement,
                        uint8_t* out_packed, uint64_t* out_qoff, void* stream);
int fmgpu_queries_unpack4(const uint8_t* packed, const uint64_t* qoff, uint64_t nq, uint8_t* out_bytes, void* stream);

/* fmgpu_search_exact / fmgpu_search_scheme / fmgpu_search_ng21 for a packed batch: every result (intervals and miss rows, hit records, out_count,
 * stats.lf_steps / hits / table_*) is exactly what the byte call returns for fmgpu_queries_unpack4(packed).  Exact search on the pair table (with or without
 * the interval table in front) and on the one-symbol blocks reads the packed form itself and stays asynchronous for device buffers; exact search behind k-step /
 * walk tables, on symbol planes, the wavelet tree or reference blocks, and both scheme searches unpack the batch into a per-call byte scratch first, which is
 * freed on return: those calls synchronise `stream`. */
int fmgpu_search_exact_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                          uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats, void* stream);
int fmgpu_search_scheme_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                           const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                           fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream);
int fmgpu_search_ng21_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                         const fmgpu_expanded_scheme* scheme, uint64_t max_hits_per_query,
                         fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream);

/* A profile of the same search: out_depth[q] = query symbols consumed until the cursor holds at most one row (0 rows included), or
 * length + 1 if it still holds several rows at the end.  The root cursor holds all n rows, so an empty read gives 1 (0 when n <= 1, where nothing
 * is consumed of any read).  A symbol >= sigma is counted as consumed and empties the cursor.  nq == 0 returns 0; a null qbuf, qoff or out_depth
 * with nq > 0 is FMGPU_ERR_INVALID.  (Tells how much of a batch the one-row walk tables can serve; bench.py reports
 * the distribution for each text.) */
int fmgpu_search_exact_depth(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, uint32_t* out_depth, void* stream);

/* Cursor steps, batched: FMIndexCursor / BiFMIndexCursor::extendLeft(symb), extendRight(symb) (fmindex/FMIndexCursor.h:33-37,
 * fmindex/BiFMIndexCursor.h:113-128) for `count` cursors {lb, lb_rev, len}, or — symb == NULL — extendLeft() / extendRight() over all
 * symbols (FMIndexCursor.h:38-53, BiFMIndexCursor.h:58-82): then every cursor yields sigma cursors, out[i * sigma + c].
 * direction 0 = left, 1 = right (BiFMIndex only).  For a unidirectional FMIndex lb_rev is ignored and may be NULL, and out_lb_rev may be NULL
 * (where it is given it receives zeros).
 * A cursor that does not lie inside the index (lb + len > n, or lb_rev + len > n on a BiFMIndex; a len of 2^64 - 1 does not wrap), or a symb[i] >= sigma,
 * yields {0, 0, 0} for that cursor — in every one of its sigma slots in the all-symbols form; no table is read for it, the other cursors of the batch
 * are not affected.  An empty cursor inside the index (len == 0, lb <= n) is stepped like any other: the result is empty and carries the reference's lb.
 * FMGPU_ERR_INVALID: a null handle; a direction other than 0 and 1; direction 1 on a unidirectional FMIndex; with count > 0 a null lb, len, out_lb
 * or out_len, and on a BiFMIndex a null lb_rev or out_lb_rev.  count == 0 returns 0 whatever the pointers.
 * symbolLeft / symbolRight of a cursor (BiFMIndexCursor.h:180-190) are fmgpu_string_query(what = 2) on bwt at lb / on bwtRev at lb_rev. */
int fmgpu_cursor_extend(fmgpu_index_t h, int32_t direction, uint64_t count, const uint64_t* lb, const uint64_t* lb_rev, const uint64_t* len,
                        const uint8_t* symb, uint64_t* out_lb, uint64_t* out_lb_rev, uint64_t* out_len, void* stream);

/* search_ng26::search<Edit=false>(index, queries, scheme, partition, delegate, n) (search/SearchNg26.h:426-433);
 * BiFMIndex only.  max_hits_per_query = n (UINT64_MAX = unlimited).  Records are appended in no particular order across
 * queries; fmgpu_hits_sort restores the reference's callback order (see fmgpu_hit).  *out_count = records produced (also when > capacity). */
int fmgpu_search_scheme(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                        const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                        fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream);

/* search_ng21::search(index, queries, search_scheme, delegate) and search_n(..., n, delegate) (search/SearchNg21.h:205-240):
 * edit-distance search over an expanded scheme; BiFMIndex only.  max_hits_per_query = n (UINT64_MAX = search).  Queries shorter than
 * scheme->length (which the reference would read out of bounds) produce nothing; of longer ones the first `length` symbols' positions
 * pi[] are searched, as in the reference.  Records as for fmgpu_search_scheme; errors <= 127.  search_best / search_best_n
 * (:242-293: first scheme of a list with any hit) are fmgpu_search_best_ng21 below. */
int fmgpu_search_ng21(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                      const fmgpu_expanded_scheme* scheme, uint64_t max_hits_per_query,
                      fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream);

/* ---- Hamming search with a scoring matrix ---------------------------------------------------------------------------------------------------
 * search_hamming_sm::search(index, queries, scheme, ScoringMatrix<QuerySigma, RefSigma>, delegate) (search/SearchHammingSM.h:188-212): the search-scheme Hamming
 * walk in which every (query symbol, text symbol) pair is a free match, a mismatch that costs one error, or not pairable.  The query alphabet may be larger than
 * the index's: a DNA read with N, an IUPAC primer on a sigma = 5 index, a 28-letter protein query alphabet on 21 ranks.  BiFMIndex only, sigma <= 32.
 *   - Matrix (host memory): query bytes 0 .. query_sigma - 1 have a row; bit r of free_mask[c] = text symbol r matches query symbol c at no cost, bit r of
 *     cost_mask[c] = the pairing costs one error.  A query byte >= query_sigma, or one whose two masks are empty, pairs with nothing.  The library treats no symbol
 *     specially: the delimiter 0 is pairable exactly where a mask says so.
 *   - The walk: one pass per search s of the scheme, in order.  Part lengths are createUniformPartition(P, m), or scheme->partition if given; a read of another
 *     total length is skipped, as in fmgpu_search_scheme.  A state is (cursor, e, part p, symbols left in the part); the part is consumed rightwards if p == 0 or
 *     pi[p-1] < pi[p], else leftwards.  At a state with symbols left, c = the next query symbol, F = the members of free_mask[c], K = those of cost_mask[c], both in
 *     ascending symbol order.  If e + 1 <= u[p] the children are the cursor extended by every r in F with e unchanged, then by every r in K with e + 1; if
 *     e + 1 > u[p], only the children of F.  Empty children are dropped.  A part that is used up continues into part p + 1 iff l[p] <= e; a new part is entered only
 *     if e <= u[p]; after the last part the cursor is reported iff l[P-1] <= e <= u[P-1].
 *   - A read with m < P produces nothing (the rule of fmgpu_search_scheme; the reference would walk empty parts).  Reads of up to 65534 symbols.
 *   - Deviation: the reference keeps noCostList / costList in the order of the setCost calls; this call walks ascending symbols, which is the reference's order when
 *     setCost is called in ascending refRank per query rank (its default constructor and its test do so).
 *   - Records: {qidx, lb, lb_rev, len, errors = e, seq = position of the report within its read in the depth-first order above}: fmgpu_hits_sort returns the
 *     reference's callback order, and the records go into fmgpu_locate_hits as they are.
 *   - max_hits_per_query = n as for fmgpu_search_scheme: the last cursor of a read is clipped to what is left of n, the read's remaining searches are skipped once n
 *     is reached, 0 produces nothing.  *out_count = the records produced, on success and on FMGPU_ERR_CAPACITY alike.
 *   - stats: lf_steps = the extensions the reference executes — one per state expanded over all symbols (e + 1 <= u[p]), |F| per state expanded in matches-only
 *     mode, empty results included; hits = records; kernel_ms = the search kernel alone; table_bytes / table_accesses as fmgpu_search_scheme's general kernel counts.
 *   - FMGPU_ERR_INVALID: a unidirectional handle (the message of fmgpu_search_scheme); scheme->edit != 0; a null matrix or mask array; query_sigma outside 1 .. 256; a
 *     mask bit >= sigma; a query symbol whose two masks overlap.  FMGPU_ERR_UNSUPPORTED: sigma > 32 (the masks are one word).  A bad scheme: the codes of
 *     fmgpu_search_scheme.  nq == 0 returns 0 before the handle is looked at.
 *   - qbuf / qoff / out may each be host or device memory; qoff[0] need not be 0.  The call returns after completion.
 *   - Not served: `_q4` batches, feeds, replicas, the best-stratum ladder, and work sharing between lanes or waves (a lane walks its read alone). */
typedef struct fmgpu_scoring_matrix {
    int32_t query_sigma;        /* 1 .. 256: query bytes 0 .. query_sigma-1 have a row */
    int32_t reserved;           /* 0 */
    const uint32_t* free_mask;  /* query_sigma words: bit r set = text symbol r matches this query symbol at no cost */
    const uint32_t* cost_mask;  /* query_sigma words: bit r set = pairing with text symbol r costs one error */
} fmgpu_scoring_matrix;         /* host memory */
int fmgpu_search_hamming_sm(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                            const fmgpu_scheme* scheme, const fmgpu_scoring_matrix* matrix, uint64_t max_hits_per_query,
                            fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats, void* stream);

/* Best-stratum search: a ladder of schemes walked over one batch in one call — what search_ng26::search_best with an explicit scheme list
 * (search/SearchNg26.h:447-469) and search_ng21::search_best / search_best_n (search/SearchNg21.h:242-293) cut per read, cut per batch on the device.
 * Marking the found reads, selecting and compacting the others and renaming qidx are device passes; neither the queries nor the found set come back to the host
 * between strata.  BiFMIndex only.
 *   - Ladder and found: stratum i is exactly fmgpu_search_scheme / fmgpu_search_ng21 with schemes[i] (its own partition and edit) and max_hits_per_query, over the
 *     reads still unfound, in batch order.  A read is found in stratum i if that stratum produced a record of it with len > 0; a found read takes no part in later
 *     strata; the ladder ends early once no read is left.  A read no stratum can search (an empty read; for ng21 a read shorter than that scheme's length) stays unfound.
 *   - Records: the records of stratum 0 come first, then stratum 1's, and so on (stats[i].hits gives the block sizes); inside a block the order is arbitrary, as for
 *     the single-scheme calls.  Every field is what the single-scheme call emits except qidx, which is the read's number in the caller's batch.  All records of one
 *     read come from one stratum: fmgpu_hits_sort on the output gives the reference's callback order, and fmgpu_locate_hits takes the output as it is.
 *   - out_stratum (nq entries or NULL; host or device memory): out_stratum[q] = the stratum that found read q, 255 if none did.
 *   - n_schemes: 0 .. 254, anything else returns FMGPU_ERR_INVALID.  n_schemes == 0 or nq == 0 returns 0 with *out_count = 0 and a non-NULL out_stratum all 255
 *     (decided before the handle is looked at).
 *   - stats (n_schemes entries or NULL): stats[i] = the stratum's own fmgpu_stats, all zero for a stratum that did not run; kernel_ms = that stratum's search kernel alone.
 *   - Capacity: stratum i writes to out + produced and may use capacity - produced records.  If a stratum overflows, the call returns FMGPU_ERR_CAPACITY with
 *     *out_count = the records produced up to and including that stratum — a lower bound of the total that always exceeds `capacity`; later strata do not run and the
 *     contents of out and out_stratum are unspecified.  A retry loop that grows to max(*out_count, 2 x capacity) ends within n_schemes rounds.
 *   - Errors: every scheme is checked before anything runs; codes and messages for a bad scheme, a unidirectional handle, null pointers (qbuf / qoff / out_count; out while
 *     capacity > 0; schemes) and sigma > 15 for `_q4` are those of the single-scheme calls.  More than 2^31 - 1 reads: FMGPU_ERR_UNSUPPORTED.
 *   - qbuf / qoff / out / out_stratum may each be host or device memory.  One 16-byte read-back per stratum (reads left, symbols left) sizes the next launch; the call
 *     returns after completion and frees its scratch (25 bytes per read, and the symbols of the reads stratum 0 left) on return.
 *   - `_q4`: `packed` in place of qbuf, the rules of the other `_q4` calls; the batch is unpacked once into a byte scratch and the ladder continues in bytes. */
int fmgpu_search_best(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                      const fmgpu_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                      fmgpu_hit* out, uint64_t capacity, uint64_t* out_count,
                      uint8_t* out_stratum, fmgpu_stats* stats, void* stream);
int fmgpu_search_best_ng21(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                           const fmgpu_expanded_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                           fmgpu_hit* out, uint64_t capacity, uint64_t* out_count,
                           uint8_t* out_stratum, fmgpu_stats* stats, void* stream);
int fmgpu_search_best_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                         const fmgpu_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                         fmgpu_hit* out, uint64_t capacity, uint64_t* out_count,
                         uint8_t* out_stratum, fmgpu_stats* stats, void* stream);
int fmgpu_search_best_ng21_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                              const fmgpu_expanded_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                              fmgpu_hit* out, uint64_t capacity, uint64_t* out_count,
                              uint8_t* out_stratum, fmgpu_stats* stats, void* stream);

/* search_backtracking::search(index, queries, maxErrors, delegate) (search/Backtracking.h:85-89); FMIndex or BiFMIndex */
int fmgpu_search_backtracking(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                              uint64_t max_errors, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count,
                              fmgpu_stats* stats, void* stream);

/* FMIndex::locate / BiFMIndex::locate (fmindex/FMIndex.h:113-124, fmindex/BiFMIndex.h:176-202), one SA row per entry:
 * out_seq/out_pos = sampled entry reached, out_steps = LF steps walked (text position = pos + steps, locate.h:46-56) */
int fmgpu_locate(fmgpu_index_t h, const uint64_t* rows, uint64_t count,
                 uint64_t* out_seq, uint64_t* out_pos, uint64_t* out_steps, fmgpu_stats* stats, void* stream);

/* One located row of a hit record: what fmc::Search reports for it (search/search.h:55-59). */
typedef struct fmgpu_position {
    uint64_t qidx;      /* the hit's qidx */
    uint64_t seq_id;    /* seqId of the sampled entry reached */
    uint64_t pos;       /* its pos + the LF steps walked = pos + offset (locate.h:46-56) */
    uint32_t errors;    /* the hit's errors & 0xff */
    uint32_t hit;       /* index of the hit record the row belongs to, low 32 bits */
} fmgpu_position;       /* 32 bytes */

/* Every row of every hit record located in one call: the loop `for (auto [seqId, pos, offset] : LocateLinear{index, cursor})` of fmc::Search
 * (search/search.h:48-75, locate.h:14-57) over a whole batch of cursors.  The rows are generated inside the locate kernels from the hits' {lb, len};
 * no array of rows is built.
 *   - Output order: one record per row; hits in the order given, inside a hit the rows lb, lb + 1, ..., lb + len - 1 — the sequence of the
 *     per-cursor loops.  After fmgpu_hits_sort the output is in fmc::Search's report order.  A hit with len == 0 produces nothing.  Positions are
 *     not deduplicated (two cursors that reach one row both report it, as in the reference).
 *   - Each record holds exactly what the locate of that row gives (seq_id = out_seq, pos = out_pos + out_steps), whichever locate kernel serves the index.
 *   - *out_count = the sum of len over the hits, on success and on FMGPU_ERR_CAPACITY alike; if it exceeds `capacity`, the call returns
 *     FMGPU_ERR_CAPACITY and writes nothing to `out`.
 *   - FMGPU_ERR_INVALID: a hit with lb + len > n (checked on the device, in the pass that sums the lengths), an index without an annotated
 *     array, or a null hits / out / out_count while count > 0.  count == 0 returns 0 with *out_count = 0 (out_count may then be NULL).
 *   - hits and out may be host or device memory.  The call reads back the sum of the lengths once (the capacity check needs it) and returns
 *     after its kernels have completed (its scratch of 16 bytes per hit is freed on return).
 *   - stats: lf_steps = LF steps walked, hits = records written, kernel_ms = the locate kernel alone. */
int fmgpu_locate_hits(fmgpu_index_t h, const fmgpu_hit* hits, uint64_t count, fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                      fmgpu_stats* stats, void* stream);

/* ---- seeds: super-maximal exact matches and matching statistics -----------------------------------------------------------------------
 * For the reads a search scheme leaves behind (more errors than its last stratum, long indels, a chimeric or clipped end): the longest stretches of every read that
 * occur in the text, with their suffix-array intervals, to be located (fmgpu_locate_hits) and extended by the caller.  A read is q[0 .. m), sigma the index's alphabet size.
 *   - Break: a query symbol outside 1 .. sigma - 1 (the delimiter 0, or anything >= sigma).  No match contains a break.
 *   - Match length: for an end e, L[e] = the largest l <= e + 1 such that q[e - l + 1 .. e] holds no break and occurs in the text; 0 if q[e] is a break or does not
 *     occur.  L[e + 1] <= L[e] + 1 always.
 *   - SMEM: the pairs (qbeg, qlen) = (e - L[e] + 1, L[e]) over the ends e with L[e] >= 1 and (e == m - 1 or L[e + 1] <= L[e]) — the maximal exact matches of the
 *     read that no other one contains.  qbeg is strictly increasing with e over the SMEMs of a read.
 *   - Filters: a seed is reported if qlen >= max(min_len, 1) and (max_rows == 0 or its interval holds at most max_rows rows).  A dropped seed is just dropped:
 *     nothing shorter is promoted in its place.
 *   - Records: ascending qidx, inside a read ascending qbeg.  out[k] = {qidx, lb, lb_rev = 0, len = rows of the interval, errors = 0, seq = index of the seed within
 *     its read}, out_span[k] = {qbeg, qlen}.  lb_rev = 0 is what fmgpu_search_backtracking writes on a unidirectional index: the cursor has been extended leftwards
 *     only.  `out` goes into fmgpu_locate_hits as it is; fmgpu_position::hit then indexes out_span.
 *   - out_match_len: NULL, or qoff[nq] - qoff[0] entries: entry i - qoff[0] = L of batch symbol i (the matching statistics).  Written whenever the call gets past
 *     its argument checks, also on FMGPU_ERR_CAPACITY.
 *   - *out_count = the seeds after the filters, on success and on FMGPU_ERR_CAPACITY alike; if it exceeds `capacity`, the call returns FMGPU_ERR_CAPACITY and writes
 *     nothing to out / out_span (the rule of fmgpu_locate_hits; one small read-back).
 *   - FMGPU_ERR_INVALID: a null handle; a null qbuf / qoff / out_count while nq > 0; a null out / out_span while capacity > 0.  nq == 0 returns 0 with *out_count = 0,
 *     decided before the handle is looked at (out_count may then be NULL).  A read of 2^32 symbols or more, or a batch of 2^32 symbols or more:
 *     FMGPU_ERR_UNSUPPORTED.  `_q4` on sigma > 15: FMGPU_ERR_UNSUPPORTED.
 *   - FMIndex or BiFMIndex, every layout, 32- and 64-bit rows; only the forward bwt is read.  Every buffer may be host or device memory.  The call returns after
 *     completion and frees its scratch: per query symbol 16 bytes with 32-bit rows, 24 with 64-bit rows (match length 4, interval 8 / 16, selection flag and
 *     scan 4), 4 fewer where out_match_len is device memory and serves as it is; `_q4` adds the unpacked byte per symbol.
 *   - stats: lf_steps = the extensions a one-symbol walk executes: the sum of L[e], plus one for every end whose walk stopped on an extension that came out empty
 *     (L[e] <= e and q[e - L[e]] is not a break; a break costs no step).  hits = records; kernel_ms = the walk kernel alone; table_bytes / table_accesses as
 *     exact search in one-symbol steps counts them on the one-symbol blocks (12 bytes per entry loaded), 0 on the other layouts.
 *   - `_q4`: `packed` in place of qbuf; the batch is unpacked into a byte scratch and the byte path runs: the results are those of the byte call on
 *     fmgpu_queries_unpack4(packed). */
typedef struct fmgpu_seed_span { uint32_t qbeg, qlen; } fmgpu_seed_span;   /* 8 bytes */
int fmgpu_search_smems(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                       uint32_t min_len, uint64_t max_rows,
                       fmgpu_hit* out, fmgpu_seed_span* out_span, uint64_t capacity, uint64_t* out_count,
                       uint32_t* out_match_len, fmgpu_stats* stats, void* stream);
int fmgpu_search_smems_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                          uint32_t min_len, uint64_t max_rows,
                          fmgpu_hit* out, fmgpu_seed_span* out_span, uint64_t capacity, uint64_t* out_count,
                          uint32_t* out_match_len, fmgpu_stats* stats, void* stream);

/* the 16-byte transport form of hit records (what a rank sends to the gathering rank): out[2k] = qidx:32 | lb:32,
 * out[2k+1] = len:32 | errors:8 | seq:24; lb_rev is dropped (it only serves further extension of the cursor).  Needs qidx, lb, len < 2^32,
 * errors < 256, seq < 2^24; a record that does not fit makes the call return FMGPU_ERR_UNSUPPORTED (checked on the device; the call
 * synchronises `stream`). */
int fmgpu_hits_pack16(const fmgpu_hit* hits, uint64_t count, uint64_t* out, void* stream);

/* the 24-byte transport form, for records as the search kernels emit them (not yet in callback order): out[3k] = qidx:32 | lb:32,
 * out[3k+1] = len:32 | errors:32, out[3k+2] = lb_rev:32 | seq:32 — the whole record, order key included, for rows and read numbers below 2^32
 * (FMGPU_ERR_UNSUPPORTED otherwise; the call synchronises `stream`). */
int fmgpu_hits_pack24(const fmgpu_hit* hits, uint64_t count, uint64_t* out, void* stream);

/* Puts `count` hit records (host or device memory) into the reference's callback order — ascending qidx, inside a query the order the
 * delegate is called in (search/SearchNg26.h:385-390) — with a stable device radix sort on (qidx, errors >> 8, seq), and normalises them:
 * seq = position of the record within its query, errors = the error count (upper bits cleared). */
int fmgpu_hits_sort(fmgpu_hit* hits, uint64_t count, void* stream);

/* ---- map: search, order and locate in one call ------------------------------------------------------------------------------------------------
 * fmc::Search{index, queries, editDistance, errors, maxResults, reportFunc}() (search/search.h:48-75) behind one call: reads in, (qidx, seqId, pos, errors) out.  The
 * pieces are the calls above — exact search or a best-stratum ladder, fmgpu_hits_sort or fmgpu_hits_from_intervals, fmgpu_locate_hits — chained on the device: the hit
 * records never visit the host between them, and the capacity-retry loop every caller of the pieces writes lives here once.
 *   - The hit list H: kinds FMGPU_MAP_SCHEME / FMGPU_MAP_NG21: exactly the records of fmgpu_search_best / fmgpu_search_best_ng21 with these schemes and
 *     max_hits_per_query, after fmgpu_hits_sort (n_schemes = 1 is the single-scheme call).  Kind FMGPU_MAP_EXACT: fmgpu_hits_from_intervals(lb, len, qoff, nq, 0,
 *     max_hits_per_query) over the results of fmgpu_search_exact.  The position list P = fmgpu_locate_hits(H).
 *   - Outputs: out = P, out_hits = H, out_stratum as the ladder defines it (kind 0: 0 for a read with a record, 255 otherwise).  P is in fmc::Search's report order:
 *     ascending qidx, then callback order, then the rows lb .. lb + len - 1; fmgpu_position::hit indexes H.  locate == 0 stops after H: *out_count = 0.
 *   - Capacity and counts: H and P are always produced in the library's own device scratch, which starts at first_records records (0 = max(1024, 4 x reads)); a stage
 *     that overflows it grows it to max(count, 2 x size) and reruns (the ladder within its documented n_schemes rounds).  So *out_hit_count and *out_count are exact
 *     totals, on success and on FMGPU_ERR_CAPACITY alike.  FMGPU_ERR_CAPACITY: P exceeds `capacity`, or out_hits is non-NULL and H exceeds hits_capacity; the contents of
 *     both output arrays are then unspecified.
 *   - stats: search_stats[i] = stratum i's fmgpu_stats of the last run (max(1, n_schemes) entries or NULL; kind 0: one entry, fmgpu_search_exact's); locate_stats (one
 *     entry or NULL) = what fmgpu_locate_hits reports.
 *   - Errors: codes and messages of the pieces, unchanged: a bad scheme, a unidirectional handle for kinds 1 and 2, an index without an annotated array when locate != 0,
 *     sigma > 15 for `_q4`, null pointers (what / qbuf / qoff / out_count; out while capacity > 0; out_hits while hits_capacity > 0).  kind, n_schemes (kinds 1, 2: 1 .. 254,
 *     kind 0: 0) and reserved are checked first (FMGPU_ERR_INVALID), then the schemes.  nq == 0 returns 0 with zero counts and leaves a non-NULL out_stratum untouched,
 *     decided before the handle is looked at.
 *   - Every buffer may be host or device memory.  The call returns after completion, frees its scratch and uses no stream of its own.
 *   - `_q4`: `packed` in place of qbuf, the rules of the other `_q4` calls.
 *
 * fmgpu_hits_from_intervals: the intervals of an exact search as hit records, in three device passes (flags, scan, scatter).
 *   - Read q produces a record iff len[q] > 0, max_rows_per_query > 0 and — qoff given (nq + 1 entries) — qoff[q + 1] > qoff[q].  DEVIATION: an empty read's cursor is
 *     the whole index and the reference would locate every row of it; here an empty read produces nothing, which is the best-stratum ladder's rule.
 *   - The record: {qidx = qidx_base + q, lb = lb[q], lb_rev = 0, len = min(len[q], max_rows_per_query), errors = 0, seq = 0}; one per producing read, ascending q.
 *   - *out_count is set on success and on FMGPU_ERR_CAPACITY alike; nothing is written to `out` when it exceeds `capacity`.  out_stratum (nq entries or NULL):
 *     out_stratum[q] = 0 if read q produced a record, else 255.  nq == 0 returns 0 with *out_count = 0.  At most 2^31 - 2 reads (FMGPU_ERR_UNSUPPORTED).
 *   - Host or device memory; asynchronous on `stream` for device buffers except for the one read-back of the count. */
#define FMGPU_MAP_EXACT  0
#define FMGPU_MAP_SCHEME 1   /* a ladder of fmgpu_scheme */
#define FMGPU_MAP_NG21   2   /* a ladder of fmgpu_expanded_scheme */
typedef struct fmgpu_map_query {
    int32_t  kind;               /* FMGPU_MAP_EXACT = 0, FMGPU_MAP_SCHEME = 1 (fmgpu_scheme ladder), FMGPU_MAP_NG21 = 2 (fmgpu_expanded_scheme ladder) */
    int32_t  n_schemes;          /* kinds 1, 2: 1 .. 254 (1 = a single scheme); kind 0: must be 0 */
    const void* schemes;         /* kinds 1, 2: n_schemes entries of the kind's scheme struct; kind 0: NULL */
    uint64_t max_hits_per_query; /* n of search_n; UINT64_MAX = unlimited */
    int32_t  locate;             /* 0: stop after the ordered hit records (no positions computed, *out_count = 0) */
    int32_t  reserved;           /* 0 */
    uint64_t first_records;      /* records the library's own hit / position scratch holds at first; 0 = max(1024, 4 x reads of the call or chunk) */
} fmgpu_map_query;               /* 40 bytes */
int fmgpu_map(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what,
              fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
              fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
              uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats, void* stream);
int fmgpu_map_q4(fmgpu_index_t h, const uint8_t* packed, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what,
                 fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                 fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                 uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats, void* stream);
int fmgpu_hits_from_intervals(const uint64_t* lb, const uint64_t* len, const uint64_t* qoff, uint64_t nq, uint64_t qidx_base,
                              uint64_t max_rows_per_query, fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, void* stream);

/* GPU index construction from sequences — replaces FMIndex(Sequences, samplingRate, threads) (fmindex/FMIndex.h:58-104) and
 * BiFMIndex(Sequences, samplingRate, threads) (fmindex/BiFMIndex.h:107-167), i.e. libsais (utils.h:97-129) + the String /
 * SparseArray constructors.  Sequence i = seqs[seq_off[i] .. seq_off[i+1]); a 0 delimiter follows every sequence
 * (utils.h:382-411).  `layout` names the reference String type being replaced: Wavelet is held as wavelet lines, every blocked layout as the LF-ready block table (the answers of a String_c do not depend on its layout).
 * keep_host != 0 additionally returns host copies of the by-products through fmgpu_built_get:
 *   part 0 BWT bytes, 1 BWT of the reversed text (BiFMIndex), 2 C (sigma+1 u64), 3 l0, 4 l1, 5 presence bits,
 *   6 / 7 DenseVector words of seqId / pos, 8 {bitCount, bits, largestValue, commonDivisor} x 2 (u64). */
typedef struct fmgpu_built* fmgpu_built_t;
int fmgpu_build_index(const uint8_t* seqs, const uint64_t* seq_off, uint64_t nseq, int32_t sigma, int32_t layout,
                      uint64_t sampling_rate, int32_t bidirectional, int32_t keep_host,
                      fmgpu_index_t* out, fmgpu_built_t* built);
int fmgpu_built_get(fmgpu_built_t b, int32_t part, const void** ptr, uint64_t* bytes);
int fmgpu_built_free(fmgpu_built_t b);

/* ---- one index on several GPUs of a node, for a caller that is ONE process (SURVEY 8b `fmgpu_set_devices`, 8e): the index file is read ONCE, onto the first listed
 * device, and copied from there to the others device to device (fmgpu_index_clone; the file is read again for a device the copy fails on;
 * ndev <= 0: every visible device; a device may be listed twice), a batch is cut into contiguous ranges of queries, every replica searches its range
 * on its own device from its own host thread and writes into its range of the caller's HOST arrays (queries are independent and the index is read-only: there
 * is no exchange between replicas; ranks of a multi-process job gather with RCCL instead — bench.py).  Results equal the single-handle calls' on the same
 * batch (hit records: the same set, query numbers of the whole batch; fmgpu_hits_sort orders them).  stats: sums, kernel_ms / prepass_ms = the slowest replica's.
 * All buffers must be host memory (FMGPU_ERR_INVALID otherwise).  fmgpu_replicas_info: count, the device of each replica, the first replica's handle (borrowed). */
typedef struct fmgpu_replicas* fmgpu_replicas_t;
int fmgpu_replicas_load(const char* path, const int32_t* devices, int32_t ndev, fmgpu_replicas_t* out);
int fmgpu_replicas_destroy(fmgpu_replicas_t r);
int fmgpu_replicas_peer_copies(fmgpu_replicas_t r, int32_t* count);   /* replicas that were made by a device-to-device copy of the first one (the others read the file) */
int fmgpu_replicas_info(fmgpu_replicas_t r, int32_t* count, int32_t* devices, int32_t capacity, fmgpu_index_t* first);
int fmgpu_replicas_search_exact(fmgpu_replicas_t r, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats);
int fmgpu_replicas_search_scheme(fmgpu_replicas_t r, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                                 fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats);
int fmgpu_replicas_search_ng21(fmgpu_replicas_t r, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_expanded_scheme* scheme, uint64_t max_hits_per_query,
                               fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats);
int fmgpu_replicas_locate(fmgpu_replicas_t r, const uint64_t* rows, uint64_t count, uint64_t* out_seq, uint64_t* out_pos, uint64_t* out_steps, fmgpu_stats* stats);

/* ---- feeds: chunked, overlapped search of HOST query batches ----------------------------------------------------------------------------
 * The one-shot calls above stage a host batch whole: one allocation, one copy from pageable memory, the kernel, one copy back, nothing overlapped.  A feed is a session
 * object bound to one index handle that owns pinned staging slots, device slots and three streams (upload, compute, download) and searches a host batch chunk by
 * chunk: chunk i + 1 is staged and uploaded and chunk i - 1 is downloaded while chunk i is being searched.  What search_no_errors::search and search_ng26::search are
 * handed in the reference is host memory (a Sequences object): this is the path such a caller takes.
 *   - Results: out_lb / out_len of fmgpu_feed_search_exact / _q4 equal, element for element, what fmgpu_search_exact / _q4 returns for the same batch on the same
 *     handle.  The hit records of fmgpu_feed_search_scheme equal, after fmgpu_hits_sort, those of fmgpu_search_scheme after fmgpu_hits_sort, field for field; qidx is the
 *     read's number in the caller's batch.  The `_v` forms (scattered reads: reads[q] points at lens[q] symbols) give the results of the flat forms on the flattened batch.
 *   - Scheme order and count: before sorting, the records of chunk c come before those of chunk c + 1.  *out_count is the batch's total, on success and on
 *     FMGPU_ERR_CAPACITY alike; every chunk still runs, as the one-shot call runs its whole kernel; on FMGPU_ERR_CAPACITY the contents of `out` are unspecified.
 *     A slot's device hit buffer that is too small for its chunk is grown and that chunk is run again: the caller never sees this.
 *   - Chunks: fmgpu_feed_plan defines them and the search calls use exactly its rule.  A chunk is the longest run of consecutive reads with at most chunk_reads reads
 *     and at most chunk_symbols symbols; it always holds at least one read, so a read longer than chunk_symbols is a chunk of its own.  out_first gets chunks + 1
 *     entries (room for capacity + 1; it may be NULL with capacity == 0), the last one is nq; *out_chunks is always set; more chunks than `capacity` return
 *     FMGPU_ERR_CAPACITY; a limit of 0 or a decreasing qoff returns FMGPU_ERR_INVALID.  fmgpu_feed_plan is pure host code and needs no device.
 *   - Defaults of the limits: chunk_reads = 1 048 576, chunk_symbols = 128 Mi (134 217 728): 101 bp reads make chunks of 114 MB in and 16 MB out, ten of them in a
 *     batch of 10 M reads — the best of the sweep in DESIGN 4.11 (64 Ki, 256 Ki and 1 Mi reads with 1, 4 and 16 host threads).  slots = 2, host_threads = 4;
 *     host_threads is never derived from the machine's CPU count.
 *   - Buffer sizes: the slots are sized for the call's largest chunk when the call starts and only ever grow (fmgpu_feed_info: pinned_bytes, device_bytes).
 *   - Host memory only: a device pointer in any argument returns FMGPU_ERR_INVALID (the rule of fmgpu_replicas_*; of a `_v` batch the two arrays and reads[0] are looked at).
 *   - Pinned host memory (fmgpu_malloc_host, hipHostMalloc, a pinned torch tensor; recognised with hipPointerGetAttributes): pinned symbols are copied from where they
 *     lie and pinned outputs are written in place (hit records are renumbered there).  last_staged_bytes counts the bytes of symbols, intervals and hit records that
 *     crossed a pinned slot, so nothing for those; the chunk's offsets (8 bytes per read) are always rewritten chunk-relative into the slot and are not counted.
 *     last_uploaded_bytes counts every byte copied to the device (offsets and symbols), last_chunks the chunks of the last call.
 *   - Offsets: qoff[0] need not be 0.  For `_q4` it may be odd and a chunk may start on an odd symbol: the chunk copies bytes qoff[first] >> 1 .. (qoff[end] + 1) >> 1
 *     and its device offsets keep the parity.  Device query buffers are 16-byte aligned and padded by 16 bytes; a chunk sits in its slot from symbol qoff[first] & ~31
 *     on, so every symbol keeps its place inside the aligned words and 16-byte pieces the readers load.
 *   - pack4: a byte batch is written into the pinned slot as nibbles (a byte >= sigma becomes 15) and searched with the `_q4` kernel, whose results the section above
 *     guarantees identical, when pack4 != 0, the handle has sigma <= 15 and exact search reads nibbles itself on the handle (the pair table with or without the interval
 *     table in front, the one-symbol blocks).  In every other case the bytes travel as they are.  Packing is host work: pinned symbols are then packed through the
 *     slot like pageable ones.  fmgpu_feed_search_scheme never packs.
 *   - stats: lf_steps, hits, table_*, kernel_ms and prepass_ms are the sums over the chunks.  A non-NULL stats of an exact call costs overlap: each chunk reads its
 *     counters back and so waits for its kernel before the next chunk is staged.
 *   - Threading: only the calling thread makes HIP calls; the host_threads workers (the calling thread is one of them) only copy or pack between caller memory and
 *     pinned slots, each on its own slice.  All chunk searches of a call run on ONE compute stream owned by the feed (the library's per-thread call scratch serves one
 *     call at a time: kernels of two chunks are never in flight on two streams); upload and download have a stream each, tied to it with events: three streams and no
 *     more, four queues with the side stream of exact search.  One feed serves one call at a time; two feeds on two host threads may use one handle concurrently.  A
 *     feed lives on the device of its handle: calls on it must be made with that device current.
 *   - An exact call with stats == NULL does not synchronise with the host between its chunks other than to wait for a slot: the shape of each chunk (symbols, longest
 *     and shortest read) is taken from the host offsets instead of a read-back.  (A `_q4` batch on a handle whose exact kernel does not read nibbles is unpacked per
 *     chunk as in fmgpu_search_exact_q4, which synchronises; scheme chunks read their record count back, as the one-shot call does.)
 *   - Errors: codes and messages for a null handle (fmgpu_feed_create), null pointers, a bad scheme, a unidirectional handle and sigma > 15 for `_q4` are those of the
 *     one-shot calls.  nq == 0 returns 0 and touches nothing.  A failing HIP call stops the enqueuing, drains the three streams and returns its code; the feed can
 *     still be destroyed afterwards.
 *   - fmgpu_feed_map / fmgpu_feed_map_v: fmgpu_map chunk by chunk.  Per chunk, on the compute stream: the search (a ladder or exact search), the ordering
 *     (fmgpu_hits_sort or fmgpu_hits_from_intervals), fmgpu_locate_hits if `locate` is set, and a rebase (qidx counts in the caller's batch, fmgpu_position::hit in the
 *     batch-wide H); the download stream then takes H, P and the chunk's out_stratum slice.  P, H and out_stratum equal, element for element, what fmgpu_map returns for the
 *     flattened batch (chunks are runs of consecutive reads: the sorted chunks one after another are the sorted batch); the counts are batch totals, exact on success and
 *     on FMGPU_ERR_CAPACITY alike, and every chunk still runs; stats are sums over the chunks.  The slots hold device and pinned buffers for hits, positions and strata
 *     that only ever grow (fmgpu_feed_info counts them); first_records applies per chunk, and a buffer too small for its chunk is grown and the stage rerun.  Pinned
 *     outputs are written in place.  Host memory only, the errors of fmgpu_map, one call at a time; no further stream.
 * Read-file text (LINES / FASTA / FASTQ bytes) is served by fmgpu_feed_map_text, declared behind fmgpu_queries_parse below.
 * Not served through a feed: backtracking, smems, fmgpu_search_hamming_sm, `_q4` batches for map, text for the plain search calls; feeds over replicas. */
typedef struct fmgpu_feed* fmgpu_feed_t;
typedef struct fmgpu_feed_config {
    uint64_t chunk_reads;    /* 0 = default */
    uint64_t chunk_symbols;  /* 0 = default */
    int32_t  slots;          /* 0 = 2; 2 .. 4 */
    int32_t  host_threads;   /* 0 = 4; 1 .. 16; never derived from the machine's CPU count */
    int32_t  pack4;          /* != 0: byte batches travel as nibbles where that is exact (above) */
    int32_t  reserved;       /* 0 */
} fmgpu_feed_config;
int fmgpu_feed_create(fmgpu_index_t h, const fmgpu_feed_config* cfg /* NULL = defaults */, fmgpu_feed_t* out);
int fmgpu_feed_destroy(fmgpu_feed_t f);
int fmgpu_feed_plan(const uint64_t* qoff, uint64_t nq, uint64_t chunk_reads, uint64_t chunk_symbols,
                    uint64_t* out_first, uint64_t capacity, uint64_t* out_chunks);
int fmgpu_feed_search_exact   (fmgpu_feed_t f, const uint8_t* qbuf,   const uint64_t* qoff, uint64_t nq,
                               uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats);
int fmgpu_feed_search_exact_q4(fmgpu_feed_t f, const uint8_t* packed, const uint64_t* qoff, uint64_t nq,
                               uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats);
int fmgpu_feed_search_exact_v (fmgpu_feed_t f, const uint8_t* const* reads, const uint64_t* lens, uint64_t nq,
                               uint64_t* out_lb, uint64_t* out_len, fmgpu_stats* stats);
int fmgpu_feed_search_scheme  (fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                               const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                               fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats);
int fmgpu_feed_search_scheme_v(fmgpu_feed_t f, const uint8_t* const* reads, const uint64_t* lens, uint64_t nq,
                               const fmgpu_scheme* scheme, uint64_t max_hits_per_query,
                               fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, fmgpu_stats* stats);
int fmgpu_feed_map  (fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const fmgpu_map_query* what,
                     fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                     fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                     uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats);
int fmgpu_feed_map_v(fmgpu_feed_t f, const uint8_t* const* reads, const uint64_t* lens, uint64_t nq, const fmgpu_map_query* what,
                     fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                     fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                     uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats);
int fmgpu_feed_info(fmgpu_feed_t f, uint64_t* pinned_bytes, uint64_t* device_bytes,
                    uint64_t* last_chunks, uint64_t* last_staged_bytes, uint64_t* last_uploaded_bytes);

/* ---- query text: LINES / FASTA / FASTQ bytes to a query batch on the device --------------------------------------------------------------
 * fmgpu_queries_parse turns the raw bytes of a read file (or of a chunk of one) into the byte form every search call takes: out_qbuf (one symbol per byte) and
 * out_qoff (reads + 1 offsets, out_qoff[0] = 0).  No index handle is involved.  `text` and every output may each be host or device memory (host buffers are staged);
 * symbol_of is host memory.  The call returns after completion and frees its scratch (about 0.8 byte per text byte for read files).
 *   Lines
 *   - The buffer is cut at '\n'.  A '\r' that is the last byte of a line belongs to the terminator and is not part of the line: a '\r' directly in front of
 *     '\n', or the last byte of a `final` buffer.  Any other '\r' is an ordinary byte.  The last line may lack its '\n'; a buffer that ends in '\n' has no
 *     further empty line behind it.  Lines are numbered from 0.
 *   final
 *   - final != 0: the buffer ends the input, so the last record is complete where the buffer ends.  final == 0: only the records the buffer proves complete are
 *     parsed, and result->consumed tells where the next chunk starts: a file is parsed chunk by chunk with the unconsumed tail carried over.
 *   FMGPU_TEXT_LINES
 *   - Every line is a read, an empty line an empty read.  A line is complete when '\n' ends it, or with `final`.  consumed = the offset just behind the last complete line.
 *   FMGPU_TEXT_FASTA
 *   - A line whose first byte is '>' is a header and starts a record; every other non-empty line is a sequence line of the current record (multi-line records);
 *     empty lines are ignored everywhere; a '>' that is not the first byte of its line is an ordinary byte.  A record without a sequence line is an empty read.
 *   - A non-empty line in front of the first header is a text error.
 *   - A record is complete when another header starts behind it inside the buffer, or with `final`.  consumed = the offset of that next header's '>', or `bytes`
 *     with `final`.  final == 0 and fewer than two headers: the call succeeds with reads == 0, consumed == 0 (the caller needs a larger chunk).
 *   FMGPU_TEXT_FASTQ
 *   - Strict four-line records: lines 4r, 4r + 1, 4r + 2, 4r + 3 are header, sequence, separator and quality of read r.  The line's position alone decides its role
 *     (a quality line that starts with '@' or '+' is a quality line); multi-line FASTQ is not supported.
 *   - Text errors: a header whose first byte is not '@', a separator whose first byte is not '+', a quality line whose byte length differs from its sequence
 *     line's (terminators excluded, before any dropping).
 *   - With `final`, empty lines at the very end of the buffer are discarded first; a line count that is then no multiple of four is a text error (a truncated
 *     file) at the first line of the incomplete record.  With final == 0 a trailing incomplete record is neither consumed nor validated.
 *   - consumed = the offset just behind the last complete record's quality line and its terminator.
 *   Symbols
 *   - Every byte of a sequence line (terminator excluded) maps through symbol_of[256]: FMGPU_SYM_DROP produces nothing, FMGPU_SYM_FOREIGN is written as 255 (a
 *     byte outside every alphabet) and counted in result->foreign, any other value is written as it is.  The entries for '\n' and for a terminating '\r' are never
 *     consulted.  Header, separator and quality bytes produce nothing.  Reads keep the file's order.
 *   Spans (NULL, or read_capacity entries; offsets relative to `text`)
 *   - out_names[r] = the header line of read r without its first byte and without its terminator; LINES: {0, 0}.
 *   - out_quals[r] = the quality line of read r; LINES and FASTA: {0, 0}.
 *   Counts and capacity
 *   - *result is written in full once the argument checks pass: on success, on FMGPU_ERR_CAPACITY and on a text error alike.  reads / symbols: the complete
 *     records and the symbols they produce.  On a text error error_line / error_offset name the FIRST offending line (the lowest one, whatever else is wrong
 *     behind it), reads / symbols / consumed / foreign describe the records in front of the offending record, and nothing is written to the outputs.
 *   - FMGPU_ERR_CAPACITY: symbols > symbol_capacity or reads > read_capacity; nothing is written to the outputs.
 *   - The counting call: out_qbuf == NULL && out_qoff == NULL (and both span pointers NULL) returns 0 with the counts and writes nothing.  A caller sizes its
 *     buffers exactly with two calls, or takes the bound symbols <= bytes, reads <= bytes.
 *   Errors
 *   - FMGPU_ERR_INVALID: a text error; a null result or symbol_of; a null text while bytes > 0; exactly one of out_qbuf / out_qoff null; span pointers in a
 *     counting call; an unknown format.  These argument checks come before the first use of the device.
 *   - bytes == 0 returns 0 with a zero result (and out_qoff[0] = 0 if out_qoff is given).
 *   - bytes > 2^32 - 2: FMGPU_ERR_UNSUPPORTED (positions are 32-bit words on the device): parse in chunks, each starting at the previous call's `consumed`. */
#define FMGPU_TEXT_LINES 0   /* one read per line */
#define FMGPU_TEXT_FASTA 1   /* '>' header lines, sequence lines concatenated (multi-line records) */
#define FMGPU_TEXT_FASTQ 2   /* strict four-line records */
#define FMGPU_SYM_DROP    254 /* symbol_of value: the byte produces nothing */
#define FMGPU_SYM_FOREIGN 255 /* symbol_of value: written as 255 (a byte outside every alphabet) and counted */
typedef struct fmgpu_text_span { uint64_t offset, len; } fmgpu_text_span;   /* bytes of the input buffer */
typedef struct fmgpu_parse_result {
    uint64_t reads, symbols;            /* complete records found; symbols they produce */
    uint64_t consumed;                  /* bytes of the buffer those records span, from byte 0: the next chunk starts here */
    uint64_t foreign;                   /* symbols written as 255 */
    uint64_t error_line, error_offset;  /* a text error: 0-based line number and byte offset of the first offending line (0 otherwise) */
} fmgpu_parse_result;
int fmgpu_queries_parse(const uint8_t* text, uint64_t bytes, int32_t format, int32_t final, const uint8_t* symbol_of,
                        uint8_t* out_qbuf, uint64_t symbol_capacity, uint64_t* out_qoff, uint64_t read_capacity,
                        fmgpu_text_span* out_names, fmgpu_text_span* out_quals, fmgpu_parse_result* result, void* stream);

/* ---- read-file bytes to positions through a feed -------------------------------------------------------------------------------------------
 * fmgpu_feed_map_text takes the raw bytes of a read file (host memory) and returns what fmgpu_map returns for its reads: the text is the only thing uploaded, it is
 * parsed on the feed's compute stream in front of the search, and nothing but results comes back.  Device memory stays bounded by the window size, not by the file.
 *   Results
 *   - Let Q be what fmgpu_queries_parse(text, bytes, format, final, symbol_of, ...) produces for the whole text.  out, out_hits, out_stratum, *out_count and
 *     *out_hit_count equal, element for element, what fmgpu_map returns for Q with the same `what`; qidx is the read's number in the file, fmgpu_position::hit indexes
 *     the batch-wide hit list.  out_names[r] / out_quals[r] are the spans of the whole-text parse (offsets relative to `text`), out_lens[r] = Q.qoff[r + 1] - Q.qoff[r].
 *   - *result equals the whole-text parse's result in every field; consumed counts from byte 0 of `text`, and with final == 0 tells where the next call starts.
 *   Pieces
 *   - B = chunk_bytes; 0 means 64 MiB; 1 .. 15 return FMGPU_ERR_INVALID.  Window c is text[c B, min((c + 1) B, bytes)), c = 0 .. ceil(bytes / B) - 1.  Piece c is the
 *     carry followed by window c: the carry of piece 0 is empty, the carry of piece c + 1 is what piece c did not consume.  A piece is parsed under the rules of
 *     fmgpu_queries_parse, with `final` for the last window of a call whose own `final` is set.  A piece with no complete record is carried whole.
 *   - What only later bytes can settle, a piece in front of the last one leaves unconsumed: a '\r' as its last byte with no '\n' behind it yet counts as a terminator to come
 *     (so such a line is empty, not a FASTA text error), and FASTQ records that lie wholly or partly in empty lines at the very end of the piece are not yet records
 *     (the end of the text may discard those lines).  With this the pieces give the whole-text result for every text and every B.
 *   - last_chunks (fmgpu_feed_info) is the number of windows.  chunk_reads / chunk_symbols of the feed's config do not apply: a piece is a chunk.
 *   - A piece of more than 2^32 - 2 bytes returns FMGPU_ERR_UNSUPPORTED (a record longer than that, or B too large); the whole text may be larger.
 *   Where the bytes go
 *   - A slot's device text buffer holds window c from a fixed offset H (the headroom) on: the upload does not depend on any parse result, so window c + 1 travels
 *     while piece c is parsed and searched.  Pageable text goes through the slot's pinned buffer, moved by the feed's host workers (last_staged_bytes counts it);
 *     pinned text is copied from where it lies.  The carry is copied device to device, on the compute stream, from the previous slot into [H - carry, H).  H starts as
 *     min(B, 1 MiB); a carry longer than H regrows that slot's buffer with a headroom of twice the carry (rare, synchronised, not visible).
 *   - last_uploaded_bytes counts the text bytes (and nothing else: the 256-byte table is not counted).
 *   Capacity and counts
 *   - out_stratum, out_names, out_quals and out_lens each hold read_capacity entries; any may be NULL, and with all four NULL read_capacity is ignored.  More reads
 *     than read_capacity with any of them given: FMGPU_ERR_CAPACITY.  Positions and hits overflow as in fmgpu_feed_map.  In every capacity case all pieces still run,
 *     all counts and *result are exact totals, and the contents of the arrays are unspecified.
 *   Text errors
 *   - FMGPU_ERR_INVALID with the message of fmgpu_queries_parse ("text error in line ..."), line and offset those of the whole text; *result as the whole-text parse
 *     reports it (the records in front of the offending one).  Pieces behind the error do not run; the arrays are unspecified.  The feed serves further calls.
 *   Errors, memory, streams
 *   - Before any use of the device, FMGPU_ERR_INVALID for: a null f, result, symbol_of, what or out_count; a null text with bytes > 0; a null out with capacity > 0; a
 *     null out_hits with hits_capacity > 0; an unknown format; chunk_bytes in 1 .. 15; what fmgpu_feed_map refuses in `what`.  bytes == 0 returns 0 with zero counts
 *     and a zero result.  A device pointer in any argument returns FMGPU_ERR_INVALID (the feed rule).
 *   - Text, parse scratch, batch, records and spans live in the slots and only ever grow (fmgpu_feed_info counts them): in steady state a piece allocates nothing.
 *     DESIGN.md §4.15 lists the bytes per slot.  The feed's three streams are used and no more; each piece's parse reads two
 *     words back (the compute stream is synchronised, as the search behind it does anyway).  One call at a time per feed.
 *   - Not built: gzip input, multi-line FASTQ, `_q4` slots (both strands: fmgpu_feed_map_text_strands below), text through the plain search calls (locate = 0 returns ordered hit records),
 *     overlap of one piece's search with the next piece's parse (one compute stream). */
int fmgpu_feed_map_text(fmgpu_feed_t f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final,
                        const uint8_t* symbol_of, uint64_t chunk_bytes, const fmgpu_map_query* what,
                        fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                        fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                        uint8_t* out_stratum, fmgpu_text_span* out_names, fmgpu_text_span* out_quals, uint64_t* out_lens,
                        uint64_t read_capacity, fmgpu_parse_result* result,
                        fmgpu_stats* search_stats, fmgpu_stats* locate_stats);

/* ---- both strands: the reverse complements made on the device, and the best stratum per read -----------------------------------------------------
 * A DNA read mapper searches a read and its reverse complement.  These calls make the second strand on the device, so that only the forward strand crosses the
 * bus, and teach the best-stratum ladder that two reads are the strands of one: once either strand is found, neither goes on.
 * fmgpu_queries_strands: the doubled batch D of a byte batch, in the interleaved numbering fmgpu_queries_pack4 uses with a complement table: read 2q of D is read q,
 * read 2q + 1 is read q reversed and complemented.
 *   - complement: host memory, n entries, n in 1 .. 256.  A byte c < n becomes complement[c]; a byte >= n stays as it is (255 stays 255; fmgpu_queries_pack4 writes
 *     15 instead).  The forward strand is copied as it is.
 *   - out_qoff: 2 nq + 1 entries, closed-form: out_qoff[2q] = 2 (qoff[q] - qoff[0]), out_qoff[2q + 1] = out_qoff[2q] + (qoff[q + 1] - qoff[q]); out_qoff[0] = 0 and
 *     qoff[0] need not be 0.  out_qbuf: 2 (qoff[nq] - qoff[0]) bytes.
 *   - Every buffer but `complement` may be host or device memory (host buffers are staged).  One streaming pass: a thread makes 16 output bytes from aligned 16-byte
 *     loads, reversed in registers for strand 1, and stores them as one aligned 16-byte piece (a device out_qbuf that is not 16-byte aligned is written byte by
 *     byte).  The offsets are checked on the device and read back once before the symbols are touched; the call returns after completion.
 *   - Errors: FMGPU_ERR_INVALID for n outside 1 .. 256, a null pointer while nq > 0, a decreasing qoff; FMGPU_ERR_UNSUPPORTED for nq > 2^30 - 1 (D stays inside the
 *     ladder's 2^31 - 1 reads and the 2^31 - 2 of fmgpu_hits_from_intervals).  n and nq are checked before the first use of the device.  nq == 0 returns 0 and
 *     writes out_qoff[0] = 0 if out_qoff is given.
 * fmgpu_search_best_pairs / fmgpu_search_best_ng21_pairs: fmgpu_search_best / _ng21 over a batch whose reads 2j and 2j + 1 are a pair (the two strands of D).
 *   - nq must be even (FMGPU_ERR_INVALID, checked with n_schemes before anything else).  Stratum i is the single-scheme call over the reads of the pairs still
 *     unfound, in batch order.  A pair is found in stratum i if either of its reads produced a record with len > 0 there; both reads of a found pair leave the ladder.
 *   - out_stratum (nq entries): BOTH entries of a found pair carry its stratum, an unfound pair's entries are 255; the records tell which strand has hits.
 *   - Records, their order, max_hits_per_query (per read of the batch, that is per strand), the capacity rule, stats, error codes and the one read-back per stratum
 *     are those of fmgpu_search_best.  An empty read, or an ng21 read shorter than the scheme, finds nothing; its pair is found through the other read only.
 *   - The records are a sub-multiset of fmgpu_search_best's on the same batch: a strand that the independent ladder would search again in a later stratum is not.
 * fmgpu_map_strands: fmgpu_map over both strands.  Let D = fmgpu_queries_strands(batch, strands->complement, strands->n).
 *   - pair == 0: every output equals, element for element, what fmgpu_map returns for D.  pair == 1: the same with fmgpu_search_best_pairs / _ng21_pairs in place of
 *     the ladder.  Kind FMGPU_MAP_EXACT has no ladder: pair is accepted and changes nothing.
 *   - qidx in H and P counts in D: read = qidx >> 1, strand = qidx & 1.  out_stratum has 2 nq entries.  pos is where the searched string lies on the indexed text: for
 *     strand 1 the leftmost position of the reverse complement (what a SAM record with flag 16 holds); nothing is converted.
 *   - Only the forward strand is staged; D is made in the call's scratch (2 x symbols + 16 bytes, 16 nq + 24 bytes of offsets).
 *   - Errors, in this order: what fmgpu_map checks first in `what`; FMGPU_ERR_INVALID for a null strands or complement, n outside 1 .. 256, pair outside 0 .. 1;
 *     nq == 0 returns 0 with zero counts before the handle is looked at; nq > 2^30 - 1 is FMGPU_ERR_UNSUPPORTED; then the schemes, the handle and the null pointers
 *     with the codes and messages of fmgpu_map.
 * fmgpu_feed_map_strands / fmgpu_feed_map_text_strands: fmgpu_feed_map / fmgpu_feed_map_text with the same `strands`.
 *   - Per chunk or piece, on the compute stream: the upload of the forward reads or of the text and the parse are unchanged; then the doubled batch is made in the
 *     slot's own buffers (they only ever grow; fmgpu_feed_info counts them), the chain runs on 2 x reads, and the records are rebased by 2 x the chunk's first read.
 *   - Results equal fmgpu_map_strands on the flattened batch (for text: on the whole-text parse), for every chunk and window size: chunks are runs of consecutive
 *     reads, so a pair never straddles one.
 *   - chunk_reads / chunk_symbols count forward reads.  out_stratum, where given, holds 2 x nq entries (text: 2 x read_capacity); out_names / out_quals / out_lens stay
 *     per read of the file.  last_uploaded_bytes stays the forward bytes (and offsets) or the text bytes: the second strand never crosses the bus.
 *   - Host memory only, the feed's three streams and no more; errors and capacity behaviour are those of the calls they extend, the strands checks behind `what`'s.
 * Not built: `_v` and `_q4` forms of the strands calls, `_q4` forms of the pair ladder, strands over replicas, strands for fmgpu_search_hamming_sm. */
typedef struct fmgpu_strands {
    const uint8_t* complement;   /* host memory, n entries */
    int32_t n;                   /* 1 .. 256 */
    int32_t pair;                /* 0: the strands are independent reads; 1: best stratum per read (the pair ladder) */
} fmgpu_strands;                 /* 16 bytes */
int fmgpu_queries_strands(const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq, const uint8_t* complement, int32_t n,
                          uint8_t* out_qbuf, uint64_t* out_qoff, void* stream);
int fmgpu_search_best_pairs(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                            const fmgpu_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                            fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream);
int fmgpu_search_best_ng21_pairs(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                                 const fmgpu_expanded_scheme* schemes, int32_t n_schemes, uint64_t max_hits_per_query,
                                 fmgpu_hit* out, uint64_t capacity, uint64_t* out_count, uint8_t* out_stratum, fmgpu_stats* stats, void* stream);
int fmgpu_map_strands(fmgpu_index_t h, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                      const fmgpu_map_query* what, const fmgpu_strands* strands,
                      fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                      fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                      uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats, void* stream);
int fmgpu_feed_map_strands(fmgpu_feed_t f, const uint8_t* qbuf, const uint64_t* qoff, uint64_t nq,
                           const fmgpu_map_query* what, const fmgpu_strands* strands,
                           fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                           fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                           uint8_t* out_stratum, fmgpu_stats* search_stats, fmgpu_stats* locate_stats);
int fmgpu_feed_map_text_strands(fmgpu_feed_t f, const uint8_t* text, uint64_t bytes, int32_t format, int32_t final,
                                const uint8_t* symbol_of, uint64_t chunk_bytes, const fmgpu_map_query* what, const fmgpu_strands* strands,
                                fmgpu_position* out, uint64_t capacity, uint64_t* out_count,
                                fmgpu_hit* out_hits, uint64_t hits_capacity, uint64_t* out_hit_count,
                                uint8_t* out_stratum, fmgpu_text_span* out_names, fmgpu_text_span* out_quals, uint64_t* out_lens,
                                uint64_t read_capacity, fmgpu_parse_result* result,
                                fmgpu_stats* search_stats, fmgpu_stats* locate_stats);

/* ---- positions to text: located hits formatted as lines on the device ---------------------------------------------------------------------------
 * fmgpu_positions_format is the mirror image of fmgpu_queries_parse: fmgpu_position records in, text lines out, so that a run which writes a file moves the text
 * (about 20 bytes per record, fewer than the record's 32) over the bus instead of the records, and no host loop formats them.
 *   - Lines: record i becomes line i: its columns in the order of spec->cols, spec->sep between two columns, '\n' behind the last; the lines are concatenated in record
 *     order.  Decimal columns have no sign, no padding and no leading zero; the value 0 is "0".  A column may appear more than once.  With cols = {0, 1, 2, 3}, sep = ' '
 *     and pos_add = 0 the output is byte for byte what `fprintf(out, "%zu %zu %zu %zu\n", qidx, seq_id, pos, errors)` writes per record.
 *   - Names: FMGPU_COL_READ_NAME copies the bytes of row (qidx >> strand_shift) of spec->read_names, FMGPU_COL_SEQ_NAME those of row seq_id of spec->seq_names (what
 *     fmgpu_queries_parse / fmgpu_feed_map_text return as out_names, with the text as `bytes`).  name_stop = 1 ends a name in front of its first ' ' or '\t'.
 *   - out_line_off: NULL, or count + 1 entries in host or device memory: out_line_off[i] = the byte offset of line i, out_line_off[count] = *out_bytes.  It is written
 *     whenever the call gets past its checks, also on FMGPU_ERR_CAPACITY (the rule of out_match_len).
 *   - *out_bytes = the exact size of the text, on success and on FMGPU_ERR_CAPACITY alike; if it exceeds `capacity` the call returns FMGPU_ERR_CAPACITY and writes nothing
 *     to `out`.  out == NULL with capacity == 0 is the counting call: it returns 0 with *out_bytes (and out_line_off) and writes no text.
 *   - count == 0 returns 0 with *out_bytes = 0 before anything else is looked at; a host out_line_off[0] is set to 0 (a device one by a memset).
 *   - Before the first use of the device, FMGPU_ERR_INVALID, each with a message of its own, for: a null spec, positions or out_bytes; a null out while capacity > 0;
 *     n_cols outside 1 .. 8; an unknown column code; strand_shift or name_stop outside 0 .. 1; reserved != 0; a name column whose table pointer is null, or whose table
 *     has a null bytes with n_bytes > 0 or a null spans with count > 0.  2^32 - 256 records and more: FMGPU_ERR_UNSUPPORTED.
 *   - On the device, in the pass that measures the lines: a name column whose row (read or seq_id) is >= its table's count, or a span with offset + len > n_bytes, returns
 *     FMGPU_ERR_INVALID; nothing is written (out_line_off neither) and the message names the lowest offending record index.  A name span of 2^31 bytes or more, or a line
 *     of 2^32 bytes or more, returns FMGPU_ERR_UNSUPPORTED in the same way (an FMGPU_ERR_INVALID record anywhere in the batch goes first).
 *   - Every buffer (positions, out, out_line_off, and the bytes and spans of each table) may be host or device memory; host buffers are staged.  A device `out` needs no
 *     alignment: the text leaves in 16-byte stores aligned to the output address, and only the first and last bytes of a workgroup's range are stored byte by byte.
 *   - Three passes (measure, hipcub exclusive scan, write) and one read-back: the size of the text and the error words together.  The call returns after completion and
 *     frees its scratch of 12 bytes per record (a 4-byte length, an 8-byte offset) plus the scan's own.
 * Not built: PAF records (SAM records: fmgpu_positions_sam below), text per chunk inside fmgpu_map or the feeds, fmgpu_hit records or seed spans as text, compressed output, columns from a caller's arrays. */
#define FMGPU_COL_QIDX      0   /* qidx, decimal */
#define FMGPU_COL_SEQ_ID    1   /* seq_id, decimal */
#define FMGPU_COL_POS       2   /* pos + spec->pos_add, decimal (wraps mod 2^64) */
#define FMGPU_COL_ERRORS    3   /* errors, decimal */
#define FMGPU_COL_HIT       4   /* hit, decimal */
#define FMGPU_COL_READ      5   /* qidx >> strand_shift, decimal */
#define FMGPU_COL_STRAND    6   /* one byte: '-' if strand_shift == 1 and (qidx & 1), else '+' */
#define FMGPU_COL_READ_NAME 7   /* bytes of read_names row (qidx >> strand_shift) */
#define FMGPU_COL_SEQ_NAME  8   /* bytes of seq_names row seq_id */
typedef struct fmgpu_name_table {          /* 32 bytes; bytes and spans may each be host or device memory */
    const uint8_t* bytes;
    uint64_t n_bytes;
    const fmgpu_text_span* spans;          /* span offsets are relative to `bytes` */
    uint64_t count;
} fmgpu_name_table;
typedef struct fmgpu_format_spec {         /* 40 bytes, host memory */
    int32_t n_cols;                        /* 1 .. 8 */
    uint8_t cols[8];                       /* FMGPU_COL_*; a column may appear more than once */
    uint8_t sep;                           /* the byte between two columns */
    uint8_t strand_shift;                  /* 0: read = qidx; 1: read = qidx >> 1, strand = qidx & 1 (the numbering of the *_strands calls) */
    uint8_t name_stop;                     /* 0: a name is its whole span; 1: it ends in front of its first ' ' or '\t' */
    uint8_t reserved;                      /* 0 */
    uint64_t pos_add;                      /* added to pos (1 = SAM's one-based positions) */
    const fmgpu_name_table* read_names;    /* NULL unless a READ_NAME column is asked for */
    const fmgpu_name_table* seq_names;     /* NULL unless a SEQ_NAME column is asked for */
} fmgpu_format_spec;
int fmgpu_positions_format(const fmgpu_position* positions, uint64_t count, const fmgpu_format_spec* spec,
                           uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* out_line_off, void* stream);

/* ---- positions to SAM: located hits as SAM records on the device -------------------------------------------------------------------------------
 * fmgpu_positions_sam writes the positions of fmgpu_map* as SAM alignment lines; fmgpu_sam_header (host code) writes the header in front of them.  Nothing is aligned
 * here: the searches most callers run are ungapped (exact search, Hamming schemes, fmgpu_search_hamming_sm), so their CIGAR is "<m>M"; for edit-distance hits SAM allows
 * '*'.  SEQ comes from the query batch the caller holds, QUAL from the spans fmgpu_queries_parse returns, FLAG from the both-strand numbering, MAPQ and NH from counts.
 *   - Input order: `positions` is what fmgpu_map* returns: the read number (qidx >> shift; shift = 1 with spec->strands, else 0) does not decrease over the records.
 *     cnt[r] = the number of records of read r.
 *   - Output order: reads ascending; a read with records gets one line per record, in record order; a read without records gets one unmapped line iff emit_unmapped.
 *     *out_lines (may be NULL) = the number of lines.  out_line_off: NULL, or *out_lines + 1 entries (size it for the bound count + nq + 1): the byte offset of every
 *     line, the last entry = *out_bytes; written whenever the call gets past its checks, also on FMGPU_ERR_CAPACITY.
 *   - Mapped line, tabs between the fields and '\n' behind the last: QNAME FLAG RNAME POS MAPQ CIGAR * 0 0 SEQ QUAL NM:i:<errors> NH:i:<cnt[r]>
 *     Unmapped line: QNAME 4 * 0 0 * * 0 0 SEQ QUAL, with SEQ and QUAL of the forward read.
 *   - The primary record of a read is the one with the fewest errors, the lowest record index among equals.  FLAG = (strand ? 16 : 0) | (not the primary ? 256 : 0).
 *     MAPQ: the primary record gets mapq_unique if it is the read's only record with the minimal errors, else mapq_multi; every secondary record gets mapq_multi.
 *   - POS = pos + 1 (mod 2^64).  CIGAR = m in decimal and 'M' if cigar == 1 and the read's length m > 0, else '*'.
 *   - QNAME = row `read` of read_names, RNAME = row seq_id of seq_names: the name up to its first ' ' or '\t'; an empty result is written as '*'.  Without the table:
 *     the read number, or seq_id, in decimal.
 *   - SEQ: strand 0: byte j = char_of[q[j]]; strand 1: byte j = char_of[comp(q[m - 1 - j])] with comp(c) = complement[c] for c < n, c otherwise (the rule of
 *     fmgpu_queries_strands).  m = 0 gives '*'; so does a secondary record unless secondary_seq.
 *   - QUAL: '*' if quals is NULL, if the span's len is 0 or if SEQ is '*'; else the bytes of row `read` of quals, reversed for strand 1.
 *   - *out_bytes and *out_lines are exact, on success and on FMGPU_ERR_CAPACITY alike (then nothing is written to `out`); out == NULL with capacity == 0 is the counting
 *     call.  Without a line (count == 0 and either nq == 0 or emit_unmapped == 0) the call returns 0 behind its argument checks and size limits with zero counts and out_line_off[0] = 0;
 *     count == 0 with emit_unmapped = 1 writes nq unmapped lines.
 *   - Before the first use of the device, FMGPU_ERR_INVALID, each with a message of its own, for: a null spec, char_of or out_bytes; a null qbuf or qoff while nq > 0;
 *     null positions while count > 0; a null out while capacity > 0; cigar, emit_unmapped or secondary_seq outside 0 .. 1; reserved != 0; a strands with a null complement
 *     or n outside 1 .. 256; a table with a null bytes while n_bytes > 0 or a null spans while count > 0.  Then FMGPU_ERR_UNSUPPORTED where count, nq or
 *     count + (emit_unmapped ? nq : 0), the bound on the lines, reaches 2^32 - 256 (records and reads are numbered in 32 bits; this comes before the call looks whether
 *     there is a line at all).
 *   - On the device, FMGPU_ERR_INVALID, looked for in this order; nothing is written (out_line_off neither) and the message names the lowest offender: a record whose
 *     read number is >= nq; a record whose read number lies below its predecessor's; a read r with qoff[r + 1] < qoff[r] ("read r"); then, per line in line order and
 *     inside a line in this order: a read_names row beyond its table or a span beyond its bytes, the same for quals, a quality span whose len is neither 0 nor m, the
 *     same two for seq_names.  The line is named by its record ("record i"), an unmapped line by its read ("unmapped read r").  A read of 2^31 symbols or more, a name
 *     or quality span of 2^31 bytes or more, or a line of 2^32 bytes or more returns FMGPU_ERR_UNSUPPORTED in the same way; an FMGPU_ERR_INVALID line anywhere goes first.
 *   - Every buffer (positions, qbuf, qoff, out, out_line_off, the bytes and spans of each table) may be host or device memory; host buffers are staged (qbuf: its first
 *     qoff[nq] bytes).  The spec, char_of and complement are host memory.  A device `out` needs no alignment: the text is cut into windows of 16 KiB aligned to 16 bytes
 *     of the output address, one per workgroup, which leave as aligned 16-byte stores; only the first and last bytes of the text are stored byte by byte.
 *   - Passes: per record (order, range, each read's records and primary), per record (records at the minimum), per read (offsets, lines), a scan to each read's first
 *     line, per line (length, names and spans), a scan to 64-bit offsets, ONE read-back (size, lines, error words), the write pass.  The call returns after completion and
 *     frees its scratch: 32 bytes per read and 12 bytes per line of the bound count + (emit_unmapped ? nq : 0), plus the scans' own.
 * fmgpu_sam_header: "@HD\tVN:1.6\tSO:unknown\n", one "@SQ\tSN:<name up to its first blank>\tLN:<length>\n" per sequence, and "@PG\tID:<program_id>\n" if program_id
 * is not NULL.  Host memory only, no device.  The counting and capacity rule above.  FMGPU_ERR_INVALID for a null out_bytes, a null out while capacity > 0, a null
 * seq_names or seq_lengths while nseq > 0, a table of fewer than nseq rows, a span beyond the table's bytes, an empty SN.
 * Not built: PAF, CIGAR for edit-distance hits, mate fields in this call (RNEXT, PNEXT, TLEN stay * 0 0; paired-end records: fmgpu_positions_sam_mates below), SAM text per chunk inside fmgpu_map or the feeds, BAM or compression. */
typedef struct fmgpu_sam_spec {            /* 72 bytes, host memory */
    const uint8_t*  qbuf;                  /* the FORWARD batch the positions were mapped from; host or device */
    const uint64_t* qoff;                  /* nq + 1 entries, qoff[0] need not be 0 */
    uint64_t        nq;
    const uint8_t*  char_of;               /* host, 256 entries: the SEQ byte of symbol value c (255 -> 'N' is the caller's choice) */
    const fmgpu_strands* strands;          /* NULL: read = qidx.  Else read = qidx >> 1, strand = qidx & 1; `pair` is ignored */
    const fmgpu_name_table* read_names;    /* NULL: QNAME = the read number in decimal */
    const fmgpu_name_table* quals;         /* NULL: QUAL = '*' */
    const fmgpu_name_table* seq_names;     /* NULL: RNAME = seq_id in decimal */
    uint8_t cigar;                         /* 0: '*';  1: "<m>M" (the caller states the search was ungapped) */
    uint8_t emit_unmapped;                 /* 1: a read without records gets one flag-4 line at its place */
    uint8_t secondary_seq;                 /* 0: SEQ and QUAL of secondary records are '*' */
    uint8_t mapq_unique, mapq_multi;
    uint8_t reserved[3];                   /* 0 */
} fmgpu_sam_spec;
int fmgpu_positions_sam(const fmgpu_position* positions, uint64_t count, const fmgpu_sam_spec* spec,
                        uint8_t* out, uint64_t capacity, uint64_t* out_bytes,
                        uint64_t* out_line_off, uint64_t* out_lines, void* stream);
int fmgpu_sam_header(const fmgpu_name_table* seq_names, const uint64_t* seq_lengths, uint64_t nseq,
                     const char* program_id, uint8_t* out, uint64_t capacity, uint64_t* out_bytes);   /* host memory only, no device */

/* ---- positions to mate pairs: the located hits of paired-end mates joined on the device -------------------------------------------------------
 * fmgpu_positions_mates takes the positions fmgpu_map* returned for the two mates of every fragment and writes one fmgpu_mate_pair per concordant pair of records.
 * It needs no index handle: it reads position records and read offsets only.  Mapping, the feeds and fmgpu_positions_sam are as they were.
 *   - Input order: both arrays are what fmgpu_map* returns: the read number (qidx >> strand_shift) does not decrease over the records (fmgpu_positions_sam's rule).
 *     Separate mode (interleaved = 0): batch A holds mate A of every fragment and batch B mate B, both have n_fragments reads, fragment = read.  Interleaved mode:
 *     positions_b is NULL with count_b = 0 and qoff_b is NULL; the one batch has 2 n_fragments reads, and reads 2f and 2f + 1 are mates A and B of fragment f.
 *   - Geometry of a record x: s(x) its strand (qidx & 1 with strand_shift = 1, else 0), p(x) = pos, m(x) the length of its read (qoff[read + 1] - qoff[read]: only the
 *     lengths of the offsets are used), e(x) = p(x) + m(x).  The read's length stands in for the length of the matched text, also for edit-distance hits: the
 *     convention of fmgpu_positions_sam's "<m>M".
 *   - Record a of mate A and record b of mate B of one fragment are a concordant pair iff a.seq_id == b.seq_id, min_tlen <= tlen <= max_tlen with
 *     tlen = max(e(a), e(b)) - min(p(a), p(b)), and under FMGPU_MATES_FR also s(a) != s(b) and, with f the strand-0 and r the strand-1 record of the two,
 *     p(f) <= p(r) and e(f) <= e(r): the forward mate lies upstream and there is no dovetail.  FMGPU_MATES_ANY drops the strand and order conditions.  With
 *     strand_shift = 0 every strand is 0 and FR finds nothing: that is the rule, not an error.
 *   - Output: one fmgpu_mate_pair per concordant pair; with best = 1 only a fragment's pairs with its minimal errors (a.errors + b.errors in 32 bits).  Order:
 *     fragments ascending, inside a fragment by ascending a, then by ascending (p(b), b).  out_off: NULL, or n_fragments + 1 entries: each fragment's first pair
 *     record, the last entry = *out_count.  out_class: NULL, or n_fragments bytes: 0 neither mate has a record; 1 only A has; 2 only B has; 3 both have, no concordant
 *     pair; 4 at least one pair record; 5 not joined because one of its mates has more than max_records records (max_records > 0).  out_off and out_class are written
 *     whenever the call gets past its checks, also on FMGPU_ERR_CAPACITY.
 *   - *out_count is exact on success and on FMGPU_ERR_CAPACITY alike (then nothing is written to `out`); out == NULL with capacity == 0 is the counting call.
 *   - Before the first use of the device, FMGPU_ERR_INVALID, each with a message of its own, for: a null spec or out_count.  Then n_fragments == 0 returns 0 with
 *     *out_count = 0 and out_off[0] = 0 before anything else is looked at.  Then FMGPU_ERR_INVALID for: a null qoff_a; strand_shift, interleaved, orientation or best out
 *     of range; reserved != 0; min_tlen > max_tlen; a qoff_b or positions_b (or count_b) that does not match the mode; null positions while their count is > 0; a null
 *     out while capacity > 0.  Then FMGPU_ERR_UNSUPPORTED where count_a or count_b reaches 2^32 - 256 or n_fragments reaches 2^31 - 1.
 *   - On the device, in the first passes, FMGPU_ERR_INVALID, looked for in this order and for array A before array B; nothing is written (out_off and out_class
 *     neither, *out_count = 0) and the message names the array and the lowest offender: a record whose read number lies beyond the batch; a record whose read number lies
 *     below its predecessor's; a read r with qoff[r + 1] < qoff[r]; a record with pos >= 2^62 (so that pos + m does not wrap for any m below 2^62).
 *   - Every array (positions, offsets, out, out_off, out_class) may be host or device memory; host arrays are staged.  The spec is host memory.  Device arrays need
 *     no alignment beyond their element's.
 *   - Passes: per record (order, range, pos, each read's records), per read (offsets), per fragment (classes 0, 1, 2, 5), the B-side records ordered by (read, seq_id,
 *     pos, index) with three stable hipcub radix sorts of index values and gathered into 32-byte records, per A-side record a bisection of its fragment's B-records to the
 *     first one with its seq_id and pos >= p(a) - max_tlen and a walk up to pos <= p(a) + max_tlen (tlen >= |p(a) - p(b)|: the window suffices, the join is never
 *     quadratic in a fragment's records) that counts — with best after a walk that takes the minimum —, two scans, ONE read-back (the number of pairs and the error
 *     words), and the walk again to write.  The call returns after completion and frees its scratch: 37 bytes per fragment, 12 per A-side record and 56 per B-side record
 *     (interleaved mode: 68 per record), plus hipcub's own.
 * Not built: a call that maps and joins (paired-end SAM records from the pairs: fmgpu_positions_sam_mates below), mates through the feeds, RF / FF orientations, rescue of an unmapped mate, insert-size
 * estimation, pair lines as text. */
#define FMGPU_MATES_FR  0   /* mates on opposite strands, the forward one upstream, no dovetail */
#define FMGPU_MATES_ANY 1   /* any strands, any order */
typedef struct fmgpu_mate_pair {           /* 32 bytes */
    uint64_t fragment;                     /* the fragment's number */
    uint64_t tlen;                         /* max(e(a), e(b)) - min(p(a), p(b)) */
    uint32_t a, b;                         /* record index of mate A in positions_a, of mate B in positions_b (interleaved mode: both index positions_a) */
    uint32_t errors;                       /* errors of record a + errors of record b */
    uint32_t flags;                        /* bit 0: pos of a <= pos of b (mate A is the leftmost) */
} fmgpu_mate_pair;
typedef struct fmgpu_mates_spec {          /* 56 bytes, host memory */
    const uint64_t* qoff_a;                /* read offsets of batch A (its reads + 1 entries, host or device, qoff[0] need not be 0): only the lengths are used */
    const uint64_t* qoff_b;                /* the same for batch B; NULL in interleaved mode */
    uint64_t n_fragments;
    uint64_t min_tlen, max_tlen;           /* inclusive */
    uint64_t max_records;                  /* 0 = no limit; else a fragment one of whose mates has more records is not joined (class 5) */
    uint8_t  strand_shift;                 /* 0: read = qidx, strand 0; 1: read = qidx >> 1, strand = qidx & 1 (the *_strands numbering) */
    uint8_t  interleaved;                  /* 0: A holds mate 1 of every fragment, B mate 2, fragment = read; 1: one batch, fragment = read >> 1, mate = read & 1 */
    uint8_t  orientation;                  /* FMGPU_MATES_FR, FMGPU_MATES_ANY */
    uint8_t  best;                         /* 1: of a fragment's concordant pairs only those with the minimal a.errors + b.errors */
    uint8_t  reserved[4];                  /* 0 */
} fmgpu_mates_spec;
int fmgpu_positions_mates(const fmgpu_position* positions_a, uint64_t count_a,
                          const fmgpu_position* positions_b, uint64_t count_b,
                          const fmgpu_mates_spec* spec,
                          fmgpu_mate_pair* out, uint64_t capacity, uint64_t* out_count,
                          uint64_t* out_off, uint8_t* out_class, void* stream);

/* ---- positions and mate pairs to paired-end SAM records on the device -------------------------------------------------------------------------
 * fmgpu_positions_sam_mates writes the two mates of every fragment as two SAM lines with the mate fields filled in: the positions fmgpu_map* returned for the two
 * batches and the pair records of fmgpu_positions_mates go in, exactly 2 n_fragments lines come out, line 2f for mate A of fragment f and line 2f + 1 for mate B.  It
 * needs no index handle.  fmgpu_positions_sam, fmgpu_positions_mates and their structs are as they were; fmgpu_sam_header writes the header in front.
 *   - Reads: separate mode (interleaved = 0): mate A of fragment f is read f of batch A (qbuf_a / qoff_a, quals_a), mate B read f of batch B (qbuf_b / qoff_b, quals_b).
 *     Interleaved mode: positions_b is NULL with count_b = 0, qbuf_b, qoff_b and quals_b are NULL, the one batch has 2 n_fragments reads, mates A and B of fragment f are
 *     its reads 2f and 2f + 1 (quals_a rows 2f and 2f + 1), and pairs[].b indexes positions_a: the convention of fmgpu_positions_mates.  Both record arrays are ordered
 *     as fmgpu_map* returns them (the read number qidx >> shift does not decrease; shift = 1 with spec->strands, else 0).
 *   - The policy, one alignment per mate: from a pair record only fragment, a and b are read; errors and tlen are recomputed from the two position records.  The chosen
 *     pair of a fragment is its pair record with the smallest a.errors + b.errors (in 32 bits), among equals the one with the lowest index in `pairs`, which need not be
 *     sorted by fragment.  A fragment with a chosen pair is proper and its two mates take that pair's records.  In every other fragment each mate takes its own primary
 *     record by fmgpu_positions_sam's rule (fewest errors, lowest record index), or none if its read has no record.  No secondary lines are written.
 *   - Fields of mate X with its own record x (or none) and the other mate's record y (or none); p = pos, m = the read's length, e = p + m, s = strand:
 *     QNAME  the row of mate A's read in read_names (row f, interleaved 2f) up to its first ' ' or '\t'; with strip_mate_suffix a result of 3 bytes or more that ends in
 *            "/1" or "/2" loses those two bytes; an empty result is '*'; without a table f in decimal.  Both lines of a fragment carry the same QNAME.
 *     FLAG   1 + (A: 64, B: 128) + (proper: 2) + (x absent: 4) + (y absent: 8) + (x present, s(x) = 1: 16) + (y present, s(y) = 1: 32)
 *     RNAME POS   x present: x's name by fmgpu_positions_sam's RNAME rule and p(x) + 1; x absent, y present: y's (the unmapped mate is placed at its mate); else * 0
 *     MAPQ   x absent: 0; proper: mapq_unique if exactly one pair record of the fragment has the minimal error sum, else mapq_multi; else fmgpu_positions_sam's rule
 *     CIGAR  "<m>M" if x is present, cigar == 1 and m > 0, else '*'
 *     RNEXT  both absent: '*'; exactly one absent, or both on one seq_id: '='; else y's RNAME
 *     PNEXT  y present: p(y) + 1; y absent, x present: p(x) + 1; else 0
 *     TLEN   both present on one seq_id: t = max(e(x), e(y)) - min(p(x), p(y)); the mate with the smaller pos writes t, the other -t, with equal pos A writes t and B
 *            -t; t = 0 is written as 0; in every other case 0
 *     SEQ QUAL    fmgpu_positions_sam's rules for the strand of x, forward if x is absent; m = 0 gives '*', a quality span with len 0 gives '*'
 *     tags   NM:i:<errors of x> NH:i:<records of this mate's read> if x is present, none otherwise
 *   - out_line_off: NULL, or 2 n_fragments + 1 entries, the last = *out_bytes; written whenever the call gets past its checks, also on FMGPU_ERR_CAPACITY.  *out_bytes is
 *     exact on success and on FMGPU_ERR_CAPACITY alike (then nothing is written to `out`); out == NULL with capacity == 0 is the counting call.  n_fragments == 0 returns 0
 *     behind the argument checks with zero bytes and out_line_off[0] = 0.
 *   - Before the first use of the device, FMGPU_ERR_INVALID, each with a message of its own, for: a null spec, char_of or out_bytes; a null qbuf_a or qoff_a while
 *     n_fragments > 0; interleaved, cigar or strip_mate_suffix outside 0 .. 1; reserved != 0; in interleaved mode a qbuf_b, qoff_b, quals_b, positions_b or count_b that
 *     is set, in separate mode a null qbuf_b or qoff_b while n_fragments > 0; null positions or null pairs while their count is > 0; a null out while capacity > 0; a
 *     strands with a null complement or n outside 1 .. 256; a table with a null bytes while n_bytes > 0 or a null spans while count > 0.  Then FMGPU_ERR_UNSUPPORTED where
 *     count_a, count_b or n_pairs reaches 2^32 - 256 or n_fragments reaches 2^31 - 1.
 *   - On the device, FMGPU_ERR_INVALID, looked for in this order and for A before B; nothing is written (out_line_off neither) and the message names the array and the
 *     lowest offender: a record whose read lies beyond its batch; a record whose read lies below its predecessor's; a read whose offsets decrease; a record with
 *     pos >= 2^62; a pair ("pair i") whose fragment is >= n_fragments, whose a or b lies beyond its array, or whose record a or b does not belong to mate A or mate B of
 *     that fragment; then per line in line order ("fragment f mate A" / "mate B") and inside a line in this order: the read_names row beyond its table or its span
 *     beyond the bytes, the same for the quality row, a quality span whose len is neither 0 nor m, the same two for the seq_names row of RNAME and then of RNEXT.  A read
 *     of 2^31 symbols or more, a name or quality span of 2^31 bytes or more, or a line of 2^32 bytes or more returns FMGPU_ERR_UNSUPPORTED in the same way; an
 *     FMGPU_ERR_INVALID line anywhere goes first.
 *   - Every array (positions, pairs, qbuf, qoff, out, out_line_off, the bytes and spans of each table) may be host or device memory; host arrays are staged.  The spec,
 *     char_of and complement are host memory.  A device `out` needs no alignment (the windows of fmgpu_positions_sam).
 *   - Passes: per record of A and of B (range, order, pos, each read's records and primary), per record (records at the minimum), per pair (validity, the minimal key per
 *     fragment), per pair (pairs at the minimum), per fragment (offsets of its two reads, the record of each mate), per line (length, names and spans), one scan to 64-bit
 *     offsets, ONE read-back (size, error words, the symbols of the batches), the write pass over 16 KiB windows of the output.  No lane loops over a fragment's records
 *     or pairs.  The call returns after completion and frees its scratch: 84 bytes per fragment (24 per mate, 12 for the chosen pair, 12 per line), nothing per record or per pair, plus the scan's own.
 * Not built: secondary or supplementary lines, MC / MQ tags, CIGAR for edit-distance hits, RF / FF orientations, rescue of an unmapped mate, insert-size estimation, a
 * call that maps, joins and writes, paired SAM per chunk in the feeds, BAM. */
typedef struct fmgpu_sam_mates_spec {      /* 96 bytes, host memory */
    const uint8_t*  qbuf_a;                /* the FORWARD batch of mate A (interleaved: the one batch, 2 n_fragments reads); host or device */
    const uint64_t* qoff_a;                /* its reads + 1 entries, qoff[0] need not be 0 */
    const uint8_t*  qbuf_b;                /* the batch of mate B; NULL in interleaved mode */
    const uint64_t* qoff_b;
    uint64_t        n_fragments;
    const uint8_t*  char_of;               /* host, 256 entries: the SEQ byte of symbol value c */
    const fmgpu_strands* strands;          /* NULL: strand 0 everywhere, read = qidx.  Else read = qidx >> 1, strand = qidx & 1; `pair` is ignored */
    const fmgpu_name_table* read_names;    /* NULL: QNAME = the fragment's number in decimal; else the rows of batch A's reads */
    const fmgpu_name_table* quals_a;       /* NULL: QUAL = '*' */
    const fmgpu_name_table* quals_b;       /* the same for batch B; NULL in interleaved mode */
    const fmgpu_name_table* seq_names;     /* NULL: RNAME = seq_id in decimal */
    uint8_t interleaved;                   /* 0: two batches, fragment = read; 1: one batch, fragment = read >> 1, mate = read & 1 */
    uint8_t cigar;                         /* 0: '*';  1: "<m>M" (the caller states the search was ungapped) */
    uint8_t strip_mate_suffix;             /* 1: a QNAME of 3 bytes or more that ends in "/1" or "/2" loses those two bytes */
    uint8_t mapq_unique, mapq_multi;
    uint8_t reserved[3];                   /* 0 */
} fmgpu_sam_mates_spec;
int fmgpu_positions_sam_mates(const fmgpu_position* positions_a, uint64_t count_a,
                              const fmgpu_position* positions_b, uint64_t count_b,
                              const fmgpu_mate_pair* pairs, uint64_t n_pairs,
                              const fmgpu_sam_mates_spec* spec,
                              uint8_t* out, uint64_t capacity, uint64_t* out_bytes, uint64_t* out_line_off, void* stream);

/* ---- located seeds to collinear chains on the device ------------------------------------------------------------------------------------------
 * fmgpu_seeds_chain takes the positions fmgpu_locate_hits returned for the records of fmgpu_search_smems, with the seed spans, and says which anchors belong together:
 * every query's anchors joined to collinear chains, best first.  A chain gives the approximate mapping position of a read no search scheme reaches, and the window for
 * an aligner behind it.  It needs no index handle: it reads position records and seed spans only.  Every other call and struct is as it was.
 *   - Input: qidx does not decrease over `positions`; hit indexes `spans`; errors is ignored.  Anchor i is (qidx, seq_id, t = pos, q = spans[hit].qbeg,
 *     l = spans[hit].qlen).  The two strands of a read in the both-strand numbering are two queries: a chain never mixes qidx values.
 *   - Order: inside a query the anchors are ordered by (seq_id, t, q, index in `positions`).  A run is a maximal stretch with one (qidx, seq_id).
 *   - Scores: for anchor i the candidates j are the up to max_lookback anchors directly in front of it in its run.  A candidate must satisfy dt = t_i - t_j >= 1,
 *     dq = q_i - q_j >= 1, dt <= max_gap, dq <= max_gap and dd = |dt - dq| <= max_skew.  gain = min(l_i, dq, dt) - ((gap_cost_q8 * dd) >> 8), in 64 bits; a candidate
 *     counts only with gain >= 1.  value = f(j) + gain.  f(i) = l_i with no predecessor, unless the best value is GREATER than l_i: then f(i) = that value and p(i) = the
 *     candidate that gave it, among equal values the one nearest to i in the order.  f grows strictly along links, and with q + l < 2^31 every f is below 2^32.
 *   - Chains (minimap2's rule, best ends first and backtrack until a used anchor, stated so that it runs in parallel): t(i) = the largest f over the anchors reachable
 *     from i through links, i included.  The heir of j is its child with the largest t, among equals the child earliest in the order.  A chain starts at every anchor that
 *     is not the heir of its predecessor and follows heirs to a leaf.  Its score is f(leaf), or f(leaf) - f(p(start)) if the start has a predecessor; then bit 0 of flags
 *     is set: a branch off a better chain.
 *   - Filters: a chain is reported if score >= min_score and n_anchors >= max(min_anchors, 1).  max_chains then applies to what remains.
 *   - Output order: ascending qidx; inside a query descending score, then the place of the chain's first anchor in the order above.  out_anchor: NULL, or `count`
 *     entries: for the reported chains only and in output order the indices into `positions` of each chain's anchors, first to last (chain k: out_anchor[first ..
 *     first + n_anchors)); what lies behind them is unspecified.  out_off: NULL, or nq + 1 entries: each query's first chain, the last entry = *out_count.  out_class:
 *     NULL, or nq bytes: 0 no anchor; 1 at least one chain reported; 2 anchors, but no chain past the filters; 3 left out by max_anchors.
 *   - *out_count is exact on success and on FMGPU_ERR_CAPACITY alike (then nothing is written to `out` or out_anchor); out_off and out_class are written whenever the call
 *     gets past its checks; out == NULL with capacity == 0 is the counting call.  nq == 0 or count == 0 returns 0 (behind the checks of the next item) with
 *     *out_count = 0, offsets 0 and classes 0.
 *   - Before the first use of the device, FMGPU_ERR_INVALID, each with a message of its own, for: a null spec or out_count; max_gap or max_skew outside 1 .. 2^31 - 1;
 *     gap_cost_q8 above 65536; max_lookback outside 1 .. 256; reserved != 0; null positions or spans while count > 0; a null out while capacity > 0.  Then
 *     FMGPU_ERR_UNSUPPORTED where count or n_spans reaches 2^32 - 256.
 *   - On the device, FMGPU_ERR_INVALID, looked for in this order; nothing is written (out_off and out_class neither, *out_count = 0) and the message names the lowest
 *     offending record: qidx >= nq; a qidx below its predecessor's; hit >= n_spans; pos >= 2^62; a record whose span has qlen == 0 or qbeg + qlen >= 2^31 (spans no
 *     record names are not looked at).
 *   - Every array (positions, spans, out, out_anchor, out_off, out_class) may be host or device memory; host arrays are staged.  The spec is host memory.
 *   - Passes: per record (the checks, each query's records); the order by four stable hipcub radix sorts of index values (q, t, seq_id, qidx); a gather into 16-byte
 *     anchor records that also settles the runs of one anchor; run boundaries; three sweeps per run (f and p forward; t, heir, chain length and leaf backward; each
 *     anchor's chain start and rank forward), runs of up to 32 anchors one per lane, longer runs one per wave with the last max_lookback anchors in an LDS ring and one
 *     cross-lane maximum per step; filters and two scans; ONE read-back (the number of chains, the error words); one sort of the kept chains; chain records; a scatter
 *     in which every anchor writes itself to first + rank.  No lane walks a chain or loops over more than max_lookback candidates, nothing is quadratic in a run.
 *   - Cost of long runs: a run of n anchors takes n x ceil(max_lookback / 64) wave steps in each of the first two sweeps and n in the third, one behind the other on ONE
 *     wave: a single run of 10^5 anchors (a read of a tandem repeat) is 10^5 x ceil(max_lookback / 64) dependent steps per sweep and bounds the call, however small the
 *     rest of the batch.  max_anchors is the caller's guard for it, beside fmgpu_search_smems' max_rows.
 *   - The call returns after completion and frees its scratch: 85 bytes per anchor (24 the sorts, 16 the anchor record, 45 the sweeps' and the passes' words), 25 per
 *     query, 12 per reported chain, plus hipcub's own.
 * Not built: extension of chains past their ends (fmgpu_chains_align below aligns what lies between a chain's ends), chains across the two strands of a query, MAPQ,
 * chaining inside fmgpu_map or the feeds, rescue of an unmapped mate. */
typedef struct fmgpu_chain {               /* 56 bytes */
    uint64_t qidx, seq_id;
    uint64_t tbeg, tend;                   /* pos of the first anchor; pos + qlen of the last */
    uint32_t qbeg, qend;                   /* qbeg of the first anchor; qbeg + qlen of the last */
    uint32_t score, n_anchors;
    uint32_t first;                        /* the chain's anchors are out_anchor[first .. first + n_anchors) */
    uint32_t flags;                        /* bit 0: a branch: the chain's first anchor has a predecessor in a better chain, score = f(leaf) - f(that predecessor) */
} fmgpu_chain;
typedef struct fmgpu_chain_spec {          /* 48 bytes, host memory */
    uint64_t nq;                           /* queries in the numbering of qidx (doubled for the both-strand numbering) */
    uint32_t max_gap, max_skew;            /* each 1 .. 2^31 - 1 */
    uint32_t gap_cost_q8;                  /* 0 .. 65536: penalty per base of skew, 8 fractional bits */
    uint32_t max_lookback;                 /* 1 .. 256 */
    uint32_t min_score, min_anchors;
    uint32_t max_chains;                   /* 0 = all; else the first max_chains of a query in output order */
    uint32_t max_anchors;                  /* 0 = no limit; else a query with more anchors is left out (class 3) */
    uint8_t  reserved[8];                  /* 0 */
} fmgpu_chain_spec;
#ifdef __cplusplus
static_assert(sizeof(fmgpu_chain) == 56 && sizeof(fmgpu_chain_spec) == 48, "fmgpu_chain / fmgpu_chain_spec: the sizes stated above");
#endif
int fmgpu_seeds_chain(const fmgpu_position* positions, uint64_t count,
                      const fmgpu_seed_span* spans, uint64_t n_spans,
                      const fmgpu_chain_spec* spec,
                      fmgpu_chain* out, uint64_t capacity, uint64_t* out_count,
                      uint32_t* out_anchor,   /* NULL, or `count` entries */
                      uint64_t* out_off,      /* NULL, or nq + 1 entries */
                      uint8_t* out_class,     /* NULL, or nq bytes */
                      void* stream);

/* ---- seed chains to CIGAR alignments on the device ---------------------------------------------------------------------------------------------
 * fmgpu_chains_align takes the chains and anchors fmgpu_seeds_chain wrote, the positions and spans that call read, the query batch and the text under every chain, and
 * returns one alignment per chain: the read from its first to its last symbol against the text window [tbeg, tend), as BAM-coded operations.  The anchors of a chain are
 * exact matches; what is aligned are the gaps between consecutive anchors, each a small banded dynamic program of its own.  It needs no index handle.  Every other call
 * and struct is as it was.
 *   - Input: chains[n_chains] and anchors[n_anchor] as fmgpu_seeds_chain wrote them (out and out_anchor); positions[count] and spans[n_spans] as that call read them;
 *     qbuf / qoff: spec->nq reads in the numbering of qidx (the doubled batch for both-strand mapping: the call knows nothing of strands), read r at qbuf[qoff[r] ..
 *     qoff[r + 1]); tbuf / toff: window c, the ranks of the text [tbeg, tend) of chain c, at tbuf[toff[c] .. toff[c + 1]); toff[0] need not be 0.  This is what ONE
 *     fmgpu_extract call returns for the ranges {seq_id, tbeg, tend - tbeg} in chain order.
 *   - The rule.  For chain c with anchors k = 0 .. n - 1 (anchor k = positions[anchors[first + k]]: q_k = its span's qbeg, l_k = its span's qlen, t_k = pos), m the
 *     length of read qidx, Q the read and T the window (T[x] is text position tbeg + x):
 *       Pieces: l'_k = min(l_k, q_{k+1} - q_k, t_{k+1} - t_k) for k < n - 1, l'_{n-1} = l_{n-1}: the term the chain score uses.  Piece k matches Q[q_k, q_k + l'_k) to
 *       T[t_k, t_k + l'_k).  Pieces never overlap and none is empty, and each anchor decides from its successor alone.
 *       Gaps: gap k lies between piece k and piece k + 1: gq = q_{k+1} - q_k - l'_k read symbols, gt = t_{k+1} - t_k - l'_k text symbols.  gq = 0 gives `D gt` when
 *       gt > 0, gt = 0 gives `I gq` when gq > 0, both 0 give nothing.  Otherwise the gap is aligned globally with unit costs on the band lo <= b - a <= hi, lo =
 *       min(0, gt - gq) - band, hi = max(0, gt - gq) + band (a read symbols and b text symbols consumed): D(0, 0) = 0, D(a, b) = the minimum over its in-band
 *       predecessors of D(a - 1, b - 1) + [Q != T], D(a, b - 1) + 1, D(a - 1, b) + 1.  The traceback runs from (gq, gt) and takes at each cell the first that applies:
 *       the diagonal if a, b > 0 and D(a - 1, b - 1) + [Q != T] = D(a, b): `=` or `X`; else the left cell if b > 0, (a, b - 1) is in the band and D(a, b - 1) + 1 =
 *       D(a, b): `D`; else `I`.  With ties the traceback is the definition: the output is reproducible to the byte.
 *       The line: `S qbeg` (qbeg > 0); per k `= l'_k` and the operations of gap k; `S (m - qend)` (m > qend); then the canonical form: neighbours with the same
 *       operation are merged and no operation has length 0.  No extension beyond the chain's ends: the clips are soft clips.
 *       Left out: a chain with a gap of gq > 0 and gt > 0 for which max(gq, gt) > max_gap_len or (gq + 1) * (hi - lo + 1) > max_cells has status 1, n_ops 0 and zero
 *       counts; its first_op stays in the running sequence.  Every other chain has status 0.
 *   - Output: out[n_chains], one record per chain in chain order: first_op ascends with c.  out_ops: one uint32_t per operation, len << 4 | op with BAM's codes I = 1,
 *     D = 2, S = 4, `=` = 7, X = 8.  n_match, n_mismatch, n_ins, n_del count the bases under `=`, X, I and D.  *out_ops_count is exact on success and on
 *     FMGPU_ERR_CAPACITY alike; on FMGPU_ERR_CAPACITY no operation is written and `out` is still written, with its offsets.  out_ops == NULL with ops_capacity == 0 is
 *     the counting call.  n_chains == 0 returns 0 behind the checks of the next item, with *out_ops_count = 0.
 *   - Before the first use of the device, FMGPU_ERR_INVALID, each with a message of its own, for: a null spec or out_ops_count; band or max_gap_len above 65535;
 *     max_cells outside 1 .. 2^30; reserved != 0; with n_chains > 0 a null chains, anchors, positions,
 *     spans, qbuf, qoff, tbuf, toff or out; a null out_ops while ops_capacity > 0.  Then FMGPU_ERR_UNSUPPORTED where n_chains, n_anchor, count or n_spans reaches
 *     2^32 - 256.
 *   - On the device, FMGPU_ERR_INVALID, looked for in this order; nothing is written (*out_ops_count = 0) and the message names the lowest offending chain:
 *     (1) n_anchors == 0, first + n_anchors > n_anchor, or the anchors of chains 0 .. c together more than n_anchor; (2) an anchor index >= count; (3) a hit >=
 *     n_spans, or a span with qlen == 0; (4) qidx >= nq, or an anchor whose qidx / seq_id differs from the chain's; (5) two consecutive anchors not strictly ascending
 *     in both q and t; (6) tbeg / tend / qbeg / qend not what the first and the last anchor give; (7) qend > m; (8) toff[c + 1] - toff[c] != tend - tbeg; (9) a piece
 *     whose text differs from the read: the message names the chain and the anchor.  Check 9 makes every returned line a true alignment of the read against the
 *     window.  A read or a window of 2^28 symbols or more is FMGPU_ERR_UNSUPPORTED (an operation's length has 28 bits).
 *   - Every array (chains, anchors, positions, spans, qbuf, qoff, tbuf, toff, out, out_ops) may be host or device memory; host arrays are staged.  The spec is host
 *     memory.
 *   - Passes: per chain (its own fields, the read, the window); a scan of n_anchors that numbers the (chain, anchor) elements; per element (the anchor's checks, l',
 *     the piece against the text, gq and gt, trivial gaps settled, the other gaps appended to one of four task lists, left-out chains marked); the gap tasks, COUNTING
 *     (runs, first and last operation, bases): gaps of up to 15 x 15 one per lane with the matrix's directions in LDS, larger ones one per wave: the lanes across 64
 *     text columns of a row, the row's left-to-right dependency as a min-plus prefix scan over the lanes, the previous row in the wave's scratch, the directions as two
 *     ballots per 64 cells (2 bits per cell); per element the operations that remain after merging (flags from the neighbours' first and last operations); a scan; per
 *     chain its record; ONE read-back (the operation count, the error words); then per element the clips, pieces and trivial gaps, and the gap tasks again, WRITING.
 *     A writing call fills every matrix twice: nothing between the two passes is kept but 32 bytes per element.  Merged `=` runs are summed with atomic adds into
 *     zeroed slots.  Where the lane tier ends (15 x 15) is not tuned.
 *   - The call returns after completion and frees its scratch: 116 bytes per anchor, 49 per chain, plus hipcub's own, plus the traceback scratch: a wave whose gap needs
 *     up to 16 KiB (directions and one row) keeps it in LDS; above that up to 256 waves take 512 KiB each of a fixed budget of 128 MiB, and gaps that need more than 512 KiB go through
 *     ONE slice of at most 2^28 + 2^21 bytes one behind the other on one wave: what max_cells guards.  No call takes more than 258 MiB of traceback scratch, and none
 *     takes more than band, max_gap_len and max_cells can ask for.
 * Not built: extension past the ends of a chain, affine gaps, CIGAR for the edit-distance hits of the search calls, SAM or PAF lines of chains, alignment inside
 * fmgpu_map or the feeds. */
typedef struct fmgpu_chain_alignment {     /* 32 bytes */
    uint64_t first_op;                     /* the chain's operations are out_ops[first_op .. first_op + n_ops) */
    uint32_t n_ops;
    uint32_t status;                       /* 0 aligned; 1 left out by max_gap_len or max_cells */
    uint32_t n_match, n_mismatch, n_ins, n_del;
} fmgpu_chain_alignment;
typedef struct fmgpu_align_spec {          /* 32 bytes, host memory */
    uint64_t nq;                           /* reads in the numbering of qidx: qoff has nq + 1 entries */
    uint64_t max_cells;                    /* 1 .. 2^30: a gap whose band holds more cells leaves its chain out */
    uint32_t band;                         /* w, 0 .. 65535 */
    uint32_t max_gap_len;                  /* 0 .. 65535: a gap with more read or text symbols leaves its chain out */
    uint8_t  reserved[8];                  /* 0 */
} fmgpu_align_spec;
#ifdef __cplusplus
static_assert(sizeof(fmgpu_chain_alignment) == 32 && sizeof(fmgpu_align_spec) == 32, "fmgpu_chain_alignment / fmgpu_align_spec: the sizes stated above");
#endif
#define FMGPU_OP_I  1u
#define FMGPU_OP_D  2u
#define FMGPU_OP_S  4u
#define FMGPU_OP_EQ 7u
#define FMGPU_OP_X  8u
int fmgpu_chains_align(const fmgpu_chain* chains, uint64_t n_chains,
                       const uint32_t* anchors, uint64_t n_anchor,
                       const fmgpu_position* positions, uint64_t count,
                       const fmgpu_seed_span* spans, uint64_t n_spans,
                       const uint8_t* qbuf, const uint64_t* qoff,
                       const uint8_t* tbuf, const uint64_t* toff,
                       const fmgpu_align_spec* spec,
                       fmgpu_chain_alignment* out,
                       uint32_t* out_ops, uint64_t ops_capacity, uint64_t* out_ops_count,
                       void* stream);

/* device memory helpers for callers that keep queries / results resident in HBM; fmgpu_malloc_host / fmgpu_free_host: pinned host memory, what a feed copies from and to in place */
int fmgpu_malloc(void** ptr, uint64_t bytes);
int fmgpu_free(void* ptr);
int fmgpu_malloc_host(void** ptr, uint64_t bytes);
int fmgpu_free_host(void* ptr);
int fmgpu_memcpy_h2d(void* dst, const void* src, uint64_t bytes);
int fmgpu_memcpy_d2h(void* dst, const void* src, uint64_t bytes);
int fmgpu_synchronize(void* stream);

#ifdef __cplusplus
}
#endif
#endif
