"""ctypes binding of libfmgpu.so (include/fmgpu.h).  No fallback: if the HIP library is missing, importing fails loudly."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMGPU_LIBRARY") or os.path.join(HERE, "libfmgpu.so")   # (FMGPU_LIBRARY: another build of the same ABI, e.g. a tuning variant)

u8p = C.POINTER(C.c_uint8)
u16p = C.POINTER(C.c_uint16)
u64p = C.POINTER(C.c_uint64)

LAYOUTS = {
    "IB8": 0, "IB16": 1, "IB32": 2, "IB16A": 3, "IBP16": 4,
    "EPR8": 5, "EPR16": 6, "EPR32": 7,
    "EPRV2_8": 8, "EPRV2_16": 9, "EPRV2_32": 10, "WAVELET": 11,
    "EPRV3_8": 12, "EPRV3_16": 13, "EPRV3_32": 14, "EPRV4": 15, "EPRV5": 16, "IEPRV7": 17,
    "FBV_64_64K": 18, "FBV_512_64K": 19, "FBV_2048_64K": 20,
}
LAYOUT_NAMES = {v: k for k, v in LAYOUTS.items()}
UINT64_MAX = (1 << 64) - 1

FMGPU_OK = 0
FMGPU_ERR_INVALID = -1
FMGPU_ERR_UNSUPPORTED = -2
FMGPU_ERR_HIP = -3
FMGPU_ERR_NO_DEVICE = -4
FMGPU_ERR_CAPACITY = -5
FMGPU_ERR_NOMEM = -6


class FmgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fmgpu error {code}: {msg}")
        self.code = code


class WaveletNode(C.Structure):
    _fields_ = [("superblocks", u64p), ("n_superblocks", C.c_uint64), ("blocks", u8p), ("n_blocks", C.c_uint64),
                ("bits", u64p), ("n_bits", C.c_uint64), ("total_length", C.c_uint64)]


class StringDesc(C.Structure):
    _fields_ = [("layout", C.c_int32), ("sigma", C.c_int32), ("n", C.c_uint64),
                ("blocks", C.c_void_p), ("blocks_bytes", C.c_uint64),
                ("super_blocks", u64p), ("n_super_blocks", C.c_uint64),
                ("nodes", C.POINTER(WaveletNode)), ("n_nodes", C.c_uint64),
                ("levels", C.c_void_p * 3), ("level_bytes", C.c_uint64 * 3)]


class DenseVectorDesc(C.Structure):
    _fields_ = [("data", u64p), ("n_words", C.c_uint64), ("bit_count", C.c_uint64), ("bits", C.c_uint32),
                ("largest_value", C.c_uint64), ("common_divisor", C.c_uint64)]


class SparseArrayDesc(C.Structure):
    _fields_ = [("n", C.c_uint64), ("l0", u64p), ("n_l0", C.c_uint64), ("l1", u16p), ("n_l1", C.c_uint64),
                ("bits", u64p), ("n_bit_words", C.c_uint64), ("field", DenseVectorDesc * 2)]


class IndexDesc(C.Structure):
    _fields_ = [("bwt", StringDesc), ("bwt_rev", C.POINTER(StringDesc)), ("C", u64p),
                ("annotated_array", C.POINTER(SparseArrayDesc))]


class Hit(C.Structure):
    _fields_ = [("qidx", C.c_uint64), ("lb", C.c_uint64), ("lb_rev", C.c_uint64), ("len", C.c_uint64),
                ("errors", C.c_uint32), ("seq", C.c_uint32)]


HIT_DTYPE = np.dtype([("qidx", "<u8"), ("lb", "<u8"), ("lb_rev", "<u8"), ("len", "<u8"), ("errors", "<u4"), ("seq", "<u4")])
assert HIT_DTYPE.itemsize == C.sizeof(Hit) == 40


class Position(C.Structure):
    """fmgpu_position: one located row of a hit record (fmgpu_locate_hits)"""
    _fields_ = [("qidx", C.c_uint64), ("seq_id", C.c_uint64), ("pos", C.c_uint64), ("errors", C.c_uint32), ("hit", C.c_uint32)]


POSITION_DTYPE = np.dtype([("qidx", "<u8"), ("seq_id", "<u8"), ("pos", "<u8"), ("errors", "<u4"), ("hit", "<u4")])
assert POSITION_DTYPE.itemsize == C.sizeof(Position) == 32


class TextRange(C.Structure):
    """fmgpu_text_range: symbols pos .. pos + len - 1 of sequence seq_id (fmgpu_extract)"""
    _fields_ = [("seq_id", C.c_uint64), ("pos", C.c_uint64), ("len", C.c_uint64)]


TEXT_RANGE_DTYPE = np.dtype([("seq_id", "<u8"), ("pos", "<u8"), ("len", "<u8")])
assert TEXT_RANGE_DTYPE.itemsize == C.sizeof(TextRange) == 24


class SeedSpan(C.Structure):
    """fmgpu_seed_span: where in its read a seed lies (fmgpu_search_smems)"""
    _fields_ = [("qbeg", C.c_uint32), ("qlen", C.c_uint32)]


SEED_SPAN_DTYPE = np.dtype([("qbeg", "<u4"), ("qlen", "<u4")])
assert SEED_SPAN_DTYPE.itemsize == C.sizeof(SeedSpan) == 8


class Scheme(C.Structure):
    _fields_ = [("n_searches", C.c_int32), ("n_parts", C.c_int32), ("pi", u64p), ("l", u64p), ("u", u64p),
                ("partition", u64p), ("edit", C.c_int32), ("reserved", C.c_int32)]


class ExpandedScheme(C.Structure):
    _fields_ = [("n_searches", C.c_int32), ("reserved", C.c_int32), ("length", C.c_uint64), ("pi", u64p), ("l", u64p), ("u", u64p)]


class ScoringMatrix(C.Structure):
    """fmgpu_scoring_matrix: per query symbol, the text symbols it matches for free and at the cost of one error (fmgpu_search_hamming_sm); host memory"""
    _fields_ = [("query_sigma", C.c_int32), ("reserved", C.c_int32), ("free_mask", C.POINTER(C.c_uint32)), ("cost_mask", C.POINTER(C.c_uint32))]


class Stats(C.Structure):
    _fields_ = [("lf_steps", C.c_uint64), ("hits", C.c_uint64), ("kernel_ms", C.c_float), ("prepass_ms", C.c_float),
                ("table_bytes", C.c_uint64), ("table_accesses", C.c_uint64), ("table_steps", C.c_uint64)]


class FeedConfig(C.Structure):
    """fmgpu_feed_config: 0 in a field = the library's default"""
    _fields_ = [("chunk_reads", C.c_uint64), ("chunk_symbols", C.c_uint64), ("slots", C.c_int32), ("host_threads", C.c_int32),
                ("pack4", C.c_int32), ("reserved", C.c_int32)]


class MapQuery(C.Structure):
    """fmgpu_map_query: what fmgpu_map / fmgpu_feed_map run over a batch (kind: MAP_EXACT, MAP_SCHEME, MAP_NG21)"""
    _fields_ = [("kind", C.c_int32), ("n_schemes", C.c_int32), ("schemes", C.c_void_p), ("max_hits_per_query", C.c_uint64),
                ("locate", C.c_int32), ("reserved", C.c_int32), ("first_records", C.c_uint64)]


MAP_EXACT, MAP_SCHEME, MAP_NG21 = 0, 1, 2
assert C.sizeof(MapQuery) == 40


class Strands(C.Structure):
    """fmgpu_strands: the complement table (host memory, n entries) of the both-strand calls, and whether the ladder treats the two strands of a read as a pair"""
    _fields_ = [("complement", u8p), ("n", C.c_int32), ("pair", C.c_int32)]


assert C.sizeof(Strands) == 16


class TextSpan(C.Structure):
    """fmgpu_text_span: bytes offset .. offset + len - 1 of a parsed text (fmgpu_queries_parse: a read's name or quality line)"""
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64)]


TEXT_SPAN_DTYPE = np.dtype([("offset", "<u8"), ("len", "<u8")])
assert TEXT_SPAN_DTYPE.itemsize == C.sizeof(TextSpan) == 16


class ParseResult(C.Structure):
    """fmgpu_parse_result: what fmgpu_queries_parse found (written on success, on a capacity error and on a text error alike)"""
    _fields_ = [("reads", C.c_uint64), ("symbols", C.c_uint64), ("consumed", C.c_uint64), ("foreign", C.c_uint64),
                ("error_line", C.c_uint64), ("error_offset", C.c_uint64)]


assert C.sizeof(ParseResult) == 48
TEXT_LINES, TEXT_FASTA, TEXT_FASTQ = 0, 1, 2
SYM_DROP, SYM_FOREIGN = 254, 255


class NameTable(C.Structure):
    """fmgpu_name_table: the names a READ_NAME / SEQ_NAME column of fmgpu_positions_format copies: bytes, and one span per row (each host or device memory)"""
    _fields_ = [("bytes", C.c_void_p), ("n_bytes", C.c_uint64), ("spans", C.c_void_p), ("count", C.c_uint64)]


class FormatSpec(C.Structure):
    """fmgpu_format_spec: the columns of a line of fmgpu_positions_format and how they are written (host memory)"""
    _fields_ = [("n_cols", C.c_int32), ("cols", C.c_uint8 * 8), ("sep", C.c_uint8), ("strand_shift", C.c_uint8), ("name_stop", C.c_uint8), ("reserved", C.c_uint8),
                ("pos_add", C.c_uint64), ("read_names", C.POINTER(NameTable)), ("seq_names", C.POINTER(NameTable))]


assert C.sizeof(NameTable) == 32 and C.sizeof(FormatSpec) == 40


class SamSpec(C.Structure):
    """fmgpu_sam_spec: the batch, the tables and the switches of fmgpu_positions_sam (host memory)"""
    _fields_ = [("qbuf", C.c_void_p), ("qoff", C.c_void_p), ("nq", C.c_uint64), ("char_of", C.c_void_p), ("strands", C.POINTER(Strands)),
                ("read_names", C.POINTER(NameTable)), ("quals", C.POINTER(NameTable)), ("seq_names", C.POINTER(NameTable)),
                ("cigar", C.c_uint8), ("emit_unmapped", C.c_uint8), ("secondary_seq", C.c_uint8), ("mapq_unique", C.c_uint8), ("mapq_multi", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


assert C.sizeof(SamSpec) == 72


class MatePair(C.Structure):
    """fmgpu_mate_pair: one concordant pair of records of the two mates of a fragment (fmgpu_positions_mates)"""
    _fields_ = [("fragment", C.c_uint64), ("tlen", C.c_uint64), ("a", C.c_uint32), ("b", C.c_uint32), ("errors", C.c_uint32), ("flags", C.c_uint32)]


MATE_PAIR_DTYPE = np.dtype([("fragment", "<u8"), ("tlen", "<u8"), ("a", "<u4"), ("b", "<u4"), ("errors", "<u4"), ("flags", "<u4")])
assert MATE_PAIR_DTYPE.itemsize == C.sizeof(MatePair) == 32


class MatesSpec(C.Structure):
    """fmgpu_mates_spec: the read offsets, the fragment count, the template length bounds and the switches of fmgpu_positions_mates (host memory)"""
    _fields_ = [("qoff_a", C.c_void_p), ("qoff_b", C.c_void_p), ("n_fragments", C.c_uint64), ("min_tlen", C.c_uint64), ("max_tlen", C.c_uint64),
                ("max_records", C.c_uint64), ("strand_shift", C.c_uint8), ("interleaved", C.c_uint8), ("orientation", C.c_uint8), ("best", C.c_uint8),
                ("reserved", C.c_uint8 * 4)]


assert C.sizeof(MatesSpec) == 56


class SamMatesSpec(C.Structure):
    """fmgpu_sam_mates_spec: the two batches, the tables and the switches of fmgpu_positions_sam_mates (host memory)"""
    _fields_ = [("qbuf_a", C.c_void_p), ("qoff_a", C.c_void_p), ("qbuf_b", C.c_void_p), ("qoff_b", C.c_void_p), ("n_fragments", C.c_uint64), ("char_of", C.c_void_p),
                ("strands", C.POINTER(Strands)), ("read_names", C.POINTER(NameTable)), ("quals_a", C.POINTER(NameTable)), ("quals_b", C.POINTER(NameTable)),
                ("seq_names", C.POINTER(NameTable)), ("interleaved", C.c_uint8), ("cigar", C.c_uint8), ("strip_mate_suffix", C.c_uint8), ("mapq_unique", C.c_uint8),
                ("mapq_multi", C.c_uint8), ("reserved", C.c_uint8 * 3)]


assert C.sizeof(SamMatesSpec) == 96


class Chain(C.Structure):
    """fmgpu_chain: one collinear chain of located seeds (fmgpu_seeds_chain)"""
    _fields_ = [("qidx", C.c_uint64), ("seq_id", C.c_uint64), ("tbeg", C.c_uint64), ("tend", C.c_uint64), ("qbeg", C.c_uint32), ("qend", C.c_uint32),
                ("score", C.c_uint32), ("n_anchors", C.c_uint32), ("first", C.c_uint32), ("flags", C.c_uint32)]


CHAIN_DTYPE = np.dtype([("qidx", "<u8"), ("seq_id", "<u8"), ("tbeg", "<u8"), ("tend", "<u8"), ("qbeg", "<u4"), ("qend", "<u4"), ("score", "<u4"), ("n_anchors", "<u4"),
                        ("first", "<u4"), ("flags", "<u4")])
assert CHAIN_DTYPE.itemsize == C.sizeof(Chain) == 56


class ChainSpec(C.Structure):
    """fmgpu_chain_spec: the query count, the link conditions, the filters and the guards of fmgpu_seeds_chain (host memory)"""
    _fields_ = [("nq", C.c_uint64), ("max_gap", C.c_uint32), ("max_skew", C.c_uint32), ("gap_cost_q8", C.c_uint32), ("max_lookback", C.c_uint32),
                ("min_score", C.c_uint32), ("min_anchors", C.c_uint32), ("max_chains", C.c_uint32), ("max_anchors", C.c_uint32), ("reserved", C.c_uint8 * 8)]


assert C.sizeof(ChainSpec) == 48


class ChainAlignment(C.Structure):
    """fmgpu_chain_alignment: where a chain's operations stand, its status and the bases under =, X, I and D (fmgpu_chains_align)"""
    _fields_ = [("first_op", C.c_uint64), ("n_ops", C.c_uint32), ("status", C.c_uint32), ("n_match", C.c_uint32), ("n_mismatch", C.c_uint32), ("n_ins", C.c_uint32),
                ("n_del", C.c_uint32)]


CHAIN_ALIGNMENT_DTYPE = np.dtype([("first_op", "<u8"), ("n_ops", "<u4"), ("status", "<u4"), ("n_match", "<u4"), ("n_mismatch", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4")])
assert CHAIN_ALIGNMENT_DTYPE.itemsize == C.sizeof(ChainAlignment) == 32


class AlignSpec(C.Structure):
    """fmgpu_align_spec: the read count, the band and the two guards of fmgpu_chains_align (host memory)"""
    _fields_ = [("nq", C.c_uint64), ("max_cells", C.c_uint64), ("band", C.c_uint32), ("max_gap_len", C.c_uint32), ("reserved", C.c_uint8 * 8)]


assert C.sizeof(AlignSpec) == 32
OP_I, OP_D, OP_S, OP_EQ, OP_X = 1, 2, 4, 7, 8                    # BAM's operation codes: an operation is len << 4 | code
OP_CHARS = {OP_I: "I", OP_D: "D", OP_S: "S", OP_EQ: "=", OP_X: "X"}
CHAIN_CLASSES = ("none", "chained", "filtered", "skipped")
MATES_FR, MATES_ANY = 0, 1
MATE_CLASSES = ("none", "only_a", "only_b", "discordant", "paired", "skipped")
COL_QIDX, COL_SEQ_ID, COL_POS, COL_ERRORS, COL_HIT, COL_READ, COL_STRAND, COL_READ_NAME, COL_SEQ_NAME = range(9)
COLUMNS = {"qidx": COL_QIDX, "seq_id": COL_SEQ_ID, "pos": COL_POS, "errors": COL_ERRORS, "hit": COL_HIT, "read": COL_READ, "strand": COL_STRAND,
           "read_name": COL_READ_NAME, "seq_name": COL_SEQ_NAME}


# every symbol include/fmgpu.h declares (tests check that the library exports all of them)
EXPORTS = [
    "fmgpu_abi_version", "fmgpu_last_error", "fmgpu_device_count", "fmgpu_set_device",
    "fmgpu_index_create", "fmgpu_index_destroy", "fmgpu_index_info", "fmgpu_string_query",
    "fmgpu_search_exact", "fmgpu_search_exact_packed", "fmgpu_search_scheme", "fmgpu_search_ng21", "fmgpu_search_backtracking", "fmgpu_locate", "fmgpu_locate_hits",
    "fmgpu_malloc", "fmgpu_free", "fmgpu_memcpy_h2d", "fmgpu_memcpy_d2h", "fmgpu_synchronize",
    "fmgpu_build_index", "fmgpu_built_free", "fmgpu_built_get", "fmgpu_index_accelerate", "fmgpu_index_accelerate_search",
    "fmgpu_index_accelerate_exact", "fmgpu_index_accelerate_locate", "fmgpu_hits_sort", "fmgpu_hits_pack16",
    "fmgpu_index_row_bits", "fmgpu_index_accelerate_lf", "fmgpu_search_exact_depth", "fmgpu_cursor_extend", "fmgpu_hits_pack24",
    "fmgpu_index_save", "fmgpu_index_load",
    "fmgpu_replicas_load", "fmgpu_replicas_destroy", "fmgpu_replicas_info", "fmgpu_replicas_search_exact", "fmgpu_replicas_search_scheme",
    "fmgpu_replicas_search_ng21", "fmgpu_replicas_locate",
    "fmgpu_set_option", "fmgpu_get_option", "fmgpu_index_formats", "fmgpu_index_clone", "fmgpu_replicas_peer_copies",
    "fmgpu_index_accelerate_extract", "fmgpu_sequence_lengths", "fmgpu_extract",
    "fmgpu_queries_pack4", "fmgpu_queries_unpack4", "fmgpu_search_exact_q4", "fmgpu_search_scheme_q4", "fmgpu_search_ng21_q4",
    "fmgpu_search_best", "fmgpu_search_best_ng21", "fmgpu_search_best_q4", "fmgpu_search_best_ng21_q4",
    "fmgpu_search_smems", "fmgpu_search_smems_q4", "fmgpu_search_hamming_sm",
    "fmgpu_feed_create", "fmgpu_feed_destroy", "fmgpu_feed_plan", "fmgpu_feed_search_exact", "fmgpu_feed_search_exact_q4", "fmgpu_feed_search_exact_v",
    "fmgpu_feed_search_scheme", "fmgpu_feed_search_scheme_v", "fmgpu_feed_info", "fmgpu_malloc_host", "fmgpu_free_host",
    "fmgpu_map", "fmgpu_map_q4", "fmgpu_hits_from_intervals", "fmgpu_feed_map", "fmgpu_feed_map_v",
    "fmgpu_queries_parse", "fmgpu_feed_map_text",
    "fmgpu_queries_strands", "fmgpu_search_best_pairs", "fmgpu_search_best_ng21_pairs", "fmgpu_map_strands", "fmgpu_feed_map_strands", "fmgpu_feed_map_text_strands",
    "fmgpu_positions_format",
    "fmgpu_positions_sam", "fmgpu_sam_header",
    "fmgpu_positions_mates",
    "fmgpu_positions_sam_mates",
    "fmgpu_seeds_chain",
    "fmgpu_chains_align",
]

# fmgpu_option (include/fmgpu.h) and the defaults the library starts with
OPTIONS = {"pair_table": 0, "dense_dna": 1, "symbol_planes": 2, "expand_dna": 3, "lf_table": 4, "fused_locate": 5, "heavy_first": 6,
           "force_wide": 7, "kernel_select": 8, "fail_scratch": 9, "bucket_rows": 10, "suffix_sorter": 11, "sample_chain": 12}
OPTION_DEFAULTS = {"pair_table": 1, "dense_dna": 1, "symbol_planes": 1, "expand_dna": 1, "lf_table": 1, "fused_locate": 1, "heavy_first": 1,
                   "force_wide": 0, "kernel_select": 0, "fail_scratch": 0, "bucket_rows": 0, "suffix_sorter": 0, "sample_chain": 1}
# FMGPU_SEL_* bits of the kernel_select option
SEL_GENERAL_DFS, SEL_NO_PREFIX_TABLE, SEL_NO_LF3, SEL_NO_LF_GENERAL, SEL_NO_WALK_TABLE, SEL_NO_LENGTH_BUCKETS = 2, 4, 8, 16, 32, 64
SEL_EXACT_ON_TREE, SEL_EXACT_ONE_SYMBOL, SEL_LOCATE_PER_LANE, SEL_NO_SHARING, SEL_NO_EXACT_LUT, SEL_LEAN_FORMAT_A, SEL_NO_LEAN = 1 << 21, 1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 29, 1 << 30
SEL_NO_BOARD = 1 << 26
SEL_UNPACK_QUERIES = 1 << 27
SEL_NO_SAMPLE_CHAIN = 1 << 28
# fmgpu_index_formats bits: what a handle holds beside (or as) the layout it was given
FMT_BLOCKS, FMT_PAIRS, FMT_DENSE, FMT_PLANES, FMT_TREE, FMT_REFERENCE, FMT_LF, FMT_KSTEP, FMT_INTERVALS, FMT_WALK, FMT_PREFIX, FMT_LOCATE, FMT_FUSED = (1 << k for k in range(13))
FMT_EXTRACT = 1 << 13
FMT_CHAIN = 1 << 14

_lib = None


def _one_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so (same sonames as /opt/rocm's).  A process that loads
    libfmgpu.so first binds the system runtime, and a later `import torch` brings the bundled copy in beside it: two HIP runtimes in one
    process, and the second one to initialise does not find the GPU (hipErrorNoDevice).  Tensors and streams are shared with torch, so the
    runtime has to be ONE: if torch is installed but not imported yet, its copies are loaded first and libfmgpu.so binds to them by soname
    (exactly what happens when torch is imported first).  FMGPU_SYSTEM_HIP=1 leaves the loader alone."""
    import importlib.util
    import sys
    if "torch" in sys.modules or os.environ.get("FMGPU_SYSTEM_HIP") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing — build it with __graft_entry__.build() "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _one_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.fmgpu_last_error.restype = C.c_char_p
    L.fmgpu_device_count.argtypes = [C.POINTER(C.c_int)]
    L.fmgpu_set_device.argtypes = [C.c_int]
    L.fmgpu_index_create.argtypes = [C.POINTER(IndexDesc), C.POINTER(C.c_void_p)]
    L.fmgpu_index_destroy.argtypes = [C.c_void_p]
    L.fmgpu_index_info.argtypes = [C.c_void_p, u64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), u64p]
    L.fmgpu_string_query.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.fmgpu_search_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                     C.POINTER(Stats), C.c_void_p]
    L.fmgpu_search_scheme.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Scheme), C.c_uint64,
                                      C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats), C.c_void_p]
    if hasattr(L, "fmgpu_search_exact_packed"):
        L.fmgpu_search_exact_packed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(Stats), C.c_void_p]
    if hasattr(L, "fmgpu_search_ng21"):
        L.fmgpu_search_ng21.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ExpandedScheme), C.c_uint64,
                                        C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats), C.c_void_p]
    L.fmgpu_search_backtracking.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                            C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats), C.c_void_p]
    L.fmgpu_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(Stats), C.c_void_p]
    L.fmgpu_locate_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats), C.c_void_p]
    L.fmgpu_index_accelerate_extract.argtypes = [C.c_void_p, C.c_int32]
    L.fmgpu_sequence_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    L.fmgpu_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats), C.c_void_p]
    if hasattr(L, "fmgpu_index_accelerate"):
        L.fmgpu_index_accelerate.argtypes = [C.c_void_p, C.c_int32]
    if hasattr(L, "fmgpu_hits_pack16"):
        L.fmgpu_hits_pack16.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.fmgpu_hits_pack24.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    if hasattr(L, "fmgpu_hits_sort"):
        L.fmgpu_hits_sort.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    if hasattr(L, "fmgpu_index_accelerate_locate"):
        L.fmgpu_index_accelerate_locate.argtypes = [C.c_void_p, C.c_int32]
    if hasattr(L, "fmgpu_index_accelerate_exact"):
        L.fmgpu_index_accelerate_exact.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    if hasattr(L, "fmgpu_index_accelerate_search"):
        L.fmgpu_index_accelerate_search.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.fmgpu_index_row_bits.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.fmgpu_index_accelerate_lf.argtypes = [C.c_void_p, C.c_int32]
    L.fmgpu_search_exact_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.fmgpu_cursor_extend.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmgpu_index_save.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    L.fmgpu_index_load.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.fmgpu_index_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    if hasattr(L, "fmgpu_replicas_load"):
        L.fmgpu_replicas_load.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
        L.fmgpu_replicas_destroy.argtypes = [C.c_void_p]
        L.fmgpu_replicas_peer_copies.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.fmgpu_replicas_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
        L.fmgpu_replicas_search_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.fmgpu_replicas_search_scheme.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Scheme), C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats)]
        L.fmgpu_replicas_search_ng21.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ExpandedScheme), C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats)]
        L.fmgpu_replicas_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
    L.fmgpu_queries_pack4.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.fmgpu_queries_unpack4.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.fmgpu_search_exact_q4.argtypes = L.fmgpu_search_exact.argtypes
    L.fmgpu_search_scheme_q4.argtypes = L.fmgpu_search_scheme.argtypes
    L.fmgpu_search_ng21_q4.argtypes = L.fmgpu_search_ng21.argtypes
    L.fmgpu_search_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Scheme), C.c_int32, C.c_uint64,
                                    C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.POINTER(Stats), C.c_void_p]
    L.fmgpu_search_best_ng21.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ExpandedScheme), C.c_int32, C.c_uint64,
                                         C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.POINTER(Stats), C.c_void_p]
    L.fmgpu_search_best_q4.argtypes = L.fmgpu_search_best.argtypes
    L.fmgpu_search_best_ng21_q4.argtypes = L.fmgpu_search_best_ng21.argtypes
    L.fmgpu_search_smems.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64,
                                     C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.POINTER(Stats), C.c_void_p]
    L.fmgpu_search_smems_q4.argtypes = L.fmgpu_search_smems.argtypes
    L.fmgpu_search_hamming_sm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Scheme), C.POINTER(ScoringMatrix), C.c_uint64,
                                          C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats), C.c_void_p]
    if hasattr(L, "fmgpu_feed_create"):                       # (FMGPU_LIBRARY may name an older build of the same ABI: tools/feed_probe.py times one)
        L.fmgpu_feed_create.argtypes = [C.c_void_p, C.POINTER(FeedConfig), C.POINTER(C.c_void_p)]
        L.fmgpu_feed_destroy.argtypes = [C.c_void_p]
        L.fmgpu_feed_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, u64p]
        L.fmgpu_feed_search_exact.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.fmgpu_feed_search_exact_q4.argtypes = L.fmgpu_feed_search_exact.argtypes
        L.fmgpu_feed_search_exact_v.argtypes = L.fmgpu_feed_search_exact.argtypes
        L.fmgpu_feed_search_scheme.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(Scheme), C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.POINTER(Stats)]
        L.fmgpu_feed_search_scheme_v.argtypes = L.fmgpu_feed_search_scheme.argtypes
        L.fmgpu_feed_info.argtypes = [C.c_void_p, u64p, u64p, u64p, u64p, u64p]
        L.fmgpu_malloc_host.argtypes = [C.POINTER(C.c_void_p), C.c_uint64]
        L.fmgpu_free_host.argtypes = [C.c_void_p]
    if hasattr(L, "fmgpu_map"):                               # (FMGPU_LIBRARY may name an older build of the same ABI: tools/map_probe.py times one)
        L.fmgpu_map.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(MapQuery), C.c_void_p, C.c_uint64, u64p,
                                C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.POINTER(Stats), C.POINTER(Stats), C.c_void_p]
        L.fmgpu_map_q4.argtypes = L.fmgpu_map.argtypes
        L.fmgpu_hits_from_intervals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p]
        L.fmgpu_feed_map.argtypes = L.fmgpu_map.argtypes[:-1]
        L.fmgpu_feed_map_v.argtypes = L.fmgpu_feed_map.argtypes
    if hasattr(L, "fmgpu_queries_parse"):                     # (FMGPU_LIBRARY may name an older build of the same ABI)
        L.fmgpu_queries_parse.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                          C.c_void_p, C.c_void_p, C.POINTER(ParseResult), C.c_void_p]
    if hasattr(L, "fmgpu_feed_map_text"):
        L.fmgpu_feed_map_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(MapQuery),
                                          C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_uint64, u64p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ParseResult), C.POINTER(Stats), C.POINTER(Stats)]
    if hasattr(L, "fmgpu_map_strands"):                       # (FMGPU_LIBRARY may name an older build of the same ABI)
        L.fmgpu_queries_strands.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.fmgpu_search_best_pairs.argtypes = L.fmgpu_search_best.argtypes
        L.fmgpu_search_best_ng21_pairs.argtypes = L.fmgpu_search_best_ng21.argtypes
        L.fmgpu_map_strands.argtypes = L.fmgpu_map.argtypes[:5] + [C.POINTER(Strands)] + L.fmgpu_map.argtypes[5:]
        L.fmgpu_feed_map_strands.argtypes = L.fmgpu_map_strands.argtypes[:-1]
        L.fmgpu_feed_map_text_strands.argtypes = L.fmgpu_feed_map_text.argtypes[:8] + [C.POINTER(Strands)] + L.fmgpu_feed_map_text.argtypes[8:]
    if hasattr(L, "fmgpu_positions_format"):                  # (FMGPU_LIBRARY may name an older build of the same ABI)
        L.fmgpu_positions_format.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(FormatSpec), C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p]
    if hasattr(L, "fmgpu_positions_sam"):                     # (FMGPU_LIBRARY may name an older build of the same ABI)
        L.fmgpu_positions_sam.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(SamSpec), C.c_void_p, C.c_uint64, u64p, C.c_void_p, u64p, C.c_void_p]
        L.fmgpu_sam_header.argtypes = [C.POINTER(NameTable), C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_uint64, u64p]
    if hasattr(L, "fmgpu_positions_mates"):
        L.fmgpu_positions_mates.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(MatesSpec), C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "fmgpu_positions_sam_mates"):
        L.fmgpu_positions_sam_mates.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(SamMatesSpec), C.c_void_p, C.c_uint64, u64p,
                                                C.c_void_p, C.c_void_p]
    if hasattr(L, "fmgpu_seeds_chain"):
        L.fmgpu_seeds_chain.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(ChainSpec), C.c_void_p, C.c_uint64, u64p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    if hasattr(L, "fmgpu_chains_align"):
        L.fmgpu_chains_align.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(AlignSpec), C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p]
    L.fmgpu_set_option.argtypes = [C.c_int32, C.c_int64]
    L.fmgpu_get_option.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
    L.fmgpu_index_formats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.fmgpu_malloc.argtypes = [C.POINTER(C.c_void_p), C.c_uint64]
    L.fmgpu_free.argtypes = [C.c_void_p]
    L.fmgpu_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.fmgpu_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.fmgpu_synchronize.argtypes = [C.c_void_p]
    if hasattr(L, "fmgpu_build_index"):
        L.fmgpu_build_index.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.c_uint64, C.c_int32,
                                        C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.fmgpu_built_free.argtypes = [C.c_void_p]
        L.fmgpu_built_get.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), u64p]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise FmgpuError(rc, lib().fmgpu_last_error().decode("utf-8", "replace"))


def set_option(name, value):
    """fmgpu_set_option by name (OPTIONS) or number"""
    check(lib().fmgpu_set_option(OPTIONS[name] if isinstance(name, str) else int(name), int(value)))


def get_option(name):
    v = C.c_int64()
    check(lib().fmgpu_get_option(OPTIONS[name] if isinstance(name, str) else int(name), C.byref(v)))
    return int(v.value)


def ptr(a):
    """numpy array / int device pointer / None -> void*"""
    if a is None:
        return None
    if isinstance(a, (int, np.integer)):
        return C.c_void_p(int(a))
    if hasattr(a, "ptr") and hasattr(a, "nbytes") and not hasattr(a, "ctypes"):   # DeviceBuffer or any (ptr, nbytes) device view
        return C.c_void_p(a.ptr)
    return C.c_void_p(a.ctypes.data)


class DeviceBuffer:
    """a chunk of HBM owned by the caller (queries / results that stay resident)"""

    def __init__(self, nbytes):
        p = C.c_void_p()
        check(lib().fmgpu_malloc(C.byref(p), nbytes))
        self.ptr, self.nbytes = p.value, nbytes

    @classmethod
    def from_array(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(max(a.nbytes, 8))
        check(lib().fmgpu_memcpy_h2d(C.c_void_p(b.ptr), C.c_void_p(a.ctypes.data), a.nbytes))
        return b

    def to_array(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        check(lib().fmgpu_memcpy_d2h(C.c_void_p(out.ctypes.data), C.c_void_p(self.ptr), out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().fmgpu_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PinnedBuffer:
    """pinned host memory (fmgpu_malloc_host): what a feed copies from and writes to in place.  `.array(dtype, count)` is a numpy view of it (keep the buffer alive)."""

    def __init__(self, nbytes):
        p = C.c_void_p()
        check(lib().fmgpu_malloc_host(C.byref(p), nbytes))
        self.ptr, self.nbytes = p.value, nbytes

    def array(self, dtype, count=None):
        dtype = np.dtype(dtype)
        count = self.nbytes // dtype.itemsize if count is None else count
        assert count * dtype.itemsize <= self.nbytes
        return np.frombuffer((C.c_uint8 * self.nbytes).from_address(self.ptr), dtype=dtype, count=count)

    @classmethod
    def from_array(cls, a):
        a = np.ascontiguousarray(a)
        b = cls(max(a.nbytes, 8))
        b.array(np.uint8, a.nbytes)[:] = a.view(np.uint8).reshape(-1)
        return b

    def free(self):
        if self.ptr:
            lib().fmgpu_free_host(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
