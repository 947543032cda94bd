"""fmindex-collection_amd — MI355X-native backward-search engine (host-side Python mirror over the C-ABI).

The product is libfmgpu.so (hand-written HIP for gfx950, include/fmgpu.h); this package is the thin Python
host layer used by the tests and bench.py.  It mirrors the reference's names for the hot path:
FMIndex / BiFMIndex (fmindex/FMIndex.h, fmindex/BiFMIndex.h), search_no_errors.search (search/SearchNoErrors.h),
search_backtracking.search (search/Backtracking.h), search_ng26.search (search/SearchNg26.h), LocateLinear
(locate.h), search_scheme.* (search_scheme/).  The C++ mirror of the template API is include/fmc_gpu.hpp.

There is no CPU fallback anywhere in this package: without libfmgpu.so and a GPU every compute call raises.
"""
import ctypes as C
import os

import numpy as np

from . import capi
from .capi import FmgpuError, DeviceBuffer, PinnedBuffer, LAYOUTS, UINT64_MAX, HIT_DTYPE, POSITION_DTYPE, TEXT_RANGE_DTYPE, SEED_SPAN_DTYPE, TEXT_SPAN_DTYPE, MATE_PAIR_DTYPE, CHAIN_DTYPE
from . import search_scheme  # noqa: F401

__all__ = ["FMIndex", "BiFMIndex", "search_no_errors", "search_backtracking", "search_ng26", "search_ng21", "search", "search_n", "search_best", "search_smems", "search_hamming_sm", "ScoringMatrix", "LocateLinear", "search_locate", "reconstruct_text",
           "search_scheme", "FmgpuError", "DeviceBuffer", "flatten", "device_count", "Replicas", "options",
           "PackedQueries", "pack_queries", "unpack_queries", "pack_queries_device", "Feed", "PinnedBuffer",
           "symbol_table", "parse_queries", "parse_stream", "ParsedQueries", "MappedText", "TextError", "format_positions", "pack_names", "format_sam", "sam_header", "char_table", "join_mates", "MatePairs", "format_sam_mates", "chain_seeds", "SeedChains", "align_chains", "ChainAlignments", "LINES", "FASTA", "FASTQ", "DROP", "FOREIGN"]


class _Options:
    """the library's process-wide options (fmgpu_set_option, include/fmgpu.h): `options["pair_table"] = 0`, `del options["pair_table"]` puts the default back,
    `with options(pair_table=0, kernel_select=capi.SEL_GENERAL_DFS): ...` sets and restores"""

    def __setitem__(self, name, value):
        capi.set_option(name, value)

    def __getitem__(self, name):
        return capi.get_option(name)

    def __delitem__(self, name):
        capi.set_option(name, capi.OPTION_DEFAULTS[name])

    def pop(self, name, default=None):
        del self[name]

    def __call__(self, **kw):
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: self[k] for k in kw}
            try:
                for k, v in kw.items():
                    self[k] = v
                yield self
            finally:
                for k, v in old.items():
                    self[k] = v
        return scope()


options = _Options()


def device_count():
    n = C.c_int()
    capi.check(capi.lib().fmgpu_device_count(C.byref(n)))
    return n.value


def flatten(sequences):
    """Sequences (list of byte sequences) -> (qbuf uint8[total], qoff uint64[nq+1]) — the ABI's query format"""
    lens = np.fromiter((len(q) for q in sequences), dtype=np.uint64, count=len(sequences))
    qoff = np.zeros(len(sequences) + 1, dtype=np.uint64)
    np.cumsum(lens, out=qoff[1:])
    total = int(qoff[-1])
    qbuf = np.zeros(max(total, 1), dtype=np.uint8)
    if total:
        qbuf[:total] = np.concatenate([np.asarray(q, dtype=np.uint8) for q in sequences if len(q)])
    return qbuf, qoff


def _u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64))


def _buffer(a):
    """(void*, bytes) of a numpy array, a DeviceBuffer / (ptr, nbytes) device view or a torch tensor (its memory in place)"""
    if hasattr(a, "data_ptr") and hasattr(a, "element_size"):
        return C.c_void_p(a.data_ptr()), a.numel() * a.element_size()
    return capi.ptr(a), a.nbytes


class _StringArrays:
    """host arrays of one reference String object, kept alive while the descriptor is in use"""

    def __init__(self, layout, sigma, n, blocks=None, super_blocks=None, nodes=None, levels=None, super_row=None):
        self.layout, self.sigma, self.n = layout, sigma, n
        self.super_row = super_row or sigma                      # entries per super-block row (FlattenedBitvectors2L::l0 has sigma + 1)
        # EPRV3/4/5/7: `blocks` = the bits array, `levels` = counter arrays bottom-up (None where the layout has none)
        self.levels = None if levels is None else [None if a is None else np.ascontiguousarray(a).view(np.uint8) for a in levels]
        self.blocks = None if blocks is None else np.ascontiguousarray(blocks).view(np.uint8)
        self.super_blocks = None if super_blocks is None else _u64(super_blocks).reshape(-1)
        self.nodes = nodes  # list of (superblocks u64, blocks u8, bits u64, total_length)
        self._node_arr = None

    def desc(self):
        d = capi.StringDesc()
        d.layout = LAYOUTS[self.layout]
        d.sigma = self.sigma
        d.n = self.n
        if self.blocks is not None:
            d.blocks = self.blocks.ctypes.data
            d.blocks_bytes = self.blocks.nbytes
            d.super_blocks = self.super_blocks.ctypes.data_as(capi.u64p)
            d.n_super_blocks = self.super_blocks.size // self.super_row
        if self.levels is not None:
            for k, a in enumerate(self.levels[:3]):
                if a is not None and a.size:
                    d.levels[k] = a.ctypes.data
                    d.level_bytes[k] = a.nbytes
        if self.nodes is not None:
            arr = (capi.WaveletNode * len(self.nodes))()
            keep = []
            for k, (sb, bl, bits, total) in enumerate(self.nodes):
                sb, bl, bits = _u64(sb), np.ascontiguousarray(bl, dtype=np.uint8), _u64(bits)
                keep.append((sb, bl, bits))
                arr[k].superblocks = sb.ctypes.data_as(capi.u64p); arr[k].n_superblocks = sb.size
                arr[k].blocks = bl.ctypes.data_as(capi.u8p); arr[k].n_blocks = bl.size
                arr[k].bits = bits.ctypes.data_as(capi.u64p); arr[k].n_bits = bits.size
                arr[k].total_length = int(total)
            self._node_arr, self._keep = arr, keep
            d.nodes = arr
            d.n_nodes = len(self.nodes)
        return d


class FMIndex:
    """fmindex/FMIndex.h:14-134 (bidirectional=False) / fmindex/BiFMIndex.h:17-216 (BiFMIndex subclass), resident in HBM.

    Construct from the arrays a reference index object holds (`from_reference_arrays`) or from sequences with the
    GPU builder (`from_sequences`, replaces the libsais-based constructor fmindex/FMIndex.h:58-104)."""

    bidirectional = False

    def __init__(self, handle, keep=None, built=None):
        self._h = handle
        self._keep = keep
        self._built = built
        n, sigma, layout, bidir, dbytes = C.c_uint64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        capi.check(capi.lib().fmgpu_index_info(self._h, C.byref(n), C.byref(sigma), C.byref(layout), C.byref(bidir), C.byref(dbytes)))
        self.n, self.Sigma, self.layout, self.device_bytes = n.value, sigma.value, capi.LAYOUT_NAMES[layout.value], dbytes.value
        self.bidirectional = bool(bidir.value)

    # -------------------------------------------------------------- construction
    @classmethod
    def from_reference_arrays(cls, bwt, C_array, bwt_rev=None, sparse=None):
        """bwt / bwt_rev: dict(layout, sigma, n, blocks, super_blocks | nodes); sparse: dict(n, l0, l1, bits, fields[2])"""
        sa = _StringArrays(**bwt)
        desc = capi.IndexDesc()
        desc.bwt = sa.desc()
        keep = [sa]
        if bwt_rev is not None:
            sr = _StringArrays(**bwt_rev)
            rdesc = sr.desc()
            desc.bwt_rev = C.pointer(rdesc)
            keep += [sr, rdesc]
        Carr = _u64(C_array)
        desc.C = Carr.ctypes.data_as(capi.u64p)
        keep.append(Carr)
        if sparse is not None:
            sd = capi.SparseArrayDesc()
            l0, l1, bits = _u64(sparse["l0"]), np.ascontiguousarray(sparse["l1"], dtype=np.uint16), _u64(sparse["bits"])
            sd.n = sparse["n"]
            sd.l0 = l0.ctypes.data_as(capi.u64p); sd.n_l0 = l0.size
            sd.l1 = l1.ctypes.data_as(capi.u16p); sd.n_l1 = l1.size
            sd.bits = bits.ctypes.data_as(capi.u64p); sd.n_bit_words = bits.size
            keep += [l0, l1, bits]
            for f in range(2):
                fd = sparse["fields"][f]
                data = _u64(fd["data"])
                keep.append(data)
                sd.field[f].data = data.ctypes.data_as(capi.u64p); sd.field[f].n_words = data.size
                sd.field[f].bit_count = int(fd["bitCount"]); sd.field[f].bits = int(fd["bits"])
                sd.field[f].largest_value = int(fd["largestValue"]); sd.field[f].common_divisor = int(fd["commonDivisor"])
            desc.annotated_array = C.pointer(sd)
            keep.append(sd)
        h = C.c_void_p()
        capi.check(capi.lib().fmgpu_index_create(C.byref(desc), C.byref(h)))
        return cls(h, keep=None)   # the library copied everything; host arrays may go

    @classmethod
    def from_sequences(cls, sequences, sigma, layout="IB16", sampling_rate=16, bidirectional=None, keep_host=False):
        """GPU construction from Sequences (list of rank sequences, or (qbuf, qoff) already flattened / resident in HBM)"""
        if bidirectional is None:
            bidirectional = cls.bidirectional
        if isinstance(sequences, tuple):
            sbuf, soff = sequences
            nseq = (soff.nbytes // 8 if not hasattr(soff, "__len__") else len(soff)) - 1
        else:
            sbuf, soff = flatten(sequences)
            nseq = len(sequences)
        h, b = C.c_void_p(), C.c_void_p()
        capi.check(capi.lib().fmgpu_build_index(capi.ptr(sbuf), capi.ptr(soff), nseq, sigma, LAYOUTS[layout], sampling_rate,
                                                1 if bidirectional else 0, 1 if keep_host else 0, C.byref(h),
                                                C.byref(b) if keep_host else None))
        return cls(h, built=b if keep_host else None)

    # -------------------------------------------------------------- index file (replaces saveIndex / loadIndex, fmindex/diskStorage.h:12-27)
    def save(self, path, tables=True):
        """write the index to this library's own flat file (header + every device array with a checksum); tables=True keeps the optional tables the
        handle holds right now.  Not the reference's cereal format (include/fmgpu.h)"""
        capi.check(capi.lib().fmgpu_index_save(self._h, os.fsencode(path), 1 if tables else 0))
        return self

    @classmethod
    def load(cls, path):
        """an index written by save(); FMIndex.load returns a BiFMIndex object for a bidirectional file (and vice versa): the file says what it holds"""
        h = C.c_void_p()
        capi.check(capi.lib().fmgpu_index_load(os.fsencode(path), C.byref(h)))
        x = FMIndex(h)
        if x.bidirectional:
            x.__class__ = BiFMIndex
        return x

    def clone(self):
        """a copy of the handle on the calling thread's current device, made device to device (fmgpu_index_clone): every array incl. the optional tables"""
        h = C.c_void_p()
        capi.check(capi.lib().fmgpu_index_clone(self._h, C.byref(h)))
        x = FMIndex(h)
        if x.bidirectional:
            x.__class__ = BiFMIndex
        return x

    def built_array(self, part, dtype=np.uint8):
        """host copy of a construction by-product (keep_host=True): 0 = BWT bytes, 1 = BWT of the reversed text, 2 = C"""
        if not self._built:
            raise ValueError("index was not built with keep_host=True")
        p, nb = C.c_void_p(), C.c_uint64()
        capi.check(capi.lib().fmgpu_built_get(self._built, part, C.byref(p), C.byref(nb)))
        if nb.value == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_uint8 * nb.value).from_address(p.value)
        return np.frombuffer(buf, dtype=dtype)

    def close(self):
        if getattr(self, "_built", None):
            capi.lib().fmgpu_built_free(self._built)
            self._built = None
        if getattr(self, "_h", None):
            capi.lib().fmgpu_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        return self.n

    @property
    def row_bits(self):
        """32 or 64: the width of the device tables the index is held in (include/fmgpu.h, "row width")"""
        b = C.c_int32()
        capi.check(capi.lib().fmgpu_index_row_bits(self._h, C.byref(b)))
        return b.value

    @property
    def formats(self):
        """FMT_* bits (capi): what the bwt is held in at this moment — which kernel serves a search"""
        m = C.c_uint32()
        capi.check(capi.lib().fmgpu_index_formats(self._h, C.byref(m)))
        return m.value

    def _refresh_bytes(self):
        dbytes = C.c_uint64()
        capi.check(capi.lib().fmgpu_index_info(self._h, None, None, None, None, C.byref(dbytes)))
        self.device_bytes = dbytes.value
        return self

    def accelerate_lf(self, enable=True):
        """build / drop the explicit LF tables (one word per row and direction); without them the index is the bit-packed occurrence table alone"""
        capi.check(capi.lib().fmgpu_index_accelerate_lf(self._h, 1 if enable else 0))
        return self._refresh_bytes()

    # -------------------------------------------------------------- cursor steps (fmindex/FMIndexCursor.h:33-53, fmindex/BiFMIndexCursor.h:58-128)
    def extend(self, lb, lb_rev, length, symb=None, right=False):
        """extendLeft / extendRight of a batch of cursors.  symb = one symbol per cursor -> (lb, lb_rev, len) arrays of the same shape;
        symb = None -> extendLeft() / extendRight() over all symbols: arrays of shape (count, Sigma)"""
        lb, length = _u64(lb).reshape(-1), _u64(length).reshape(-1)
        rev = _u64(lb_rev).reshape(-1) if lb_rev is not None else None
        fan = 1 if symb is not None else self.Sigma
        sy = None if symb is None else np.ascontiguousarray(np.broadcast_to(np.asarray(symb, dtype=np.uint8), lb.shape))
        olb, olen = np.empty(lb.size * fan, dtype=np.uint64), np.empty(lb.size * fan, dtype=np.uint64)
        orev = np.empty(lb.size * fan, dtype=np.uint64) if rev is not None else None
        capi.check(capi.lib().fmgpu_cursor_extend(self._h, 1 if right else 0, lb.size, capi.ptr(lb), capi.ptr(rev), capi.ptr(length), capi.ptr(sy),
                                                  capi.ptr(olb), capi.ptr(orev), capi.ptr(olen), None))
        if fan > 1:
            olb, olen = olb.reshape(-1, fan), olen.reshape(-1, fan)
            orev = None if orev is None else orev.reshape(-1, fan)
        return olb, orev, olen

    def accelerate_search(self, prefix_len=11, walk=True):
        """BiFMIndex: prefix table for the exact first part of a search + walk tables (walk: True / 1 = LF, LF^2, LF^3 per row; 2 = LF^16 with
        the 16 symbols met; 3 = both); results are unchanged"""
        capi.check(capi.lib().fmgpu_index_accelerate_search(self._h, prefix_len, int(walk)))
        dbytes = C.c_uint64()
        capi.check(capi.lib().fmgpu_index_info(self._h, None, None, None, None, C.byref(dbytes)))
        self.device_bytes = dbytes.value
        return self

    def accelerate_locate(self, enable=True):
        """keep the (seqId, pos, steps) answer of every row (12 bytes per row): locate becomes one load per row; results are unchanged"""
        capi.check(capi.lib().fmgpu_index_accelerate_locate(self._h, 1 if enable else 0))
        dbytes = C.c_uint64()
        capi.check(capi.lib().fmgpu_index_info(self._h, None, None, None, None, C.byref(dbytes)))
        self.device_bytes = dbytes.value
        return self

    def accelerate(self, kstep=3, lut_len=0, walk=False):
        """add (kstep >= 2) or drop (0) the multi-symbol-step table used by exact search; lut_len > 0 adds the table of the
        intervals of all strings of that many symbols, walk=True the per-row LF^J + symbols table; results are unchanged"""
        capi.check(capi.lib().fmgpu_index_accelerate_exact(self._h, kstep, lut_len, int(walk)))      # walk: False / True (LF^J) / 2 (LF^J and LF^2J)
        n, sigma, layout, bidir, dbytes = C.c_uint64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        capi.check(capi.lib().fmgpu_index_info(self._h, C.byref(n), C.byref(sigma), C.byref(layout), C.byref(bidir), C.byref(dbytes)))
        self.device_bytes = dbytes.value
        return self

    # -------------------------------------------------------------- String_c batch (string/concepts.h:25-87)
    def _string_query(self, which, idx, symb, what):
        idx = _u64(idx)
        symb = np.ascontiguousarray(np.broadcast_to(np.asarray(symb, dtype=np.uint8), idx.shape))
        what = np.ascontiguousarray(np.broadcast_to(np.asarray(what, dtype=np.uint8), idx.shape))
        out = np.empty(idx.shape, dtype=np.uint64)
        capi.check(capi.lib().fmgpu_string_query(self._h, which, capi.ptr(idx), capi.ptr(symb), capi.ptr(what), idx.size,
                                                 capi.ptr(out), None))
        return out

    def rank(self, idx, symb, rev=False):
        return self._string_query(1 if rev else 0, idx, symb, 0)

    def prefix_rank(self, idx, symb, rev=False):
        return self._string_query(1 if rev else 0, idx, symb, 1)

    def symbol(self, idx, rev=False):
        return self._string_query(1 if rev else 0, idx, 0, 2)

    # -------------------------------------------------------------- locate (fmindex/FMIndex.h:113-124)
    def locate(self, rows, want_stats=False):
        rows = _u64(rows)
        seq, pos, steps = (np.empty(rows.shape, dtype=np.uint64) for _ in range(3))
        st = capi.Stats()
        capi.check(capi.lib().fmgpu_locate(self._h, capi.ptr(rows), rows.size, capi.ptr(seq), capi.ptr(pos), capi.ptr(steps),
                                           C.byref(st) if want_stats else None, None))
        return (seq, pos, steps, st) if want_stats else (seq, pos, steps)


    def locate_hits(self, hits, capacity=None, want_stats=False, out=None, stream=None):
        """every row of every hit record located in one call (fmgpu_locate_hits): the loop over LocateLinear{index, cursor} of fmc::Search for a
        whole batch.  hits = HIT_DTYPE array, DeviceBuffer or torch tensor (in HBM: used in place).  Returns a POSITION_DTYPE array, one record per
        row — hits in the given order, inside a hit rows lb .. lb + len - 1.  out = a device buffer / tensor to write the records into instead
        (then the record count is returned); stream = a hipStream_t (int) or a torch stream."""
        if isinstance(hits, np.ndarray):
            hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        hp, hbytes = _buffer(hits)
        count = hbytes // HIT_DTYPE.itemsize
        st, cnt = capi.Stats(), C.c_uint64()
        sp = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
        if out is not None:
            op, obytes = _buffer(out)
            capi.check(capi.lib().fmgpu_locate_hits(self._h, hp, count, op, obytes // POSITION_DTYPE.itemsize, C.byref(cnt),
                                                    C.byref(st) if want_stats else None, sp))
            return (cnt.value, st) if want_stats else cnt.value
        cap = capacity if capacity is not None else max(1024, 4 * count)
        for _ in range(2):                                            # once more with the size the call reported
            res = np.zeros(max(cap, 1), dtype=POSITION_DTYPE)
            rc = capi.lib().fmgpu_locate_hits(self._h, hp, count, capi.ptr(res), cap, C.byref(cnt), C.byref(st) if want_stats else None, sp)
            if rc != capi.FMGPU_ERR_CAPACITY:
                break
            cap = int(cnt.value)
        capi.check(rc)
        res = res[: cnt.value]
        return (res, st) if want_stats else res


    # -------------------------------------------------------------- text extraction (utils.h:672-703 as LF walks on the device)
    def accelerate_extract(self, enable=True):
        """build / drop the text map and the sampled rows in text order (fmgpu_index_accelerate_extract) that extract() and sequence_lengths() read.
        Not saved with the index and not cloned: build it again after load() / clone()"""
        capi.check(capi.lib().fmgpu_index_accelerate_extract(self._h, 1 if enable else 0))
        return self._refresh_bytes()

    def sequence_lengths(self):
        """(seq_ids, lengths): every seqId of the text map, ascending, and its length without its last delimiter"""
        cnt = C.c_uint64()
        rc = capi.lib().fmgpu_sequence_lengths(self._h, None, None, 0, C.byref(cnt))
        if rc != capi.FMGPU_ERR_CAPACITY:
            capi.check(rc)
        ids, lens = np.zeros(cnt.value, dtype=np.uint64), np.zeros(cnt.value, dtype=np.uint64)
        capi.check(capi.lib().fmgpu_sequence_lengths(self._h, capi.ptr(ids), capi.ptr(lens), cnt.value, C.byref(cnt)))
        return ids, lens

    def extract(self, seq_ids, pos=None, lens=None, out=None, want_stats=False):
        """the text symbols of ranges (fmgpu_extract): extract(seq_ids, pos, lens) with three arrays, or extract(ranges) with a TEXT_RANGE_DTYPE array,
        DeviceBuffer or torch tensor of records (in HBM: used in place).  Returns (symbols uint8, offsets uint64[count + 1]): range i is
        symbols[offsets[i]:offsets[i + 1]].  out = a device buffer / tensor to write the symbols into instead (then (symbol count, offsets) is returned)."""
        if pos is None:
            ranges = seq_ids
            if isinstance(ranges, np.ndarray):
                ranges = np.ascontiguousarray(ranges, dtype=TEXT_RANGE_DTYPE)
            rp, rbytes = _buffer(ranges)
            count = rbytes // TEXT_RANGE_DTYPE.itemsize
            if isinstance(ranges, np.ndarray):
                host = ranges
            elif isinstance(ranges, DeviceBuffer):
                host = ranges.to_array(TEXT_RANGE_DTYPE, count)
            else:
                host = np.frombuffer(ranges.cpu().numpy().tobytes(), dtype=TEXT_RANGE_DTYPE)[:count]
        else:
            host = np.zeros(np.size(seq_ids), dtype=TEXT_RANGE_DTYPE)
            host["seq_id"], host["pos"], host["len"] = _u64(seq_ids).reshape(-1), _u64(pos).reshape(-1), _u64(lens).reshape(-1)
            rp, count = capi.ptr(host), host.size
        offsets = np.zeros(count + 1, dtype=np.uint64)
        np.cumsum(host["len"], out=offsets[1:])
        total = int(offsets[-1])
        st, cnt = capi.Stats(), C.c_uint64()
        if out is not None:
            op, obytes = _buffer(out)
            capi.check(capi.lib().fmgpu_extract(self._h, rp, count, op, obytes, C.byref(cnt), C.byref(st) if want_stats else None, None))
            return (cnt.value, offsets, st) if want_stats else (cnt.value, offsets)
        res = np.zeros(max(total, 1), dtype=np.uint8)
        capi.check(capi.lib().fmgpu_extract(self._h, rp, count, capi.ptr(res), total, C.byref(cnt), C.byref(st) if want_stats else None, None))
        res = res[: cnt.value]
        return (res, offsets, st) if want_stats else (res, offsets)


class BiFMIndex(FMIndex):
    bidirectional = True


class PackedQueries:
    """a batch in the 4-bit packed query form (include/fmgpu.h): symbol i = nibble i & 1 of byte i >> 1 of `packed`, the even index in the low nibble; `qoff` as in the
    byte form (nq + 1 symbol offsets).  Both are numpy arrays or DeviceBuffers.  Accepted wherever (qbuf, qoff) is: the `_q4` entry points serve it."""

    def __init__(self, packed, qoff, nq=None):
        self.packed, self.qoff = packed, qoff
        self.nq = int(nq) if nq is not None else len(qoff) - 1

    def host(self):
        """(packed, qoff) as numpy arrays (copied back where they are DeviceBuffers)"""
        qoff = self.qoff if isinstance(self.qoff, np.ndarray) else self.qoff.to_array(np.uint64, self.nq + 1)
        packed = self.packed if isinstance(self.packed, np.ndarray) else self.packed.to_array(np.uint8, (int(qoff[-1]) + 1) // 2)
        return packed, qoff


def _host_batch(queries):
    if isinstance(queries, tuple):
        return np.asarray(queries[0], dtype=np.uint8), np.asarray(queries[1], dtype=np.uint64)
    return flatten(queries)


def pack_queries(queries, sigma, complement=None):
    """(qbuf, qoff) or a list of sequences -> PackedQueries of numpy arrays, byte for byte what fmgpu_queries_pack4 makes: a byte >= sigma becomes 15, the batch starts
    at symbol 0, a nibble left over in the last byte is 0.  complement (sigma entries): 2 nq reads, read 2q = read q, read 2q + 1 = read q reversed with
    complement[c] for c < sigma and 15 for the rest."""
    if not 2 <= sigma <= 15:
        raise ValueError("4-bit packed queries need 2 <= sigma <= 15")
    qbuf, qoff = _host_batch(queries)
    nq = len(qoff) - 1
    first, last = (int(qoff[0]), int(qoff[-1])) if nq >= 0 and len(qoff) else (0, 0)
    sym = qbuf[first:last].astype(np.uint8)
    start = (qoff[:-1] - qoff[0]).astype(np.int64)
    lens = np.diff(qoff.astype(np.int64))
    fwd = np.where(sym < sigma, sym, 15).astype(np.uint8)
    if complement is None:
        nib, out_qoff = fwd, (qoff - qoff[0]).astype(np.uint64)
    else:
        comp = np.full(256, 15, dtype=np.uint8)
        comp[:sigma] = np.asarray(complement, dtype=np.uint8)[:sigma]
        comp[comp >= sigma] = 15
        rid = np.repeat(np.arange(nq), lens)
        j = np.arange(sym.size, dtype=np.int64) - start[rid]
        nib = np.zeros(2 * sym.size, dtype=np.uint8)
        nib[2 * start[rid] + j] = fwd
        nib[2 * start[rid] + 2 * lens[rid] - 1 - j] = comp[sym]
        out_qoff = np.zeros(2 * nq + 1, dtype=np.uint64)
        out_qoff[0:-1:2] = 2 * start
        out_qoff[1::2] = 2 * start + lens
        out_qoff[-1] = 2 * sym.size
    if nib.size & 1:
        nib = np.concatenate([nib, np.zeros(1, dtype=np.uint8)])
    packed = (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)
    return PackedQueries(packed, out_qoff)


def unpack_queries(queries):
    """PackedQueries or (packed, qoff) -> (qbuf, qoff) of the byte form, starting at symbol 0: nibble 15 comes back as 255 (what fmgpu_queries_unpack4 writes)"""
    packed, qoff = queries.host() if isinstance(queries, PackedQueries) else (np.asarray(queries[0], dtype=np.uint8), np.asarray(queries[1], dtype=np.uint64))
    first, last = int(qoff[0]), int(qoff[-1])
    at = np.arange(first, last, dtype=np.int64)
    nib = (packed[at >> 1] >> (4 * (at & 1)).astype(np.uint8)) & 15
    qbuf = np.where(nib == 15, 255, nib).astype(np.uint8)
    return qbuf, (qoff - qoff[0]).astype(np.uint64)


def pack_queries_device(queries, sigma, complement=None, stream=None):
    """fmgpu_queries_pack4: the batch ((qbuf, qoff) of numpy arrays or DeviceBuffers, or a list of sequences) packed on the device -> PackedQueries of DeviceBuffers"""
    qbuf, qoff, nq = _queries(queries)
    ends = qoff if isinstance(qoff, np.ndarray) else qoff.to_array(np.uint64, nq + 1)
    total = (int(ends[-1]) - int(ends[0])) * (2 if complement is not None else 1)
    nreads = 2 * nq if complement is not None else nq
    packed, out_qoff = DeviceBuffer(max((total + 1) // 2, 8)), DeviceBuffer((nreads + 1) * 8)
    comp = None if complement is None else np.ascontiguousarray(np.asarray(complement, dtype=np.uint8))
    if nq == 0:
        capi.check(capi.lib().fmgpu_memcpy_h2d(capi.ptr(out_qoff), capi.ptr(np.zeros(1, dtype=np.uint64)), 8))
    capi.check(capi.lib().fmgpu_queries_pack4(capi.ptr(qbuf), capi.ptr(qoff), nq, sigma, capi.ptr(comp), capi.ptr(packed), capi.ptr(out_qoff), stream))
    return PackedQueries(packed, out_qoff, nreads)


DNA5_COMPLEMENT = (0, 4, 3, 2, 1)                           # ranks $ A C G T: what strands="dna5" names


def _complement(complement):
    """a complement table (or "dna5") as a contiguous uint8 array of 1 .. 256 entries"""
    comp = np.ascontiguousarray(np.asarray(DNA5_COMPLEMENT if isinstance(complement, str) and complement == "dna5" else complement, dtype=np.uint8)).reshape(-1)
    if not 1 <= comp.size <= 256:
        raise ValueError("a complement table has 1 .. 256 entries")
    return comp


def both_strands(queries, complement="dna5"):
    """(qbuf, qoff) or a list of sequences -> (qbuf, qoff) of the doubled batch, byte for byte what fmgpu_queries_strands makes: read 2q = read q, read 2q + 1 = read q
    reversed with complement[c] for a byte c < len(complement) and the byte itself otherwise; the batch starts at symbol 0."""
    comp = _complement(complement)
    qbuf, qoff = _host_batch(queries)
    nq = len(qoff) - 1
    if nq <= 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    first, last = int(qoff[0]), int(qoff[-1])
    sym = qbuf[first:last].astype(np.uint8)
    start = (qoff[:-1] - qoff[0]).astype(np.int64)
    lens = np.diff(qoff.astype(np.int64))
    table = np.arange(256, dtype=np.uint8)
    table[:comp.size] = comp
    rid = np.repeat(np.arange(nq), lens)
    j = np.arange(sym.size, dtype=np.int64) - start[rid]
    out = np.zeros(2 * sym.size, dtype=np.uint8)
    out[2 * start[rid] + j] = sym
    out[2 * start[rid] + 2 * lens[rid] - 1 - j] = table[sym]
    out_qoff = np.zeros(2 * nq + 1, dtype=np.uint64)
    out_qoff[0:-1:2] = 2 * start
    out_qoff[1::2] = 2 * start + lens
    out_qoff[-1] = 2 * sym.size
    return out, out_qoff


def both_strands_device(queries, complement="dna5", stream=None):
    """fmgpu_queries_strands: the batch ((qbuf, qoff) of numpy arrays or DeviceBuffers, or a list of sequences) doubled on the device -> (qbuf, qoff) of DeviceBuffers
    (2 nq reads; the symbol buffer is padded by 16 bytes)"""
    comp = _complement(complement)
    qbuf, qoff, nq = _queries(queries)
    ends = qoff if isinstance(qoff, np.ndarray) else qoff.to_array(np.uint64, nq + 1)
    total = 2 * (int(ends[-1]) - int(ends[0])) if nq > 0 else 0
    out, out_qoff = DeviceBuffer(total + 16), DeviceBuffer((2 * nq + 1) * 8)
    capi.check(capi.lib().fmgpu_queries_strands(capi.ptr(qbuf), capi.ptr(qoff), nq, capi.ptr(comp), comp.size, capi.ptr(out), capi.ptr(out_qoff), stream))
    return out, out_qoff


def _strands(strands, pair):
    """(capi.Strands or None, objects to keep alive) for map_reads / Feed.map / Feed.map_text"""
    if strands is None:
        if pair:
            raise ValueError("pair=True needs strands=")
        return None, None
    comp = _complement(strands)
    return capi.Strands(comp.ctypes.data_as(capi.u8p), comp.size, 1 if pair else 0), comp


def _q4(queries, byte_call, q4_call):
    """the entry point that takes `queries`: the `_q4` one for a PackedQueries"""
    return q4_call if isinstance(queries, PackedQueries) else byte_call


def _host_bytes(queries):
    """the batch as host (qbuf, qoff, nq) of the byte form, for the facades that split a batch by length on the host"""
    if isinstance(queries, PackedQueries):
        qbuf, qoff = unpack_queries(queries)
        return qbuf, qoff, queries.nq
    qbuf, qoff, nq = _queries(queries)
    if not isinstance(qoff, np.ndarray):
        qoff = qoff.to_array(np.uint64, nq + 1) if isinstance(qoff, DeviceBuffer) else np.asarray(qoff)
    if not isinstance(qbuf, np.ndarray):
        qbuf = qbuf.to_array(np.uint8, int(qoff[-1]))
    return qbuf, qoff, nq


def _queries(queries):
    if isinstance(queries, PackedQueries):
        return queries.packed, queries.qoff, queries.nq
    if isinstance(queries, tuple):
        qbuf, qoff = queries
        nq = (qoff.nbytes // 8 if not hasattr(qoff, "__len__") else len(qoff)) - 1
        return qbuf, qoff, nq
    qbuf, qoff = flatten(queries)
    return qbuf, qoff, len(queries)


class search_no_errors:
    """search/SearchNoErrors.h"""

    @staticmethod
    def search(index, queries, out=None, want_stats=False):
        """returns (lb, len) arrays — cursor_t{lb, len} per query (len == 0: the reference reports nothing).
        `queries` = list of sequences or (qbuf, qoff); numpy arrays or DeviceBuffers.  `out` = (lb, len) DeviceBuffers
        to keep results in HBM."""
        qbuf, qoff, nq = _queries(queries)
        if out is None:
            lb, ln = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint64)
        else:
            lb, ln = out
        st = capi.Stats()
        call = _q4(queries, capi.lib().fmgpu_search_exact, capi.lib().fmgpu_search_exact_q4)
        capi.check(call(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, capi.ptr(lb), capi.ptr(ln), C.byref(st) if want_stats else None, None))
        return (lb, ln, st) if want_stats else (lb, ln)


    @staticmethod
    def depth(index, queries):
        """per query: symbols consumed until the cursor holds at most one row (length + 1: still several rows at the end)"""
        qbuf, qoff, nq = _queries(queries)
        out = np.empty(nq, dtype=np.uint32)
        capi.check(capi.lib().fmgpu_search_exact_depth(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, capi.ptr(out), None))
        return out

    @staticmethod
    def search_packed(index, queries, out=None, want_stats=False):
        """the same cursors as one word per query, lb << 32 | len (the form a rank's intervals are gathered in)"""
        qbuf, qoff, nq = _queries(queries)
        word = np.empty(nq, dtype=np.uint64) if out is None else out
        st = capi.Stats()
        capi.check(capi.lib().fmgpu_search_exact_packed(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, capi.ptr(word),
                                                        C.byref(st) if want_stats else None, None))
        return (word, st) if want_stats else word


def _run_hits(call, capacity):
    while True:
        out = np.zeros(max(capacity, 1), dtype=HIT_DTYPE)
        cnt = C.c_uint64()
        st = capi.Stats()
        rc = call(out, capacity, cnt, st)
        if rc == capi.FMGPU_ERR_CAPACITY:
            capacity = int(cnt.value)
            continue
        capi.check(rc)
        hits = np.ascontiguousarray(out[: cnt.value])
        # the reference invokes the delegate in ascending qidx, inside a query in DFS order: (qidx, seq) restores it (sorted on the device)
        capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(hits), hits.size, None))
        return hits, st


def _run_best(call, nq, n_schemes, capacity, want_stratum, want_stats):
    """a best-stratum call into host records in callback order.  On FMGPU_ERR_CAPACITY the count is a lower bound of the total (the records up to the stratum
    that overflowed): growing to max(count, 2 x capacity) ends within n_schemes rounds."""
    capacity = capacity if capacity is not None else max(1024, 4 * nq)
    stratum = np.full(max(nq, 1), 255, dtype=np.uint8)
    stats = (capi.Stats * max(n_schemes, 1))()
    while True:
        out = np.zeros(max(capacity, 1), dtype=HIT_DTYPE)
        cnt = C.c_uint64()
        rc = call(out, capacity, cnt, stratum, stats)
        if rc == capi.FMGPU_ERR_CAPACITY:
            capacity = max(int(cnt.value), 2 * capacity)
            continue
        capi.check(rc)
        hits = np.ascontiguousarray(out[: cnt.value])
        capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(hits), hits.size, None))     # all records of a read come from one stratum: the reference's callback order
        res = (hits,) + ((stratum[:nq],) if want_stratum else ()) + (([stats[i] for i in range(n_schemes)],) if want_stats else ())
        return res if len(res) > 1 else hits


class search_backtracking:
    """search/Backtracking.h"""

    @staticmethod
    def search(index, queries, max_errors, capacity=None, want_stats=False):
        qbuf, qoff, nq = _queries(queries)
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        hits, st = _run_hits(lambda out, c, cnt, st: capi.lib().fmgpu_search_backtracking(
            index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, max_errors, capi.ptr(out), c, C.byref(cnt), C.byref(st), None), cap)
        return (hits, st) if want_stats else hits


class search_ng26:
    """search/SearchNg26.h: Hamming distance (Edit = false, default here) or edit distance (edit=True, the reference's default)"""

    @staticmethod
    def search(index, queries, scheme, partition=None, n=UINT64_MAX, capacity=None, want_stats=False, edit=False):
        """scheme = (pi, l, u) arrays [searches][parts]; partition = explicit part lengths or None (uniform per query)"""
        qbuf, qoff, nq = _queries(queries)
        pi, l, u = (_u64(x) for x in scheme)
        sc = capi.Scheme()
        sc.n_searches, sc.n_parts = pi.shape
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        part = _u64(partition) if partition is not None else None
        sc.partition = part.ctypes.data_as(capi.u64p) if part is not None else None
        sc.edit = 1 if edit else 0
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        call = _q4(queries, capi.lib().fmgpu_search_scheme, capi.lib().fmgpu_search_scheme_q4)
        hits, st = _run_hits(lambda out, c, cnt, st: call(
            index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(sc), n, capi.ptr(out), c, C.byref(cnt), C.byref(st), None), cap)
        return (hits, st) if want_stats else hits


class ScoringMatrix:
    """search_hamming_sm::ScoringMatrix<QuerySigma, RefSigma> (search/SearchHammingSM.h:16-45) as the two mask arrays of fmgpu_scoring_matrix: bit r of free_mask[c] = text
    rank r matches query rank c at no cost, bit r of cost_mask[c] = the pairing costs one error; neither = not pairable.  Default-constructed like the reference's: identity
    free, every other pair of ranks 1.. at cost 1 (rank 0, the delimiter, pairs with nothing).  The search walks the members of a mask in ascending rank."""

    def __init__(self, query_sigma, ref_sigma=None):
        ref_sigma = query_sigma if ref_sigma is None else ref_sigma
        if not (1 <= query_sigma <= 256 and 1 <= ref_sigma <= 32):
            raise ValueError("ScoringMatrix: query_sigma in 1..256, ref_sigma in 1..32")
        self.query_sigma, self.ref_sigma = int(query_sigma), int(ref_sigma)
        self.free_mask = np.zeros(self.query_sigma, dtype=np.uint32)
        self.cost_mask = np.zeros(self.query_sigma, dtype=np.uint32)
        for y in range(1, self.ref_sigma):
            for x in range(1, self.query_sigma):
                self.set_cost(x, y, 0 if x == y else 1)

    def set_cost(self, query_rank, ref_rank, cost):
        """setCost: cost 0 = a free match, 1 = a mismatch that costs one error"""
        if cost not in (0, 1):
            raise ValueError("ScoringMatrix.set_cost: cost is 0 or 1")
        self.set_unpairable(query_rank, ref_rank)
        (self.cost_mask if cost else self.free_mask)[query_rank] |= np.uint32(1 << ref_rank)
        return self

    def set_unpairable(self, query_rank, ref_rank=None):
        """query_rank pairs with ref_rank (or, None, with any rank) neither for free nor at a cost"""
        if not 0 <= query_rank < self.query_sigma or (ref_rank is not None and not 0 <= ref_rank < self.ref_sigma):
            raise ValueError("ScoringMatrix: rank out of range")
        keep = np.uint32(0) if ref_rank is None else np.uint32(~(1 << ref_rank) & 0xffffffff)
        self.free_mask[query_rank] &= keep
        self.cost_mask[query_rank] &= keep
        return self

    # ranks 5..15 of iupac_dna() and the bases (ranks 1..4 = A C G T) each stands for
    IUPAC = {"R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}

    @classmethod
    def iupac_dna(cls):
        """query ranks 1..4 = A C G T, 5..15 = R Y S W K M B D H V N on a sigma = 5 index: every code is free for its bases and costs one error for the others"""
        sm = cls(16, 5)
        for k, bases in enumerate(cls.IUPAC.values()):
            for r, base in enumerate("ACGT", start=1):
                sm.set_cost(5 + k, r, 0 if base in bases else 1)
        return sm

    def _struct(self):
        m = capi.ScoringMatrix()
        m.query_sigma, m.reserved = self.query_sigma, 0
        m.free_mask = self.free_mask.ctypes.data_as(C.POINTER(C.c_uint32))
        m.cost_mask = self.cost_mask.ctypes.data_as(C.POINTER(C.c_uint32))
        m._masks = (self.free_mask, self.cost_mask)                  # (the struct keeps the arrays it points into alive)
        return m


class search_hamming_sm:
    """search/SearchHammingSM.h: the search-scheme Hamming walk with a scoring matrix (fmgpu_search_hamming_sm)"""

    @staticmethod
    def search(index, queries, scheme, matrix, partition=None, n=UINT64_MAX, capacity=None, want_stats=False):
        """scheme = (pi, l, u) arrays [searches][parts]; matrix = a ScoringMatrix; `queries` in the byte form (a list of sequences or (qbuf, qoff)): query symbols may be
        any byte below matrix.query_sigma.  Returns the hit records in the reference's callback order."""
        if isinstance(queries, PackedQueries):
            raise TypeError("search_hamming_sm takes the byte form of a batch (4-bit packed batches are not served)")
        qbuf, qoff, nq = _queries(queries)
        pi, l, u = (_u64(x) for x in scheme)
        sc = capi.Scheme()
        sc.n_searches, sc.n_parts = pi.shape
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        part = _u64(partition) if partition is not None else None
        sc.partition = part.ctypes.data_as(capi.u64p) if part is not None else None
        sc.edit = 0
        sm = matrix._struct()
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        hits, st = _run_hits(lambda out, c, cnt, st: capi.lib().fmgpu_search_hamming_sm(
            index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(sc), C.byref(sm), n, capi.ptr(out), c, C.byref(cnt), C.byref(st), None), cap)
        return (hits, st) if want_stats else hits


class Feed:
    """a feed (fmgpu_feed_*, include/fmgpu.h): HOST batches searched chunk by chunk on one index, the upload of the next chunk and the download of the previous one
    running beside the search of the current one.  0 / None in an argument = the library's default.  `queries` = a flat (qbuf, qoff) of numpy arrays (pinned memory,
    e.g. PinnedBuffer.array(...), is copied from where it lies), a list of sequences (searched through the `_v` calls, without flattening) or a PackedQueries of
    numpy arrays.  One feed serves one call at a time; a context manager."""

    def __init__(self, index, chunk_reads=0, chunk_symbols=0, slots=0, host_threads=0, pack4=False):
        cfg = capi.FeedConfig(int(chunk_reads or 0), int(chunk_symbols or 0), int(slots or 0), int(host_threads or 0), 1 if pack4 else 0, 0)
        h = C.c_void_p()
        capi.check(capi.lib().fmgpu_feed_create(index._h, C.byref(cfg), C.byref(h)))
        self._f, self._index = h, index                      # (the handle outlives the feed)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._f:
            capi.check(capi.lib().fmgpu_feed_destroy(self._f))
            self._f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """dict: pinned_bytes, device_bytes the feed holds; chunks, staged_bytes, uploaded_bytes of the last call"""
        v = [C.c_uint64() for _ in range(5)]
        capi.check(capi.lib().fmgpu_feed_info(self._f, *(C.byref(x) for x in v)))
        return dict(zip(("pinned_bytes", "device_bytes", "chunks", "staged_bytes", "uploaded_bytes"), (int(x.value) for x in v)))

    @staticmethod
    def _batch(queries):
        """(suffix of the entry point, first argument, second argument, nq, objects to keep alive)"""
        if isinstance(queries, PackedQueries):
            return "_q4", capi.ptr(queries.packed), capi.ptr(queries.qoff), queries.nq, None
        if isinstance(queries, tuple):
            qbuf, qoff, nq = _queries(queries)
            return "", capi.ptr(qbuf), capi.ptr(qoff), nq, None
        reads = [np.ascontiguousarray(q, dtype=np.uint8) for q in queries]
        lens = np.fromiter((r.size for r in reads), dtype=np.uint64, count=len(reads))
        ptrs = np.fromiter((r.ctypes.data for r in reads), dtype=np.uint64, count=len(reads))
        return "_v", capi.ptr(ptrs), capi.ptr(lens), len(reads), (reads, lens, ptrs)

    def search_exact(self, queries, out=None, want_stats=False):
        """(lb, len) of every read, what search_no_errors.search returns; `out` = (lb, len) uint64 arrays to write into (pinned ones are written in place)"""
        suffix, a, b, nq, keep = self._batch(queries)
        lb, ln = (np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint64)) if out is None else out
        st = capi.Stats()
        call = getattr(capi.lib(), "fmgpu_feed_search_exact" + suffix)
        capi.check(call(self._f, a, b, nq, capi.ptr(lb), capi.ptr(ln), C.byref(st) if want_stats else None))
        del keep
        return (lb, ln, st) if want_stats else (lb, ln)

    def search_scheme(self, queries, scheme, partition=None, n=UINT64_MAX, capacity=None, want_stats=False, edit=False):
        """hit records in callback order, what search_ng26.search returns (a PackedQueries is not taken: the scheme kernels read bytes)"""
        suffix, a, b, nq, keep = self._batch(queries)
        if suffix == "_q4":
            raise ValueError("a feed searches schemes over byte batches")
        pi, l, u = (_u64(x) for x in scheme)
        sc = capi.Scheme()
        sc.n_searches, sc.n_parts = pi.shape
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        part = _u64(partition) if partition is not None else None
        sc.partition = part.ctypes.data_as(capi.u64p) if part is not None else None
        sc.edit = 1 if edit else 0
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        call = getattr(capi.lib(), "fmgpu_feed_search_scheme" + suffix)
        hits, st = _run_hits(lambda out, c, cnt, st: call(self._f, a, b, nq, C.byref(sc), n, capi.ptr(out), c, C.byref(cnt), C.byref(st) if want_stats else None), cap)
        del keep
        return (hits, st) if want_stats else hits

    def map(self, queries, errors=None, schemes=None, ng21=False, edit=True, n=UINT64_MAX, locate=True, want_hits=False, want_stratum=False, want_stats=False,
            first_records=0, out=None, strands=None, pair=False):
        """fmgpu_feed_map: what map_reads returns, chunk by chunk (a PackedQueries is not taken).  `out` = a POSITION_DTYPE array to write into (a pinned one is
        written in place; it must hold every position).  strands= / pair= as map_reads (fmgpu_feed_map_strands; a flat batch)."""
        suffix, a, b, nq, keep = self._batch(queries)
        if suffix == "_q4":
            raise ValueError("a feed maps byte batches")
        what, alive = _map_query(errors, schemes, ng21, edit, n, locate, first_records)
        st, comp = _strands(strands, pair)
        if st is not None:
            if suffix:                                       # (no `_v` form: a list of reads is flattened)
                keep = flatten(queries)
                a, b = capi.ptr(keep[0]), capi.ptr(keep[1])
            res = _run_map(lambda *args: capi.lib().fmgpu_feed_map_strands(self._f, a, b, nq, C.byref(what), C.byref(st), *args), 2 * nq, what, want_hits, want_stratum,
                           want_stats, out, False)
            del keep, alive, comp
            return res
        call = getattr(capi.lib(), "fmgpu_feed_map" + suffix)
        res = _run_map(lambda *args: call(self._f, a, b, nq, C.byref(what), *args), nq, what, want_hits, want_stratum, want_stats, out, False)
        del keep, alive
        return res

    def map_text(self, data, format, table, final=True, chunk_bytes=0, want_hits=False, want_stratum=False, want_names=False, want_quals=False, want_lens=False,
                 want_stats=False, errors=None, schemes=None, ng21=False, edit=True, n=UINT64_MAX, locate=True, first_records=0, out=None, capacities=None,
                 strands=None, pair=False):
        """fmgpu_feed_map_text: the bytes of a read file -> MappedText, what map_reads(parse_queries(data)) returns plus the spans of the whole-text parse.  The text is
        the only thing uploaded: it travels in windows of chunk_bytes (0 = 64 MiB), each parsed and mapped on the device.  `data`: bytes, a numpy array (an np.memmap
        included) or a pinned buffer (PinnedBuffer.array(...), copied from where it lies); format / table as parse_queries; the mapping arguments as Feed.map.  The
        capacities (positions, hit records, reads) start as guesses, or as `capacities`; a capacity error reports the exact totals and the call runs once more with
        them.  A text error raises TextError.  strands= / pair= as map_reads (fmgpu_feed_map_text_strands): qidx and the stratum array (2 entries per read) count
        in the doubled batch; names, quals and lens stay per read of the file."""
        fmt = _TEXT_FORMATS[format] if isinstance(format, str) else int(format)
        table = np.ascontiguousarray(np.asarray(table, dtype=np.uint8))
        if table.size != 256:
            raise ValueError("a symbol table has 256 entries")
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = np.frombuffer(data, dtype=np.uint8)
        if isinstance(data, np.ndarray):
            if not data.flags.c_contiguous:
                data = np.ascontiguousarray(data)
            text = data.view(np.uint8).reshape(-1)
            p, nbytes = (text.ctypes.data if text.size else None), text.size
        else:
            p, nbytes = _buffer(data)
            text = data
        what, alive = _map_query(errors, schemes, ng21, edit, n, locate, first_records)
        nst = max(1, what.n_schemes)
        sstats, lstats = (capi.Stats * nst)(), capi.Stats()
        L, res = capi.lib(), capi.ParseResult()
        want_reads = want_stratum or want_names or want_quals or want_lens
        st, comp = _strands(strands, pair)
        mult = 2 if st is not None else 1
        call = L.fmgpu_feed_map_text if st is None else (lambda *a: L.fmgpu_feed_map_text_strands(*a[:8], C.byref(st), *a[8:]))
        rcap = max(1024, nbytes // 64) if want_reads else 0
        cap = len(out) if out is not None else (max(1024, 4 * rcap, nbytes // 16) if locate else 0)
        hcap = max(1024, 4 * rcap, nbytes // 16) if want_hits else 0
        if capacities is not None:
            cap, hcap, rcap = (len(out) if out is not None else (int(capacities[0]) if locate else 0)), (int(capacities[1]) if want_hits else 0), (int(capacities[2]) if want_reads else 0)
        cnt, hcnt = C.c_uint64(), C.c_uint64()
        for _ in range(2):
            pos = out if out is not None else np.zeros(max(cap, 1), dtype=POSITION_DTYPE)
            hits = np.zeros(max(hcap, 1), dtype=HIT_DTYPE) if want_hits else None
            stratum = np.full(max(mult * rcap, 1), 255, dtype=np.uint8) if want_stratum else None
            names = np.zeros(max(rcap, 1), dtype=capi.TEXT_SPAN_DTYPE) if want_names else None
            quals = np.zeros(max(rcap, 1), dtype=capi.TEXT_SPAN_DTYPE) if want_quals else None
            lens = np.zeros(max(rcap, 1), dtype=np.uint64) if want_lens else None
            rc = call(self._f, p, nbytes, fmt, 1 if final else 0, capi.ptr(table), int(chunk_bytes or 0), C.byref(what), capi.ptr(pos), cap, C.byref(cnt),
                                       capi.ptr(hits), hcap, C.byref(hcnt), capi.ptr(stratum), capi.ptr(names), capi.ptr(quals), capi.ptr(lens), rcap, C.byref(res),
                                       sstats if want_stats else None, C.byref(lstats) if want_stats else None)
            if rc != capi.FMGPU_ERR_CAPACITY:
                break
            if out is not None and int(cnt.value) > cap:
                break
            cap = cap if out is not None else max(cap, int(cnt.value))
            hcap = max(hcap, int(hcnt.value)) if want_hits else 0
            rcap = max(rcap, int(res.reads)) if want_reads else 0
        if rc == capi.FMGPU_ERR_INVALID and L.fmgpu_last_error().startswith(b"text error"):
            raise TextError(rc, L.fmgpu_last_error().decode("utf-8", "replace"), int(res.error_line), int(res.error_offset))
        capi.check(rc)
        del alive, text
        reads = int(res.reads)
        m = MappedText()
        m.positions = pos[: cnt.value]
        m.hits = np.ascontiguousarray(hits[: hcnt.value]) if want_hits else None
        m.stratum = None if stratum is None else stratum[:mult * reads]
        m.names, m.quals, m.lens = (None if a is None else a[:reads] for a in (names, quals, lens))
        m.reads, m.symbols, m.consumed, m.foreign = reads, int(res.symbols), int(res.consumed), int(res.foreign)
        m.stats = ([sstats[i] for i in range(nst)], lstats) if want_stats else None
        return m

    def map_file(self, path, format, table, **kw):
        """map_text over the file's bytes as they lie in the page cache (np.memmap): the file is never read into a Python object"""
        if os.path.getsize(path) == 0:
            return self.map_text(b"", format, table, **kw)
        return self.map_text(np.memmap(path, dtype=np.uint8, mode="r"), format, table, **kw)


class MappedText:
    """what Feed.map_text returns: positions (POSITION_DTYPE, qidx = the read's number in the text), hits (HIT_DTYPE) / stratum / names / quals / lens where asked for
    (else None; names and quals are TEXT_SPAN_DTYPE spans into the text), reads / symbols / consumed / foreign of the whole-text parse, stats = (search stats per
    stratum, locate stats) or None"""


class Replicas:
    """one index file on several GPUs of this process (fmgpu_replicas_*; SURVEY 8b `fmgpu_set_devices`): a batch is cut into contiguous ranges, one per
    replica, searched concurrently; results land in host arrays in batch order.  devices=None: every visible device."""

    def __init__(self, handle):
        self._r = handle
        n = C.c_int32()
        capi.check(capi.lib().fmgpu_replicas_info(self._r, C.byref(n), None, 0, None))
        dev = (C.c_int32 * n.value)()
        capi.check(capi.lib().fmgpu_replicas_info(self._r, None, dev, n.value, None))
        self.devices = list(dev)
        pc = C.c_int32()
        capi.check(capi.lib().fmgpu_replicas_peer_copies(self._r, C.byref(pc)))
        self.peer_copies = pc.value                 # replicas made by a device-to-device copy of the first one (the file was read once)

    @classmethod
    def load(cls, path, devices=None):
        h = C.c_void_p()
        d = (C.c_int32 * len(devices))(*devices) if devices else None
        capi.check(capi.lib().fmgpu_replicas_load(os.fsencode(path), d, len(devices) if devices else 0, C.byref(h)))
        return cls(h)

    def search_exact(self, queries, want_stats=False):
        qbuf, qoff, nq = _queries(queries)
        lb, ln = np.empty(nq, dtype=np.uint64), np.empty(nq, dtype=np.uint64)
        st = capi.Stats()
        capi.check(capi.lib().fmgpu_replicas_search_exact(self._r, capi.ptr(qbuf), capi.ptr(qoff), nq, capi.ptr(lb), capi.ptr(ln), C.byref(st)))
        return (lb, ln, st) if want_stats else (lb, ln)

    def search_scheme(self, queries, scheme, partition=None, n=UINT64_MAX, capacity=None, want_stats=False, edit=False):
        qbuf, qoff, nq = _queries(queries)
        pi, l, u = (_u64(x) for x in scheme)
        sc = capi.Scheme()
        sc.n_searches, sc.n_parts = pi.shape
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        part = _u64(partition) if partition is not None else None
        sc.partition = part.ctypes.data_as(capi.u64p) if part is not None else None
        sc.edit = 1 if edit else 0
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        hits, st = _run_hits(lambda out, c, cnt, st: capi.lib().fmgpu_replicas_search_scheme(
            self._r, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(sc), n, capi.ptr(out), c, C.byref(cnt), C.byref(st)), cap)
        return (hits, st) if want_stats else hits

    def search_ng21(self, queries, scheme, n=UINT64_MAX, capacity=None, want_stats=False):
        """search_ng21::search / search_n over an expanded scheme (pi, l, u arrays [searches][query length])"""
        qbuf, qoff, nq = _queries(queries)
        pi, l, u = (_u64(x) for x in scheme)
        sc = capi.ExpandedScheme()
        sc.n_searches, sc.length = (pi.shape if pi.ndim == 2 else (0, 0))
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        hits, st = _run_hits(lambda out, c, cnt, st: capi.lib().fmgpu_replicas_search_ng21(
            self._r, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(sc), n, capi.ptr(out), c, C.byref(cnt), C.byref(st)), cap)
        return (hits, st) if want_stats else hits

    def locate(self, rows):
        """(seq, pos, steps) of every row (FMIndex::locate), the rows sharded over the replicas"""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        out = [np.empty(len(rows), dtype=np.uint64) for _ in range(3)]
        capi.check(capi.lib().fmgpu_replicas_locate(self._r, capi.ptr(rows), len(rows), capi.ptr(out[0]), capi.ptr(out[1]), capi.ptr(out[2]), None))
        return tuple(out)

    def close(self):
        if self._r:
            capi.check(capi.lib().fmgpu_replicas_destroy(self._r))
            self._r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class search_ng21:
    """search/SearchNg21.h: edit-distance search over an EXPANDED scheme — search_scheme.expand(scheme, query length), one {pi, l, u} entry
    per query symbol, so all queries of a call have that length (the reference indexes query[pi[k]] without a check)"""

    @staticmethod
    def search(index, queries, scheme, capacity=None, want_stats=False, n=UINT64_MAX):
        """search_ng21::search (:205-217); scheme = (pi, l, u) arrays [searches][query length]"""
        qbuf, qoff, nq = _queries(queries)
        pi, l, u = (_u64(x) for x in scheme)
        sc = capi.ExpandedScheme()
        sc.n_searches, sc.length = (pi.shape if pi.ndim == 2 else (0, 0))
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        cap = capacity if capacity is not None else max(1024, 4 * nq)
        call = _q4(queries, capi.lib().fmgpu_search_ng21, capi.lib().fmgpu_search_ng21_q4)
        hits, st = _run_hits(lambda out, c, cnt, st: call(
            index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(sc), n, capi.ptr(out), c, C.byref(cnt), C.byref(st), None), cap)
        return (hits, st) if want_stats else hits

    @staticmethod
    def search_n(index, queries, scheme, n, capacity=None, want_stats=False):
        """search_ng21::search_n (:220-240): at most n rows per query, the last cursor clipped"""
        return search_ng21.search(index, queries, scheme, capacity, want_stats, n)

    @staticmethod
    def search_best(index, queries, schemes, n=UINT64_MAX, capacity=None, want_stratum=False, want_stats=False, pairs=False):
        """search_ng21::search_best (:242-264): per query the first scheme of the list that reports any row — one fmgpu_search_best_ng21 call: the ladder is cut on
        the device, so `queries` may be DeviceBuffers or a PackedQueries as they are.  want_stratum: also the uint8 array out_stratum (255 = no scheme found the
        read); want_stats: also the list of the strata's Stats.  Returned as (hits[, stratum][, stats]).  pairs=True: reads 2j and 2j + 1 are the strands of one read
        (fmgpu_search_best_ng21_pairs; byte batches)."""
        qbuf, qoff, nq = _queries(queries)
        keep = [tuple(_u64(x) for x in sch) for sch in schemes]
        arr = (capi.ExpandedScheme * max(len(keep), 1))()
        for sc, (pi, l, u) in zip(arr, keep):
            sc.n_searches, sc.length = (pi.shape if pi.ndim == 2 else (0, 0))
            sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        if pairs and isinstance(queries, PackedQueries):
            raise ValueError("the pair ladder takes byte batches")
        call = capi.lib().fmgpu_search_best_ng21_pairs if pairs else _q4(queries, capi.lib().fmgpu_search_best_ng21, capi.lib().fmgpu_search_best_ng21_q4)
        return _run_best(lambda out, c, cnt, stratum, st: call(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, arr, len(keep), n, capi.ptr(out), c, C.byref(cnt),
                                                               capi.ptr(stratum), st, None), nq, len(keep), capacity, want_stratum, want_stats)

    @staticmethod
    def search_best_n(index, queries, schemes, n, **kw):
        """search_ng21::search_best_n (:267-293)"""
        return search_ng21.search_best(index, queries, schemes, n, **kw)


def _auto_scheme_search(index, queries, errors, n, edit, compat_auto_scheme):
    """search_ng26::search<Edit>(index, queries, maxErrors, delegate, n) (search/SearchNg26.h:436-444): per query length the cached scheme
    h2(maxErrors + (length == 2 ? 1 : 2), 0, maxErrors) (CachedSearchScheme.h:16-36) with a uniform partition"""
    qbuf, qoff, nq = _host_bytes(queries)                     # the facade splits the batch by length on the host
    lens = np.diff(qoff.astype(np.int64))

    def scheme_for(short):
        sc = search_scheme.h2(errors + (1 if short else 2), 0, errors)
        return search_scheme.limitToHamming(sc) if (compat_auto_scheme and not edit) else sc

    parts = []
    for short in (False, True):
        sel = np.nonzero((lens == 2) == short)[0]
        if sel.size == 0:
            continue
        sub = [qbuf[int(qoff[i]): int(qoff[i + 1])] for i in sel] if sel.size != nq else None
        batch = (queries if isinstance(queries, PackedQueries) else (qbuf, qoff)) if sub is None else flatten(sub)     # (a packed batch of one length class goes down as it is)
        hits = search_ng26.search(index, batch, scheme_for(short), None, n, edit=edit)
        if sub is not None:
            hits = hits.copy()
            hits["qidx"] = sel.astype(np.uint64)[hits["qidx"].astype(np.int64)]
        parts.append(hits)
    if not parts:
        return np.zeros(0, dtype=HIT_DTYPE)
    hits = np.concatenate(parts)
    return hits[np.lexsort((hits["seq"], hits["qidx"]))]


def search(index, queries, errors, n=UINT64_MAX, compat_auto_scheme=False, edit=False):
    """fmc::search<EditDistance> (search/search.h:26-35; edit=False: Hamming, edit=True: edit distance, the reference's default):
    errors == 0 -> search_no_errors, else search_ng26 with h2(errors+2, 0, errors) and a uniform partition.  For Hamming distance the
    reference's convenience overload additionally applies limitToHamming to the un-expanded scheme (search/CachedSearchScheme.h:26-30),
    which loses hits; compat_auto_scheme=True reproduces exactly that."""
    if errors == 0:
        lb, ln = search_no_errors.search(index, queries)
        keep = np.nonzero(ln)[0]
        hits = np.zeros(keep.size, dtype=HIT_DTYPE)
        hits["qidx"], hits["lb"], hits["len"] = keep, lb[keep], ln[keep]
        return hits
    return _auto_scheme_search(index, queries, errors, n, edit, compat_auto_scheme)


def search_n(index, queries, errors, n, edit=True, compat_auto_scheme=False):
    """fmc::search_n<EditDistance> (search/search.h:38-46): at most n rows per query, always through search_ng26 (also for errors == 0)"""
    return _auto_scheme_search(index, queries, errors, n, edit, compat_auto_scheme)


def search_best(index, queries, max_errors, n=UINT64_MAX, edit=True, schemes=None, capacity=None, want_stratum=False, want_stats=False, pairs=False):
    """search_ng26::search_best (search/SearchNg26.h:447-487).
    schemes=None: the convenience overload (:476-487) — the whole batch is searched with 0, 1, ... max_errors - 1 errors (the loop ends
    BEFORE max_errors, as in the reference) and stops at the first error count for which ANY query reports a hit: a host loop, nothing is cut per read.
    schemes=[(scheme, partition), ...]: the explicit overload (:447-473) — per query the first scheme that reports anything wins: one fmgpu_search_best call, the
    ladder is cut on the device, so `queries` may be DeviceBuffers or a PackedQueries as they are.  want_stratum: also the uint8 array out_stratum (255 = no scheme
    found the read); want_stats: also the list of the strata's Stats.  Returned as (hits[, stratum][, stats]).  pairs=True (explicit schemes, byte batches): reads 2j and
    2j + 1 are the two strands of one read — fmgpu_search_best_pairs: once either is found, neither goes on, and both stratum entries name that stratum."""
    if pairs and (schemes is None or isinstance(queries, PackedQueries)):
        raise ValueError("the pair ladder takes explicit schemes and byte batches")
    if schemes is None:
        for k in range(int(max_errors)):
            hits = _auto_scheme_search(index, queries, k, n, edit, False)
            if len(hits):
                return hits
        return np.zeros(0, dtype=HIT_DTYPE)
    qbuf, qoff, nq = _queries(queries)
    keep = [tuple(_u64(x) for x in sch) + ((_u64(part),) if part is not None else (None,)) for sch, part in schemes]
    arr = (capi.Scheme * max(len(keep), 1))()
    for sc, (pi, l, u, part) in zip(arr, keep):
        sc.n_searches, sc.n_parts = pi.shape
        sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        sc.partition = part.ctypes.data_as(capi.u64p) if part is not None else None
        sc.edit = 1 if edit else 0
    call = capi.lib().fmgpu_search_best_pairs if pairs else _q4(queries, capi.lib().fmgpu_search_best, capi.lib().fmgpu_search_best_q4)
    return _run_best(lambda out, c, cnt, stratum, st: call(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, arr, len(keep), n, capi.ptr(out), c, C.byref(cnt),
                                                           capi.ptr(stratum), st, None), nq, len(keep), capacity, want_stratum, want_stats)


def search_smems(index, queries, min_len=1, max_rows=0, capacity=None, want_lengths=False, want_stats=False):
    """fmgpu_search_smems: the super-maximal exact matches of every read — seeds for the reads a search scheme left behind.  `queries` as for the other searches
    (list of reads, (qbuf, qoff) of numpy arrays or DeviceBuffers, PackedQueries).  A seed is kept if it has at least min_len symbols and (max_rows == 0 or) at most
    max_rows rows.  Returns (hits, spans[, lengths][, stats]): hits = HIT_DTYPE records in ascending (qidx, qbeg) with seq = the seed's index within its read, ready for
    index.locate_hits; spans = SEED_SPAN_DTYPE records (qbeg, qlen), one per hit; lengths = the match length of every batch symbol (uint32, symbol qoff[0] first)."""
    qbuf, qoff, nq = _queries(queries)
    lengths = None
    if want_lengths:
        ends = qoff if isinstance(qoff, np.ndarray) else qoff.to_array(np.uint64, nq + 1)
        lengths = np.zeros(int(ends[-1]) - int(ends[0]) if nq else 0, dtype=np.uint32)
    call = _q4(queries, capi.lib().fmgpu_search_smems, capi.lib().fmgpu_search_smems_q4)
    cap = capacity if capacity is not None else max(1024, 4 * nq)
    st, cnt = capi.Stats(), C.c_uint64()
    for _ in range(2):                                            # once more with the size the call reported
        hits, spans = np.zeros(max(cap, 1), dtype=HIT_DTYPE), np.zeros(max(cap, 1), dtype=SEED_SPAN_DTYPE)
        rc = call(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, min_len, max_rows, capi.ptr(hits), capi.ptr(spans), cap, C.byref(cnt),
                  capi.ptr(lengths) if lengths is not None and lengths.size else None, C.byref(st) if want_stats else None, None)
        if rc != capi.FMGPU_ERR_CAPACITY:
            break
        cap = int(cnt.value)
    capi.check(rc)
    res = (np.ascontiguousarray(hits[: cnt.value]), np.ascontiguousarray(spans[: cnt.value]))
    return res + ((lengths,) if want_lengths else ()) + ((st,) if want_stats else ())


class LocateLinear:
    """locate.h:14-57: iterate a cursor's rows -> (seqId, pos, offset); batched over many cursors here"""

    def __init__(self, index, lb, length):
        self.index = index
        lb, length = _u64(lb).reshape(-1), _u64(length).reshape(-1)
        self.owner = np.repeat(np.arange(lb.size, dtype=np.uint64), length.astype(np.int64))
        starts = np.repeat(lb, length.astype(np.int64))
        first = np.repeat(np.cumsum(length) - length, length.astype(np.int64))
        self.rows = starts + (np.arange(self.owner.size, dtype=np.uint64) - first)

    def __call__(self):
        seq, pos, steps = self.index.locate(self.rows)
        return self.owner, seq, pos, steps


def _device_hits(index, qbuf, qoff, nq, scheme, n, edit, q4=False):
    """search_ng26 over one batch with the hit records left in HBM and put into callback order there: (DeviceBuffer, count)"""
    pi, l, u = (_u64(x) for x in scheme)
    sc = capi.Scheme()
    sc.n_searches, sc.n_parts = pi.shape
    sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
    sc.partition, sc.edit = None, 1 if edit else 0
    cap, cnt = max(1024, 4 * nq), C.c_uint64()
    for _ in range(2):
        buf = DeviceBuffer(cap * HIT_DTYPE.itemsize)
        call = capi.lib().fmgpu_search_scheme_q4 if q4 else capi.lib().fmgpu_search_scheme
        rc = call(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(sc), n, capi.ptr(buf), cap, C.byref(cnt), None, None)
        if rc != capi.FMGPU_ERR_CAPACITY:
            break
        buf.free()
        cap = int(cnt.value)
    capi.check(rc)
    capi.check(capi.lib().fmgpu_hits_sort(capi.ptr(buf), cnt.value, None))
    return buf, int(cnt.value)


def _device_positions(index, hits, count):
    """fmgpu_locate_hits from hit records in HBM into HBM; one copy of the records to the host"""
    if count == 0:
        return np.zeros(0, dtype=POSITION_DTYPE)
    cap, cnt = max(1024, 4 * count), C.c_uint64()
    for _ in range(2):
        out = DeviceBuffer(cap * POSITION_DTYPE.itemsize)
        rc = capi.lib().fmgpu_locate_hits(index._h, capi.ptr(hits), count, capi.ptr(out), cap, C.byref(cnt), None, None)
        if rc != capi.FMGPU_ERR_CAPACITY:
            break
        out.free()
        cap = int(cnt.value)
    capi.check(rc)
    return out.to_array(POSITION_DTYPE, int(cnt.value))


def search_locate(index, queries, errors, n=UINT64_MAX, edit=True, compat_auto_scheme=False):
    """fmc::Search{index, queries, editDistance=edit, errors, maxResults=n}() (search/search.h:48-75): search, then every row of every reported
    cursor located — what the reference reports as reportFunc(qidx, seqId, pos + offset, errors), in the same order and with the same duplicates.
    The k > 0 pipeline keeps the hit records in HBM (search_ng26 -> fmgpu_hits_sort -> fmgpu_locate_hits); the only copy to the host is the
    result: an array of (qidx, seq_id, pos, errors) records.  n = maxResults (UINT64_MAX = none: fmc::search, else fmc::search_n)."""
    fields = ["qidx", "seq_id", "pos", "errors"]
    if errors == 0 and n == UINT64_MAX:                       # search_no_errors: one cursor per query, its {lb, len} come back anyway
        hits = search(index, queries, 0)
        return index.locate_hits(hits)[fields]
    qbuf, qoff, nq = _host_bytes(queries)                     # the length classes are split on the host, as in _auto_scheme_search
    lens = np.diff(qoff.astype(np.int64))
    parts = []
    for short in (False, True):
        sel = np.nonzero((lens == 2) == short)[0]
        if sel.size == 0:
            continue
        sc = search_scheme.h2(errors + (1 if short else 2), 0, errors)
        if compat_auto_scheme and not edit:
            sc = search_scheme.limitToHamming(sc)
        whole = sel.size == nq
        qb, qo = (qbuf, qoff) if whole else flatten([qbuf[int(qoff[i]): int(qoff[i + 1])] for i in sel])
        if whole and isinstance(queries, PackedQueries):      # (a packed batch of one length class goes down as it is)
            qb, qo = queries.packed, queries.qoff
        hits, count = _device_hits(index, qb, qo, sel.size, sc, n, edit, q4=whole and isinstance(queries, PackedQueries))
        pos = _device_positions(index, hits, count)
        hits.free()
        if sel.size != nq:
            pos["qidx"] = sel.astype(np.uint64)[pos["qidx"].astype(np.int64)]
        parts.append(pos)
    if not parts:
        return np.zeros(0, dtype=POSITION_DTYPE)[fields]
    pos = parts[0] if len(parts) == 1 else np.concatenate(parts)
    if len(parts) > 1:
        pos = pos[np.argsort(pos["qidx"], kind="stable")]     # the two length classes hold different queries: ascending qidx, each query's rows in order
    return pos[fields]


def _map_query(errors, schemes, ng21, edit, n, locate, first_records):
    """(capi.MapQuery, objects to keep alive) for map_reads / Feed.map.  errors=k: k == 0 is exact search (FMGPU_MAP_EXACT), k > 0 the ladder h2(j + 2, 0, j), j = 0 .. k,
    with uniform partitions (Hamming for edit=False).  schemes=[...]: an explicit ladder — (scheme, partition) pairs, or bare (pi, l, u) schemes; with ng21=True expanded
    schemes (search_scheme.expand) for the search_ng21 ladder."""
    if (errors is None) == (schemes is None):
        raise ValueError("give either errors or schemes")
    what = capi.MapQuery()
    what.max_hits_per_query, what.locate, what.first_records = n, 1 if locate else 0, int(first_records or 0)
    if schemes is None and int(errors) == 0:
        what.kind = capi.MAP_EXACT
        return what, None
    if schemes is None:
        schemes = [(search_scheme.h2(j + 2, 0, j), None) for j in range(int(errors) + 1)]
    if ng21:
        keep = [tuple(_u64(x) for x in sch) for sch in schemes]
        arr = (capi.ExpandedScheme * len(keep))()
        for sc, (pi, l, u) in zip(arr, keep):
            sc.n_searches, sc.length = (pi.shape if pi.ndim == 2 else (0, 0))
            sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
        what.kind = capi.MAP_NG21
    else:
        pairs = [s if len(s) == 2 else (s, None) for s in schemes]
        keep = [tuple(_u64(x) for x in sch) + ((_u64(part),) if part is not None else (None,)) for sch, part in pairs]
        arr = (capi.Scheme * len(keep))()
        for sc, (pi, l, u, part) in zip(arr, keep):
            sc.n_searches, sc.n_parts = pi.shape
            sc.pi, sc.l, sc.u = (x.ctypes.data_as(capi.u64p) for x in (pi, l, u))
            sc.partition = part.ctypes.data_as(capi.u64p) if part is not None else None
            sc.edit = 1 if edit else 0
        what.kind = capi.MAP_SCHEME
    what.n_schemes, what.schemes = len(keep), C.cast(arr, C.c_void_p)
    return what, (keep, arr)


def _run_map(call, nq, what, want_hits, want_stratum, want_stats, out, with_stream):
    """one fmgpu_map / fmgpu_feed_map call into host arrays: the counts are exact also on FMGPU_ERR_CAPACITY, so one more call with them always fits"""
    nst = max(1, what.n_schemes)
    stratum = np.full(max(nq, 1), 255, dtype=np.uint8) if want_stratum else None
    sstats, lstats = (capi.Stats * nst)(), capi.Stats()
    cap = len(out) if out is not None else (max(1024, 4 * nq) if what.locate else 0)
    hcap = max(1024, 4 * nq) if want_hits else 0
    cnt, hcnt = C.c_uint64(), C.c_uint64()
    for _ in range(2):
        pos = out if out is not None else np.zeros(max(cap, 1), dtype=POSITION_DTYPE)
        hits = np.zeros(max(hcap, 1), dtype=HIT_DTYPE) if want_hits else None
        args = (capi.ptr(pos), cap, C.byref(cnt), capi.ptr(hits), hcap, C.byref(hcnt), capi.ptr(stratum), sstats if want_stats else None,
                C.byref(lstats) if want_stats else None) + ((None,) if with_stream else ())
        rc = call(*args)
        if rc != capi.FMGPU_ERR_CAPACITY or out is not None:
            break
        cap, hcap = max(cap, int(cnt.value)), (max(hcap, int(hcnt.value)) if want_hits else 0)
    capi.check(rc)
    res = (pos[: cnt.value],)
    if want_hits:
        res += (np.ascontiguousarray(hits[: hcnt.value]),)
    if want_stratum:
        res += (stratum[:nq],)
    if want_stats:
        res += (([sstats[i] for i in range(nst)], lstats),)
    return res if len(res) > 1 else res[0]


def map_reads(index, queries, errors=None, schemes=None, ng21=False, edit=True, n=UINT64_MAX, locate=True, want_hits=False, want_stratum=False, want_stats=False,
              first_records=0, strands=None, pair=False):
    """fmgpu_map: fmc::Search's whole path in one call — search (exact, a best-stratum ladder of schemes, or a search_ng21 ladder), the records put into callback order
    and every row located, all on the device.  `queries` as for the searches (list of reads, (qbuf, qoff) of numpy arrays or DeviceBuffers, PackedQueries); see
    _map_query for errors / schemes.  Returns the POSITION_DTYPE records (qidx, seq_id, pos, errors, hit) in the reference's report order[, the HIT_DTYPE records `hit`
    indexes][, the uint8 stratum of every read, 255 = unfound][, (search stats per stratum, locate stats)].  locate=False stops after the hit records.
    strands= (a complement table, or "dna5"): fmgpu_map_strands — both strands of every read, the second made on the device; qidx and the stratum array count in the
    doubled batch (read = qidx >> 1, strand = qidx & 1).  pair=True: best stratum per read (the pair ladder)."""
    qbuf, qoff, nq = _queries(queries)
    what, alive = _map_query(errors, schemes, ng21, edit, n, locate, first_records)
    st, comp = _strands(strands, pair)
    if st is not None:
        if isinstance(queries, PackedQueries):
            raise ValueError("both strands are mapped from byte batches")
        res = _run_map(lambda *args: capi.lib().fmgpu_map_strands(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(what), C.byref(st), *args), 2 * nq, what, want_hits,
                       want_stratum, want_stats, None, True)
        del alive, comp
        return res
    call = _q4(queries, capi.lib().fmgpu_map, capi.lib().fmgpu_map_q4)
    res = _run_map(lambda *args: call(index._h, capi.ptr(qbuf), capi.ptr(qoff), nq, C.byref(what), *args), nq, what, want_hits, want_stratum, want_stats, None, True)
    del alive
    return res


def reconstruct_text(index, seq_nbr=None):
    """reconstructText(index, seqNbr) / reconstructText(index) (utils.h:672-703).  seq_nbr = a sentinel ROW (0 .. C[1] - 1): the symbols from the previous
    delimiter of that row's seqId (or pos 0) up to the row's delimiter.  None: one text per sentinel row, ordered by (seqId, row).  The sentinel rows are
    located on the host side's behalf by fmgpu_locate; the symbols come from ONE fmgpu_extract call (the table is built for the call if the index lacks
    it, and dropped again).  Returns a uint8 array, or a list of them."""
    nsent = int(index.rank(np.array([index.n], dtype=np.uint64), 0)[0])          # rank(size(), 0) + C[0] (C[0] = 0)
    if seq_nbr is not None and not 0 <= int(seq_nbr) < nsent:
        raise ValueError(f"seq_nbr {seq_nbr}: the index has {nsent} sentinel rows")
    rows = np.arange(nsent, dtype=np.uint64)
    seq, pos, steps = index.locate(rows)
    pos = pos + steps
    order = np.lexsort((pos, seq))                                                 # the delimiters of every seqId in text order
    prev = np.zeros(nsent, dtype=np.uint64)                                        # pos just behind the previous delimiter of the same seqId
    same = np.zeros(nsent, dtype=bool)
    if nsent > 1:
        same[order[1:]] = seq[order[1:]] == seq[order[:-1]]
        prev[order[1:]] = np.where(same[order[1:]], pos[order[:-1]] + 1, 0)
    pick = np.array([seq_nbr], dtype=np.int64) if seq_nbr is not None else np.lexsort((rows, seq))
    built = not (index.formats & capi.FMT_EXTRACT)
    if built:
        index.accelerate_extract()
    try:
        sym, off = index.extract(seq[pick], prev[pick], pos[pick] - prev[pick])
    finally:
        if built:
            index.accelerate_extract(False)
    texts = [sym[int(off[i]): int(off[i + 1])] for i in range(len(pick))]
    return texts[0] if seq_nbr is not None else texts


# ---- query text (fmgpu_queries_parse): LINES / FASTA / FASTQ bytes -> (qbuf, qoff) on the device --------------------------------------------
LINES, FASTA, FASTQ = capi.TEXT_LINES, capi.TEXT_FASTA, capi.TEXT_FASTQ
DROP, FOREIGN = capi.SYM_DROP, capi.SYM_FOREIGN
_TEXT_FORMATS = {"lines": LINES, "fasta": FASTA, "fastq": FASTQ}


def symbol_table(letters="ACGT", first_rank=1, case_insensitive=True, other=FOREIGN, drop=b"", extra={}):
    """the 256-entry uint8 table fmgpu_queries_parse maps sequence bytes through: letters[i] -> first_rank + i (both cases unless case_insensitive is False), the bytes
    of `drop` -> DROP (they produce nothing), `extra` = {byte or one-character string: value} on top, every other byte -> `other` (FOREIGN: written as 255 and counted)"""
    t = np.full(256, other, dtype=np.uint8)
    for i, ch in enumerate(letters):
        for c in ((ch.upper(), ch.lower()) if case_insensitive else (ch,)):
            t[ord(c)] = first_rank + i
    for b in (drop.encode() if isinstance(drop, str) else bytes(drop)):
        t[b] = DROP
    for k, v in extra.items():
        t[ord(k) if isinstance(k, str) else int(k)] = v
    return t


def _dna5(unknown_to_a=False):
    """$ A C G T = 0 .. 4 (the example's and the datasets' ranks); any other byte is FOREIGN, or rank 1 with unknown_to_a (the example's --convertUnknownChar)"""
    return symbol_table("ACGT", 1, True, 1 if unknown_to_a else FOREIGN, extra={"$": 0})


def _dna6(unknown_to_n=False):
    """$ A C G T N = 0 .. 5; any other byte is FOREIGN, or rank 5 with unknown_to_n"""
    return symbol_table("ACGTN", 1, True, 5 if unknown_to_n else FOREIGN, extra={"$": 0})


def _protein(letters="ACDEFGHIKLMNPQRSTVWY", **kw):
    """the amino-acid letters in alphabetical order = ranks 1 .. 20 ('$' = 0); keyword arguments as symbol_table's (e.g. extra={"X": 21}, drop=b"*-")"""
    kw.setdefault("extra", {"$": 0})
    return symbol_table(letters, 1, **kw)


symbol_table.dna5, symbol_table.dna6, symbol_table.protein = _dna5, _dna6, _protein


class TextError(FmgpuError):
    """a text error of fmgpu_queries_parse: `.line` (0-based) and `.offset` of the first offending line"""

    def __init__(self, code, msg, line, offset):
        super().__init__(code, msg)
        self.line, self.offset = line, offset


class ParsedQueries:
    """what parse_queries returns: qbuf / qoff (numpy arrays, or DeviceBuffers with device=True), `batch` = (qbuf, qoff) as the search calls take it, reads / symbols,
    names / quals (TEXT_SPAN_DTYPE arrays of spans into the text, or None), consumed (where the next chunk starts) and foreign (symbols written as 255)"""

    def __init__(self, qbuf, qoff, result, names, quals):
        self.qbuf, self.qoff, self.names, self.quals = qbuf, qoff, names, quals
        self.reads, self.symbols, self.consumed, self.foreign = int(result.reads), int(result.symbols), int(result.consumed), int(result.foreign)

    @property
    def batch(self):
        return self.qbuf, self.qoff

    @staticmethod
    def texts(data, spans):
        """the bytes of each span of `data` (the text the spans were made from)"""
        view = memoryview(data).cast("B") if not isinstance(data, np.ndarray) else data.view(np.uint8).reshape(-1)
        return [bytes(view[int(s["offset"]): int(s["offset"] + s["len"])]) for s in spans]


def _text_buffer(data):
    """(void*, bytes, keep-alive) of bytes, a numpy array, a torch tensor (host, pinned or device) or a DeviceBuffer / (ptr, nbytes) device view"""
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(data, dtype=np.uint8)
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    p, n = _buffer(data)
    return p, n, data


def parse_queries(data, format, table, final=True, device=False, want_names=False, want_quals=False, stream=None):
    """fmgpu_queries_parse: the bytes of a read file (or of a chunk of one: final=False, continue at `.consumed`) -> ParsedQueries.  format: LINES / FASTA / FASTQ or
    their lower-case names; table: symbol_table(...).  `data`: bytes, a numpy array, a torch tensor (host, pinned or device) or a DeviceBuffer.  device=True leaves qbuf / qoff
    in HBM as DeviceBuffers, which every search call, pack_queries_device and map_reads take as they are.  A text error raises TextError with the line number."""
    fmt = _TEXT_FORMATS[format] if isinstance(format, str) else int(format)
    table = np.ascontiguousarray(np.asarray(table, dtype=np.uint8))
    if table.size != 256:
        raise ValueError("a symbol table has 256 entries")
    p, nbytes, alive = _text_buffer(data)
    staged = None
    if nbytes and isinstance(alive, np.ndarray):              # host text: uploaded once for the two calls below
        staged = DeviceBuffer.from_array(alive)
        p = capi.ptr(staged)
    L, res = capi.lib(), capi.ParseResult()

    def call(qbuf, ncap, qoff, rcap, names, quals):
        rc = L.fmgpu_queries_parse(p, nbytes, fmt, 1 if final else 0, capi.ptr(table), capi.ptr(qbuf), ncap, capi.ptr(qoff), rcap, capi.ptr(names), capi.ptr(quals), C.byref(res), stream)
        if rc == capi.FMGPU_ERR_INVALID and L.fmgpu_last_error().startswith(b"text error"):
            raise TextError(rc, L.fmgpu_last_error().decode("utf-8", "replace"), int(res.error_line), int(res.error_offset))
        capi.check(rc)

    call(None, 0, None, 0, None, None)                        # the counting call sizes the outputs exactly
    reads, symbols = int(res.reads), int(res.symbols)
    if device:
        qbuf, qoff = DeviceBuffer(max(symbols, 8)), DeviceBuffer((reads + 1) * 8)
    else:
        qbuf, qoff = np.zeros(max(symbols, 1), dtype=np.uint8), np.zeros(reads + 1, dtype=np.uint64)
    names = np.zeros(reads, dtype=capi.TEXT_SPAN_DTYPE) if want_names else None
    quals = np.zeros(reads, dtype=capi.TEXT_SPAN_DTYPE) if want_quals else None
    call(qbuf, symbols, qoff, reads, names, quals)
    del alive, staged
    return ParsedQueries(qbuf, qoff, res, names, quals)


def parse_stream(fileobj, format, table, chunk_bytes=64 << 20, max_chunk_bytes=1 << 30, device=False, want_names=False, want_quals=False):
    """a generator of ParsedQueries over a binary file object: the file is read chunk by chunk into ONE pinned buffer (fmgpu_malloc_host), each chunk is parsed with
    final=False and its unconsumed tail is carried to the front of the buffer; only the last chunk is final.  A chunk that holds no complete read makes the buffer grow
    (doubling, up to max_chunk_bytes; beyond that ValueError).  With want_names / want_quals a batch carries `name_texts` / `qual_texts` (lists of bytes): the spans
    point into the buffer, which the next chunk overwrites."""
    size = max(int(chunk_bytes), 16)
    pinned = PinnedBuffer(size)
    try:
        buf, fill, eof = pinned.array(np.uint8), 0, False
        while not eof:
            while fill < size:
                got = fileobj.readinto(memoryview(buf)[fill:size])
                if not got:
                    eof = True
                    break
                fill += got
            if eof and fill == 0:
                break
            batch = parse_queries(buf[:fill], format, table, final=eof, device=device, want_names=want_names, want_quals=want_quals)
            if want_names:
                batch.name_texts = ParsedQueries.texts(buf, batch.names)
            if want_quals:
                batch.qual_texts = ParsedQueries.texts(buf, batch.quals)
            if batch.reads or eof:
                yield batch
            tail = fill - batch.consumed
            if not eof and batch.consumed == 0:               # no complete read in a full buffer: a larger one
                if size >= max_chunk_bytes:
                    raise ValueError(f"no complete read in {size} bytes of text (max_chunk_bytes)")
                bigger = PinnedBuffer(min(2 * size, int(max_chunk_bytes)))
                bigger.array(np.uint8)[:fill] = buf[:fill]
                del buf
                pinned.free()
                pinned, size = bigger, bigger.nbytes
                buf = pinned.array(np.uint8)
            elif batch.consumed:
                buf[:tail] = buf[batch.consumed:fill].copy()
            fill = tail
    finally:
        buf = None
        pinned.free()


# ---- positions to text lines on the device (fmgpu_positions_format)
def pack_names(names):
    """a list of bytes / str -> (data uint8[total], spans TEXT_SPAN_DTYPE[len(names)]): the names back to back, the shape of a name table of format_positions"""
    raw = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    spans = np.zeros(len(raw), dtype=TEXT_SPAN_DTYPE)
    lens = np.fromiter((len(n) for n in raw), dtype=np.uint64, count=len(raw))
    spans["len"] = lens
    if len(raw):
        spans["offset"][1:] = np.cumsum(lens)[:-1]
    return np.frombuffer(b"".join(raw), dtype=np.uint8), spans


def _name_table(names):
    """(capi.NameTable, keep-alive) of a (data, spans) pair — data as parse_queries takes it, spans a TEXT_SPAN_DTYPE array or a device buffer — or of a list of names"""
    if not (isinstance(names, tuple) and len(names) == 2):
        names = pack_names(names)
    data, spans = names
    p, nbytes, alive = _text_buffer(data)
    if isinstance(spans, np.ndarray):
        spans = np.ascontiguousarray(spans, dtype=TEXT_SPAN_DTYPE)
    sp, sbytes = _buffer(spans)
    table = capi.NameTable(p.value if nbytes else None, nbytes, sp.value if sbytes else None, sbytes // TEXT_SPAN_DTYPE.itemsize)
    return table, (alive, spans)


def format_positions(positions, columns=("qidx", "seq_id", "pos", "errors"), sep=" ", strands=False, name_stop=False, pos_add=0, read_names=None, seq_names=None,
                     device=False, want_line_offsets=False, stream=None):
    """fmgpu_positions_format: one text line per located position, made on the device.  positions: a POSITION_DTYPE array, or a DeviceBuffer / torch tensor of such
    records (used in place).  columns: names from capi.COLUMNS (or their codes), at most eight; a decimal column is written without padding, `sep` (one byte) stands
    between two columns and a newline ends the line; the default is the `qidx seq_id pos errors` line of the example.  strands=True reads qidx as the both-strand calls
    number it: "read" and "read_name" use qidx >> 1, "strand" is '-' for an odd qidx.  read_names / seq_names: a (data, spans) pair — what parse_queries and
    Feed.map_text return with want_names=True, with the text as data — or a list of bytes / str; name_stop ends a name at its first blank.  pos_add is added to pos.
    Returns the text as bytes, or with device=True (DeviceBuffer, bytes); with want_line_offsets also the uint64 offsets of the lines (count + 1 entries)."""
    if isinstance(positions, np.ndarray):
        positions = np.ascontiguousarray(positions, dtype=POSITION_DTYPE)
    pp, pbytes = _buffer(positions)
    count = pbytes // POSITION_DTYPE.itemsize
    cols = [capi.COLUMNS[c] if isinstance(c, str) else int(c) for c in columns]
    if not 1 <= len(cols) <= 8:
        raise ValueError("a line has 1 .. 8 columns")
    sep = sep.encode("latin-1") if isinstance(sep, str) else bytes(sep)
    if len(sep) != 1:
        raise ValueError("sep is one byte")
    spec = capi.FormatSpec(len(cols), (C.c_uint8 * 8)(*cols), sep[0], 1 if strands else 0, 1 if name_stop else 0, 0, int(pos_add) & UINT64_MAX, None, None)
    keep = []
    for field, names, code in (("read_names", read_names, capi.COL_READ_NAME), ("seq_names", seq_names, capi.COL_SEQ_NAME)):
        if code in cols:
            if names is None:
                raise ValueError(f"a {field[:-1]} column needs {field}")
            table, alive = _name_table(names)
            keep.append((table, alive))
            setattr(spec, field, C.pointer(table))
    sp = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
    L, nbytes = capi.lib(), C.c_uint64()
    off = np.zeros(count + 1, dtype=np.uint64) if want_line_offsets else None
    capi.check(L.fmgpu_positions_format(pp, count, C.byref(spec), None, 0, C.byref(nbytes), None, sp))       # the counting call sizes the text exactly
    total = int(nbytes.value)
    out = DeviceBuffer(max(total, 8)) if device else np.zeros(max(total, 1), dtype=np.uint8)
    capi.check(L.fmgpu_positions_format(pp, count, C.byref(spec), capi.ptr(out), total, C.byref(nbytes), capi.ptr(off), sp))
    del keep
    res = (out, total) if device else out[:total].tobytes()
    return (res, off) if want_line_offsets else res


# ---- positions to SAM records on the device (fmgpu_positions_sam, fmgpu_sam_header)
def char_table(letters="ACGT", first_rank=1, other="N", extra=None):
    """the inverse of symbol_table: the 256-entry uint8 table a SEQ byte is read from: value first_rank + i -> letters[i], `extra` = {value: byte or one-character
    string} on top, every other value (255, the FOREIGN symbol, among them) -> `other`.  char_table("dna5") is the inverse of symbol_table.dna5(): $ A C G T = 0 .. 4."""
    if letters == "dna5":
        return char_table("ACGT", 1, "N", {0: "$"})
    t = np.full(256, ord(other) if isinstance(other, str) else int(other), dtype=np.uint8)
    for i, ch in enumerate(letters):
        t[first_rank + i] = ord(ch)
    for k, v in (extra or {}).items():
        t[int(k)] = ord(v) if isinstance(v, str) else int(v)
    return t


def format_sam(positions, queries, char_of="dna5", strands=None, read_names=None, quals=None, seq_names=None, cigar=True, emit_unmapped=True, secondary_seq=False,
               mapq=(60, 0), device=False, want_line_offsets=False, stream=None):
    """fmgpu_positions_sam: the positions of map_reads / Feed.map as SAM alignment lines, made on the device.  positions: a POSITION_DTYPE array, or a DeviceBuffer /
    torch tensor of such records; queries: the FORWARD batch they were mapped from ((qbuf, qoff) of numpy arrays or DeviceBuffers, or a list of sequences); char_of: a
    char_table (or "dna5").  strands: the complement table the reads were mapped with (or "dna5"): qidx counts both strands, an odd one is written reversed and
    complemented with flag 16.  read_names / quals / seq_names: a (data, spans) pair — what parse_queries returns with want_names / want_quals, with the text as data —
    or a list of bytes / str; without them QNAME and RNAME are numbers and QUAL is '*'.  cigar=True states that the search was ungapped ("<m>M"); mapq = (unique, multi).
    Returns the text as bytes, or with device=True (DeviceBuffer, bytes); with want_line_offsets also the uint64 offsets of the lines (lines + 1 entries)."""
    if isinstance(positions, np.ndarray):
        positions = np.ascontiguousarray(positions, dtype=POSITION_DTYPE)
    pp, pbytes = _buffer(positions)
    count = pbytes // POSITION_DTYPE.itemsize
    if isinstance(queries, PackedQueries):
        raise ValueError("format_sam takes the byte form of the batch")
    qbuf, qoff, nq = _queries(queries)
    if isinstance(qoff, np.ndarray):
        qoff = _u64(qoff)
    if isinstance(qbuf, np.ndarray):
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
    table = char_table("dna5") if isinstance(char_of, str) and char_of == "dna5" else np.ascontiguousarray(np.asarray(char_of, dtype=np.uint8))
    if table.size != 256:
        raise ValueError("a character table has 256 entries")
    st, comp = _strands(strands, False)
    spec = capi.SamSpec(_buffer(qbuf)[0] if nq > 0 else None, _buffer(qoff)[0] if nq > 0 else None, max(nq, 0), table.ctypes.data, C.pointer(st) if st is not None else None,
                        None, None, None, 1 if cigar else 0, 1 if emit_unmapped else 0, 1 if secondary_seq else 0, int(mapq[0]), int(mapq[1]), (C.c_uint8 * 3)(0, 0, 0))
    keep = [comp, table, qbuf, qoff]
    for field, names in (("read_names", read_names), ("quals", quals), ("seq_names", seq_names)):
        if names is not None:
            t, alive = _name_table(names)
            keep.append((t, alive))
            setattr(spec, field, C.pointer(t))
    sp = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
    L, nbytes, nlines = capi.lib(), C.c_uint64(), C.c_uint64()
    capi.check(L.fmgpu_positions_sam(pp, count, C.byref(spec), None, 0, C.byref(nbytes), None, C.byref(nlines), sp))       # the counting call sizes the text exactly
    total, lines = int(nbytes.value), int(nlines.value)
    off = np.zeros(lines + 1, dtype=np.uint64) if want_line_offsets else None
    out = DeviceBuffer(max(total, 8)) if device else np.zeros(max(total, 1), dtype=np.uint8)
    capi.check(L.fmgpu_positions_sam(pp, count, C.byref(spec), capi.ptr(out), total, C.byref(nbytes), capi.ptr(off), C.byref(nlines), sp))
    del keep
    res = (out, total) if device else out[:total].tobytes()
    return (res, off) if want_line_offsets else res


def sam_header(seq_names, lengths, program=None):
    """fmgpu_sam_header: the @HD line, one @SQ line per sequence (its name up to the first blank, its length) and, with `program`, a @PG line, as bytes.  seq_names: a
    list of bytes / str or a host (data, spans) pair."""
    lengths = _u64(lengths).reshape(-1)
    table, alive = _name_table(seq_names)
    prog = None if program is None else (program.encode("utf-8") if isinstance(program, str) else bytes(program))
    L, nbytes = capi.lib(), C.c_uint64()
    capi.check(L.fmgpu_sam_header(C.byref(table), capi.ptr(lengths), lengths.size, prog, None, 0, C.byref(nbytes)))
    out = np.zeros(max(int(nbytes.value), 1), dtype=np.uint8)
    capi.check(L.fmgpu_sam_header(C.byref(table), capi.ptr(lengths), lengths.size, prog, capi.ptr(out), int(nbytes.value), C.byref(nbytes)))
    del alive
    return out[:int(nbytes.value)].tobytes()


# ---- positions of paired-end mates joined to concordant pairs on the device (fmgpu_positions_mates)
class MatePairs:
    """what join_mates returns: pairs (a MATE_PAIR_DTYPE array: fragment, tlen, a, b, errors, flags), off (uint64, fragments + 1 entries: each fragment's first pair
    record) and cls (uint8 per fragment, an index into capi.MATE_CLASSES)"""

    def __init__(self, pairs, off, cls):
        self.pairs, self.off, self.cls = pairs, off, cls

    def __len__(self):
        return len(self.pairs)


def _records(positions):
    """(void*, count, keep-alive) of a POSITION_DTYPE array, or of a DeviceBuffer / torch tensor of such records (used in place)"""
    if positions is None:
        return None, 0, None
    if isinstance(positions, np.ndarray):
        positions = np.ascontiguousarray(positions, dtype=POSITION_DTYPE)
    p, nbytes = _buffer(positions)
    count = nbytes // POSITION_DTYPE.itemsize
    return (p if count else None), count, positions


def join_mates(positions_a, qoff_a, positions_b=None, qoff_b=None, strands=True, interleaved=False, orientation="fr", min_tlen=0, max_tlen=1000, best=False,
               max_records=0, stream=None):
    """fmgpu_positions_mates: the positions map_reads returned for the two mates of every fragment joined to concordant pairs, on the device.  positions_a / positions_b:
    POSITION_DTYPE arrays, or DeviceBuffers / torch tensors of such records; qoff_a / qoff_b: the read offsets of the two batches (arrays or DeviceBuffers; only the read
    lengths are used).  interleaved=True: one batch (positions_b and qoff_b stay None) whose reads 2f and 2f + 1 are the mates of fragment f.  strands=True reads qidx
    as the both-strand calls number it (read = qidx >> 1, strand = qidx & 1).  orientation: "fr" (opposite strands, the forward mate upstream, no dovetail) or "any".
    min_tlen <= template length <= max_tlen.  best=True keeps only a fragment's pairs with the fewest errors; max_records > 0 leaves a fragment unjoined (class 5) if one
    of its mates has more records.  Returns a MatePairs (pairs, off, cls); the counting call sizes `pairs` exactly."""
    pa, count_a, keep_a = _records(positions_a)
    pb, count_b, keep_b = _records(positions_b)
    if interleaved and (positions_b is not None or qoff_b is not None):
        raise ValueError("an interleaved batch has no positions_b and no qoff_b")
    if not interleaved and (positions_b is None or qoff_b is None):
        raise ValueError("separate batches need positions_b and qoff_b")
    offs = []
    for q in (qoff_a, qoff_b):
        if q is not None and not (hasattr(q, "ptr") and not hasattr(q, "ctypes")) and not hasattr(q, "data_ptr"):
            q = _u64(q).reshape(-1)
        offs.append(q)
    reads_a = _buffer(offs[0])[1] // 8 - 1
    if reads_a < 0 or (interleaved and reads_a % 2):
        raise ValueError("qoff_a holds reads + 1 offsets, an even number of reads in an interleaved batch")
    n = reads_a // 2 if interleaved else reads_a
    if not interleaved and _buffer(offs[1])[1] // 8 - 1 != n:
        raise ValueError("both batches have one read per fragment")
    kinds = {"fr": capi.MATES_FR, "any": capi.MATES_ANY}
    if orientation not in kinds:
        raise ValueError('orientation is "fr" or "any"')
    spec = capi.MatesSpec(_buffer(offs[0])[0], None if interleaved else _buffer(offs[1])[0], n, int(min_tlen), int(max_tlen), int(max_records), 1 if strands else 0,
                          1 if interleaved else 0, kinds[orientation], 1 if best else 0, (C.c_uint8 * 4)(0, 0, 0, 0))
    sp = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
    L, total = capi.lib(), C.c_uint64()
    off, cls = np.zeros(n + 1, dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
    capi.check(L.fmgpu_positions_mates(pa, count_a, pb, count_b, C.byref(spec), None, 0, C.byref(total), None, None, sp))       # the counting call sizes the pairs exactly
    pairs = np.zeros(int(total.value), dtype=capi.MATE_PAIR_DTYPE)
    capi.check(L.fmgpu_positions_mates(pa, count_a, pb, count_b, C.byref(spec), capi.ptr(pairs) if pairs.size else None, pairs.size, C.byref(total), capi.ptr(off),
                                       capi.ptr(cls), sp))
    del keep_a, keep_b, offs
    return MatePairs(pairs[:int(total.value)], off, cls[:n])


# ---- located seeds joined to collinear chains on the device (fmgpu_seeds_chain)
class SeedChains:
    """what chain_seeds returns: chains (a CHAIN_DTYPE array in output order: queries ascending, inside a query the best chain first), off (uint64, nq + 1 entries: each
    query's first chain), cls (uint8 per query, an index into capi.CHAIN_CLASSES) and anchors (uint32: the indices into `positions` of every chain's anchors, chain k's at
    [first, first + n_anchors); None without want_anchors)"""

    def __init__(self, chains, off, cls, anchors):
        self.chains, self.off, self.cls, self.anchors = chains, off, cls, anchors

    def __len__(self):
        return len(self.chains)

    def anchors_of(self, k):
        """the indices into `positions` of chain k's anchors, first to last"""
        if self.anchors is None:
            raise ValueError("chain_seeds(want_anchors=False) kept no anchors")
        c = self.chains[k]
        return self.anchors[int(c["first"]): int(c["first"]) + int(c["n_anchors"])]


def chain_seeds(positions, spans, nq, max_gap=5000, max_skew=500, gap_cost=0.5, max_lookback=64, min_score=0, min_anchors=1, max_chains=0, max_anchors=0,
                want_anchors=True, stream=None):
    """fmgpu_seeds_chain: the located seeds of every query joined to collinear chains, on the device.  positions: what index.locate_hits returned for the hits of
    search_smems (a POSITION_DTYPE array, or a DeviceBuffer / torch tensor of such records); spans: the SEED_SPAN_DTYPE records of the same search_smems call (array or
    DeviceBuffer); nq: the queries in the numbering of qidx (twice the reads for a both_strands batch).  A link needs 1 <= dt, dq <= max_gap and |dt - dq| <= max_skew and
    costs gap_cost per base of skew (kept in 8 fractional bits); max_lookback (1 .. 256) candidates are looked at per anchor.  A chain is reported with score >= min_score
    and at least min_anchors anchors, max_chains > 0 keeps the best max_chains per query, max_anchors > 0 leaves a query with more anchors out (class 3).  Returns a
    SeedChains (chains, off, cls, anchors); the counting call sizes `chains` exactly."""
    pp, count, keep_p = _records(positions)
    if isinstance(spans, np.ndarray):
        spans = np.ascontiguousarray(spans, dtype=SEED_SPAN_DTYPE)
    sp_ptr, sp_bytes = _buffer(spans)
    n_spans = sp_bytes // SEED_SPAN_DTYPE.itemsize
    q8 = int(round(float(gap_cost) * 256))
    if q8 < 0:
        raise ValueError("gap_cost is not negative")
    nq = int(nq)
    spec = capi.ChainSpec(nq, int(max_gap), int(max_skew), q8, int(max_lookback), int(min_score), int(min_anchors), int(max_chains), int(max_anchors), (C.c_uint8 * 8)())
    sp = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
    L, total = capi.lib(), C.c_uint64()
    args = (pp, count, sp_ptr if n_spans else None, n_spans, C.byref(spec))
    capi.check(L.fmgpu_seeds_chain(*args, None, 0, C.byref(total), None, None, None, sp))                 # the counting call sizes the chains exactly
    chains = np.zeros(int(total.value), dtype=CHAIN_DTYPE)
    off, cls = np.zeros(nq + 1, dtype=np.uint64), np.zeros(max(nq, 1), dtype=np.uint8)
    anchors = np.zeros(max(count, 1), dtype=np.uint32) if want_anchors else None
    capi.check(L.fmgpu_seeds_chain(*args, capi.ptr(chains) if chains.size else None, chains.size, C.byref(total), capi.ptr(anchors) if want_anchors else None,
                                   capi.ptr(off), capi.ptr(cls), sp))
    del keep_p
    if want_anchors:
        anchors = np.ascontiguousarray(anchors[: int(chains["n_anchors"].sum(dtype=np.uint64))])
    return SeedChains(chains[: int(total.value)], off, cls[:nq], anchors)


# ---- seed chains to CIGAR alignments on the device (fmgpu_chains_align)
class ChainAlignments:
    """what align_chains returns: alignments (a CHAIN_ALIGNMENT_DTYPE array, one record per chain in chain order: first_op, n_ops, status, n_match, n_mismatch, n_ins,
    n_del) and ops (uint32, len << 4 | code with BAM's codes I = 1, D = 2, S = 4, '=' = 7, X = 8; chain k's at [first_op, first_op + n_ops))"""

    def __init__(self, alignments, ops):
        self.alignments, self.ops = alignments, ops

    def __len__(self):
        return len(self.alignments)

    def ops_of(self, k):
        """the operations of chain k as (length, code) pairs; none for a chain that was left out (status 1)"""
        r = self.alignments[k]
        w = self.ops[int(r["first_op"]): int(r["first_op"]) + int(r["n_ops"])]
        return [(int(x) >> 4, int(x) & 15) for x in w]

    def cigar(self, k, extended=True):
        """the CIGAR string of chain k: with '=' and 'X', or (extended=False, for SAM) both folded into 'M'.  '*' for a chain that was left out"""
        ops = self.ops_of(k)
        if not ops:
            return "*"
        if extended:
            return "".join("%d%s" % (n, capi.OP_CHARS[c]) for n, c in ops)
        out = []
        for n, c in ops:
            ch = "M" if c in (capi.OP_EQ, capi.OP_X) else capi.OP_CHARS[c]
            if out and out[-1][1] == ch:
                out[-1][0] += n
            else:
                out.append([n, ch])
        return "".join("%d%s" % (n, ch) for n, ch in out)


def align_chains(index, chained, positions, spans, queries, band=64, max_gap_len=5000, max_cells=1 << 24, text=None, stream=None):
    """fmgpu_chains_align: every chain of chain_seeds aligned between its ends, on the device: the anchors are exact matches, the gaps between consecutive anchors are
    aligned globally with unit costs on a band of `band` diagonals around the gap's own, and each chain becomes one line of operations with soft clips at the read's
    ends.  chained: what chain_seeds returned (with its anchors), or (chains, anchors) as arrays or DeviceBuffers; positions and spans: what chain_seeds read; queries:
    the batch in the numbering of qidx ((qbuf, qoff) or a list of sequences: the doubled batch for both_strands).  text=None reads the window of every chain from
    `index` with ONE extract call (the extract table is built for the call if the index lacks it, and dropped again); text=(tbuf, toff) hands the windows in (window c
    at tbuf[toff[c]:toff[c + 1]], arrays or DeviceBuffers) and needs no index.  A chain with a gap longer than max_gap_len on either side, or whose band holds more than
    max_cells cells, is left out (status 1).  Returns a ChainAlignments (alignments, ops); the counting call sizes `ops` exactly."""
    if isinstance(chained, SeedChains):
        if chained.anchors is None:
            raise ValueError("chain_seeds(want_anchors=False) kept no anchors")
        chains, anchors = chained.chains, chained.anchors
    else:
        chains, anchors = chained
    if isinstance(chains, np.ndarray):
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DTYPE)
    if isinstance(anchors, np.ndarray):
        anchors = np.ascontiguousarray(anchors, dtype=np.uint32)
    cp, cbytes = _buffer(chains)
    n_chains = cbytes // CHAIN_DTYPE.itemsize
    ap, abytes = _buffer(anchors)
    n_anchor = abytes // 4
    pp, count, keep_p = _records(positions)
    if isinstance(spans, np.ndarray):
        spans = np.ascontiguousarray(spans, dtype=SEED_SPAN_DTYPE)
    sp_ptr, sp_bytes = _buffer(spans)
    n_spans = sp_bytes // SEED_SPAN_DTYPE.itemsize
    if isinstance(queries, PackedQueries):
        raise ValueError("align_chains takes the byte form of the batch")
    qbuf, qoff, nq = _queries(queries)
    if isinstance(qoff, np.ndarray):
        qoff = _u64(qoff)
    if isinstance(qbuf, np.ndarray):
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
    if n_chains == 0:
        return ChainAlignments(np.zeros(0, dtype=capi.CHAIN_ALIGNMENT_DTYPE), np.zeros(0, dtype=np.uint32))
    if text is None:
        host = chains if isinstance(chains, np.ndarray) else chains.to_array(CHAIN_DTYPE, n_chains)
        built = not (index.formats & capi.FMT_EXTRACT)
        if built:
            index.accelerate_extract()
        try:
            tbuf, toff = index.extract(host["seq_id"], host["tbeg"], host["tend"] - host["tbeg"])
        finally:
            if built:
                index.accelerate_extract(False)
        if tbuf.size == 0:
            tbuf = np.zeros(1, dtype=np.uint8)
    else:
        tbuf, toff = text
        if isinstance(toff, np.ndarray):
            toff = _u64(toff)
        if isinstance(tbuf, np.ndarray):
            tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
    spec = capi.AlignSpec(max(nq, 0), int(max_cells), int(band), int(max_gap_len), (C.c_uint8 * 8)())
    st = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
    L, total = capi.lib(), C.c_uint64()
    out = np.zeros(n_chains, dtype=capi.CHAIN_ALIGNMENT_DTYPE)
    args = (cp, n_chains, ap, n_anchor, pp, count, sp_ptr if n_spans else None, n_spans, _buffer(qbuf)[0], _buffer(qoff)[0], _buffer(tbuf)[0], _buffer(toff)[0], C.byref(spec),
            capi.ptr(out))
    capi.check(L.fmgpu_chains_align(*args, None, 0, C.byref(total), st))                                  # the counting call sizes the operations exactly
    ops = np.zeros(max(int(total.value), 1), dtype=np.uint32)
    capi.check(L.fmgpu_chains_align(*args, capi.ptr(ops), int(total.value), C.byref(total), st))
    del keep_p
    return ChainAlignments(out, ops[: int(total.value)])


# ---- positions and mate pairs to paired-end SAM records on the device (fmgpu_positions_sam_mates)
def format_sam_mates(positions_a, queries_a, positions_b=None, queries_b=None, pairs=None, interleaved=False, char_of="dna5", strands=None, read_names=None, quals_a=None,
                     quals_b=None, seq_names=None, cigar=True, strip_mate_suffix=True, mapq=(60, 0), device=False, want_line_offsets=False, stream=None):
    """fmgpu_positions_sam_mates: the two mates of every fragment as two SAM lines with the mate fields filled in (flags 1, 2, 8, 32, 64, 128, RNEXT, PNEXT, TLEN), made
    on the device: line 2f is mate A of fragment f, line 2f + 1 mate B.  positions_a / positions_b: what map_reads returned for the two batches (POSITION_DTYPE arrays,
    DeviceBuffers or torch tensors); queries_a / queries_b: the FORWARD batches ((qbuf, qoff) of numpy arrays or DeviceBuffers, or lists of sequences); pairs: what
    join_mates returned (a MatePairs), a MATE_PAIR_DTYPE array or a DeviceBuffer of such records, None for no pair.  interleaved=True: one batch (positions_b and
    queries_b stay None) whose reads 2f and 2f + 1 are the mates of fragment f.  A fragment with pairs takes the pair with the fewest errors, the first one among
    equals, and is proper; in every other fragment each mate takes its own primary record.  strands, char_of, the tables, cigar and mapq as format_sam takes them
    (read_names: the names of batch A; quals_b stays None for an interleaved batch); strip_mate_suffix removes a trailing "/1" or "/2" from QNAME.
    Returns the text as bytes, or with device=True (DeviceBuffer, bytes); with want_line_offsets also the uint64 offsets of the lines (2 fragments + 1 entries)."""
    pa, count_a, keep_a = _records(positions_a)
    pb, count_b, keep_b = _records(positions_b)
    if interleaved and (positions_b is not None or queries_b is not None or quals_b is not None):
        raise ValueError("an interleaved batch has no positions_b, no queries_b and no quals_b")
    if not interleaved and (positions_b is None or queries_b is None):
        raise ValueError("separate batches need positions_b and queries_b")
    if isinstance(pairs, MatePairs):
        pairs = pairs.pairs
    if isinstance(pairs, np.ndarray):
        pairs = np.ascontiguousarray(pairs, dtype=capi.MATE_PAIR_DTYPE)
    pp, n_pairs = (None, 0) if pairs is None else _buffer(pairs)
    n_pairs //= capi.MATE_PAIR_DTYPE.itemsize
    batches = []
    for queries in (queries_a,) if interleaved else (queries_a, queries_b):
        if isinstance(queries, PackedQueries):
            raise ValueError("format_sam_mates takes the byte form of the batches")
        qbuf, qoff, nq = _queries(queries)
        if isinstance(qoff, np.ndarray):
            qoff = _u64(qoff)
        if isinstance(qbuf, np.ndarray):
            qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8)
        batches.append((qbuf, qoff, max(nq, 0)))
    reads = batches[0][2]
    if interleaved and reads % 2:
        raise ValueError("an interleaved batch holds an even number of reads")
    if not interleaved and batches[1][2] != reads:
        raise ValueError("both batches have one read per fragment")
    n = reads // 2 if interleaved else reads
    table = char_table("dna5") if isinstance(char_of, str) and char_of == "dna5" else np.ascontiguousarray(np.asarray(char_of, dtype=np.uint8))
    if table.size != 256:
        raise ValueError("a character table has 256 entries")
    st, comp = _strands(strands, False)
    ptrs = [_buffer(b)[0] if n > 0 else None for batch in batches for b in batch[:2]] + [None, None]
    spec = capi.SamMatesSpec(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n, table.ctypes.data, C.pointer(st) if st is not None else None, None, None, None, None,
                             1 if interleaved else 0, 1 if cigar else 0, 1 if strip_mate_suffix else 0, int(mapq[0]), int(mapq[1]), (C.c_uint8 * 3)(0, 0, 0))
    keep = [comp, table, batches, keep_a, keep_b, pairs]
    for field, names in (("read_names", read_names), ("quals_a", quals_a), ("quals_b", quals_b), ("seq_names", seq_names)):
        if names is not None:
            t, alive = _name_table(names)
            keep.append((t, alive))
            setattr(spec, field, C.pointer(t))
    sp = None if stream is None else C.c_void_p(stream if isinstance(stream, int) else getattr(stream, "cuda_stream", 0))
    L, nbytes = capi.lib(), C.c_uint64()
    pp = pp if n_pairs else None
    capi.check(L.fmgpu_positions_sam_mates(pa, count_a, pb, count_b, pp, n_pairs, C.byref(spec), None, 0, C.byref(nbytes), None, sp))     # the counting call sizes the text exactly
    total = int(nbytes.value)
    off = np.zeros(2 * n + 1, dtype=np.uint64) if want_line_offsets else None
    out = DeviceBuffer(max(total, 8)) if device else np.zeros(max(total, 1), dtype=np.uint8)
    capi.check(L.fmgpu_positions_sam_mates(pa, count_a, pb, count_b, pp, n_pairs, C.byref(spec), capi.ptr(out), total, C.byref(nbytes), capi.ptr(off), sp))
    del keep
    res = (out, total) if device else out[:total].tobytes()
    return (res, off) if want_line_offsets else res
