"""fmgpu_extract on the host side: the range record the Python mirror writes, the exports, the argument checks (no device needed)."""
import ctypes as C

import numpy as np

from fmindex_collection_amd import capi


def test_text_range_record_is_24_bytes_and_matches_the_dtype():
    assert C.sizeof(capi.TextRange) == capi.TEXT_RANGE_DTYPE.itemsize == 24
    for name, _ in capi.TextRange._fields_:
        assert getattr(capi.TextRange, name).offset == capi.TEXT_RANGE_DTYPE.fields[name][1], name
    rec = np.zeros(1, dtype=capi.TEXT_RANGE_DTYPE)
    rec["seq_id"], rec["pos"], rec["len"] = 3, 5, 7
    r = capi.TextRange.from_buffer_copy(rec.tobytes())
    assert (r.seq_id, r.pos, r.len) == (3, 5, 7)


def test_extract_entry_points_are_exported():
    for name in ("fmgpu_extract", "fmgpu_sequence_lengths", "fmgpu_index_accelerate_extract"):
        assert name in capi.EXPORTS
        assert hasattr(capi.lib(), name), name
    assert capi.FMT_EXTRACT == 1 << 13


def test_argument_checks_without_a_device():
    L = capi.lib()
    r = np.zeros(2, dtype=capi.TEXT_RANGE_DTYPE)
    out = np.zeros(16, dtype=np.uint8)
    ids, lens = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    cnt = C.c_uint64(0)
    # a null handle
    assert L.fmgpu_extract(None, capi.ptr(r), 2, capi.ptr(out), 16, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_extract(None, None, 0, None, 0, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_sequence_lengths(None, capi.ptr(ids), capi.ptr(lens), 4, C.byref(cnt)) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_index_accelerate_extract(None, 1) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_index_accelerate_extract(None, 0) == capi.FMGPU_ERR_INVALID
    # null buffers while count > 0 (checked before the handle is looked at)
    bogus = C.c_void_p(0x1000)
    assert L.fmgpu_extract(bogus, None, 2, capi.ptr(out), 16, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_extract(bogus, capi.ptr(r), 2, None, 16, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_extract(bogus, capi.ptr(r), 2, capi.ptr(out), 16, None, None, None) == capi.FMGPU_ERR_INVALID
    assert b"null" in L.fmgpu_last_error()
