"""fmgpu_locate_hits on the host side: the record layout the Python mirror reads, the export, the argument checks (no device needed)."""
import ctypes as C

import numpy as np

from fmindex_collection_amd import capi


def test_position_record_is_32_bytes_and_matches_the_dtype():
    assert C.sizeof(capi.Position) == capi.POSITION_DTYPE.itemsize == 32
    for name, _ in capi.Position._fields_:
        assert getattr(capi.Position, name).offset == capi.POSITION_DTYPE.fields[name][1], name
    rec = np.zeros(1, dtype=capi.POSITION_DTYPE)
    rec["qidx"], rec["seq_id"], rec["pos"], rec["errors"], rec["hit"] = 3, 5, 7, 2, 11
    p = capi.Position.from_buffer_copy(rec.tobytes())
    assert (p.qidx, p.seq_id, p.pos, p.errors, p.hit) == (3, 5, 7, 2, 11)


def test_locate_hits_is_exported():
    assert "fmgpu_locate_hits" in capi.EXPORTS
    assert hasattr(capi.lib(), "fmgpu_locate_hits")


def test_argument_checks_without_a_device():
    L = capi.lib()
    hits = np.zeros(2, dtype=capi.HIT_DTYPE)
    out = np.zeros(4, dtype=capi.POSITION_DTYPE)
    cnt = C.c_uint64(0)
    # a null handle
    assert L.fmgpu_locate_hits(None, capi.ptr(hits), 2, capi.ptr(out), 4, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_locate_hits(None, None, 0, None, 0, None, None, None) == capi.FMGPU_ERR_INVALID
    # null pointers while count > 0 (checked before the handle is looked at)
    bogus = C.c_void_p(0x1000)
    assert L.fmgpu_locate_hits(bogus, None, 2, capi.ptr(out), 4, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_locate_hits(bogus, capi.ptr(hits), 2, None, 4, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_locate_hits(bogus, capi.ptr(hits), 2, capi.ptr(out), 4, None, None, None) == capi.FMGPU_ERR_INVALID
    assert b"null" in L.fmgpu_last_error()
