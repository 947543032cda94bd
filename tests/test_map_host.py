"""fmgpu_map, fmgpu_map_q4, fmgpu_hits_from_intervals, fmgpu_feed_map and fmgpu_feed_map_v (include/fmgpu.h) on the host: the symbols, the ABI version and option count
they leave alone, the layout of fmgpu_map_query in the header text against capi, and what the calls decide before a handle or a device is looked at.

fmgpu_map_query: the declaration the calls were specified with (two int32, a pointer, a uint64, two int32, a uint64) is 40 bytes under the C layout rules, not the 48 that
were quoted beside it; the test computes the size and every offset from the header text by those rules and holds capi.MapQuery to them."""
import ctypes as C
import os
import re

import numpy as np

from fmindex_collection_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("fmgpu_map", "fmgpu_map_q4", "fmgpu_hits_from_intervals", "fmgpu_feed_map", "fmgpu_feed_map_v")


def header():
    with open(os.path.join(ROOT, "include", "fmgpu.h")) as f:
        return f.read()


def test_symbols_exist_and_abi_version_and_option_count_stay():
    L = capi.lib()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header()), name
    assert L.fmgpu_abi_version() == 6
    assert re.search(r"#define FMGPU_ABI_VERSION 6\b", header())
    assert re.search(r"FMGPU_OPT_COUNT_ = 13\b", header()) and len(capi.OPTIONS) == 13
    v = C.c_int64()
    assert L.fmgpu_get_option(12, C.byref(v)) == 0 and L.fmgpu_get_option(13, C.byref(v)) == capi.FMGPU_ERR_INVALID


def test_map_query_layout_matches_the_header_text():
    body = re.search(r"typedef struct fmgpu_map_query \{(.*?)\} fmgpu_map_query;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    sizes = {"int32_t": 4, "uint64_t": 8, "const void*": 8}
    fields, at = [], 0
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(int32_t|uint64_t|const void\*)\s+(\w+)", decl)
        assert m, decl
        size = sizes[m.group(1)]
        at = (at + size - 1) // size * size                          # natural alignment
        fields.append((m.group(2), at, size))
        at += size
    total = (at + 7) // 8 * 8
    assert [f[0] for f in fields] == ["kind", "n_schemes", "schemes", "max_hits_per_query", "locate", "reserved", "first_records"]
    assert [f[0] for f in fields] == [f[0] for f in capi.MapQuery._fields_]
    for name, offset, size in fields:
        d = getattr(capi.MapQuery, name)
        assert (d.offset, d.size) == (offset, size), name
    assert C.sizeof(capi.MapQuery) == total == 40
    assert re.search(r"#define FMGPU_MAP_EXACT\s+0\b", header()) and re.search(r"#define FMGPU_MAP_SCHEME\s+1\b", header()) and re.search(r"#define FMGPU_MAP_NG21\s+2\b", header())
    assert (capi.MAP_EXACT, capi.MAP_SCHEME, capi.MAP_NG21) == (0, 1, 2)


def map_calls():
    L = capi.lib()
    return [(name, getattr(L, name), () if "feed" in name else (None,)) for name in CALLS if name != "fmgpu_hits_from_intervals"]


def test_no_reads_return_zero_counts_without_a_device():
    L = capi.lib()
    sch = (capi.Scheme * 2)()
    for name, call, tail in map_calls():
        for what in (capi.MapQuery(capi.MAP_EXACT, 0, None, 7, 1, 0, 0), capi.MapQuery(capi.MAP_SCHEME, 2, C.cast(sch, C.c_void_p), 7, 1, 0, 0),
                     capi.MapQuery(capi.MAP_NG21, 1, None, 7, 0, 0, 1)):
            cnt, hcnt = C.c_uint64(7), C.c_uint64(7)
            stratum = np.full(4, 9, dtype=np.uint8)
            sstats, lstats = (capi.Stats * 2)(), capi.Stats()
            sstats[0].hits = lstats.hits = 3
            assert call(None, None, None, 0, C.byref(what), None, 0, C.byref(cnt), None, 0, C.byref(hcnt), capi.ptr(stratum), sstats, C.byref(lstats), *tail) == 0, name
            assert cnt.value == 0 and hcnt.value == 0, name
            assert (stratum == 9).all(), name                          # untouched
            assert sstats[0].hits == 0 and lstats.hits == 0, name
            assert call(None, None, None, 0, C.byref(what), None, 0, None, None, 0, None, None, None, None, *tail) == 0, name
    cnt = C.c_uint64(7)
    assert L.fmgpu_hits_from_intervals(None, None, None, 0, 5, 1, None, 0, C.byref(cnt), None, None) == 0 and cnt.value == 0
    assert L.fmgpu_hits_from_intervals(None, None, None, 0, 5, 1, None, 0, None, None, None) == 0


def test_bad_kind_n_schemes_and_reserved_are_refused_before_the_handle():
    L = capi.lib()
    sch = (capi.Scheme * 2)()
    p = C.cast(sch, C.c_void_p)
    one = np.zeros(8, dtype=np.uint64)
    bad = [(capi.MapQuery(-1, 0, None, 1, 1, 0, 0), b"kind"), (capi.MapQuery(3, 1, p, 1, 1, 0, 0), b"kind"),
           (capi.MapQuery(capi.MAP_EXACT, 1, None, 1, 1, 0, 0), b"n_schemes"), (capi.MapQuery(capi.MAP_SCHEME, 0, p, 1, 1, 0, 0), b"n_schemes"),
           (capi.MapQuery(capi.MAP_SCHEME, 255, p, 1, 1, 0, 0), b"n_schemes"), (capi.MapQuery(capi.MAP_NG21, -1, p, 1, 1, 0, 0), b"n_schemes"),
           (capi.MapQuery(capi.MAP_EXACT, 0, None, 1, 1, 1, 0), b"reserved"), (capi.MapQuery(capi.MAP_SCHEME, 2, p, 1, 0, 5, 0), b"reserved")]
    for name, call, tail in map_calls():
        for nq in (0, 1):                                              # also for an empty batch: the query is looked at first
            for what, word in bad:
                cnt = C.c_uint64(7)
                rc = call(None, capi.ptr(one), capi.ptr(one), nq, C.byref(what), None, 0, C.byref(cnt), None, 0, None, None, None, None, *tail)
                assert rc == capi.FMGPU_ERR_INVALID and word in L.fmgpu_last_error(), (name, nq, word, L.fmgpu_last_error())
                assert cnt.value == 0
        cnt = C.c_uint64(7)
        assert call(None, capi.ptr(one), capi.ptr(one), 1, None, None, 0, C.byref(cnt), None, 0, None, None, None, None, *tail) == capi.FMGPU_ERR_INVALID, name
        # a good query and a null handle / feed: refused as the pieces refuse it
        good = capi.MapQuery(capi.MAP_EXACT, 0, None, 1, 0, 0, 0)
        assert call(None, capi.ptr(one), capi.ptr(one), 1, C.byref(good), None, 0, C.byref(cnt), None, 0, None, None, None, None, *tail) == capi.FMGPU_ERR_INVALID, name
        assert (b"feed" if "feed" in name else b"handle") in L.fmgpu_last_error(), name
    # fmgpu_hits_from_intervals: null arrays while there are reads
    cnt = C.c_uint64(7)
    assert L.fmgpu_hits_from_intervals(None, capi.ptr(one), None, 1, 0, 1, None, 0, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_hits_from_intervals(capi.ptr(one), capi.ptr(one), None, 1, 0, 1, None, 0, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_hits_from_intervals(capi.ptr(one), capi.ptr(one), None, 1, 0, 1, None, 3, C.byref(cnt), None, None) == capi.FMGPU_ERR_INVALID
