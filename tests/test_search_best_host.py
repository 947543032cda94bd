"""The best-stratum calls (include/fmgpu.h: fmgpu_search_best*) on the host: the symbols, the ABI version they leave alone, and the argument errors that need no GPU."""
import ctypes as C

import numpy as np

from fmindex_collection_amd import capi

CALLS = ("fmgpu_search_best", "fmgpu_search_best_ng21", "fmgpu_search_best_q4", "fmgpu_search_best_ng21_q4")


def test_symbols_exist_and_the_abi_version_stays():
    L = capi.lib()
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert L.fmgpu_abi_version() == 6                                 # the calls are additions: no device format changed


def test_argument_errors_without_a_gpu():
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    rec = np.zeros(40, dtype=np.uint8)
    cnt = C.c_uint64(7)
    for name in CALLS:
        call = getattr(L, name)
        schemes = (capi.ExpandedScheme * 2)() if "ng21" in name else (capi.Scheme * 2)()
        # a null handle
        assert call(None, capi.ptr(one), capi.ptr(one), 1, schemes, 1, 1, capi.ptr(rec), 1, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID, name
        # n_schemes outside 0 .. 254, whatever else is passed
        for n in (-1, 255):
            assert call(None, None, None, 1, schemes, n, 1, None, 0, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID, (name, n)
            assert b"n_schemes" in L.fmgpu_last_error()
        # no read, or no scheme: 0 records, out_stratum all 255
        cnt.value = 7
        assert call(None, None, None, 0, schemes, 2, 1, None, 0, C.byref(cnt), None, None, None) == 0 and cnt.value == 0, name
        strat = np.zeros(5, dtype=np.uint8)
        cnt.value = 7
        assert call(None, None, None, 5, None, 0, 1, None, 0, C.byref(cnt), capi.ptr(strat), None, None) == 0 and cnt.value == 0, name
        assert (strat == 255).all(), name
        stats = (capi.Stats * 2)()
        stats[1].hits = 3
        assert call(None, None, None, 0, schemes, 2, 1, None, 0, None, None, stats, None) == 0 and stats[1].hits == 0, name
