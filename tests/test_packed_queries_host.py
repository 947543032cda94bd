"""The 4-bit packed query form (include/fmgpu.h) on the host: the format pinned by a literal, pack / unpack round trips, the both-strand form, and the
argument errors of the new calls — everything that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

import fmindex_collection_amd as fm
from fmindex_collection_amd import capi


def test_format_literal():
    pq = fm.pack_queries([np.array([1, 2, 3], dtype=np.uint8), np.array([4, 0], dtype=np.uint8)], 5)
    assert pq.packed.tobytes() == bytes([0x21, 0x43, 0x00])          # the even symbol index is the low nibble; the nibble left over is 0
    assert pq.qoff.tolist() == [0, 3, 5] and pq.qoff.dtype == np.uint64 and pq.nq == 2
    pq = fm.pack_queries([np.array([9, 1, 255], dtype=np.uint8)], 5)
    assert pq.packed.tobytes() == bytes([0x1f, 0x0f])                 # a byte >= sigma is nibble 15
    pq = fm.pack_queries([np.array([9, 14, 15], dtype=np.uint8)], 15)
    assert pq.packed.tobytes() == bytes([0xe9, 0x0f])


def _batch(rng, lengths, sigma, foreign=True):
    reads = []
    for m in lengths:
        r = rng.integers(0, sigma, size=m, dtype=np.uint8)
        if foreign and m and rng.integers(0, 3) == 0:
            r[int(rng.integers(0, m))] = [sigma, 200, 255][int(rng.integers(0, 3))]
        reads.append(r)
    return reads


@pytest.mark.parametrize("sigma", [5, 15])
def test_round_trip(sigma):
    rng = np.random.default_rng(3)
    for lengths in (list(range(41)), [0, 0, 1, 0, 3, 0, 0], [1, 3, 5, 7, 9, 11, 13], list(rng.permutation(41)), [], [0]):
        reads = _batch(rng, lengths, sigma)
        qbuf, qoff = fm.flatten(reads)
        pq = fm.pack_queries((qbuf, qoff), sigma)
        assert pq.nq == len(reads) and pq.packed.size == (int(qoff[-1]) + 1) // 2
        back, boff = fm.unpack_queries(pq)
        want = np.where(qbuf[: int(qoff[-1])] >= sigma, 255, qbuf[: int(qoff[-1])]).astype(np.uint8)
        assert np.array_equal(back, want) and np.array_equal(boff, qoff)


def test_round_trip_with_an_odd_first_offset():
    rng = np.random.default_rng(4)
    reads = _batch(rng, [5, 0, 8, 3, 1], 5)
    qbuf, qoff = fm.flatten(reads)
    for lead in (1, 3, 6):
        sbuf = np.concatenate([np.full(lead, 7, dtype=np.uint8), qbuf]); soff = qoff + np.uint64(lead)
        pq = fm.pack_queries((sbuf, soff), 5)                        # the packed batch starts at symbol 0 whatever the input's first offset
        assert np.array_equal(pq.packed, fm.pack_queries((qbuf, qoff), 5).packed) and pq.qoff[0] == 0
        # a packed batch whose first symbol is nibble `lead` of its buffer: the nibbles before it belong to someone else
        nib = np.concatenate([np.full(lead, 15, dtype=np.uint8), np.where(qbuf[: int(qoff[-1])] >= 5, 15, qbuf[: int(qoff[-1])]).astype(np.uint8)])
        nib = np.concatenate([nib, np.zeros(nib.size & 1, dtype=np.uint8)])
        packed = nib[0::2] | (nib[1::2] << 4)
        back, boff = fm.unpack_queries(fm.PackedQueries(packed, soff))
        assert np.array_equal(back, np.where(qbuf[: int(qoff[-1])] >= 5, 255, qbuf[: int(qoff[-1])])) and np.array_equal(boff, qoff)


def test_complement_form_equals_packing_the_both_strand_batch():
    rng = np.random.default_rng(5)
    comp = np.array([0, 4, 3, 2, 1], dtype=np.uint8)
    reads = _batch(rng, list(range(41)) + [101, 7, 0, 9], 5)
    both = []
    for r in reads:
        both.append(r)
        both.append(np.array([comp[c] if c < 5 else 255 for c in r[::-1]], dtype=np.uint8))
    a, b = fm.pack_queries(reads, 5, complement=comp), fm.pack_queries(both, 5)
    assert a.packed.tobytes() == b.packed.tobytes() and np.array_equal(a.qoff, b.qoff) and a.nq == 2 * len(reads)


def test_argument_errors_without_a_gpu():
    L = capi.lib()
    one = np.zeros(8, dtype=np.uint64)
    assert L.fmgpu_search_exact_q4(None, None, None, 1, None, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_search_scheme_q4(None, None, None, 1, None, 1, None, 0, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_search_ng21_q4(None, None, None, 1, None, 1, None, 0, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_queries_pack4(None, None, 1, 5, None, None, None, None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_queries_pack4(capi.ptr(one), capi.ptr(one), 1, 5, None, None, capi.ptr(one), None) == capi.FMGPU_ERR_INVALID
    assert L.fmgpu_queries_unpack4(None, capi.ptr(one), 1, capi.ptr(one), None) == capi.FMGPU_ERR_INVALID
    for sigma in (16, 1, 0, 28):
        assert L.fmgpu_queries_pack4(capi.ptr(one), capi.ptr(one), 1, sigma, None, capi.ptr(one), capi.ptr(one), None) == capi.FMGPU_ERR_UNSUPPORTED, sigma
    assert L.fmgpu_queries_pack4(None, None, 0, 5, None, None, None, None) == 0 and L.fmgpu_queries_unpack4(None, None, 0, None, None) == 0
    with pytest.raises(ValueError):
        fm.pack_queries([np.array([1], dtype=np.uint8)], 16)


def test_new_select_bit_is_part_of_the_mask():
    L = capi.lib()
    assert L.fmgpu_set_option(capi.OPTIONS["kernel_select"], capi.SEL_UNPACK_QUERIES) == 0
    v = C.c_int64()
    assert L.fmgpu_get_option(capi.OPTIONS["kernel_select"], C.byref(v)) == 0 and v.value == capi.SEL_UNPACK_QUERIES
    assert L.fmgpu_set_option(capi.OPTIONS["kernel_select"], 0) == 0
    assert L.fmgpu_abi_version() == 6
