"""fmgpu_search_smems without a GPU: the symbols, the record size, the argument checks that need no device, and the brute-force oracle of
tests/test_gpu_smems.py (tests/smem_brute.py) against the textbook definition of a super-maximal exact match."""
import ctypes as C

import numpy as np

from fmindex_collection_amd import capi
from tests import smem_brute as sb


def test_symbols_and_record_size():
    L = capi.lib()
    for name in ("fmgpu_search_smems", "fmgpu_search_smems_q4"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert L.fmgpu_abi_version() == 6
    assert C.sizeof(capi.SeedSpan) == 8 and capi.SEED_SPAN_DTYPE.itemsize == 8
    assert capi.SEED_SPAN_DTYPE.names == ("qbeg", "qlen")


def test_argument_checks_without_a_device():
    L = capi.lib()
    qbuf, qoff = np.array([1, 2, 3], dtype=np.uint8), np.array([0, 3], dtype=np.uint64)
    hits, spans = np.zeros(4, dtype=capi.HIT_DTYPE), np.zeros(4, dtype=capi.SEED_SPAN_DTYPE)
    for call in (L.fmgpu_search_smems, L.fmgpu_search_smems_q4):
        cnt = C.c_uint64(99)
        assert call(None, capi.ptr(qbuf), capi.ptr(qoff), 1, 1, 0, capi.ptr(hits), capi.ptr(spans), 4, C.byref(cnt), None, None, None) == capi.FMGPU_ERR_INVALID
        # nq == 0 is decided before the handle is looked at
        assert call(None, None, None, 0, 1, 0, None, None, 0, C.byref(cnt), None, None, None) == 0 and cnt.value == 0
        assert call(None, None, None, 0, 1, 0, None, None, 0, None, None, None, None) == 0
    assert not hits.view(np.uint8).any() and not spans.view(np.uint8).any()


def random_case(rng, sigma=5):
    seqs = [rng.integers(1, sigma, size=int(l), dtype=np.uint8) for l in rng.integers(0, 40, size=int(rng.integers(1, 4)))]
    src = np.concatenate(seqs + [np.zeros(1, dtype=np.uint8)])
    m = int(rng.integers(0, 30))
    if src.size > 1 and m and rng.random() < 0.7:                 # a window of the text with a few substitutions, delimiters and foreign bytes
        at = int(rng.integers(0, src.size))
        read = np.resize(src[at:], m).copy()
        for _ in range(int(rng.integers(0, 4))):
            read[int(rng.integers(0, m))] = rng.choice([0, 1, 2, 3, 4, sigma, 255])
    else:
        read = rng.integers(0, sigma + 1, size=m, dtype=np.uint8)
    return seqs, read


def test_brute_oracle_is_the_textbook_definition():
    rng = np.random.default_rng(17)
    seen = 0
    for _ in range(60):
        seqs, read = random_case(rng)
        text = sb.join_text(seqs)
        found, L = sb.smems(text, read, 5)
        assert L == sb.match_lengths_naive(text, read, 5)
        assert all(L[e + 1] <= L[e] + 1 for e in range(len(L) - 1))
        assert [(b, l) for b, l, _ in found] == sb.textbook_smems(text, read, 5)
        assert [b for b, _, _ in found] == sorted({b for b, _, _ in found})          # qbeg strictly increasing
        for b, l, rows in found:
            pat = bytes(read[b: b + l])
            assert rows == sum(1 for i in range(len(text)) if text[i: i + l] == pat) >= 1
        # the step count is what a walk of every end executes, counted one extension at a time
        steps = 0
        for e in range(len(read)):
            l = 0
            while l <= e and not sb.is_break(read[e - l], 5):
                steps += 1
                if bytes(read[e - l: e + 1]) not in text:
                    break
                l += 1
            assert l == L[e]
        assert steps == sb.walk_steps(bytes(read), L, 5)
        seen += len(found)
    assert seen > 60


def test_brute_filters_and_numbering():
    seqs = [np.array([1, 2, 3, 4, 1, 2, 3, 4, 1, 2], dtype=np.uint8), np.array([4, 4, 3], dtype=np.uint8)]
    reads = [np.array([1, 2, 3, 4, 0, 4, 4, 3, 3], dtype=np.uint8), np.zeros(0, dtype=np.uint8), np.array([2, 3, 4, 1, 2, 3, 4, 1, 2, 2], dtype=np.uint8)]
    b = sb.Batch(seqs, reads, 5)
    assert b.seeds() == [(0, 0, 4, 0, 2), (0, 5, 3, 1, 1), (0, 8, 1, 2, 3), (2, 0, 9, 0, 1), (2, 9, 1, 1, 3)]
    assert b.seeds(min_len=3) == [(0, 0, 4, 0, 2), (0, 5, 3, 1, 1), (2, 0, 9, 0, 1)]
    assert b.seeds(max_rows=1) == [(0, 5, 3, 0, 1), (2, 0, 9, 0, 1)]              # a dropped seed is dropped: nothing shorter in its place
    assert b.lengths == [1, 2, 3, 4, 0, 1, 2, 3, 1] + [1, 2, 3, 4, 5, 6, 7, 8, 9, 1]
