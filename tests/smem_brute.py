"""brute-force restatement of fmgpu_search_smems (include/fmgpu.h): match lengths, seeds and the step count from the definitions, by substring search in the
delimiter-joined text.  Plain Python / numpy; the oracle of tests/test_gpu_smems.py, kept honest by tests/test_smems_host.py."""
import numpy as np


def as_bytes(read):
    return read if isinstance(read, bytes) else bytes(np.asarray(read, dtype=np.uint8))


def join_text(seqs):
    """the indexed text: every sequence followed by its delimiter 0"""
    return b"".join(as_bytes(s) + b"\0" for s in seqs)


def is_break(c, sigma):
    return not 1 <= int(c) < sigma


def occurs(text, read, beg, end, sigma):
    """read[beg:end] holds no break and occurs in the text"""
    return beg < end and not any(is_break(c, sigma) for c in read[beg:end]) and bytes(read[beg:end]) in text


def count_occurrences(text, pattern):
    """occurrences of a non-empty pattern, overlapping ones included"""
    n, at = 0, text.find(pattern)
    while at >= 0:
        n += 1
        at = text.find(pattern, at + 1)
    return n


def match_lengths_naive(text, read, sigma):
    """L[e] straight from the definition: the largest l <= e + 1 such that read[e - l + 1 .. e] holds no break and occurs"""
    read = as_bytes(read)
    return [next((l for l in range(e + 1, 0, -1) if occurs(text, read, e + 1 - l, e + 1, sigma)), 0) for e in range(len(read))]


def match_lengths(text, read, sigma):
    """the same L, trying only l <= L[e - 1] + 1 (a match ending at e without its last symbol is a match ending at e - 1)"""
    read = as_bytes(read)
    L, prev = [], 0
    for e in range(len(read)):
        l = 0
        if not is_break(read[e], sigma):
            l = prev + 1
            while l > 0 and read[e + 1 - l: e + 1] not in text:
                l -= 1
        L.append(l)
        prev = l
    return L


def walk_reads(read, sigma):
    """per end e of the read, the symbols its walk may consume: read[b + 1 .. e] behind the last break b at or before e (empty where read[e] is one).  A one-symbol
    backward search of such a piece, stopped at the first empty extension, visits the intervals the walk of end e visits: tests/exact_traffic_model.py prices them"""
    out, first = [], 0
    for e in range(len(read)):
        if is_break(read[e], sigma):
            first = e + 1
        out.append(np.asarray(read[first: e + 1], dtype=np.uint8))
    return out


def walk_steps(read, L, sigma):
    """extensions of a one-symbol walk: L[e] that succeed, plus the one that came out empty where the walk did not stop at the read's start or at a break"""
    return sum(L) + sum(1 for e in range(len(read)) if L[e] <= e and not is_break(read[e - L[e]], sigma))


def smems(text, read, sigma):
    """(qbeg, qlen, rows) of the read's SMEMs in ascending qbeg: the ends e with L[e] >= 1 and (e == m - 1 or L[e + 1] <= L[e])"""
    read = as_bytes(read)
    L = match_lengths(text, read, sigma)
    m = len(read)
    out = []
    for e in range(m):
        if L[e] >= 1 and (e == m - 1 or L[e + 1] <= L[e]):
            out.append((e - L[e] + 1, L[e], count_occurrences(text, read[e - L[e] + 1: e + 1])))
    return out, L


def textbook_smems(text, read, sigma):
    """(qbeg, qlen) of the maximal exact matches not contained in another: every occurring break-free interval of the read that no other such interval contains"""
    read = as_bytes(read)
    m = len(read)
    found = {(i, j) for i in range(m) for j in range(i + 1, m + 1) if occurs(text, read, i, j, sigma)}
    keep = [(i, j) for (i, j) in found if not any((a, b) != (i, j) and a <= i and j <= b for (a, b) in found)]
    return sorted((i, j - i) for i, j in keep)


class Batch:
    """what fmgpu_search_smems returns for `reads` on the text of `seqs`, unfiltered: L of every batch symbol, the step count, and every SMEM as
    (qidx, qbeg, qlen, rows); seeds(min_len, max_rows) applies the filters and numbers the kept seeds within their read"""

    def __init__(self, seqs, reads, sigma):
        self.text = join_text(seqs)
        self.lengths, self.all, self.steps = [], [], 0
        for q, read in enumerate(reads):
            found, L = smems(self.text, read, sigma)
            self.lengths += L
            self.steps += walk_steps(as_bytes(read), L, sigma)
            self.all += [(q, b, l, rows) for b, l, rows in found]

    def seeds(self, min_len=1, max_rows=0):
        out, seq, last = [], 0, None
        for q, b, l, rows in self.all:
            if l < max(min_len, 1) or (max_rows and rows > max_rows):
                continue
            seq = seq + 1 if q == last else 0
            last = q
            out.append((q, b, l, seq, rows))
        return out
