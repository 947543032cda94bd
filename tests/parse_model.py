"""The contract of fmgpu_queries_parse (include/fmgpu.h) restated in plain Python, line by line: what the device call is checked against."""
import numpy as np

LINES, FASTA, FASTQ = 0, 1, 2
DROP, FOREIGN = 254, 255


class Parsed:
    """reads: list of bytes (the symbols of each complete record); names / quals: (offset, len) per read; error_line is None without a text error"""

    def __init__(self):
        self.reads, self.names, self.quals = [], [], []
        self.consumed = self.foreign = 0
        self.error_line = self.error_offset = None

    @property
    def symbols(self):
        return sum(len(r) for r in self.reads)

    @property
    def qbuf(self):
        return np.frombuffer(b"".join(self.reads), dtype=np.uint8)

    @property
    def qoff(self):
        off = np.zeros(len(self.reads) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in self.reads], dtype=np.uint64)
        return off


def split_lines(text, final):
    """[(start, end)] of every line, end without the terminator: '\\n', and a '\\r' in front of it or as the last byte of a final buffer; plus how many end in '\\n'"""
    lines, terminated, s, n = [], 0, 0, len(text)
    while s < n:
        nl = text.find(b"\n", s)
        has_nl = nl >= 0
        e = nl if has_nl else n
        nxt = nl + 1 if has_nl else n
        terminated += has_nl
        if e > s and text[e - 1] == 0x0D and (has_nl or final):
            e -= 1
        lines.append((s, e))
        s = nxt
    return lines, terminated


def _symbols(text, s, e, table, out):
    foreign = 0
    for b in text[s:e]:
        v = int(table[b])
        if v == DROP:
            continue
        out.append(v)
        foreign += v == FOREIGN
    return foreign


def parse(text, fmt, table, final=True):
    text = bytes(text)
    n = len(text)
    lines, terminated = split_lines(text, final)
    start_of = lambda l: lines[l][0] if l < len(lines) else n      # noqa: E731
    res = Parsed()
    records = []            # (name span, quality span, [sequence lines])
    if fmt == LINES:
        complete = len(lines) if final else terminated
        records = [((0, 0), (0, 0), [lines[l]]) for l in range(complete)]
        res.consumed = start_of(complete)
    elif fmt == FASTA:
        found = []          # (start offset, name span, [sequence lines])
        for l, (s, e) in enumerate(lines):
            if e == s:
                continue
            if text[s] == ord(">"):
                found.append((s, (s + 1, e - s - 1), []))
            elif not found:
                res.error_line, res.error_offset = l, s
                return res
            else:
                found[-1][2].append((s, e))
        if final:
            complete, res.consumed = found, n
        elif len(found) >= 2:
            complete, res.consumed = found[:-1], found[-1][0]
        else:
            complete = []
        records = [(name, (0, 0), seq) for _, name, seq in complete]
    elif fmt == FASTQ:
        have = len(lines) if final else terminated
        if final:
            while have and lines[have - 1][0] == lines[have - 1][1]:
                have -= 1
        for r in range(have // 4):
            (hs, he), (ss, se), (ps, pe), (qs, qe) = lines[4 * r: 4 * r + 4]
            bad = None
            if he == hs or text[hs] != ord("@"):
                bad = 4 * r
            elif pe == ps or text[ps] != ord("+"):
                bad = 4 * r + 2
            elif qe - qs != se - ss:
                bad = 4 * r + 3
            if bad is not None:
                res.error_line, res.error_offset = bad, lines[bad][0]
                break
            records.append(((hs + 1, he - hs - 1), (qs, qe - qs), [(ss, se)]))
        if res.error_line is None and final and have % 4:
            res.error_line, res.error_offset = 4 * (have // 4), lines[4 * (have // 4)][0]
        res.consumed = start_of(4 * len(records))
    else:
        raise ValueError("unknown format")
    for name, qual, seq in records:
        out = bytearray()
        for s, e in seq:
            res.foreign += _symbols(text, s, e, table, out)
        res.reads.append(bytes(out))
        res.names.append(name)
        res.quals.append(qual)
    return res


def reference_fasta_reads(text, rank_of):
    """The example's documented reader rule (example/main.cpp, readFasta) on a well-formed file: a line that starts with '>' begins a record, every other line's
    bytes are appended to the current record through rank_of, line ends dropped."""
    reads = []
    for line in text.split(b"\n"):
        if line.startswith(b">"):
            reads.append(bytearray())
        elif line:
            reads[-1].extend(rank_of[b] for b in line)
    return [bytes(r) for r in reads]
