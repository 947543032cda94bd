"""fmgpu_positions_sam and fmgpu_sam_header (include/fmgpu.h) restated in plain Python, from the header's text: what the device must write, byte for byte.  A record is
any mapping with qidx, seq_id, pos and errors (a row of a POSITION_DTYPE array will do); the batch is (qbuf, qoff); a table is (data, spans): bytes, and (offset, len)
pairs relative to them — or (data, spans, n_bytes) where the table states more bytes than `data` holds (what is too long is refused by its stated sizes, before a byte
of it is read; likewise a read's length is qoff[r + 1] - qoff[r], whatever qbuf holds)."""
MASK = (1 << 64) - 1
INVALID, UNSUPPORTED = -1, -2


class SamError(Exception):
    """what the device passes refuse: code (INVALID / UNSUPPORTED), who ("record" / "read" / "unmapped read"), its index and what is wrong with it"""

    def __init__(self, code, who, index, what):
        super().__init__(f"{who} {index}: {what}")
        self.code, self.who, self.index, self.what = code, who, index, what

    @property
    def names(self):
        """the words the library's message carries"""
        return f"{self.who} {self.index} "


def _row(table, row, stop):
    """the bytes of row `row` (up to its first blank with `stop`), or the word for what is wrong with it"""
    data, spans, *stated = table
    if row >= len(spans):
        return "row"
    offset, length = int(spans[row][0]), int(spans[row][1])
    if offset + length > (stated[0] if stated else len(data)):
        return "span"
    if length >= 1 << 31:
        return "long"
    name = bytes(bytearray(data[offset: offset + length]))
    if stop:
        for k, b in enumerate(name):
            if b in b" \t":
                return name[:k]
    return name


def comp_table(complement):
    """comp(c) = complement[c] for c < n, c otherwise (the rule of fmgpu_queries_strands)"""
    table = list(range(256))
    for c, v in enumerate(complement):
        table[c] = int(v)
    return table


def format_sam(records, qbuf, qoff, char_of, complement=None, read_names=None, quals=None, seq_names=None, cigar=1, emit_unmapped=1, secondary_seq=0, mapq_unique=60,
               mapq_multi=0):
    """(text, line offsets: lines + 1 entries, the last one len(text)).  Raises SamError for what the device refuses, in the header's order."""
    nq = len(qoff) - 1 if len(qoff) else 0
    shift = 0 if complement is None else 1
    comp = comp_table(complement if complement is not None else ())
    reads = [int(r["qidx"]) >> shift for r in records]
    for i, r in enumerate(reads):
        if r >= nq:
            raise SamError(INVALID, "record", i, "range")
    for i in range(1, len(reads)):
        if reads[i - 1] > reads[i]:
            raise SamError(INVALID, "record", i, "order")
    for r in range(nq):
        if int(qoff[r + 1]) < int(qoff[r]):
            raise SamError(INVALID, "read", r, "qoff")
    of_read = [[] for _ in range(nq)]
    for i, r in enumerate(reads):
        of_read[r].append(i)

    best_of = []                                             # per read: its records with the fewest errors, in record order; the first is the primary
    for mine in of_read:
        least = min((int(records[k]["errors"]) for k in mine), default=0)
        best_of.append([k for k in mine if int(records[k]["errors"]) == least])
    lines = []                                               # (who, index, bytes or (code, word))

    def fields(r, i):
        """the line of record i of read r (i None: the unmapped line), or (code, word)"""
        m = int(qoff[r + 1]) - int(qoff[r])
        invalid, toolong = [], []
        if m >= 1 << 31:
            toolong.append("read")
        qname = b"%d" % r
        if read_names is not None:
            qname = _row(read_names, r, True)
            if isinstance(qname, str):
                (toolong if qname == "long" else invalid).append("read_names " + qname)
                qname = b""
            qname = qname or b"*"
        qual = None
        if quals is not None:
            qual = _row(quals, r, False)
            if isinstance(qual, str):
                (toolong if qual == "long" else invalid).append("quals " + qual)
                qual = None
            elif not toolong and int(quals[1][r][1]) not in (0, m):      # (the span's stated len; a line that is too long already is not looked at further)
                invalid.append("quals len")
        rec = records[i] if i is not None else None
        rname = b"*"
        if rec is not None:
            rname = b"%d" % int(rec["seq_id"])
            if seq_names is not None:
                rname = _row(seq_names, int(rec["seq_id"]), True)
                if isinstance(rname, str):
                    (toolong if rname == "long" else invalid).append("seq_names " + rname)
                    rname = b""
                rname = rname or b"*"
        if invalid:
            return INVALID, invalid[0]
        if toolong:
            return UNSUPPORTED, toolong[0]
        strand = int(rec["qidx"]) & 1 if rec is not None and shift else 0
        if rec is None:
            secondary = False
        else:
            best = best_of[r]
            secondary = i != best[0]
        star_seq = m == 0 or (secondary and not secondary_seq)
        star_qual = qual is None or int(quals[1][r][1]) == 0 or star_seq
        if rec is None:
            head, tail = [qname, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0"], []
        else:
            flag = (16 if strand else 0) | (256 if secondary else 0)
            mapq = mapq_unique if not secondary and len(best) == 1 else mapq_multi
            head = [qname, b"%d" % flag, rname, b"%d" % ((int(rec["pos"]) + 1) & MASK), b"%d" % mapq, b"%dM" % m if cigar == 1 and m > 0 else b"*", b"*", b"0", b"0"]
            tail = [b"NM:i:%d" % int(rec["errors"]), b"NH:i:%d" % len(of_read[r])]
        # the line's length from the stated sizes: every field and the byte behind it
        if sum(len(f) + 1 for f in head + tail) + (1 if star_seq else m) + 1 + (1 if star_qual else m) + 1 >= 1 << 32:
            return UNSUPPORTED, "line"
        q = [int(c) for c in qbuf[int(qoff[r]): int(qoff[r + 1])]]
        if star_seq:
            seq = b"*"
        elif strand:
            seq = bytes(int(char_of[comp[q[m - 1 - j]]]) for j in range(m))
        else:
            seq = bytes(int(char_of[c]) for c in q)
        if star_qual:
            qual = b"*"
        elif strand:
            qual = qual[::-1]
        parts = head + [seq, qual] + tail
        return b"\t".join(parts) + b"\n"

    for r in range(nq):
        if of_read[r]:
            lines += [("record", i, fields(r, i)) for i in of_read[r]]
        elif emit_unmapped:
            lines.append(("unmapped read", r, fields(r, None)))
    for code in (INVALID, UNSUPPORTED):
        for who, index, got in lines:
            if isinstance(got, tuple) and got[0] == code:
                raise SamError(code, who, index, got[1])
    offsets = [0]
    for _, _, got in lines:
        offsets.append(offsets[-1] + len(got))
    return b"".join(got for _, _, got in lines), offsets


def sam_header(seq_names, lengths, program_id=None):
    """the header's bytes; a name is a bytes object.  An empty SN raises SamError(INVALID, "sequence", s, "empty")"""
    text = b"@HD\tVN:1.6\tSO:unknown\n"
    for s, (name, length) in enumerate(zip(seq_names, lengths)):
        for k, b in enumerate(name):
            if b in b" \t":
                name = name[:k]
                break
        if not name:
            raise SamError(INVALID, "sequence", s, "empty")
        text += b"@SQ\tSN:" + name + b"\tLN:%d\n" % int(length)
    if program_id is not None:
        text += b"@PG\tID:" + program_id + b"\n"
    return text
