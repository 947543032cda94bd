"""fmgpu_positions_sam_mates (include/fmgpu.h) restated in plain Python, from the header's text: what the device must write, byte for byte, and what it must refuse, in
the header's order.  A record is any mapping with qidx, seq_id, pos and errors, a pair any mapping with fragment, a and b (rows of POSITION_DTYPE / MATE_PAIR_DTYPE arrays
will do); a batch is (qbuf, qoff); a table is (data, spans) or (data, spans, n_bytes) as in tests/sam_model.py, whose row and complement helpers are used here."""
from tests.sam_model import INVALID, MASK, UNSUPPORTED, _row, comp_table

LONG_TEXT = {"read": "is a read of 2^31 symbols or more", "name": "has a name or quality span of 2^31 bytes or more", "line": "makes a line of 2^32 bytes or more"}
BAD_TEXT = {"read_names row": "names a row beyond the read_names table", "read_names span": "has a read name span that leaves the table's bytes",
            "quals row": "names a row beyond its quality table", "quals span": "has a quality span that leaves the table's bytes",
            "quals len": "has a quality span whose len is neither 0 nor the read's length", "seq_names row": "names a row beyond the seq_names table",
            "seq_names span": "has a sequence name span that leaves the table's bytes"}


class SamMatesError(Exception):
    """what the device passes refuse: code (INVALID / UNSUPPORTED), who ("positions_a: record", "qoff_b: read", "pairs: pair", "fragment"), its index, for a line its
    mate ("A" / "B", else None), and the word for what is wrong with it"""

    def __init__(self, code, who, index, what, mate=None):
        super().__init__(f"{who} {index}{' mate ' + mate if mate else ''}: {what}")
        self.code, self.who, self.index, self.what, self.mate = code, who, index, what, mate

    @property
    def names(self):
        """the words the library's message carries"""
        return f"{self.who} {self.index} " + (f"mate {self.mate} " + (BAD_TEXT if self.code == INVALID else LONG_TEXT)[self.what] if self.mate else "")


def qname_of(name, strip):
    """a read name (cut at its first blank already) as QNAME writes it"""
    if strip and len(name) >= 3 and name[-2:] in (b"/1", b"/2"):
        name = name[:-2]
    return name or b"*"


def format_sam_mates(records_a, batch_a, records_b=None, batch_b=None, pairs=(), char_of=None, complement=None, interleaved=False, read_names=None, quals_a=None,
                     quals_b=None, seq_names=None, cigar=1, strip_mate_suffix=1, mapq_unique=60, mapq_multi=0):
    """(text, line offsets: 2 n_fragments + 1 entries, the last one len(text)).  Raises SamMatesError for what the device refuses."""
    reads = len(batch_a[1]) - 1 if len(batch_a[1]) else 0
    n = reads // 2 if interleaved else reads
    if n == 0:
        return b"", [0]
    shift = 0 if complement is None else 1
    comp = comp_table(complement if complement is not None else ())
    sides = 1 if interleaved else 2
    recs = [records_a, records_a if interleaved else records_b]
    qbufs = [batch_a[0], batch_a[0] if interleaved else batch_b[0]]
    qoffs = [batch_a[1], batch_a[1] if interleaved else batch_b[1]]
    quals = [quals_a, quals_a if interleaved else quals_b]
    read_of = [[int(r["qidx"]) >> shift for r in recs[s]] for s in range(2)]
    arrays = ("positions_a", "positions_b")
    for s in range(sides):
        for i, r in enumerate(read_of[s]):
            if r >= reads:
                raise SamMatesError(INVALID, arrays[s] + ": record", i, "range")
    for s in range(sides):
        for i in range(1, len(read_of[s])):
            if read_of[s][i - 1] > read_of[s][i]:
                raise SamMatesError(INVALID, arrays[s] + ": record", i, "order")
    for s in range(sides):
        for r in range(reads):
            if int(qoffs[s][r + 1]) < int(qoffs[s][r]):
                raise SamMatesError(INVALID, ("qoff_a", "qoff_b")[s] + ": read", r, "qoff")
    for s in range(sides):
        for i, r in enumerate(recs[s]):
            if int(r["pos"]) >= 1 << 62:
                raise SamMatesError(INVALID, arrays[s] + ": record", i, "pos")
    chosen, at_min = {}, {}                                  # per fragment: (error sum, pair index) of its chosen pair; the pairs with that sum
    for i, p in enumerate(pairs):
        f, a, b = int(p["fragment"]), int(p["a"]), int(p["b"])
        if f >= n or a >= len(recs[0]) or b >= len(recs[1]) or read_of[0][a] != (2 * f if interleaved else f) or read_of[1][b] != (2 * f + 1 if interleaved else f):
            raise SamMatesError(INVALID, "pairs: pair", i, "pair")
        total = (int(recs[0][a]["errors"]) + int(recs[1][b]["errors"])) & 0xFFFFFFFF
        if f not in chosen or total < chosen[f][0]:
            chosen[f], at_min[f] = (total, i), 1
        elif total == chosen[f][0]:
            at_min[f] += 1
    of_slot = [[] for _ in range(2 * n)]                      # slot 2f: the records of mate A of fragment f, slot 2f + 1: of mate B
    for s in range(sides):
        for i, r in enumerate(read_of[s]):
            of_slot[r if interleaved else 2 * r + s].append(i)
    mine = []                                                 # per slot: (record index or None, its records with the fewest errors)
    for line in range(2 * n):
        side, f = line & 1, line >> 1
        least = min((int(recs[side][k]["errors"]) for k in of_slot[line]), default=0)
        best = [k for k in of_slot[line] if int(recs[side][k]["errors"]) == least]
        if f in chosen:
            mine.append((int(pairs[chosen[f][1]]["ab"[side]]), best))
        else:
            mine.append((best[0] if best else None, best))

    def seq_name(seq_id, invalid, toolong):
        name = b"%d" % seq_id
        if seq_names is not None:
            name = _row(seq_names, seq_id, True)
            if isinstance(name, str):
                (toolong if name == "long" else invalid).append("name" if name == "long" else "seq_names " + name)
                name = b""
            name = name or b"*"
        return name

    def fields(line):
        """line `line`, or (code, word)"""
        side, f = line & 1, line >> 1
        row, yrow = (line, line ^ 1) if interleaved else (f, f)
        m = int(qoffs[side][row + 1]) - int(qoffs[side][row])
        my = int(qoffs[side ^ 1][yrow + 1]) - int(qoffs[side ^ 1][yrow])
        invalid, toolong = [], []
        if m >= 1 << 31:
            toolong.append("read")
        x = recs[side][mine[line][0]] if mine[line][0] is not None else None
        y = recs[side ^ 1][mine[line ^ 1][0]] if mine[line ^ 1][0] is not None else None
        qname = b"%d" % f
        if read_names is not None:
            qname = _row(read_names, 2 * f if interleaved else f, True)
            if isinstance(qname, str):
                (toolong if qname == "long" else invalid).append("name" if qname == "long" else "read_names " + qname)
                qname = b""
            qname = qname_of(qname, strip_mate_suffix)
        qual, stated = None, 0
        if quals[side] is not None:
            qual = _row(quals[side], row, False)
            if isinstance(qual, str):
                (toolong if qual == "long" else invalid).append("name" if qual == "long" else "quals " + qual)
                qual = None
            else:
                stated = int(quals[side][1][row][1])
                if not toolong and stated not in (0, m):
                    invalid.append("quals len")
        sx = int(x["qidx"]) & 1 if x is not None and shift else 0
        sy = int(y["qidx"]) & 1 if y is not None and shift else 0
        proper = f in chosen
        flag = 1 + (128 if side else 64) + (2 if proper else 0) + (4 if x is None else 0) + (8 if y is None else 0) + (16 if sx else 0) + (32 if sy else 0)
        rname, pos, rnext, pnext, tlen = b"*", 0, b"*", 0, 0
        if x is not None or y is not None:
            at = x if x is not None else y
            rname, pos = seq_name(int(at["seq_id"]), invalid, toolong), int(at["pos"]) + 1
            pnext = int((y if y is not None else x)["pos"]) + 1
            rnext = b"="
            if x is not None and y is not None and int(x["seq_id"]) != int(y["seq_id"]):
                rnext = seq_name(int(y["seq_id"]), invalid, toolong)
        if x is not None and y is not None and int(x["seq_id"]) == int(y["seq_id"]):
            px, py = int(x["pos"]), int(y["pos"])
            t = max(px + m, py + my) - min(px, py)
            tlen = -t if px > py or (px == py and side) else t
        if invalid:
            return INVALID, invalid[0]
        if toolong:
            return UNSUPPORTED, toolong[0]
        if x is None:
            mapq = 0
        elif proper:
            mapq = mapq_unique if at_min[f] == 1 else mapq_multi
        else:
            mapq = mapq_unique if len(mine[line][1]) == 1 else mapq_multi
        star_seq = m == 0
        star_qual = qual is None or stated == 0 or star_seq
        head = [qname, b"%d" % flag, rname, b"%d" % (pos & MASK), b"%d" % mapq, b"%dM" % m if x is not None and cigar == 1 and m > 0 else b"*", rnext,
                b"%d" % (pnext & MASK), b"%d" % tlen]
        tail = [] if x is None else [b"NM:i:%d" % int(x["errors"]), b"NH:i:%d" % len(of_slot[line])]
        if sum(len(v) + 1 for v in head + tail) + (1 if star_seq else m) + 1 + (1 if star_qual else m) + 1 >= 1 << 32:
            return UNSUPPORTED, "line"
        q0 = int(qoffs[side][row])
        q = [int(c) for c in qbufs[side][q0: q0 + m]]
        if star_seq:
            seq = b"*"
        elif sx:
            seq = bytes(int(char_of[comp[q[m - 1 - j]]]) for j in range(m))
        else:
            seq = bytes(int(char_of[c]) for c in q)
        if star_qual:
            qual = b"*"
        elif sx:
            qual = qual[::-1]
        return b"\t".join(head + [seq, qual] + tail) + b"\n"

    lines = [fields(line) for line in range(2 * n)]
    for code in (INVALID, UNSUPPORTED):
        for line, got in enumerate(lines):
            if isinstance(got, tuple) and got[0] == code:
                raise SamMatesError(code, "fragment", line >> 1, got[1], "AB"[line & 1])
    offsets = [0]
    for got in lines:
        offsets.append(offsets[-1] + len(got))
    return b"".join(lines), offsets
