"""fmgpu_positions_format (include/fmgpu.h) restated in plain Python: what the device must write, byte for byte.  A record is any mapping with qidx, seq_id, pos,
errors and hit (a row of a POSITION_DTYPE array will do); a name table is (data, spans): bytes, and (offset, len) pairs relative to them."""
QIDX, SEQ_ID, POS, ERRORS, HIT, READ, STRAND, READ_NAME, SEQ_NAME = range(9)
MASK = (1 << 64) - 1
INVALID, UNSUPPORTED = -1, -2


class FormatError(Exception):
    """what the pass that measures the lines refuses: code (INVALID / UNSUPPORTED), the lowest offending record and what is wrong with it ("row" / "span" / "long")"""

    def __init__(self, code, record, what):
        super().__init__(f"record {record}: {what}")
        self.code, self.record, self.what = code, record, what


def _name(table, row, name_stop):
    """the bytes of row `row`, or the word for what is wrong with it"""
    data, spans = table
    if row >= len(spans):
        return "row"
    offset, length = int(spans[row][0]), int(spans[row][1])
    if offset + length > len(data):
        return "span"
    if length >= 1 << 31:
        return "long"
    name = bytes(data[offset: offset + length])
    if name_stop:
        for k, b in enumerate(name):
            if b in b" \t":
                return name[:k]
    return name


def line(rec, cols, sep=b" ", strand_shift=0, name_stop=False, pos_add=0, read_names=None, seq_names=None):
    """one record's line, or the word for its error"""
    qidx, seq_id = int(rec["qidx"]), int(rec["seq_id"])
    read = qidx >> strand_shift
    names = {}
    if READ_NAME in cols:
        names[READ_NAME] = _name(read_names, read, name_stop)
    if SEQ_NAME in cols:
        names[SEQ_NAME] = _name(seq_names, seq_id, name_stop)
    bad = [v for v in names.values() if isinstance(v, str)]
    if bad:
        return min(bad, key=("row", "span", "long").index)
    parts = []
    for c in cols:
        if c in (READ_NAME, SEQ_NAME):
            parts.append(names[c])
        elif c == STRAND:
            parts.append(b"-" if strand_shift == 1 and qidx & 1 else b"+")
        else:
            v = {QIDX: qidx, SEQ_ID: seq_id, POS: (int(rec["pos"]) + pos_add) & MASK, ERRORS: int(rec["errors"]), HIT: int(rec["hit"]), READ: read}[c]
            parts.append(b"%d" % v)
    text = sep.join(parts) + b"\n"
    return "long" if len(text) >= 1 << 32 else text


def format_positions(records, cols=(QIDX, SEQ_ID, POS, ERRORS), sep=b" ", strand_shift=0, name_stop=False, pos_add=0, read_names=None, seq_names=None):
    """(text, line offsets: len(records) + 1 entries, the last one len(text)).  An offending record raises FormatError: a row beyond its table or a span beyond the bytes
    anywhere in the batch goes first (INVALID, the lowest such record), then a name of 2^31 bytes (UNSUPPORTED)."""
    lines = [line(r, cols, sep, strand_shift, name_stop, pos_add, read_names, seq_names) for r in records]
    for words, code in ((("row", "span"), INVALID), (("long",), UNSUPPORTED)):
        for i, got in enumerate(lines):
            if isinstance(got, str) and got in words:
                raise FormatError(code, i, got)
    offsets = [0]
    for got in lines:
        offsets.append(offsets[-1] + len(got))
    return b"".join(lines), offsets
