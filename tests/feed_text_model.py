"""The piece rule of fmgpu_feed_map_text (include/fmgpu.h, "Pieces") in plain Python: tests/parse_model.parse looped over the pieces with the carry.  Window c is
text[c B, min((c + 1) B, n)); piece c is what piece c - 1 left unconsumed followed by window c, parsed under the rules of fmgpu_queries_parse, `final` only for the last
window of a final text.  What only later bytes can settle a piece in front of the last one leaves alone (`settled`)."""
from tests import parse_model as model
from tests.parse_model import LINES, FASTA, FASTQ


def windows(nbytes, B):
    return -(-nbytes // B)


def settled(piece, fmt):
    """the prefix of a piece in front of the last one which is parsed; the bytes behind it wait for the next window.
    FASTA: a last line that is a lone '\\r' so far may be the start of an empty line's "\\r\\n" (parsed now, it would be text in front of the first header).
    FASTQ: records that lie wholly or partly in empty lines at the very end of the piece are not records yet: a final text discards such lines, so whether they hold
    a record or truncate one depends on what follows."""
    if fmt == FASTA and piece.endswith(b"\r") and (len(piece) == 1 or piece[-2:-1] == b"\n"):
        return len(piece) - 1
    if fmt == FASTQ:
        lines, terminated = model.split_lines(piece, True)
        nonempty = max((l + 1 for l, (s, e) in enumerate(lines) if e > s), default=0)
        records = min(terminated, nonempty) // 4
        return lines[4 * records][0] if 4 * records < len(lines) else len(piece)
    return len(piece)


def parse_pieces(text, fmt, table, final, B):
    """model.Parsed of the whole text, assembled piece by piece; .windows = the number of windows, .pieces = [(start, end, final)] of every piece that ran"""
    text = bytes(text)
    n = len(text)
    res = model.Parsed()
    res.windows, res.pieces = windows(n, B), []
    start = line_base = 0
    for c in range(res.windows):
        end = min((c + 1) * B, n)
        last = bool(final) and c + 1 == res.windows
        piece = text[start:end]
        res.pieces.append((start, end, last))
        sub = model.parse(piece[: settled(piece, fmt)] if c + 1 < res.windows else piece, fmt, table, last)
        res.reads += sub.reads
        res.names += [(o + start, ln) if fmt != LINES else (o, ln) for o, ln in sub.names]
        res.quals += [(o + start, ln) if fmt == FASTQ else (o, ln) for o, ln in sub.quals]
        res.foreign += sub.foreign
        if sub.error_line is not None:
            res.error_line, res.error_offset = line_base + sub.error_line, start + sub.error_offset
            res.consumed = start + sub.consumed
            return res
        line_base += piece[: sub.consumed].count(b"\n") + (1 if sub.consumed and not piece[: sub.consumed].endswith(b"\n") else 0)
        start += sub.consumed
    res.consumed = start
    return res
