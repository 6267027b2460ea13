"""The device inflater for any DEFLATE stream (csrc/inflate_any.hip; ``deflate.inflate_any``) restated in plain Python, stage by
stage, from RFC 1951 / RFC 1952 and the format notes of include/e2e_hip.h (N9): ``find`` (where non-final dynamic blocks start,
first per segment), ``count`` (one record per span), ``write`` (16-bit symbols: a byte, or ``0x8000 | j`` = byte j of the 32 KiB in
front of the span), ``windows`` (the recurrence down the chain of spans), ``resolve``, the gzip member header, and the gap rule.
tests/test_inflate_any_cpu.py pins all of it to zlib; tests/test_gpu_inflate_any.py compares the kernels with it word for word.

Bit p of a stream is bit p mod 8, least significant first, of byte p // 8; bytes behind the end read as zero."""
import struct

import numpy as np

W = 32768
MARKER = 0x8000
RECORD_WORDS = 8
(OK, BTYPE, HEADER, NO_SYMBOL, SYMBOL, DISTANCE, STORED, FINAL, BEHIND, OVERSHOOT, CAP, LENGTH, REACH, START) = range(14)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


class Bits:
    def __init__(self, data, pos):
        self.data, self.pos = bytes(data), int(pos)

    def peek(self, k):
        """the next k <= 48 bits as an integer, first bit lowest"""
        at = self.pos >> 3
        return (int.from_bytes(self.data[at:at + 8], "little") >> (self.pos & 7)) & ((1 << k) - 1)

    def take(self, k):
        v = self.peek(k)
        self.pos += k
        return v


def kraft_left(lens, maxbits):
    """what a set of code lengths leaves of the code space, in units of 2^-maxbits: < 0 over-subscribed, 0 complete"""
    return (1 << maxbits) - sum(1 << (maxbits - l) for l in lens if l)


def canonical(lens):
    """{(length, code): symbol} of the canonical Huffman code (RFC 1951, 3.2.2)"""
    code, table = 0, {}
    for length in range(1, 16):
        for s, l in enumerate(lens):
            if l == length:
                table[(length, code)] = s
                code += 1
        code <<= 1
    return table


def decode(bits, table, maxbits=15):
    """one symbol, bit by bit (Huffman codes are packed most significant bit first); None: no such code within maxbits bits"""
    code = 0
    for length in range(1, maxbits + 1):
        code = (code << 1) | ((bits.peek(length) >> (length - 1)) & 1)
        if (length, code) in table:
            bits.pos += length
            return table[(length, code)]
    return None


def dynamic_tables(bits):
    """The code lengths of a dynamic block whose three header bits have been read: (literal/length lengths, distance lengths), or
    None where a rule fails: HLIT > 29, HDIST > 29; a code-length code that is not complete; a bit pattern without a symbol; a
    repeat of nothing; a run over HLIT + HDIST; no code for 256; a literal/length code that is not complete; a distance code that is
    over-subscribed, or incomplete other than by having no code at all or one code of length 1."""
    hlit, hdist, hclen = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
    if hlit > 286 or hdist > 30:
        return None
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = bits.take(3)
    if kraft_left(cl, 7) != 0:
        return None
    table = canonical(cl)
    lens = []
    while len(lens) < hlit + hdist:
        s = decode(bits, table, 7)
        if s is None:
            return None
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                return None
            rep, val = 3 + bits.take(2), lens[-1]
        elif s == 17:
            rep, val = 3 + bits.take(3), 0
        else:
            rep, val = 11 + bits.take(7), 0
        if len(lens) + rep > hlit + hdist:
            return None
        lens += [val] * rep
    ll, d = lens[:hlit], lens[hlit:]
    if ll[256] == 0 or kraft_left(ll, 15) != 0:
        return None
    left = kraft_left(d, 15)
    used = [l for l in d if l]
    if left < 0 or (left > 0 and not (used == [] or used == [1])):
        return None
    return ll, d


def header_valid(data, pos):
    """a non-final dynamic block header is valid at bit ``pos`` and ends inside the stream"""
    bits = Bits(data, pos)
    if bits.take(3) != 4:                              # BFINAL 0, then BTYPE 10 least significant bit first
        return False
    return dynamic_tables(bits) is not None and bits.pos <= 8 * len(data)


def valid_headers(data):
    """every bit position of the stream at which ``header_valid`` holds, ascending (the three header bits and HLIT / HDIST are
    tested for all positions at once, the rest position by position)"""
    n = len(data)
    if n == 0:
        return []
    bit = np.unpackbits(np.concatenate([np.frombuffer(bytes(data), dtype=np.uint8), np.zeros(4, dtype=np.uint8)]), bitorder="little")
    p = np.arange(8 * n)
    hlit = sum(bit[p + 3 + i].astype(np.int64) << i for i in range(5))
    hdist = sum(bit[p + 8 + i].astype(np.int64) << i for i in range(5))
    cand = np.flatnonzero((bit[p] == 0) & (bit[p + 1] == 0) & (bit[p + 2] == 1) & (hlit <= 29) & (hdist <= 29))
    return [int(q) for q in cand if header_valid(data, int(q))]


def find(data, segment_bytes, headers=None):
    """``starts`` as ``e2e_inflate_find`` leaves them (int64 [nseg], -1: none in the segment), with starts[0] = 0 as the host sets it"""
    n, S = len(data), int(segment_bytes)
    nseg = -(-n // S)
    starts = np.full(max(nseg, 1), -1, dtype=np.int64)
    starts[0] = 0
    for q in (valid_headers(data) if headers is None else headers):
        s = q // (8 * S)
        if s >= 1 and starts[s] < 0:
            starts[s] = q
    return starts[:max(nseg, 1)] if nseg else starts[:1]


def compact(starts):
    return np.asarray([int(s) for s in starts if s >= 0], dtype=np.int64)


def gaps_ok(starts, n, max_span_bytes):
    """the gap rule: every span, the last one to the stream's end, has at most max_span_bytes compressed bytes"""
    edges = [int(s) for s in starts] + [8 * int(n)]
    return all(b - a <= 8 * int(max_span_bytes) for a, b in zip(edges, edges[1:]))


def largest_gap(starts, n):
    edges = [int(s) for s in starts] + [8 * int(n)]
    return max(b - a for a, b in zip(edges, edges[1:]))


class _Fail(Exception):
    pass


def parse_span(data, start, nxt, max_span_bytes, off=None, max_out=None):
    """Whole blocks from bit ``start`` until one ends at ``nxt`` (None: until the final block, which must end in the last byte).
    Returns ``(status, final, end, outlen, symbols)``; ``symbols`` (a list, only when ``off`` -- the span's absolute output
    position -- is given) holds bytes and markers.  A failed span reports only its status."""
    n = len(data)
    if start < 0 or start >= 8 * n:
        return START, 0, 0, 0, []
    bits = Bits(data, start)
    limit = 8 * int(max_span_bytes) + 64
    writing = off is not None
    out, rounds, p = [], 0, 0

    def fail(code):
        raise _Fail(code)

    try:
        while True:
            rounds += 1
            if rounds > limit:
                fail(CAP)
            final, btype = bits.take(1), bits.take(2)
            if btype == 3:
                fail(BTYPE)
            if final and nxt is not None:
                fail(FINAL)
            if btype == 0:
                bits.pos = (bits.pos + 7) & ~7
                length, nlength = bits.take(16), bits.take(16)
                if length != (~nlength & 0xFFFF):
                    fail(STORED)
                payload = bits.pos >> 3
                if payload + length > n:
                    fail(BEHIND)
                if max_out is not None and p + length > max_out:
                    fail(LENGTH)
                if writing:
                    out += list(data[payload:payload + length])
                p += length
                bits.pos = 8 * (payload + length)
            else:
                if btype == 1:
                    ll, d = FIXED_LL, FIXED_D
                else:
                    tables = dynamic_tables(bits)
                    if tables is None:
                        fail(HEADER)
                    ll, d = tables
                ll_table, d_table = canonical(ll), canonical(d)
                while True:
                    rounds += 1
                    if rounds > limit:
                        fail(CAP)
                    s = decode(bits, ll_table)
                    if s is None:
                        fail(NO_SYMBOL)
                    if s < 256:
                        if max_out is not None and p >= max_out:
                            fail(LENGTH)
                        if writing:
                            out.append(s)
                        p += 1
                        continue
                    if s == 256:
                        break
                    if s >= 286:
                        fail(SYMBOL)
                    if s < 265:
                        length = s - 254
                    elif s == 285:
                        length = 258
                    else:
                        eb = (s - 261) >> 2
                        length = 3 + ((4 + ((s - 261) & 3)) << eb) + bits.take(eb)
                    dc = decode(bits, d_table)
                    if dc is None:
                        fail(NO_SYMBOL)
                    if dc >= 30:
                        fail(DISTANCE)
                    dist = dc + 1
                    if dc >= 4:
                        eb = (dc >> 1) - 1
                        dist = 1 + ((2 + (dc & 1)) << eb) + bits.take(eb)
                    if max_out is not None and p + length > max_out:
                        fail(LENGTH)
                    if writing:
                        if off + p - dist < 0:
                            fail(REACH)
                        for i in range(length):
                            q = p - dist + i
                            out.append((MARKER | (W + q)) if q < 0 else out[q])
                    p += length
            at = bits.pos
            if at > 8 * n:
                fail(BEHIND)
            if at - start > 8 * int(max_span_bytes):
                fail(CAP)
            if final:
                if (at + 7) // 8 != n:
                    fail(FINAL)
                return OK, 1, at, p, out
            if nxt is not None and at == nxt:
                return OK, 0, at, p, out
            if nxt is not None and at > nxt:
                fail(OVERSHOOT)
    except _Fail as e:
        return e.args[0], 0, 0, 0, []


def record_words(status, final, end, outlen):
    return [status, final, end & 0xFFFFFFFF, end >> 32, outlen & 0xFFFFFFFF, outlen >> 32, 0, 0]


def count(data, starts, max_span_bytes):
    """the records of ``e2e_inflate_spans_count``: uint32 [m, 8]"""
    starts = [int(s) for s in starts]
    rows = []
    for k, s in enumerate(starts):
        status, final, end, outlen, _ = parse_span(data, s, starts[k + 1] if k + 1 < len(starts) else None, max_span_bytes)
        rows.append(record_words(status, final, end, outlen))
    return np.asarray(rows, dtype=np.uint32).reshape(len(starts), RECORD_WORDS)


def unpack_records(records):
    """(status, final, end, outlen) as int64 arrays"""
    r = np.asarray(records, dtype=np.uint32).reshape(-1, RECORD_WORDS).astype(np.int64)
    return r[:, 0], r[:, 1], r[:, 2] | (r[:, 3] << 32), r[:, 4] | (r[:, 5] << 32)


def offsets(lengths):
    """the exclusive prefix sum with the total behind it: int64 [m + 1]"""
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def write(data, starts, offs, max_span_bytes):
    """``(sym uint16 [offs[-1]], bad)``: the symbols of every span at its offset; ``bad`` counts the spans that are invalid, reach in
    front of position 0 or give another length than their offsets say (here nothing of theirs is written and 0xFFFF stays; the
    device may have stored symbols of such a span before it failed, inside the span's own range)"""
    starts, offs = [int(s) for s in starts], [int(o) for o in offs]
    sym = np.full(offs[-1], 0xFFFF, dtype=np.uint16)
    bad = 0
    for k, s in enumerate(starts):
        want = offs[k + 1] - offs[k]
        status, _, _, outlen, out = parse_span(data, s, starts[k + 1] if k + 1 < len(starts) else None, max_span_bytes, offs[k], want)
        if status != OK or outlen != want:
            bad += 1
        else:
            sym[offs[k]:offs[k + 1]] = out
    return sym, bad


def windows(sym, offs):
    """``(wins uint8 [m, W], bad)``: wins[k][j], k >= 1, is the byte at offs[k] - W + j (0 in front of the output), by the
    recurrence: carried over from wins[k - 1] where span k - 1 is shorter than W, else the symbol, resolved through wins[k - 1]
    where it is a marker.  Row 0 is zero and unused.  ``bad``: a marker in span 0."""
    offs = [int(o) for o in offs]
    m = len(offs) - 1
    wins = np.zeros((m, W), dtype=np.uint8)
    bad = 0
    for k in range(1, m):
        plen = offs[k] - offs[k - 1]
        keep = max(W - plen, 0)                        # j < keep: carried over; j >= keep: symbol offs[k] - W + j
        wins[k, :keep] = wins[k - 1, plen:plen + keep]
        s = np.asarray(sym[offs[k] - W + keep:offs[k]], dtype=np.int64)
        marked = (s & MARKER) != 0
        bad += int(k == 1 and marked.any())
        wins[k, keep:] = np.where(marked, wins[k - 1, s & 0x7FFF], s & 0xFF)
    return wins, int(bad > 0)


def resolve(sym, offs, wins):
    """the output bytes: a symbol, or the byte of the window of the last span that starts at or before the position"""
    offs = np.asarray(offs, dtype=np.int64)
    sym = np.asarray(sym, dtype=np.int64)
    out = (sym & 0xFF).astype(np.uint8)
    marked = np.flatnonzero(sym & MARKER)
    k = np.searchsorted(offs[:-1], marked, side="right") - 1
    out[marked] = wins[k, sym[marked] & 0x7FFF]
    return out


def inflate(data, segment_bytes, max_span_bytes=None, headers=None):
    """every stage in a row: the inflated bytes, or None by the rules of ``deflate.inflate_any`` (without ``nbytes``)"""
    cap = 8 * segment_bytes if max_span_bytes is None else max_span_bytes
    starts = compact(find(data, segment_bytes, headers))
    if not gaps_ok(starts, len(data), cap):
        return None
    status, final, end, lengths = unpack_records(count(data, starts, cap))
    if status.any() or not final[-1]:
        return None
    offs = offsets(lengths)
    sym, bad = write(data, starts, offs, cap)
    assert bad == 0
    wins, bad = windows(sym, offs)
    assert bad == 0
    return resolve(sym, offs, wins).tobytes()


# ------------------------------------------------------------------------------------------------------------------------- gzip
def gzip_member(data):
    """``(offset of the raw stream, crc32, isize)`` of a file that holds one gzip member (RFC 1952), the trailer read from the
    file's last 8 bytes.  ValueError: no magic, CM != 8, a reserved flag bit, a header or trailer that runs over the file's end."""
    data = bytes(data)
    if len(data) < 18 or data[:2] != b"\x1f\x8b":
        raise ValueError("no gzip member")
    if data[2] != 8:
        raise ValueError("compression method %d" % data[2])
    flags = data[3]
    if flags & 0xE0:
        raise ValueError("reserved flag bits")
    at = 10
    if flags & 4:                                      # FEXTRA
        at += 2 + struct.unpack("<H", data[at:at + 2])[0]
    for bit in (8, 16):                                # FNAME, FCOMMENT: zero-terminated
        if flags & bit:
            at = data.index(b"\x00", at) + 1
    if flags & 2:                                      # FHCRC
        at += 2
    if at + 8 > len(data):
        raise ValueError("the header runs over the end")
    crc, isize = struct.unpack("<II", data[-8:])
    return at, crc, isize
