"""The device inflater (csrc/inflate.hip, ``e2e_inflate_scan`` / ``e2e_inflate_chunks``) restated in Python: one chunk record parsed
at a byte offset, with the rules of include/e2e_hip.h (N8) for what is invalid, and a whole-stream ``inflate`` on top of it.  Slow;
small inputs only.  No device is needed to import or run it.

An output byte is an int, or ``Front(j)``: byte j of the 8 bytes in front of the record, which the parser does not know when it
scans.  A match copies whatever stands d places back, so the dependence travels with the value."""
import struct

import numpy as np

CHUNK = 32768
TAIL = 8
STORED, FIXED, DYNAMIC = 0, 1, 2
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DISTANCES = {0: (1, 0), 1: (2, 0), 3: (4, 0), 5: (7, 1)}          # distance code -> (base, extra bits); only 1, 2, 4, 8 are valid


class Invalid(Exception):
    pass


class Front(int):
    """byte j of the 8 bytes in front of the record"""

    def __repr__(self):
        return "Front(%d)" % int(self)


class _Reader:
    """bits least significant first; bytes behind the end read as zero (the record is invalid if it ends there)"""

    def __init__(self, data, start):
        self.data, self.bit = data, 8 * start

    def peek(self, n):
        """n <= 24 bits without taking them"""
        byte = self.bit >> 3
        return (int.from_bytes(self.data[byte:byte + 4], "little") >> (self.bit & 7)) & ((1 << n) - 1)

    def take(self, n):
        v = self.peek(n)
        self.bit += n
        return v

    def align(self):
        self.bit = (self.bit + 7) & ~7

    def symbol(self, code):
        """code: (table over the next maxlen bits of (symbol, length) or None, maxlen)"""
        table, maxlen = code
        e = table[self.peek(maxlen)]
        if e is None:
            raise Invalid("no symbol")
        self.bit += e[1]
        return e[0]


def _code(lengths, what):
    """The canonical code of RFC 1951 3.2.2 as a lookup over its longest length, what is left of the code space (< 0
    over-subscribed, > 0 incomplete) and the codes per length"""
    count = [0] * 16
    for v in lengths:
        count[v] += 1
    left = 1
    for length in range(1, 16):
        left = 2 * left - count[length]
        if left < 0:
            raise Invalid("%s code over-subscribed" % what)
    nxt, code = [0] * 16, 0
    for length in range(1, 16):
        code = (code + (count[length - 1] if length > 1 else 0)) << 1
        nxt[length] = code
    maxlen = max(lengths)
    table = [None] * (1 << maxlen)
    for s, v in enumerate(lengths):
        if v:
            first = int(format(nxt[v], "0%db" % v)[::-1], 2)            # Huffman codes go most significant bit first
            table[first::1 << v] = [(s, v)] * (1 << (maxlen - v))
            nxt[v] += 1
    return (table, maxlen), left, count


def parse_record(data, start, front=None):
    """One record at ``data[start:]``: a dict of ``end``, ``length``, ``kind``, ``d`` (0 without a match), ``reach`` (bytes read in
    front of the record) and ``out``, the output bytes (ints, and ``Front(j)`` where ``front`` is None).  Raises ``Invalid``."""
    if not 0 <= start < len(data):
        raise Invalid("start outside the stream")
    r = _Reader(data, start)
    if r.take(1):
        raise Invalid("BFINAL")
    btype = r.take(2)
    if btype == 3:
        raise Invalid("BTYPE 11")
    if btype == 0:
        r.align()
        length, nlength = r.take(16), r.take(16)
        if length != (~nlength & 0xFFFF) or not 0 < length <= CHUNK:
            raise Invalid("stored LEN")
        first = start + 5
        if first + length > len(data):
            raise Invalid("stored block runs past the stream")
        return {"end": first + length, "length": length, "kind": STORED, "d": 0, "reach": 0, "out": list(data[first:first + length])}
    if btype == 1:
        ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
        dl = [5] * 30 + [0] * 2
    else:
        hlit, hdist, hclen = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
        if hlit > 286 or hdist > 30:
            raise Invalid("HLIT / HDIST")
        cl = [0] * 19
        for k in range(hclen):
            cl[CL_ORDER[k]] = r.take(3)
        cl_code, left, _ = _code(cl, "code-length")
        if left:
            raise Invalid("code-length code incomplete")
        seq = []
        while len(seq) < hlit + hdist:
            s = r.symbol(cl_code)
            if s < 16:
                seq.append(s)
                continue
            if s == 16:
                if not seq:
                    raise Invalid("repeat of nothing")
                rep, val = 3 + r.take(2), seq[-1]
            elif s == 17:
                rep, val = 3 + r.take(3), 0
            else:
                rep, val = 11 + r.take(7), 0
            if len(seq) + rep > hlit + hdist:
                raise Invalid("lengths run over")
            seq += [val] * rep
        ll, dl = seq[:hlit] + [0] * (288 - hlit), seq[hlit:] + [0] * (32 - hdist)
        if ll[256] == 0:
            raise Invalid("no end-of-block code")
    ll_code, left, _ = _code(ll, "literal/length")
    if left:
        raise Invalid("literal/length code incomplete")
    d_code, left, count = _code(dl, "distance")
    if left and btype == 2 and not (sum(count[1:]) == 0 or (sum(count[1:]) == 1 and count[1] == 1)):
        raise Invalid("distance code incomplete")

    known = front is not None
    out = [Front(j) for j in range(TAIL)] if not known else list(front)        # the 8 bytes in front, then the record's
    assert len(out) == TAIL
    d_rec = reach = 0
    while True:
        s = r.symbol(ll_code)
        if s < 256:
            if len(out) - TAIL >= CHUNK:
                raise Invalid("more than a chunk")
            out.append(s)
            continue
        if s == 256:
            break
        if s > 285:
            raise Invalid("symbol > 285")
        length = LEN_BASE[s - 257] + r.take(LEN_EXTRA[s - 257])
        dc = r.symbol(d_code)
        if dc > 29 or dc not in DISTANCES:
            raise Invalid("distance code")
        d = DISTANCES[dc][0] + r.take(DISTANCES[dc][1])
        if d not in (1, 2, 4, 8) or (d_rec and d != d_rec):
            raise Invalid("distance")
        d_rec = d
        pos = len(out) - TAIL
        if pos + length > CHUNK:
            raise Invalid("more than a chunk")
        reach = max(reach, d - pos)
        for _ in range(length):
            out.append(out[-d])
    if r.take(3):
        raise Invalid("closing block header")
    r.align()
    if r.take(16) != 0 or r.take(16) != 0xFFFF:
        raise Invalid("closing block")
    end = r.bit >> 3
    if len(out) == TAIL or end > len(data):
        raise Invalid("empty record, or one that ends behind the stream")
    return {"end": end, "length": len(out) - TAIL, "kind": btype, "d": d_rec, "reach": reach, "out": out[TAIL:]}


def record_words(data, start):
    """the 8 words ``e2e_inflate_scan`` writes for the candidate ``start``"""
    try:
        r = parse_record(data, start)
    except Invalid:
        return [1, 0, 0, 0, 0, 0, 0, 0]
    tail = ([Front(j) for j in range(TAIL)] + r["out"])[-TAIL:]
    vals = bytes(0 if isinstance(b, Front) else b for b in tail)
    deps = sum((int(b) if isinstance(b, Front) else 15) << (4 * i) for i, b in enumerate(tail))
    lo, hi = struct.unpack("<II", vals)
    return [0, r["kind"] | (r["d"] << 8) | (r["reach"] << 16), r["length"], r["end"] & 0xFFFFFFFF, r["end"] >> 32, lo, hi, deps]


def scan(stream, starts):
    """the ``scan=`` hook of ``deflate.inflate`` / ``deflate.inflate_plan``"""
    data = bytes(stream)
    return np.array([record_words(data, int(s)) for s in starts], dtype=np.uint32).reshape(len(starts), 8)


def chunks(stream, starts, prev_tails, nbytes):
    """the ``chunks=`` hook: every record parsed with its resolved front bytes, on its own"""
    data = bytes(stream)
    out = bytearray()
    for k, s in enumerate(starts):
        try:
            r = parse_record(data, int(s), front=[int(v) for v in prev_tails[k]])
        except Invalid:
            raise ValueError("inflate: record %d is corrupt" % k) from None
        if k == 0 and r["reach"] > 0 or r["length"] != min(CHUNK, nbytes - CHUNK * k):
            raise ValueError("inflate: record %d is corrupt" % k)
        out += bytes(r["out"])
    return bytes(out)


def inflate(stream, nbytes):
    """``stream`` (the records without the closing 03 00) inflated record after record, every record seeing the output so far"""
    data = bytes(stream)
    out, at = bytearray(), 0
    while len(out) < nbytes:
        r = parse_record(data, at, front=list(bytes(TAIL) + bytes(out))[-TAIL:])
        if (not out and r["reach"] > 0) or r["length"] != min(CHUNK, nbytes - len(out)):
            raise Invalid("not a chain of whole chunks")
        out += bytes(r["out"])
        at = r["end"]
    if at != len(data):
        raise Invalid("bytes behind the last record")
    return bytes(out)
