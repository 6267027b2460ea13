"""The dynamic-Huffman chunk of the device DEFLATE encoder (csrc/deflate.hip, ``e2e_deflate_encode_dynamic``), restated in Python the
way ``tests.test_gpu_deflate.reference_stream`` restates the fixed format: the token list, the code lengths, the header and the bits.
Slow; small inputs only.  No device is needed to import or run it.

A chunk is the shortest of three forms: one stored block, the fixed-Huffman block (``reference_chunk``), or one dynamic block over
the same tokens; the dynamic form only when it is strictly shorter than both others.

Code lengths (``code_lengths``), for the literal/length code (286 symbols, at most 15 bits) and the code-length code (19 symbols, at
most 7 bits) alike:
  1. the used symbols are ordered by count descending, equal counts by symbol number ascending;
  2. the counts in ascending order go through the two-queue Huffman construction (Moffat and Katajainen's in-place form); when an
     internal node and a leaf weigh the same the leaf is taken first.  Only the number of leaves per depth is kept;
  3. leaves deeper than the limit are counted at the limit, which over-subscribes the code: the Kraft sum exceeds 1 by a whole number
     of 2^-limit.  Once per such unit (the step of zlib's gen_bitlen): the deepest level below the limit that has a leaf gives one
     up, which becomes an internal node with two leaves one level down, one of them taken from the limit's level.  A step lowers
     the sum by exactly 2^-limit, so the code ends complete;
  4. the lengths are dealt out along the order of 1, shortest first: of two symbols with equal counts the one with the smaller
     number never has the longer code.
A single used symbol gets length 1 (it cannot happen for the two codes above: a chunk has a literal or a match and symbol 256; its
length sequence has a non-zero length and a zero or a repeat)."""
import functools

import numpy as np

from tests.test_gpu_deflate import CHUNK, _Bits, _DIST, _LEN_BASE, _LEN_EXTRA, reference_chunk

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
STORED, FIXED, DYNAMIC = 0, 1, 2


def tokens(data, start, stop, elem):
    """the fixed route's tokens of data[start:stop]: ``v`` (0..255) a literal, ``-length`` a match of distance elem"""
    out = []
    i = start
    while i < stop:
        j = i
        while j < stop and j >= elem and data[j] == data[j - elem]:
            j += 1
        if j == i:
            out.append(data[i])
            i += 1
            continue
        run = j - i
        while run >= 258:
            out.append(-258)
            run -= 258
        if run >= 3:
            out.append(-run)
        else:
            out.extend(data[j - run:j])
        i = j
    return out


def length_symbol(length):
    """(symbol, extra bits, extra value) of a match length"""
    i = max(k for k in range(29) if _LEN_BASE[k] <= length) if length < 258 else 28
    return 257 + i, _LEN_EXTRA[i], length - _LEN_BASE[i]


def code_lengths(counts, limit):
    lengths = [0] * len(counts)
    order = sorted((s for s in range(len(counts)) if counts[s]), key=lambda s: (-counts[s], s))
    n = len(order)
    if n == 0:
        return lengths
    if n == 1:
        lengths[order[0]] = 1
        return lengths
    a = [counts[s] for s in reversed(order)]                # ascending
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1                              # depths of the internal nodes
    bl = [0] * (limit + 1)
    avbl, depth, root = 1, 0, n - 2
    while avbl > 0:
        used = 0
        while root >= 0 and a[root] == depth:
            used += 1
            root -= 1
        leaves = avbl - used
        bl[min(depth, limit)] += leaves
        avbl, depth = 2 * used, depth + 1
    excess = sum(bl[d] << (limit - d) for d in range(1, limit + 1)) - (1 << limit)      # of the Kraft sum, in units of 2^-limit
    while excess > 0:
        bits = limit - 1
        while bl[bits] == 0:
            bits -= 1
        bl[bits] -= 1
        bl[bits + 1] += 2
        bl[limit] -= 1
        excess -= 1
    at = 0
    for length in range(1, limit + 1):
        for s in order[at:at + bl[length]]:
            lengths[s] = length
        at += bl[length]
    assert at == n
    return lengths


def canonical(lengths):
    """RFC 1951 3.2.2"""
    top = max(lengths) if lengths else 0
    bl = [0] * (top + 2)
    for v in lengths:
        if v:
            bl[v] += 1
    nxt, code = [0] * (top + 2), 0
    for bits in range(1, top + 1):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(lengths)
    for s, v in enumerate(lengths):
        if v:
            codes[s] = nxt[v]
            nxt[v] += 1
    return codes


def run_code(lengths):
    """one length sequence as (code-length symbol, extra bits, extra value): zlib's scan_tree / send_tree"""
    out = []
    prev, count = -1, 0
    seq = list(lengths) + [-1]
    nextlen = seq[0]
    max_count, min_count = (138, 3) if nextlen == 0 else (7, 4)
    for k in range(len(lengths)):
        cur, nextlen = nextlen, seq[k + 1]
        count += 1
        if count < max_count and cur == nextlen:
            continue
        if count < min_count:
            out += [(cur, 0, 0)] * count
        elif cur != 0:
            if cur != prev:
                out.append((cur, 0, 0))
                count -= 1
            out.append((16, 2, count - 3))
        elif count <= 10:
            out.append((17, 3, count - 3))
        else:
            out.append((18, 7, count - 11))
        count, prev = 0, cur
        if nextlen == 0:
            max_count, min_count = 138, 3
        elif cur == nextlen:
            max_count, min_count = 6, 3
        else:
            max_count, min_count = 7, 4
    return out


def dynamic_block(data, start, stop, elem):
    """``(bytes, info)`` of the dynamic form of the chunk data[start:stop]; info holds the lengths for the tests"""
    toks = tokens(data, start, stop, elem)
    counts = [0] * 286
    counts[256] = 1
    has_match = False
    for t in toks:
        if t >= 0:
            counts[t] += 1
        else:
            counts[length_symbol(-t)[0]] += 1
            has_match = True
    ll = code_lengths(counts, 15)
    ll_codes = canonical(ll)
    hlit = max(s for s in range(286) if ll[s]) + 1
    dcode, deb, dev = _DIST[elem]
    dl = [0] * dcode + [1] if has_match else [0]
    cl_tokens = run_code(ll[:hlit]) + run_code(dl)
    cl_counts = [0] * 19
    for s, _, _ in cl_tokens:
        cl_counts[s] += 1
    cl = code_lengths(cl_counts, 7)
    cl_codes = canonical(cl)
    hclen = max(k for k in range(19) if cl[CL_ORDER[k]]) + 1
    hclen = max(hclen, 4)
    b = _Bits()
    b.put(0, 1)                                     # BFINAL
    b.put(2, 2)                                     # BTYPE 10
    b.put(hlit - 257, 5)
    b.put(len(dl) - 1, 5)
    b.put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cl[CL_ORDER[k]], 3)
    for s, eb, ev in cl_tokens:
        b.huff(cl_codes[s], cl[s])
        b.put(ev, eb)
    for t in toks:
        if t >= 0:
            b.huff(ll_codes[t], ll[t])
        else:
            s, eb, ev = length_symbol(-t)
            b.huff(ll_codes[s], ll[s])
            b.put(ev, eb)
            b.huff(0, 1)                            # the one distance code
            b.put(dev, deb)
    b.huff(ll_codes[256], ll[256])                  # end of block
    b.put(0, 3)                                     # BFINAL 0, BTYPE 00
    b.align()
    return bytes(b.out) + b"\x00\x00\xff\xff", {"ll": ll, "cl": cl, "dl": dl, "counts": counts, "cl_counts": cl_counts}


def reference_chunk_dynamic(data, start, stop, elem):
    """``(bytes, kind)`` of the chunk"""
    n = stop - start
    other = reference_chunk(data, start, stop, elem)                # fixed, or stored where that is shorter
    kind = STORED if (len(other) == n + 5 and other[0] == 0) else FIXED
    dyn, _ = dynamic_block(data, start, stop, elem)
    return (dyn, DYNAMIC) if len(dyn) < len(other) else (other, kind)


def reference_chunks_dynamic(data, elem, chunk=CHUNK):
    data = bytes(data)
    return [reference_chunk_dynamic(data, c, min(c + chunk, len(data)), elem) for c in range(0, len(data), chunk)]


def reference_stream_dynamic(data, elem, chunk=CHUNK):
    return b"".join(c for c, _ in reference_chunks_dynamic(data, elem, chunk)) + b"\x03\x00"


# ------------------------------------------------------------------------------------------------------------------- the inputs

def _balls(seed=21, shape=(24, 64, 64), n=15):
    """a uint8 label volume: n balls of labels 1..n whose radius varies from voxel to voxel (ragged borders)"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*(np.arange(s, dtype=np.float32) for s in shape), indexing="ij")
    vol = np.zeros(shape, dtype=np.uint8)
    for k in range(n):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(4, 12) + rng.uniform(-1.5, 1.5, shape)
        vol[(z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 < r * r] = k + 1
    return vol


def _fibonacci(seed=5):
    """One chunk of 22 symbols with Fibonacci counts whose Huffman tree is deeper than 15 (19; the CPU test asserts it), shuffled.
    Symbol i = 1..20 occurs Fibonacci(i + 1) times (1, 2, 3, 5, ..., 10946) and the last two share what is left of CHUNK (2056 and
    2057).  The counts start at Fibonacci(2) because the end-of-block symbol adds a count of 1: with Fibonacci(1..22) every merge of
    the tree meets a leaf of its own weight, the construction takes the leaf first, and the tree is 12 deep.  They fill the chunk
    exactly because a shuffle cut at CHUNK keeps the counts only roughly (trees 12 to 16 deep).  After the shuffle every byte that
    is the third in a row to repeat the byte 1, 2 or 4 places back changes places with a random other byte, until no run is long
    enough for a match at any elem: matches would take their bytes out of the literal counts."""
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    rest = CHUNK - sum(fib)
    fib += [rest // 2, rest - rest // 2]
    buf = np.concatenate([np.full(c, 3 * i + 1, dtype=np.uint8) for i, c in enumerate(fib)])
    rng = np.random.default_rng(seed)
    rng.shuffle(buf)
    for _ in range(200):
        bad = np.zeros(CHUNK, dtype=bool)
        for d in (1, 2, 4):
            eq = np.zeros(CHUNK, dtype=bool)
            eq[d:] = buf[d:] == buf[:-d]
            bad[2:] |= eq[2:] & eq[1:-1] & eq[:-2]
        at = np.flatnonzero(bad)
        if at.size == 0:
            return buf
        for p, q in zip(at, rng.integers(0, CHUNK, at.size)):
            buf[p], buf[q] = buf[q], buf[p]
    raise AssertionError("the shuffle kept its runs")


@functools.lru_cache(maxsize=None)
def inputs():
    """{id: uint8 array}: the inputs of the CPU and GPU tests, all from fixed seeds"""
    rng = np.random.default_rng(1951)
    out = {}
    for n in (1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 6):
        out["a%d" % n] = np.full(n, 0x3C, dtype=np.uint8)
    out["b"] = rng.integers(0, 256, 40000, dtype=np.uint8)
    out["c"] = np.arange(256, dtype=np.uint8)
    out["d"] = np.minimum(rng.geometric(0.5, CHUNK) - 1, 255).astype(np.uint8)
    out["e"] = _fibonacci()
    balls = _balls()
    out["f"] = balls.reshape(-1)
    onehot = np.stack([(balls == k) for k in range(4)]).astype(np.float16)
    noise = rng.random(onehot.shape) < 0.2
    onehot[noise] = rng.random(int(noise.sum())).astype(np.float16)
    out["g"] = onehot.view(np.uint8).reshape(-1)
    out["h"] = rng.standard_normal(24576).astype(np.float32).view(np.uint8)
    out["i"] = np.concatenate([rng.integers(0, 256, CHUNK, dtype=np.uint8), np.full(CHUNK, 0x5A, dtype=np.uint8)])
    run = rng.integers(0, 256, 2 * CHUNK + 64, dtype=np.uint8)
    run[CHUNK - 8:CHUNK + 700] = np.tile(np.arange(1, 5, dtype=np.uint8), 177)
    out["j"] = run
    for v in out.values():
        v.setflags(write=False)
    return out


def cases():
    """(id, elem) of every case: each input at every elem of 1, 2, 4 that divides it, and one at 8"""
    out = [(k, e) for k, v in inputs().items() for e in (1, 2, 4) if v.size % e == 0]
    return out + [("j", 8)]


@functools.lru_cache(maxsize=None)
def reference(case, elem):
    """the chunks ``[(bytes, kind)]`` of one case, computed once per process"""
    return tuple(reference_chunks_dynamic(inputs()[case].tobytes(), elem))
