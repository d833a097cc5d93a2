"""Constructed DEFLATE streams and forced PNG scanline filters for the device PNG decoder (csrc/png_kernels.hip).

The decoder's other suite (`test_gpu_pngdec.py`) feeds it what Pillow writes, i.e. what zlib's encoder and Pillow's filter heuristic happen to
emit.  This module WRITES streams instead (RFC 1951): a bit writer, emitters for the three block forms with explicit code lengths and explicit
tokens, `stream(blocks)` (the DEFLATE body + the Adler-32 trailer: exactly what `pngdec` hands `mt4_png_inflate`), `census(stream)` -- a plain
inflate walker that reports which forms a stream contains -- and `CASES`, one table of named rows (name, builder, features) that
`test_deflate_streams_cpu.py` checks against zlib and `test_gpu_png_streams.py` runs through the kernel.  The census is the check that a row
tests what its name says: every feature a row lists must be found in its stream, and `REQUIRED` (every form the table exists for) must be
covered by the union.

The second half holds the scanline side: `unfilter_ref` (PNG specification 9.2 - 9.4 in numpy integer arithmetic), the forward filter, the
filter cases and a PNG file assembler with chosen IDAT splits.

A plain module beside `conv_tiles.py` (`tests/` is on sys.path while pytest runs), not a conftest.  Nothing here needs the library or a GPU.
"""
import functools
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30

# what the decoder's constants are (csrc/png_kernels.hip): the cases sit on their edges
WIN, FLUSH, NEAR = 8192, 4096, 8192 - 512


class BadLengths(ValueError):
    pass


class OverSubscribed(BadLengths):
    pass


class Incomplete(BadLengths):
    pass


# ------------------------------------------------------------------------------------------------------------------ writer

class BitWriter:
    """RFC 1951 3.1.1: fields go in LSB first, Huffman codes MSB first, both packed from the low bit of each byte"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n), (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        rev = 0
        for _ in range(n):
            rev = (rev << 1) | (code & 1)
            code >>= 1
        self.bits(rev, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def getvalue(self):
        assert self.n == 0
        return bytes(self.out)


def check_lengths(lengths, alphabet):
    """refuses what inflate refuses: an over-subscribed set; an incomplete one, except a distance alphabet with no code or with one code of
    length 1 (the two forms zlib's inflate_table lets through)"""
    top = 7 if alphabet == "codelen" else 15
    if any(l < 0 or l > top for l in lengths):
        raise BadLengths(f"{alphabet}: a length outside 0..{top}")
    kraft = sum(1 << (15 - l) for l in lengths if l)
    if kraft > 1 << 15:
        raise OverSubscribed(f"{alphabet}: over-subscribed")
    if kraft < 1 << 15:
        used = [l for l in lengths if l]
        if alphabet == "dist" and (not used or used == [1]):
            return
        raise Incomplete(f"{alphabet}: incomplete")


def canonical_codes(lengths):
    """RFC 1951 3.2.2: [(code, length) or None] per symbol"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if l:
            out.append((nxt[l], l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def balanced_lengths(n, used):
    """code lengths over an alphabet of n symbols: a complete code over `used` (most important first), two adjacent lengths"""
    used = list(used)
    k = len(used)
    assert k >= 2 and len(set(used)) == k
    m = k.bit_length() - 1
    short = (2 << m) - k
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = m if i < short else m + 1
    return lens


def rle(lengths):
    """greedy run-length coding of ONE sequence (RFC 1951 3.2.7): [(symbol, extra value or None)]"""
    out, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, None)] * run
        else:
            out.append((v, None))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
            out += [(v, None)] * run
        i = j
    return out


def _unrle(items):
    out = []
    for sym, extra in items:
        if sym < 16:
            out.append(sym)
        elif sym == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if sym == 17 else 11) + extra)
    return out


class Stored:
    def __init__(self, data=b""):
        assert len(data) <= 65535
        self.data = bytes(data)


class Coded:
    """a block of Huffman-coded tokens: a literal byte (int) or a (length, distance) pair; the end-of-block code is added by the writer"""

    def __init__(self, tokens):
        self.tokens = list(tokens)


class Fixed(Coded):
    pass


class Dynamic(Coded):
    """ll_lens: 257..286 literal/length code lengths; d_lens: 1..30 distance code lengths.  The code-length sequence is `cl_items` (symbol by
    symbol, [(symbol, extra)]) or, by default, the greedy run-length coding of ll_lens + d_lens as ONE array (so runs cross the boundary
    wherever the lengths allow).  The code-length code: a complete code over the symbols used (+ `cl_extra`), HCLEN at least `hclen`."""

    def __init__(self, ll_lens, d_lens, tokens, cl_items=None, hclen=4, cl_extra=()):
        super().__init__(tokens)
        self.ll_lens, self.d_lens, self.cl_items, self.hclen, self.cl_extra = list(ll_lens), list(d_lens), cl_items, hclen, tuple(cl_extra)


def _put_tokens(w, tokens, ll_codes, d_codes):
    def put(codes, sym):
        if sym >= len(codes) or codes[sym] is None:
            raise BadLengths(f"symbol {sym} has no code")
        w.code(*codes[sym])
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t
            assert 3 <= length <= 258 and 1 <= dist <= 32768
            ls = max(i for i in range(29) if LEN_BASE[i] <= length) if length < 258 else 28
            put(ll_codes, 257 + ls)
            w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
            put(d_codes, ds)
            w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        else:
            put(ll_codes, t)
    put(ll_codes, 256)


def emit(w, block, final):
    w.bits(1 if final else 0, 1)
    if isinstance(block, Stored):
        w.bits(0, 2)
        w.align()                      # 0..7 zero bits, whatever phase the header ended on
        w.bits(len(block.data), 16)
        w.bits(len(block.data) ^ 0xFFFF, 16)
        w.raw(block.data)
    elif isinstance(block, Fixed):
        w.bits(1, 2)
        _put_tokens(w, block.tokens, canonical_codes(FIXED_LL), canonical_codes(FIXED_D + [5, 5]))
    else:
        ll, d = block.ll_lens, block.d_lens
        if not (257 <= len(ll) <= 286 and 1 <= len(d) <= 30):
            raise BadLengths("HLIT / HDIST out of range")
        check_lengths(ll, "litlen")
        check_lengths(d, "dist")
        if not ll[256]:
            raise BadLengths("no end-of-block code")
        items = block.cl_items if block.cl_items is not None else rle(ll + d)
        if _unrle(items) != ll + d:
            raise BadLengths("the code-length sequence does not expand to the lengths")
        freq = {}
        for sym, _ in items:
            freq[sym] = freq.get(sym, 0) + 1
        used = sorted(freq, key=lambda s: (-freq[s], s)) + [s for s in block.cl_extra if s not in freq]
        if len(used) < 2:              # (a one-code code-length code is incomplete: inflate refuses it)
            used.append(next(s for s in CL_ORDER if s not in used))
        cl = balanced_lengths(19, used)
        check_lengths(cl, "codelen")
        hclen = max(block.hclen, 1 + max(i for i, s in enumerate(CL_ORDER) if cl[s]))
        w.bits(2, 2)
        w.bits(len(ll) - 257, 5)
        w.bits(len(d) - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl[s], 3)
        cl_codes = canonical_codes(cl)
        for sym, extra in items:
            w.code(*cl_codes[sym])
            if sym >= 16:
                w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
        _put_tokens(w, block.tokens, canonical_codes(ll), canonical_codes(d))


def body(blocks):
    w = BitWriter()
    for i, b in enumerate(blocks):
        emit(w, b, i == len(blocks) - 1)
    w.align()
    return w.getvalue()


def expand(blocks):
    """what the blocks say, from the tokens alone (no bit stream involved)"""
    out = bytearray()
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, tuple):
                length, dist = t
                assert dist <= len(out), "a match that reaches in front of the output"
                for _ in range(length):
                    out.append(out[-dist])
            else:
                out.append(t)
    return bytes(out)


def with_trailer(deflate_body, expected):
    return deflate_body + struct.pack(">I", zlib.adler32(expected))


def stream(blocks):
    """DEFLATE body + Adler-32 of the output: what `pngdec.parse_png` leaves of a zlib stream (header stripped, trailer kept -- the decoder's
    bit reader prefetches and is sound only because 32 bits follow the last block)"""
    return with_trailer(body(blocks), expand(blocks))


def built(blocks):
    return stream(blocks), expand(blocks)


# ------------------------------------------------------------------------------------------------------------------ census

class _Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def bits(self, n):
        v = 0
        for i in range(n):
            if self.pos >= 8 * len(self.data):
                raise EOFError("the stream ends inside a block")
            v |= ((self.data[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def sym(self, table):
        code = 0
        for length in range(1, 16):
            code = (code << 1) | self.bits(1)
            s = table.get((length, code))
            if s is not None:
                return s, length
        raise ValueError("a code that is not in the table")


def _table(lengths):
    return {(c[1], c[0]): s for s, c in enumerate(canonical_codes(lengths)) if c}


def census(data):
    """Inflate `data` (DEFLATE body + 4-byte trailer) the plain way and report what it is made of.  An invalid stream gives `error` and whatever
    was seen up to there.  Keys:
      blocks       [dict per block]: type, final, phase (bit position of its header mod 8), at (output offset where it starts); stored: len,
                   end (stream offset of the byte behind it); dynamic: hlit, hdist, hclen, crossing [(symbol, value)], dist_codes (lengths != 0);
                   coded: lits {code length: count}, lens / dists / eob: sets of the code lengths USED, matches [(offset, length, distance)]
      out          the output; adler_ok: the trailer is its Adler-32; nbytes: len(data)"""
    rep = dict(blocks=[], out=b"", error=None, adler_ok=False, nbytes=len(data))
    out = bytearray()
    try:
        r = _Bits(data[:-4])
        final = 0
        while not final:
            blk = dict(phase=r.pos & 7, at=len(out))
            final = r.bits(1)
            typ = r.bits(2)
            blk.update(final=final, type=("stored", "fixed", "dynamic", "reserved")[typ])
            rep["blocks"].append(blk)
            if typ == 3:
                raise ValueError("block type 3")
            if typ == 0:
                r.pos = (r.pos + 7) & ~7
                n, nn = r.bits(16), r.bits(16)
                if n ^ 0xFFFF != nn:
                    raise ValueError("stored length mismatch")
                start = r.pos >> 3
                if start + n > len(r.data):
                    raise EOFError("stored block longer than the stream")
                out += r.data[start:start + n]
                r.pos += 8 * n
                blk.update(len=n, end=start + n)
                continue
            if typ == 1:
                ll, d = FIXED_LL, FIXED_D + [5, 5]
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                blk.update(hlit=hlit, hdist=hdist, hclen=hclen, crossing=[])
                if hlit > 286 or hdist > 30:
                    raise ValueError("HLIT / HDIST out of range")
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = r.bits(3)
                check_lengths(cl, "codelen")
                ct = _table(cl)
                seq = []
                while len(seq) < hlit + hdist:
                    s, _ = r.sym(ct)
                    if s < 16:
                        seq.append(s)
                        continue
                    if s == 16:
                        if not seq:
                            raise ValueError("repeat with nothing before it")
                        val, rep_n = seq[-1], 3 + r.bits(2)
                    else:
                        val, rep_n = 0, (3 + r.bits(3) if s == 17 else 11 + r.bits(7))
                    if len(seq) < hlit < len(seq) + rep_n:
                        blk["crossing"].append((s, val))
                    if len(seq) + rep_n > hlit + hdist:
                        raise ValueError("a run past the end of the lengths")
                    seq += [val] * rep_n
                ll, d = seq[:hlit], seq[hlit:]
                if not ll[256]:
                    raise ValueError("no end-of-block code")
                check_lengths(ll, "litlen")
                check_lengths(d, "dist")
                blk["dist_codes"] = [l for l in d if l]
            lt, dt = _table(ll), _table(d)
            blk.update(lits={}, lens=set(), dists=set(), eob=set(), matches=[])
            while True:
                s, n = r.sym(lt)
                if s < 256:
                    out.append(s)
                    blk["lits"][n] = blk["lits"].get(n, 0) + 1
                elif s == 256:
                    blk["eob"].add(n)
                    break
                else:
                    if s > 285:
                        raise ValueError("length symbol 286 / 287")
                    blk["lens"].add(n)
                    length = LEN_BASE[s - 257] + r.bits(LEN_EXTRA[s - 257])
                    ds, n = r.sym(dt)
                    if ds > 29:
                        raise ValueError("distance symbol 30 / 31")
                    blk["dists"].add(n)
                    dist = DIST_BASE[ds] + r.bits(DIST_EXTRA[ds])
                    if dist > len(out):
                        raise ValueError("a match that reaches in front of the output")
                    blk["matches"].append((len(out), length, dist))
                    for _ in range(length):
                        out.append(out[-dist])
        rep["adler_ok"] = struct.unpack(">I", data[-4:])[0] == zlib.adler32(bytes(out))
    except (ValueError, EOFError) as e:
        rep["error"] = str(e)
    rep["out"] = bytes(out)
    return rep


def features(rep):
    """the census as a flat set of names: what rows list and `REQUIRED` asks for"""
    f = set()
    blocks = rep["blocks"]
    n = rep["nbytes"]
    f.add(f"streamlen%512={n % 512}/{'short' if n < 2048 else 'long'}")
    f.add(f"outlen={len(rep['out'])}")
    if sum(b["type"] == "stored" and b["len"] > 0 for b in blocks) >= 3 and all(b["type"] == "stored" for b in blocks):
        f.add("three_stored_blocks")
    if len(blocks) >= 8:
        f.add("many_blocks")
    matches = [m for b in blocks for m in b.get("matches", ())]
    if matches:
        f.add("matches")
        if all(d == 1 for _, _, d in matches):
            f.add("all_matches_at_distance_1")
        if max(d for _, _, d in matches) <= 512 - 262:
            f.add("all_matches_within_a_512_window")
    for i, b in enumerate(blocks):
        f.add(b["type"])
        if b["type"] == "stored":
            f.add(f"stored_phase{b['phase']}")
            f.add(f"stored_end%4={b['end'] % 4}")
            if b["len"] in (0, 1, 65535):
                f.add(f"stored_len{b['len']}")
            if b["len"] == 0:
                f.add("empty_stored")
            if b["at"] % 16 and b["at"] // WIN != (b["at"] + b["len"]) // WIN:
                f.add("stored_wraps_ring_unaligned")
            continue
        if i and b["phase"] == 0 and blocks[i - 1]["type"] == "stored":
            f.add("coded_block_on_a_byte_boundary")
        if b["type"] == "dynamic":
            for k in ("hlit", "hdist", "hclen"):
                f.add(f"{k}{b[k]}")
            for sym, val in b["crossing"]:
                f.add(f"cross{sym}")
                if sym == 16 and val:
                    f.add("cross16_nonzero")
            if not b["dist_codes"]:
                f.add("literal_only")
                if b["hdist"] == 1:
                    f.add("literal_only_hdist1")
            if b["dist_codes"] == [1]:
                f.add("single_dist_code")
                if b["matches"]:
                    f.add("single_dist_code_used")
            if not b["matches"]:
                f.add("dynamic_without_matches")
            if b["lits"].get(1, 0) >= 9000:
                if set(b["lits"]) == {1}:
                    f.add("walk_1bit")
                elif b["lits"].get(2, 0) >= 1000:
                    f.add("walk_1bit_2bit")
        for k, name in (("lits", "lit"), ("lens", "len"), ("eob", "eob"), ("dists", "dist")):
            for l in b[k]:
                f.add(f"{name}_code{l}")
        prev_stored = [p for p in blocks[:i] if p["type"] == "stored" and p["len"]]
        for at, length, dist in b["matches"]:
            f.add(f"match_at%4096={at % FLUSH}")
            if dist == 1 and length in (3, 258):
                f.add(f"match_len{length}_dist1")
            if dist == length:
                f.add("match_dist=len")
            if dist == length - 1:
                f.add("match_dist=len-1")
            if dist == at:
                f.add("match_back_to_byte0")
            if length == 258 and dist in (NEAR, NEAR + 1):
                f.add(f"match_len258_dist{dist}")
            if dist == 32768:
                f.add("match_dist32768")
            if dist > 32506:
                f.add("match_beyond_zlibs_reach")
            if length == 258 and at % FLUSH in (4095, 3839, 3838):
                f.add(f"match_len258_at{at % FLUSH}")
            if at + length == len(rep["out"]):
                f.add("match_ends_the_output")
            if dist > NEAR and at % FLUSH == 0:
                f.add("far_match_first_after_flush")
            for p in prev_stored:
                if p["at"] <= at - dist < p["at"] + p["len"]:
                    f.add("match_into_stored_far" if dist > NEAR else "match_into_stored_near")
    return f


# ------------------------------------------------------------------------------------------------------------------ the cases

def _rand(n, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def _scanlines(n):
    """what filtered video rows look like: a filter byte, then small signed differences"""
    rng = np.random.default_rng(11)
    rows = []
    while sum(map(len, rows)) < n:
        rows.append(bytes([int(rng.integers(0, 5))]) + (rng.normal(0, 3, 3 * 97).round().astype(np.int64) & 255).astype(np.uint8).tobytes())
    return b"".join(rows)[:n]


def _skewed(n):
    """one byte value 19 times in 20, the rest spread thin: very short and very long codes in one block"""
    rng = np.random.default_rng(12)
    return np.where(rng.random(n) < 0.95, 7, rng.integers(0, 256, n)).astype(np.uint8).tobytes()


def _zlib_case(data, flush_at=(), **kw):
    def build():
        c = zlib.compressobj(**{"wbits": -15, **kw})
        parts, last = [], 0
        for at, mode in flush_at:
            parts += [c.compress(data[last:at]), c.flush(mode)]
            last = at
        parts += [c.compress(data[last:]), c.flush()]
        return with_trailer(b"".join(parts), data), data
    return build


def _literals_dynamic(pattern):
    """a literal-only dynamic block: 'A' 1 bit; with 'B' in the pattern: 'B' 2 bits, 'C' and end-of-block 3 bits"""
    def build():
        ll = [0] * 257
        if b"B" in pattern:
            ll[65], ll[66], ll[67], ll[256] = 1, 2, 3, 3
        else:
            ll[65], ll[256] = 1, 1
        return built([Dynamic(ll, [0], list(pattern))])
    return build


def _fixed_literals(n):
    return lambda: built([Fixed(list(_rand(n, 100 + n)))])


def _blocks(*blocks):
    return lambda: built(list(blocks))


def _cross(kind):
    def build():
        if kind == 17:      # 3 zeros at the end of the literal/length lengths + the one distance length 0: ONE 17 run of 4
            ll = balanced_lengths(260, list(range(97, 123)) + [256])
            return built([Dynamic(ll, [0], list(b"thequickbrownfoxjumpsoverthelazydog"))])
        if kind == 18:      # 12 zeros behind length symbol 257, 3 zeros in front of the two distance codes: ONE 18 run of 15
            ll = balanced_lengths(270, list(range(97, 123)) + [256, 257])
            toks = list(b"abcdefghij") + [(3, 4), (3, 5)] + list(b"xyz")
            return built([Dynamic(ll, [0, 0, 0, 1, 1], toks)])
        # 16: 'a' 1 bit, 'b' 2 bits, end-of-block and length symbol 257 3 bits; eight distance codes of 3 bits.  The greedy coder sends the 3 of
        # symbol 256 and then a 16 run of six: the 3 of symbol 257 and five DISTANCE lengths
        ll = [0] * 258
        ll[97], ll[98], ll[256], ll[257] = 1, 2, 3, 3
        toks = list(b"abbaabab") + [(3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 7), (3, 8)] + list(b"ba")
        return built([Dynamic(ll, [3] * 8, toks)])
    return build


def _smallest_header():
    """HLIT 257 / HDIST 1 and the smallest HCLEN a VALID block can have: 5.  With HCLEN 4 only the code-length symbols 16, 17, 18 and 0 have a
    code, so every length is 0 and there is no end-of-block code (`REJECTED` holds that block).  Symbol 8 is fifth in the order: 255 literals
    and end-of-block at 8 bits are a complete code."""
    ll = [8] * 255 + [0, 8]
    return built([Dynamic(ll, [0], list(_rand(40, 5, 0, 255)))])


def _largest_header():
    """HLIT 286 / HDIST 30 / HCLEN 19, and the last symbol of each alphabet in use (length 258 through symbol 285, distance symbol 29)"""
    ll = balanced_lengths(286, list(range(286)))
    d = balanced_lengths(30, list(range(30)))
    hist = _rand(24700, 6)
    toks = list(b"png") + [(258, 24577), (257, 24600), (4, 1), (130, 12289)] + list(_rand(20, 7))
    return built([Stored(hist), Dynamic(ll, d, toks, hclen=19)])


def _single_dist():
    """Z_RLE's form by hand: exactly one distance code, of length 1, used by the matches"""
    ll = balanced_lengths(286, list(range(97, 123)) + [256] + list(range(257, 286)))
    toks = list(b"ab") + [(3, 1), (258, 1)] + list(b"c") + [(17, 1)] + list(b"d")
    return built([Dynamic(ll, [1], toks)])


def _dist_chain():
    """distance codes of every length 1..15 (1, 2, ..., 14, 15, 15: a chain), each used by a match; 11..15 are longer than the first-level table"""
    d = list(range(1, 15)) + [15, 15]
    ll = balanced_lengths(286, list(range(256)) + [256] + list(range(257, 286)))
    toks = list(_rand(300, 8))
    for s in range(16):
        toks += [(3 + s, DIST_BASE[s] + (1 << DIST_EXTRA[s]) - 1), 65 + s]
    return built([Dynamic(ll, d, toks)])


def _long_litlen(L):
    """literal/length codes 1, 2, ..., L - 2 (a chain of literals) and FOUR codes of L bits: literal 'x', literal 'y', end-of-block, length
    symbol 257.  L = 11 is the last length inside the first-level table, 12 and 15 go through the canonical decode."""
    def build():
        ll = [0] * 258
        for i in range(L - 2):
            ll[48 + i] = 1 + i
        ll[120] = ll[121] = ll[256] = ll[257] = L
        toks = list(range(48, 48 + L - 2)) + [120, (3, 2), 121, 48, (3, 1), 120]
        return built([Dynamic(ll, [1, 1], toks)])
    return build


def _match_at(offset, length, dist, tail=5):
    """stored history up to `offset`, then a fixed block that STARTS with the match"""
    def build():
        hist = _rand(offset, offset + dist)
        blocks = [Stored(hist[i:i + 65535]) for i in range(0, offset, 65535)]
        return built(blocks + [Fixed([(length, dist)] + list(_rand(tail, 9)))])
    return build


def _match_in_block(offset, length, dist, tail=5):
    """fixed-code literals up to `offset`, the match, `tail` literals: all in ONE block (the flush points are met inside the symbol loop)"""
    return lambda: built([Fixed(list(_rand(offset, offset + 2 * dist)) + [(length, dist)] + list(_rand(tail, 9)))])


def _stored_phase(k):
    """k nine-bit literals in a fixed block (3 + 9 k + 7 bits) put the next header on bit phase (2 + k) % 8"""
    return _blocks(Fixed([200 + i for i in range(k)]), Stored(_rand(37, 20 + k)), Fixed(list(b"after")))


def _stored_end(n):
    """header byte + 4 length bytes + n data bytes: the bit reader restarts at stream byte 5 + n"""
    return _blocks(Stored(_rand(n, 30 + n)), Fixed(list(b"behind the stored block")))


def _into_stored():
    """a dynamic block behind 9000 stored bytes whose matches copy stored bytes: from inside the ring and from behind it (memory)"""
    ll = balanced_lengths(286, list(range(256)) + [256] + list(range(257, 286)))
    d = balanced_lengths(30, list(range(30)))
    toks = list(b"dyn") + [(40, 100), (258, 8500), (9, 9003), (100, 7000)] + list(b"end")
    return built([Stored(_rand(9000, 40)), Dynamic(ll, d, toks)])


def _sized(base, r):
    """stream length = r mod 512: three empty stored blocks, a fixed block of as many 8-bit literals as it takes, then the case's block"""
    def build():
        final = Fixed(list(_rand(base, 50, 0, 144)))
        n0 = len(stream([Stored(), Stored(), Stored(), Fixed([]), final]))
        j = (r - n0) % 512
        return built([Stored(), Stored(), Stored(), Fixed(list(_rand(j, 51, 0, 144))), final])
    return build


def _case(name, build, *feats):
    return (name, build, frozenset(feats))


_S, _K = _scanlines(12000), _skewed(12000)
CASES = []
for _tag, _d in (("scanlines", _S), ("skewed", _K)):
    CASES += [
        _case(f"zlib_fixed_{_tag}", _zlib_case(_d, strategy=zlib.Z_FIXED), "fixed", "matches"),
        _case(f"zlib_rle_{_tag}", _zlib_case(_d, strategy=zlib.Z_RLE), "dynamic", "all_matches_at_distance_1"),
        _case(f"zlib_huffman_only_{_tag}", _zlib_case(_d, strategy=zlib.Z_HUFFMAN_ONLY), "dynamic", "dynamic_without_matches"),
        _case(f"zlib_filtered_{_tag}", _zlib_case(_d, strategy=zlib.Z_FILTERED), "dynamic", "matches"),
        _case(f"zlib_memlevel1_{_tag}", _zlib_case(_d, memLevel=1), "many_blocks"),
        _case(f"zlib_wbits9_{_tag}", _zlib_case(_d, wbits=-9), "all_matches_within_a_512_window"),
        _case(f"zlib_flushes_{_tag}", _zlib_case(_d, flush_at=((4001, zlib.Z_SYNC_FLUSH), (8002, zlib.Z_FULL_FLUSH))), "empty_stored",
              "coded_block_on_a_byte_boundary"),
    ]
CASES += [
    _case("zlib_level0_140000", _zlib_case(_rand(140000, 13), level=0), "stored", "three_stored_blocks", "outlen=140000"),
    # the code-length sequence
    _case("cross16", _cross(16), "cross16", "cross16_nonzero", "matches"),
    _case("cross17", _cross(17), "cross17", "literal_only"),
    _case("cross18", _cross(18), "cross18", "matches"),
    _case("hlit257_hdist1_hclen5", _smallest_header, "hlit257", "hdist1", "hclen5", "literal_only_hdist1"),
    _case("hlit286_hdist30_hclen19", _largest_header, "hlit286", "hdist30", "hclen19", "matches"),
    _case("literal_only_hdist1", _literals_dynamic(b"AAAAAAAAAAAAA"), "literal_only_hdist1"),
    _case("single_dist_code", _single_dist, "single_dist_code_used", "match_len258_dist1"),
    # long codes
    _case("dist_codes_1_to_15", _dist_chain, *[f"dist_code{l}" for l in range(1, 16)]),
] + [
    _case(f"litlen_codes_{L}", _long_litlen(L), f"lit_code{L}", f"len_code{L}", f"eob_code{L}") for L in (11, 12, 15)
] + [
    # the literal walk
    _case("walk_1bit", _literals_dynamic(b"A" * 9001), "walk_1bit", "literal_only"),
    _case("walk_1bit_2bit", _literals_dynamic(bytes(b"AAB"[i % 3] if i % 7 else 67 for i in range(20000))), "walk_1bit_2bit"),
] + [
    _case(f"fixed_literals_{n}", _fixed_literals(n), "fixed", f"outlen={n}") for n in (1, 55, 56, 57, 4095, 4096, 4097, 8191, 8192, 8193)
] + [
    # matches
    _case("match_len3_dist1", _blocks(Fixed([65, (3, 1), 66])), "match_len3_dist1"),
    _case("match_len258_dist1", _blocks(Fixed([65, (258, 1), 66])), "match_len258_dist1"),
    _case("match_dist_eq_len", _blocks(Fixed(list(b"abcdefg") + [(7, 7), (14, 14), 33, (29, 29)])), "match_dist=len"),
    _case("match_dist_eq_len_minus_1", _blocks(Fixed(list(b"abcdefg") + [(8, 7), (3, 2)] + list(_rand(250, 17)) + [(258, 257), 33])),
          "match_dist=len-1"),
    _case("match_back_to_byte0", _blocks(Fixed(list(b"abcde") + [(5, 5), (30, 10), (258, 40)] + [33])), "match_back_to_byte0"),
    _case("match_back_to_byte0_from_9000", _match_at(9000, 258, 9000), "match_back_to_byte0"),
    _case("match_len258_dist7680", _match_in_block(7700, 258, NEAR), "match_len258_dist7680"),
    _case("match_len258_dist7681", _match_in_block(7700, 258, NEAR + 1), "match_len258_dist7681"),
    _case("match_len258_dist7680_at_stored_history", _match_at(9000, 258, NEAR), "match_len258_dist7680", "match_into_stored_near"),
    _case("match_len258_dist7681_at_stored_history", _match_at(9000, 258, NEAR + 1), "match_len258_dist7681", "match_into_stored_far"),
    _case("match_dist32768", _match_at(32768 + 500, 258, 32768), "match_dist32768", "match_beyond_zlibs_reach"),
    _case("match_dist32768_at_32768", _match_at(32768, 258, 32768), "match_dist32768", "match_back_to_byte0"),
    _case("match_dist32507", _match_at(33000, 258, 32507), "match_beyond_zlibs_reach"),
    _case("match_len258_at4095", _match_in_block(4095, 258, 300), "match_len258_at4095"),
    _case("match_len258_at3839", _match_in_block(3839, 258, 300), "match_len258_at3839"),
    _case("match_len258_at3838", _match_in_block(3838, 258, 300), "match_len258_at3838"),
    _case("match_len258_at4095_second_piece", _match_in_block(8191, 258, 1), "match_len258_at4095"),
    _case("match_ends_the_output", _match_in_block(100, 31, 64, tail=0), "match_ends_the_output"),
    _case("match_ends_the_output_on_a_flush_point", _match_in_block(4000, 96, 3999, tail=0), "match_ends_the_output", "outlen=4096"),
    _case("far_match_first_after_flush", _match_in_block(3 * FLUSH, 100, 8000), "far_match_first_after_flush"),
    _case("far_match_first_after_stored_flush", _match_at(2 * FLUSH, 258, 8192), "far_match_first_after_flush", "match_into_stored_far"),
    # stored blocks
    _case("stored_len0", _blocks(Fixed(list(b"a")), Stored(), Fixed(list(b"b"))), "stored_len0", "empty_stored"),
    _case("stored_len1", _blocks(Stored(b"\x5a")), "stored_len1", "outlen=1"),
    _case("stored_len65535", _blocks(Stored(_rand(65535, 14)), Fixed(list(b"tail"))), "stored_len65535"),
] + [
    _case(f"stored_phase{(2 + k) % 8}", _stored_phase(k), f"stored_phase{(2 + k) % 8}") for k in range(8)
] + [
    _case(f"stored_end{(5 + n) % 4}", _stored_end(n), f"stored_end%4={(5 + n) % 4}") for n in (3, 4, 5, 6)
] + [
    _case("stored_wraps_ring_unaligned", _blocks(Stored(_rand(8185, 15)), Stored(_rand(300, 16)), Fixed([(258, 400), 1, 2])),
          "stored_wraps_ring_unaligned", "match_into_stored_near"),
    _case("dynamic_into_stored", _into_stored, "match_into_stored_near", "match_into_stored_far", "dynamic"),
] + [
    _case(f"streamlen_{tag}_{r}", _sized(base, r), f"streamlen%512={r}/{tag}", "empty_stored")
    for tag, base in (("short", 10), ("long", 2300)) for r in (505, 506, 507, 508, 509, 510, 511, 0, 1, 2, 3, 4)
]

# (n + a) mod 512 in {508 .. 511, 0, 1, 4} for every start alignment a in 0..3: the stream lengths above, each run at all four alignments
PLACEMENT = sorted({(t - a) % 512 for t in (508, 509, 510, 511, 0, 1, 4) for a in range(4)})

# every form this table exists for; `test_deflate_streams_cpu.py` asserts the union of the rows' censuses covers it
REQUIRED = frozenset(
    ["stored", "fixed", "dynamic", "matches", "all_matches_at_distance_1", "dynamic_without_matches", "many_blocks",
     "all_matches_within_a_512_window", "three_stored_blocks", "empty_stored", "coded_block_on_a_byte_boundary",
     "cross16", "cross16_nonzero", "cross17", "cross18", "hlit257", "hdist1", "hclen5", "hlit286", "hdist30", "hclen19",
     "literal_only", "literal_only_hdist1", "single_dist_code_used", "walk_1bit", "walk_1bit_2bit",
     "match_len3_dist1", "match_len258_dist1", "match_dist=len", "match_dist=len-1", "match_back_to_byte0", "match_len258_dist7680",
     "match_len258_dist7681", "match_dist32768", "match_beyond_zlibs_reach", "match_len258_at4095", "match_len258_at3839",
     "match_len258_at3838", "match_ends_the_output", "far_match_first_after_flush", "match_into_stored_near", "match_into_stored_far",
     "stored_len0", "stored_len1", "stored_len65535", "stored_wraps_ring_unaligned"]
    + [f"dist_code{l}" for l in range(1, 16)]
    + [f"{k}_code{l}" for k in ("lit", "len", "eob") for l in (11, 12, 15)]
    + [f"outlen={n}" for n in (1, 55, 56, 57, 4095, 4096, 4097, 8191, 8192, 8193, 140000)]
    + [f"stored_phase{p}" for p in range(8)] + [f"stored_end%4={p}" for p in range(4)]
    + [f"streamlen%512={r}/{tag}" for tag in ("short", "long") for r in PLACEMENT])


def _hclen4():
    """HLIT 257 / HDIST 1 / HCLEN 4: code-length codes for 0 and 18 only, 258 zero lengths in two 18 runs.  Well formed up to there, but no
    symbol has a code: inflate stops at the missing end-of-block code, a checked condition (zlib: 'missing end-of-block', the kernel: 4)."""
    w = BitWriter()
    w.bits(1, 1), w.bits(2, 2), w.bits(0, 5), w.bits(0, 5), w.bits(0, 4)
    for l in (0, 0, 1, 1):            # 16, 17, 18, 0
        w.bits(l, 3)
    for run in (138, 120):            # symbol 0 has code 0, symbol 18 code 1
        w.code(1, 1)
        w.bits(run - 11, 7)
    w.align()
    return with_trailer(w.getvalue(), b""), b""


# (name, builder, status word of mt4_png_inflate): streams that end on a checked, in-bounds condition
REJECTED = [("hlit257_hdist1_hclen4", _hclen4, 4)]


@functools.lru_cache(maxsize=None)
def build_all():
    """{name: (stream, expected bytes, features asked)} -- built once per process"""
    out = {}
    for name, build, feats in CASES:
        assert name not in out, name
        s, e = build()
        out[name] = (s, e, feats)
    return out


# ------------------------------------------------------------------------------------------------------------------ scanline filters

def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))       # PNG 9.4: a, then b, then c


def unfilter_ref(raw, h, w):
    """PNG specification 9.2 - 9.4 for 8-bit RGB (3 bytes per pixel): h rows of (filter type, 3 w bytes) -> uint8 [h, w, 3].  Integer
    arithmetic on unwrapped values; left and upper-left are 0 in the first pixel, up is 0 in the first row."""
    raw = np.frombuffer(bytes(raw), np.uint8).astype(np.int64).reshape(h, 1 + 3 * w)
    out = np.zeros((h, w, 3), np.int64)
    zero_row = np.zeros((w, 3), np.int64)
    for y in range(h):
        ft, x = int(raw[y, 0]), raw[y, 1:].reshape(w, 3)
        up = out[y - 1] if y else zero_row
        if ft == 0:
            out[y] = x
        elif ft == 2:
            out[y] = (x + up) & 255
        elif ft == 1:
            out[y] = np.cumsum(x, axis=0) & 255
        elif ft in (3, 4):
            a = np.zeros(3, np.int64)
            c = np.zeros(3, np.int64)
            for i in range(w):
                b = up[i]
                pred = (a + b) // 2 if ft == 3 else _paeth(a, b, c)
                a = (x[i] + pred) & 255
                out[y, i] = a
                c = b
        else:
            raise ValueError(f"filter type {ft}")
    return out.astype(np.uint8)


def filter_rows(img, types):
    """the forward filters: image [h, w, 3] and one filter type per row -> the raw scanline bytes"""
    img = np.asarray(img).astype(np.int64)
    h, w, _ = img.shape
    a = np.zeros_like(img)
    a[:, 1:] = img[:, :-1]
    b = np.zeros_like(img)
    b[1:] = img[:-1]
    c = np.zeros_like(img)
    c[1:, 1:] = img[:-1, :-1]
    rows = []
    for y in range(h):
        ft = types[y]
        pred = [0, a[y], b[y], (a[y] + b[y]) // 2, _paeth(a[y], b[y], c[y])][ft]
        rows.append(bytes([ft]) + ((img[y] - pred) & 255).astype(np.uint8).tobytes())
    return b"".join(rows)


FILTER_SHAPES = [(h, w) for w in (1, 2, 21, 22, 43) for h in (1, 2, 5)] + [(2, 4096)]


def _filter_images(h, w):
    """decoded images to run through the forward filters: Paeth ties (every pixel one of three values, so a = b = c, a = b != c and pa = pc < pb
    all occur; the exact triples are planted in the corner), high values (v + pred wraps mod 256, Average's a + b needs the ninth bit)"""
    rng = np.random.default_rng(1000 * h + w)
    ties = rng.choice(np.array([6, 10, 12]), (h, w, 3))
    if h >= 2 and w >= 2:
        ties[0, 0], ties[0, 1], ties[1, 0] = 10, 12, 6          # c, b, a of pixel (1, 1): pa = pc = 2 < pb = 4
    if h >= 2 and w >= 4:
        ties[0, 2], ties[0, 3], ties[1, 2] = 10, 6, 6           # a = b != c
    high = rng.integers(128, 256, (h, w, 3))
    if w > 1000:                     # (the ties do not depend on the width; the serial reference is what a wide case costs)
        return {"high": high.astype(np.uint8)}
    return {"ties": ties.astype(np.uint8), "high": high.astype(np.uint8)}


@functools.lru_cache(maxsize=None)
def filter_cases(h, w):
    """[(name, raw scanline bytes)] of one frame size: every type forced on every row (the first included), the five types cycled from each
    start -- over random FILTERED bytes (valid under any type) and over the forward-filtered crafted images"""
    rng = np.random.default_rng(77 * h + w)
    plans = [(f"all{t}", [t] * h) for t in range(5)] + [(f"cycle{s}", [(s + y) % 5 for y in range(h)]) for s in range(5)]
    out = []
    for pname, types in plans:
        body = rng.integers(0, 256, (h, 3 * w), dtype=np.uint8)
        out.append((f"{pname}_random", b"".join(bytes([types[y]]) + body[y].tobytes() for y in range(h))))
        for iname, img in _filter_images(h, w).items():
            out.append((f"{pname}_{iname}", filter_rows(img, types)))
    return out


def _chunk(typ, data):
    return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data))


def png_file(raw, h, w, idat_sizes=None, empty_between=False, ancillary=False, level=6):
    """a real file around the filtered rows: signature, IHDR (8-bit RGB, no interlace), the zlib stream in IDAT chunks of `idat_sizes` bytes
    (the rest in a last one), optionally an empty IDAT between any two and tEXt / pHYs in front, IEND; CRCs in place"""
    z = zlib.compress(bytes(raw), level)
    parts, pos = [], 0
    for n in idat_sizes or ():
        parts.append(z[pos:pos + n])
        pos += n
    parts.append(z[pos:])
    chunks = [_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))]
    if ancillary:
        chunks += [_chunk(b"tEXt", b"Comment\x00forced scanline filters"), _chunk(b"pHYs", struct.pack(">IIB", 2835, 2835, 1))]
    for i, p in enumerate(parts):
        if i and empty_between:
            chunks.append(_chunk(b"IDAT", b""))
        chunks.append(_chunk(b"IDAT", p))
    return b"\x89PNG\r\n\x1a\n" + b"".join(chunks + [_chunk(b"IEND", b"")])
