"""ZSTD frames for tests, built bit by bit (RFC 8878): the flavours libzstd never writes.

Z builds a frame block by block -- raw, RLE, compressed; literals raw / RLE / Huffman (direct weights, 1 or 4 streams) /
treeless; sequences through an FSE ENCODER driven by the decoding table (for the symbol in front of state `next`, the cell of
that symbol whose [baseline, baseline + 2^nbits) holds `next`), tables Predefined / RLE / FSE_Compressed / Repeat, offsets as
repeat codes under the caller's control -- and executes the literals and sequences it is given in plain Python as it goes:
`want`, the bytes the frame stands for, never comes from the code under test.  The corpus (valid_cases / refused_cases /
invalid_cases) is shared by tests/test_zstd_frames_host.py, which proves it against libzstd and the CPU build of the kernels'
stages, and tests/test_gpu_zstd_frames.py, which feeds it to the kernels.  No GPU here.

Not built: FSE-compressed Huffman weights (what libzstd writes; the libzstd-written corpus of the older tests covers them).
Direct weights name at most 128 symbols and the implied one, so a Huffman symbol above 128 cannot be built here:
libzstd_all_quarters() is the one libzstd-written frame of the corpus, whose literals use all 256 symbols."""
import struct

import numpy as np

MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 128 << 10
LL, OF, ML = 0, 1, 2

# ------------------------------------------------------------------------------------------- codes (RFC 8878 3.1.1.3.2.1.1)
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def _bases(first, bits):
    out, v = [], first
    for b in bits:
        out.append(v)
        v += 1 << b
    return out


LL_BASE = _bases(0, LL_BITS)      # ..., 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, ..., 65536
ML_BASE = _bases(3, ML_BITS)      # ..., 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, ..., 65539
assert LL_BASE[16] == 16 and LL_BASE[25] == 64 and LL_BASE[35] == 65536 and ML_BASE[32] == 35 and ML_BASE[43] == 131 and ML_BASE[52] == 65539

PREDEFINED = {
    LL: ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6),
    OF: ([1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1], 5),
    ML: ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6),
}


def code_of(table_bases, v):
    c = len(table_bases) - 1
    while table_bases[c] > v:
        c -= 1
    return c


def ll_code(ll):
    c = code_of(LL_BASE, ll)
    return c, ll - LL_BASE[c], LL_BITS[c]


def ml_code(ml):
    c = code_of(ML_BASE, ml)
    return c, ml - ML_BASE[c], ML_BITS[c]


def of_code(ov):
    c = ov.bit_length() - 1
    return c, ov - (1 << c), c


# ------------------------------------------------------------------------------------------------------------ bit writers
class Bits:
    """Bits in the order they are written, the first in bit 0 of byte 0.  A backward stream is written last field first and
    closed with a 1 bit; a forward description is written as it is read."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def add(self, v, n):
        assert 0 <= v < (1 << n) or n == 0 and v == 0, (v, n)
        self.acc |= v << self.n
        self.n += n
        if self.n >= 64:
            k = self.n // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def close(self, end_mark):
        if end_mark:
            self.add(1, 1)
        k = (self.n + 7) // 8
        return bytes(self.out) + self.acc.to_bytes(k, "little")


# ------------------------------------------------------------------------------------------------------------------- FSE
_tables = {}


def fse_table(counts, al):
    """The decoding table of a normalised distribution (RFC 8878 4.1.1): [(symbol, baseline, nbits)] per state."""
    key = (tuple(counts), al)
    if key in _tables:
        return _tables[key]
    size = 1 << al
    assert sum(abs(c) for c in counts) == size, (sum(abs(c) for c in counts), size)
    sym = [None] * size
    high = size - 1
    for s, c in enumerate(counts):
        if c == -1:
            sym[high] = s
            high -= 1
    step, pos = (size >> 1) + (size >> 3) + 3, 0
    for s, c in enumerate(counts):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    nxt = [1 if c == -1 else c for c in counts]
    table = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nbits = al - (ns.bit_length() - 1)
        table.append((s, (ns << nbits) - size, nbits))
    _tables[key] = table
    return table


def fse_description(counts, al):
    """The normalised counts as the format stores them (the trailing zero counts are not written)."""
    b = Bits()
    b.add(al - 5, 4)
    remaining, threshold, nb = (1 << al) + 1, 1 << al, al + 1
    last = max(s for s, c in enumerate(counts) if c)
    s = 0
    while s <= last:
        c = counts[s]
        value = c + 1
        mx = (2 * threshold - 1) - remaining
        if value < mx:
            b.add(value, nb - 1)
        elif value < threshold:
            b.add(value, nb)
        else:
            b.add(value + mx, nb)
        remaining -= abs(c)
        s += 1
        if c == 0:
            zeros = 0
            while counts[s + zeros] == 0:
                zeros += 1
            s += zeros
            while zeros >= 3:
                b.add(3, 2)
                zeros -= 3
            b.add(zeros, 2)
        while remaining < threshold:
            nb -= 1
            threshold >>= 1
    assert remaining == 1
    return b.close(False)


def spread_counts(symbols, al, heavy=()):
    """A distribution of accuracy `al` over `symbols`: one cell each, the rest of the 2^al cells shared out over `heavy`
    (default: all of them) in turn."""
    symbols = sorted(set(symbols))
    counts = [0] * (max(symbols) + 1)
    for s in symbols:
        counts[s] = 1
    left = (1 << al) - len(symbols)
    assert left >= 0
    heavy = list(heavy) or symbols
    for i in range(left):
        counts[heavy[i % len(heavy)]] += 1
    return counts


class _Encoder:
    """One FSE state of the sequence encoder, run BACKWARDS over the symbols: cells(sym) -> the states that decode `sym`."""

    def __init__(self, mode, counts=None, al=0, sym=None):
        self.al = 0 if mode == "rle" else al
        if mode == "rle":
            self.cells = {sym: [(0, 0, 0)]}
        else:
            self.cells = {}
            for u, (s, base, nbits) in enumerate(fse_table(counts, al)):
                self.cells.setdefault(s, []).append((u, base, nbits))

    def last(self, sym):
        return self.cells[sym][0][0]

    def before(self, sym, nxt):
        """(state, bits, nbits): the state that decodes `sym` and goes on to state `nxt`."""
        for u, base, nbits in self.cells[sym]:
            if base <= nxt < base + (1 << nbits):
                return u, nxt - base, nbits
        raise AssertionError("no cell of symbol %d reaches state %d" % (sym, nxt))


def sequence_bitstream(triples, enc):
    """(ll, ml, offset value) per sequence -> the backward bitstream: written from the last sequence to the first, every
    field in the reverse of the order the decoder reads it (offset, match length, literal length extra bits; then the
    literal length, match length, offset state bits), the three initial states on top, the closing 1 bit."""
    b = Bits()
    nxt = None
    for ll, ml, ov in reversed(triples):
        cl, cm, co = ll_code(ll), ml_code(ml), of_code(ov)
        if nxt is None:
            st = [enc[LL].last(cl[0]), enc[OF].last(co[0]), enc[ML].last(cm[0])]
        else:
            st = []
            for t, c in ((OF, co), (ML, cm), (LL, cl)):
                u, bits, nbits = enc[t].before(c[0], nxt[t])
                b.add(bits, nbits)
                st.append(u)
            st = [st[2], st[0], st[1]]
        for c in (cl, cm, co):
            b.add(c[1], c[2])
        nxt = st
    b.add(nxt[ML], enc[ML].al)
    b.add(nxt[OF], enc[OF].al)
    b.add(nxt[LL], enc[LL].al)
    return b.close(True)


# --------------------------------------------------------------------------------------------------------------- Huffman
def huffman_codes(weights):
    """weights[symbol] (0 = absent; the LAST symbol's weight is the one the format implies) -> (max_bits,
    {symbol: (code, nbits)}): cells in the order of ascending weight, symbols of one weight in symbol order (RFC 8878 4.2.1)."""
    listed = sum(1 << (w - 1) for w in weights[:-1] if w)
    max_bits = listed.bit_length()
    rest = (1 << max_bits) - listed
    assert rest & (rest - 1) == 0 and weights[-1] == rest.bit_length() and max_bits <= 11, (listed, weights[-1])
    codes, at = {}, 0
    for w in range(1, max_bits + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (at >> (w - 1), max_bits + 1 - w)
                at += 1 << (w - 1)
    assert at == 1 << max_bits
    return max_bits, codes


def huffman_description(weights):
    """Direct representation: 127 + the number of listed weights, then a nibble each, the first of a pair in the high one."""
    listed = list(weights[:-1])
    assert 1 <= len(listed) <= 128
    out = bytearray([127 + len(listed)])
    for i in range(0, len(listed), 2):
        out.append((listed[i] << 4) | (listed[i + 1] if i + 1 < len(listed) else 0))
    return bytes(out)


def huffman_stream(symbols, codes):
    b = Bits()
    for s in reversed(symbols):
        b.add(*codes[s])
    return b.close(True)


# ------------------------------------------------------------------------------------------------------------- the frame
def frame_header(content_size=None, fcs_bytes=None, window=None, checksum=False, dict_id=None):
    """window None: single segment (the content size is then written, in >= 1 byte); else the window descriptor byte.
    fcs_bytes: 0 / 1 / 2 / 4 / 8, or None for the smallest that holds content_size."""
    single = window is None
    if fcs_bytes is None:
        fcs_bytes = 0 if content_size is None else 1 if content_size < 256 and single else 2 if 256 <= content_size < 65792 else 4 if content_size < (1 << 32) else 8
    assert fcs_bytes in (0, 1, 2, 4, 8) and (fcs_bytes != 1 or single) and (fcs_bytes != 0 or not single)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    did = b"" if dict_id is None else struct.pack("<I", dict_id)
    out = MAGIC + bytes([(flag << 6) | (0x20 if single else 0) | (0x04 if checksum else 0) | (3 if did else 0)])
    if not single:
        out += bytes([window])
    out += did
    if fcs_bytes:
        v = content_size - 256 if fcs_bytes == 2 else content_size
        out += v.to_bytes(fcs_bytes, "little")
    return out


def skippable_frame(payload=b"skip me"):
    return struct.pack("<II", 0x184D2A50, len(payload)) + payload


class Z:
    """A frame under construction.  raw() / rle() / comp() append a block and run it: self.out is what the frame means so
    far, self.rep the repeat-offset history (RFC 8878 3.1.1.5; raw and RLE blocks leave it alone)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.blocks = []          # (type, content bytes, size field)
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.huf = None           # weights of the last Huffman table
        self.tab = [None, None, None]   # the last table of each kind: a resolved spec
        self.valid = True         # False once a block was written that must not be executed
        self.marks = []           # per block: None, or (bytes of the literals header, where the sequence bitstream begins)

    # ---- blocks
    def raw(self, n):
        data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        self.blocks.append((0, data, n))
        self.marks.append(None)
        self.out += data
        return self

    def rle(self, n, byte=None):
        byte = int(self.rng.integers(0, 256)) if byte is None else byte
        self.blocks.append((1, bytes([byte]), n))
        self.marks.append(None)
        self.out += bytes([byte]) * n
        return self

    def _literals(self, n, lits):
        """-> (header, the bytes behind it, the literal bytes).  fmt: raw / RLE -- the header's bytes (1..3); Huffman -- the size
        format (0..3)."""
        kind = lits[0]
        opt = lits[-1] if isinstance(lits[-1], dict) else {}
        fmt = opt.get("fmt")
        if kind in ("raw", "rle"):
            if kind == "raw":
                data = self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
                body = data[: opt.get("declare", n)]
            else:
                body = bytes([int(self.rng.integers(0, 256))])
                data = body * n
            size = opt.get("declare", n)
            hdr = (1 if size < 32 else 2 if size < 4096 else 3) if fmt is None else fmt
            t = 0 if kind == "raw" else 1
            if hdr == 1:
                assert size < 32
                head = bytes([t | (size << 3)])
            elif hdr == 2:
                assert size < 4096
                head = struct.pack("<H", t | (1 << 2) | (size << 4))
            else:
                head = (t | (3 << 2) | (size << 4)).to_bytes(3, "little")
            return head, body, data
        if kind == "huf":
            weights, streams = list(lits[1]), lits[2]
            self.huf = weights
            desc = opt.get("description", None)
            desc = huffman_description(weights) if desc is None else desc
            t = 2
        else:
            assert kind == "treeless" and (self.huf is not None or not self.valid)
            weights, streams, desc, t = self.huf or [1, 1], lits[1], b"", 3
        _, codes = huffman_codes(weights)
        present = np.array(sorted(codes))
        p = np.array([2.0 ** -codes[s][1] for s in present])
        data = self.rng.choice(present, n, p=p / p.sum()).astype(np.uint8)
        if n >= len(present):
            data[self.rng.permutation(n)[: len(present)]] = present       # every symbol of the table is used
        syms = data.tolist()
        if streams == 1:
            body = huffman_stream(syms, codes)
        else:
            per = (n + 3) // 4
            parts = [huffman_stream(syms[i * per: (i + 1) * per], codes) for i in range(4)]
            body = struct.pack("<HHH", *(len(x) for x in parts[:3])) + b"".join(parts)
        comp = len(desc) + len(body)
        if fmt is None:
            fmt = (0 if streams == 1 else 1) if max(n, comp) < 1024 else 2 if max(n, comp) < 16384 else 3
        assert (fmt == 0) == (streams == 1)
        bits = 10 if fmt < 2 else 14 if fmt == 2 else 18
        assert max(n, comp) < (1 << bits), (n, comp, bits)
        head = (t | (fmt << 2) | (n << 4) | (comp << (4 + bits))).to_bytes(3 if fmt < 2 else fmt + 2, "little")
        return head, desc + body, data.tobytes()

    def _table(self, t, spec):
        """spec: "predefined" | ("rle", symbol) | ("fse", counts, al[, description bytes]) | "repeat" -> (mode, bytes, encoder)."""
        if spec == "repeat":
            assert self.tab[t] is not None or not self.valid
            return 3, b"", _Encoder(*(self.tab[t] or ("fse",) + PREDEFINED[t]))
        if spec == "predefined":
            r = ("fse",) + PREDEFINED[t]
            mode, desc = 0, b""
        elif spec[0] == "rle":
            r = ("rle", None, 0, spec[1])
            mode, desc = 1, bytes([spec[1]])
        else:
            r = ("fse", list(spec[1]), spec[2])
            mode, desc = 2, spec[3] if len(spec) > 3 else fse_description(spec[1], spec[2])
        self.tab[t] = r
        return mode, desc, _Encoder(*r)

    def comp(self, seqs, tail=0, lits=("raw",), tables=None, tamper=None):
        """A compressed block.  seqs: (literal length, match length, offset) with offset an int (a real offset, written as
        offset + 3) or ("r", 1..3) (written as that repeat code); `tail`: literals behind the last sequence.
        tables: {LL / OF / ML: spec}, Predefined where nothing is said.  tamper: {"bitstream": f(bytes) -> bytes} to damage
        the sequence bitstream, {"execute": False} for a block that cannot be run (its sizes are then taken as written)."""
        tamper = tamper or {}
        tables = tables or {}
        nlit = sum(s[0] for s in seqs) + tail
        head, body, literals = self._literals(nlit, lits)
        section, bits_at = head + body, None
        n = len(seqs)
        count = bytes([n]) if n < 128 else bytes([(n >> 8) + 128, n & 255]) if n < 0x7F00 else b"\xff" + struct.pack("<H", n - 0x7F00)
        content = section + count
        triples = [(ll, ml, off[1] if isinstance(off, tuple) else off + 3) for ll, ml, off in seqs]
        if n:
            modes, descs, enc = 0, b"", {}
            for t in (LL, OF, ML):
                mode, desc, enc[t] = self._table(t, tables.get(t, "predefined"))
                modes |= mode << (6 - 2 * t)
                descs += desc
            bits = sequence_bitstream(triples, enc)
            bits = tamper["bitstream"](bits) if "bitstream" in tamper else bits
            bits_at = len(content) + 1 + len(descs)
            content += bytes([modes]) + descs + bits
        self.blocks.append((2, content, len(content)))
        self.marks.append((len(head), bits_at))
        if tamper.get("execute", True) and self.valid:
            self._run(triples, literals)
        else:
            self.valid = False
            self.out += bytes(sum(s[0] + s[1] for s in seqs) + tail)
        return self

    def _run(self, triples, literals):
        out, rep, at = self.out, self.rep, 0
        start = len(out)
        for ll, ml, ov in triples:
            out += literals[at: at + ll]
            at += ll
            if ov > 3:
                off = ov - 3
                rep[:] = [off, rep[0], rep[1]]
            else:
                idx = ov - 1 + (1 if ll == 0 else 0)
                if idx == 0:
                    off = rep[0]
                elif idx == 1:
                    off = rep[1]
                    rep[:] = [off, rep[0], rep[2]]
                else:
                    off = rep[2] if idx == 2 else rep[0] - 1
                    rep[:] = [off, rep[0], rep[1]]
            assert 0 < off <= len(out), ("offset", off, len(out))
            if off >= ml:
                out += out[len(out) - off: len(out) - off + ml]
            else:
                pattern = bytes(out[len(out) - off:])
                out += (pattern * (ml // off + 1))[:ml]
        out += literals[at:]
        assert len(out) - start <= BLOCK_MAX, len(out) - start

    # ---- the frame
    def frame(self, declared=None, **header):
        """The frame's bytes.  Single segment with the smallest content-size field unless `header` says otherwise
        (frame_header); declared: the content size to write instead of the true one."""
        n = len(self.out) if declared is None else declared
        if "window" in header and "fcs_bytes" not in header:
            header["fcs_bytes"] = 0
        parts = [frame_header(content_size=n, **header)]
        at = len(parts[0])
        self.literals_at, self.bitstream_at = [], []      # positions in the frame, per compressed block
        for i, (t, content, size) in enumerate(self.blocks):
            parts.append(((1 if i == len(self.blocks) - 1 else 0) | (t << 1) | (size << 3)).to_bytes(3, "little"))
            parts.append(content)
            if self.marks[i]:
                self.literals_at.append(at + 3 + self.marks[i][0])
                self.bitstream_at.append(None if self.marks[i][1] is None else at + 3 + self.marks[i][1])
            at += 3 + len(content)
        return b"".join(parts)

    @property
    def want(self):
        assert self.valid
        return bytes(self.out)


def case(z, dtype="uint8", **header):
    want = z.want
    assert len(want) % np.dtype(dtype).itemsize == 0 and len(want) > 0
    frame = z.frame(**header)
    return dict(dtype=dtype, frame=frame, want=want, literals_at=z.literals_at, bitstream_at=z.bitstream_at)


# ------------------------------------------------------------------------------------------------------ the corpus: valid
def _seqs(rng, n, pos, ll=(0, 6), ml=(3, 12), reach=None):
    """n sequences with random small lengths and real offsets into the `pos` bytes before them (and what they add)."""
    out = []
    for _ in range(n):
        l, m = int(rng.integers(ll[0], ll[1] + 1)), int(rng.integers(ml[0], ml[1] + 1))
        l = max(l, 1) if pos == 0 else l
        pos += l
        out.append((l, m, int(rng.integers(1, min(pos, reach or pos) + 1))))
        pos += m
    return out


def _z1_block_types():
    """Z1: compressed, RLE, compressed, raw, compressed in one buffer.  Blocks 2 and 4 begin with the repeat codes 1, 2 and 3
    (with literals in front: the codes mean the history as block 0 left it, through the RLE / raw block between); block 4
    has a match that reaches back across the raw block and the RLE block into block 0."""
    z = Z(1)
    z.comp([(40, 5, 7), (3, 4, 19), (2, 6, 33), (1, 9, 11)], tail=3)          # history 11, 33, 19
    z.rle(300)
    z.comp([(2, 5, ("r", 1)), (1, 4, ("r", 2)), (3, 7, ("r", 3)), (4, 5, 350)], tail=2)
    assert z.rep == [350, 19, 33]
    z.raw(1000)
    z.comp([(1, 6, ("r", 1)), (2, 4, ("r", 2)), (1, 5, ("r", 3)), (2, 30, 1000 + 300 + 60), (0, 8, len(z.out) - 3)], tail=5)
    return case(z)


def _z1_rle_sizes():
    """Z1: RLE blocks of 1 (a literal and a match of length 0), 2 and 131072 bytes; the first block of the buffer is RLE."""
    z = Z(2)
    z.rle(1).comp([(3, 4, 2)], tail=1).rle(2).rle(BLOCK_MAX).comp([(0, 10, BLOCK_MAX + 5), (2, 3, ("r", 1))], tail=4)
    return case(z)


def _z1_raw_first():
    """Z1: a raw block first, then matches into it; repeat codes against 1 / 4 / 8 behind it."""
    z = Z(3)
    z.raw(777).comp([(1, 5, ("r", 2)), (2, 6, 700), (1, 3, ("r", 3))], tail=9)
    return case(z)


def _z2_rle_literals():
    """Z2: RLE literals with 1-, 2- and 3-byte headers (the third forced on a short run, and on 5000)."""
    z = Z(10)
    z.comp([(5, 4, 2), (9, 3, 7)], tail=6, lits=("rle",))                    # 20 literals: 1 byte
    z.comp([(100, 4, 50), (200, 5, 99)], tail=33, lits=("rle",))             # 333: 2 bytes
    z.comp([(2, 4, 50)], tail=3, lits=("rle", dict(fmt=3)))                  # 5 in 3 bytes
    z.comp([(2500, 40, 1000)], tail=2500, lits=("rle",))                     # 5000: 3 bytes
    z.comp([(4, 4, 9)], tail=7, lits=("rle", dict(fmt=2)))                   # 11 in 2 bytes
    return case(z)


def _z2_raw_alignment():
    """Z2: raw literals beginning at every alignment 0..3 of the body (a buffer's frame begins on an 8-byte boundary of the
    body, so a position in the frame is a position in the body modulo 4): eight blocks with 1-, 2- and 3-byte literal headers;
    block i's literals begin at residue i modulo 4, which the trailing literals of block i - 1 (0..3 of them) see to."""
    def build(tails):
        z = Z(11)
        for i, t in enumerate(tails):
            fmt = (1, 2, 3, 1, 1, 3, 2, 1)[i]
            z.comp([(5 + i, 4, 2), (2, 3, 5)], tail=t, lits=("raw", dict(fmt=fmt)))
        return z
    z = build([0] * 8)
    z.frame()
    plain, tails, shift = z.literals_at, [0] * 8, 0
    for i in range(1, 8):
        tails[i - 1] = (i - plain[i] - shift) % 4
        shift += tails[i - 1]
    c = case(build(tails))
    assert [x % 4 for x in c["literals_at"]][1:] == [1, 2, 3, 0, 1, 2, 3]
    return c


W_SMALL = [4, 3, 2, 1, 1]                       # 5 symbols, 4 bits at most
W_TEXT = [0] * 32 + [5] + [0] * 11 + [3, 0, 2] + [0] * 50 + [2] * 16 + [1] * 10      # ' ' , . a..p q..y and z, the implied one: 6 bits at most


def _fix_last(weights):
    """The weights with the last one replaced by the one the format implies (None if they do not complete a power of two)."""
    listed = sum(1 << (w - 1) for w in weights[:-1] if w)
    rest = (1 << listed.bit_length()) - listed
    return weights[:-1] + [rest.bit_length()] if rest & (rest - 1) == 0 else None


def _z2_huffman_streams():
    """Z2: one Huffman stream; four streams of 6, 7, 1023, 1024, 16383 and 16384 literals -- the 3-, 4- and 5-byte size
    formats, a last stream of 0 and of 1 literal."""
    z = Z(12)
    z.comp([(30, 4, 5), (50, 6, 20)], tail=20, lits=("huf", W_SMALL, 1))
    for n in (6, 7, 1023, 1024, 16383, 16384):
        z.comp([(n // 2, 5, 17)], tail=n - n // 2, lits=("huf", W_SMALL, 4))
    z.comp([(300, 4, 5)], tail=33, lits=("huf", W_SMALL, 4, dict(fmt=3)))    # 5-byte header on a small section
    z.comp([(300, 4, 5)], tail=33, lits=("huf", W_SMALL, 4, dict(fmt=2)))
    return case(z)


def _z2_treeless():
    """Z2: treeless literals in the block after their table; and two compressed blocks after it, with a raw-literal block
    and an RLE block between (and a raw block, and a block with RLE literals)."""
    z = Z(13)
    z.comp([(60, 4, 5)], tail=40, lits=("huf", W_TEXT, 1))
    z.comp([(70, 4, 9)], tail=10, lits=("treeless", 1))
    z.comp([(8, 4, 9)], tail=2)                     # raw literals
    z.rle(50)
    z.raw(9)
    z.comp([(8, 4, 9)], tail=2, lits=("rle",))
    z.comp([(700, 4, 9)], tail=500, lits=("treeless", 4))
    return case(z)


def _huf_case(seed, weights, n=400, streams=1):
    z = Z(seed)
    z.comp([(n // 3, 4, 6), (n // 3, 5, 40)], tail=n - 2 * (n // 3), lits=("huf", weights, streams))
    return case(z)


def huffman_tables():
    """Z3: name -> weights.  two: 2 symbols; full_128: 128 listed symbols and the implied one; eleven_bits: the longest code is
    11 bits; wave_fill: weights 8 (128 cells >= 64: the whole-wave fill) owned by three symbols, in two quarters;
    quarters: weight 3 (4 cells < 64: the lane fill) owned by symbols below 64, in 64..127 and by 128, the implied one -- the
    highest symbol direct weights can name (symbols from 129 on: libzstd_all_quarters)."""
    t = {"two": [1, 1]}
    t["full_128"] = _fix_last([1] * 127 + [1, 0])               # 128 ones and the implied weight: 128 -> 256, weight 8
    assert t["full_128"][-1] == 8
    w = [0] * 129
    w[3], w[70], w[100] = 8, 8, 8                                # 3 x 128 cells
    w[5], w[64], w[127] = 6, 6, 6                                # 3 x 32
    w[60], w[63] = 4, 4                                          # 2 x 8
    w[0], w[1], w[126], w[125], w[124], w[10] = 3, 3, 2, 2, 2, 1 # 4 + 4 + 2 + 2 + 2 + 1, 511 so far; the implied one: 1 -> 512
    t["wave_fill"] = _fix_last(w)
    assert t["wave_fill"][-1] == 1
    w = [0] * 129
    for s in (2, 40, 63, 64, 90, 127):
        w[s] = 3                                                 # 6 x 4 cells, both quarters; with the implied one (4): 28
    w[10], w[11], w[12] = 2, 1, 1                                # 4: 32 cells with the implied weight 3
    w[128] = 3
    t["quarters"] = _fix_last(w)
    assert t["quarters"][-1] == 3
    w = [0] * 40
    w[0], w[7], w[8], w[9], w[20], w[21], w[22], w[23], w[30], w[31] = 11, 10, 9, 8, 7, 6, 5, 4, 3, 2   # 2046
    w[33], w[39] = 1, 1
    t["eleven_bits"] = _fix_last(w)
    assert huffman_codes(t["eleven_bits"])[0] == 11
    return t


def _z3_long_stream():
    """Z3: one literal stream of 625 bytes (1000 literals of 5 bits), then four of 2500 bytes each: longer than the 512 bytes
    of a stream the kernel keeps in LDS, so SlidingWords slides."""
    z = Z(25)
    z.comp([(500, 4, 6)], tail=500, lits=("huf", [1] * 32, 1))       # (libzstd wants an even number >= 2 of weight-1 symbols)
    z.comp([(9000, 4, 6)], tail=7000, lits=("treeless", 4))
    assert len(z.blocks[0][1]) > 625 and len(z.blocks[1][1]) > 10000
    return case(z)


FSE_LL5 = ("fse", spread_counts(range(0, 20), 5), 5)
FSE_OF5 = ("fse", spread_counts(range(0, 12), 5), 5)
FSE_ML5 = ("fse", spread_counts(range(0, 24), 5), 5)


def _z4_repeat_each(t):
    """Z4: FSE_Compressed in block 0 (accuracy log 5), Repeat in block 1, for one table; the others Predefined."""
    z = Z(30 + t)
    spec = (FSE_LL5, FSE_OF5, FSE_ML5)[t]
    z.comp(_seqs(z.rng, 40, 0), tail=3, tables={t: spec})
    z.comp(_seqs(z.rng, 50, len(z.out)), tail=1, tables={t: "repeat"})
    return case(z)


def _z4_three_sources():
    """Z4: all three tables Repeat at once, from three DIFFERENT blocks: block 0 describes literal lengths, block 1 offsets
    (literal lengths repeated), block 2 match lengths (the other two repeated), block 3 repeats all three; a block without
    sequences and an RLE block lie between."""
    z = Z(34)
    z.comp(_seqs(z.rng, 30, 0), tail=3, tables={LL: FSE_LL5})
    z.comp(_seqs(z.rng, 30, len(z.out)), tables={LL: "repeat", OF: FSE_OF5})
    z.comp([], tail=12)
    z.comp(_seqs(z.rng, 30, len(z.out)), tables={LL: "repeat", OF: "repeat", ML: FSE_ML5})
    z.rle(17)
    z.comp(_seqs(z.rng, 70, len(z.out)), tail=2, tables={LL: "repeat", OF: "repeat", ML: "repeat"})
    return case(z)


def _z4_rle_and_predefined_repeated():
    """Z4: RLE mode for each table (offsets: code 4, match lengths: code 6, literal lengths: code 2), then Repeat of the RLE
    tables; Predefined tables, then Repeat of them."""
    z = Z(35)
    z.comp([(30, 4, 5)], tail=1)
    rle = [(2, 9, 16 - 3 + int(z.rng.integers(0, 16))) for _ in range(20)]        # offset values 16..31: code 4
    z.comp(rle, tables={LL: ("rle", 2), OF: ("rle", 4), ML: ("rle", 6)})
    z.comp(rle[:7], tail=3, tables={LL: "repeat", OF: "repeat", ML: "repeat"})
    z.comp(_seqs(z.rng, 20, len(z.out)), tail=1)
    z.comp(_seqs(z.rng, 20, len(z.out)), tables={LL: "repeat", OF: "repeat", ML: "repeat"})
    return case(z)


def _z4_max_accuracy():
    """Z4: descriptions of the maximum accuracy, 9 / 8 / 9, over all 36 / 20 / 53 codes."""
    z = Z(36)
    z.raw(3000)
    tables = {LL: ("fse", spread_counts(range(36), 9), 9), OF: ("fse", spread_counts(range(20), 8), 8), ML: ("fse", spread_counts(range(53), 9), 9)}
    seqs = _seqs(z.rng, 300, len(z.out), ll=(0, 40), ml=(3, 80))
    z.comp(seqs, tail=5, tables=tables, lits=("huf", W_TEXT, 4))
    return case(z)


LESS_THAN_ONE = [6, 0, 0, 0, 0, 0, 0, 0, 8, -1, 0, 0, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 12, -1]     # 32 cells; zero runs of 7, 2 and 12


def _z4_less_than_one():
    """Z4: a description with two "less than 1" probabilities and zero runs of 7, 2 and 12 symbols: behind the first zero of a
    run the 2-bit repeat flags 3, 3, 0 -- 1 -- 3, 3, 3, 2 (3: another flag follows)."""
    z = Z(37)
    z.raw(50)
    assert len(LESS_THAN_ONE) == 27 and sum(abs(c) for c in LESS_THAN_ONE) == 32
    desc = fse_description(LESS_THAN_ONE, 5)
    seqs = [(ll, 5, 9) for ll in (0, 8, 9, 12, 64, 130, 9, 100, 12, 8, 0, 200, 9)]
    z.comp(seqs, tail=2, tables={LL: ("fse", LESS_THAN_ONE, 5, desc)}, lits=("rle",))
    return case(z)


NSEQ = (1, 63, 64, 65, 127, 128, 255, 256, 257, 32511, 32512)


def _z5_count(n, tail):
    """Z5: a block of n sequences (ll = 1, ml = 3; 4 bytes each): the 1- / 2- / 3-byte counts, the 64-sequence group, `per`
    (descriptors per slice, (n + 1 + 255) / 256 rounded up) going from 1 to 2 at 256; with `tail` literals behind the last
    sequence or without (then the literals-only descriptor does not exist and the last slice is full where n is a
    multiple of `per`)."""
    z = Z(40 + n)
    z.raw(64)
    rng = z.rng
    offs = rng.integers(1, 65, n)
    seqs = [(1, 3, int(o)) for o in offs]
    z.comp(seqs, tail=tail)
    pad = (-len(z.out)) % 8
    if pad:
        z.rle(pad)
    return case(z, "int64")


def _z6_positions():
    """Z6: the repeat codes 1, 2, 3 with literals and without (value 3 without: rep0 - 1) as the FIRST sequence of a frame
    (history 1 / 4 / 8; the frame begins with a raw block so there is something to copy), one frame each; value 3 without
    literals comes third, behind a fresh offset (as the first it is rep0 - 1 = 0: invalid_cases)."""
    out = {}
    for code in (1, 2, 3):
        for ll in (2, 0):
            if (code, ll) == (3, 0):
                continue          # rep0 - 1 with rep0 = 1: invalid_cases()
            z = Z(60 + 2 * code + ll)
            z.raw(16)
            z.comp([(ll, 5, ("r", code)), (1, 4, ("r", 2)), (2, 4, 9), (0, 3, ("r", 3)), (0, 6, ("r", 1))], tail=2)
            out["z6_first_code%d_ll%d" % (code, ll)] = case(z)
    return out


def _z6_boundaries(n, at):
    """Z6: a block of n sequences (fresh offsets, each different) where the sequences around index `at` are the repeat codes
    1, 2, 3 with and without literals: at - 3 .. at + 2, six of them either side of the boundary."""
    z = Z(70 + n + at)
    z.raw(200)
    seqs = []
    for i in range(n):
        k = i - (at - 3)
        if 0 <= k < 6:
            seqs.append((0 if k % 2 else 1, 4, ("r", 1 + (k * 5 + at) % 3)))
        else:
            seqs.append((int(z.rng.integers(0, 3)), 4, int(z.rng.integers(20, 190))))
    z.comp(seqs, tail=1)
    # the next block begins with repeat codes: a block boundary
    z.comp([(0, 4, ("r", 3)), (0, 5, ("r", 1)), (1, 3, ("r", 3)), (0, 4, ("r", 2)), (2, 3, ("r", 2))], tail=1)
    return case(z)


def _z6_only_repeats():
    """Z6: a block of 400 sequences that are ALL repeat codes (every slice's function is symbolic: only zstd_layout, with the
    history block 0 left, can resolve them), between two ordinary blocks, a raw block in front of it."""
    z = Z(80)
    z.comp([(300, 4, 250), (2, 5, 131), (1, 4, 77)], tail=2)
    z.raw(33)
    seqs = [(int(z.rng.integers(0, 2)), 3 + int(z.rng.integers(0, 3)), ("r", int(z.rng.integers(1, 4)))) for _ in range(400)]
    z.comp(seqs, tail=1)
    z.comp([(1, 4, ("r", 2)), (0, 4, ("r", 3))], tail=3)
    return case(z)


def _z7_longest_codes():
    """Z7: literal-length code 35 (65536 + 16 extra bits: 70000 literals), match-length code 52 (65539 + 16 bits: 131000) and
    the largest offset the buffer has room for with ALL extra bits set: 2^18 - 4 (value 2^18 - 1, code 17) in the third
    128 KiB block."""
    z = Z(90)
    z.comp([(70000, 50000, 3)], tail=5)
    z.comp([(2, 131000, 70000)], tail=1)
    z.raw(BLOCK_MAX - 2000)
    assert len(z.out) > (1 << 18)
    z.comp([(3, 900, (1 << 18) - 4), (0, 3, ("r", 1))], tail=2)
    return case(z)


def _z7_fat_sequences(lead):
    """Z7: 220 sequences of 58 to 59 bits each, as fat as a 128 KiB block has room for 200 of (the worst case, 88 bits, needs
    lengths of 64 KiB): offset codes 17 / 18 (17 or 18 extra bits), match-length code 43 (7), literal-length code 27 (8) and,
    every ninth, literal length 0; tables of the maximum accuracy where those codes own ONE cell, so every state takes
    9 + 8 + 9 bits.  1.6 KiB of bitstream: the 1 KiB window is refilled before every group of 64.  `lead` literals behind the
    last sequence shift where the bitstream begins: every alignment 0..3 (the host test looks)."""
    z = Z(95)
    z.raw(BLOCK_MAX).raw(BLOCK_MAX)
    tables = {LL: ("fse", spread_counts(range(36), 9, heavy=[1, 2, 3]), 9), OF: ("fse", spread_counts(range(20), 8, heavy=[1, 2]), 8),
              ML: ("fse", spread_counts(range(53), 9, heavy=[0, 1]), 9)}
    seqs, pos = [], len(z.out)
    for i in range(220):
        ll = int(z.rng.integers(256, 300)) if i % 9 else 0
        ml = int(z.rng.integers(131, 200))
        pos += ll
        seqs.append((ll, ml, int(z.rng.integers(1 << 17, pos))))
        pos += ml
    z.comp(seqs, tail=lead, tables=tables)
    return case(z)


def _z8_headers():
    """Z8: name -> case.  Single segment with a 1-, 2- (256 and 65791), 4- and 8-byte content size; a window descriptor and
    no content size (only zstd_layout checks the size); a window descriptor with mantissa 5 (1 KiB + 5/8) and a 4-byte size."""
    out = {}
    for name, n, kw in (("fcs1", 200, dict(fcs_bytes=1)), ("fcs2_256", 256, dict(fcs_bytes=2)), ("fcs2_65791", 65791, dict(fcs_bytes=2)),
                        ("fcs4", 300, dict(fcs_bytes=4)), ("fcs8", 300, dict(fcs_bytes=8)), ("window_no_size", 5000, dict(window=0x10)),
                        ("window_mantissa", 1600, dict(window=0x05, fcs_bytes=4))):
        z = Z(100 + n)
        z.comp([(20, 4, 3), (3, 5, ("r", 2))], tail=3)
        left = n - len(z.out)
        if left > 1000:
            z.raw(min(left - 600, 1200 if "window" in kw else BLOCK_MAX))
            left = n - len(z.out)
        if left > 40:
            z.comp([(5, left - 40, 17)], tail=35)
        else:
            z.rle(left)
        assert len(z.out) == n
        out["z8_" + name] = case(z, **kw)
    return out


_valid = None


def valid_cases():
    """name -> case (dtype, frame, want).  Every frame is valid: tests/test_zstd_frames_host.py holds libzstd to that.  Built
    once per process (the two 32.5 k-sequence cases take a second each)."""
    global _valid
    if _valid is not None:
        return _valid
    c = {}
    c["z1_block_types"] = _z1_block_types()
    c["z1_rle_sizes"] = _z1_rle_sizes()
    c["z1_raw_first"] = _z1_raw_first()
    c["z2_rle_literals"] = _z2_rle_literals()
    c["z2_raw_alignment"] = _z2_raw_alignment()
    c["z2_huffman_streams"] = _z2_huffman_streams()
    c["z2_treeless"] = _z2_treeless()
    for i, (name, w) in enumerate(huffman_tables().items()):
        c["z3_" + name] = _huf_case(20 + i, w, streams=4 if name == "quarters" else 1)
    c["z3_long_stream"] = _z3_long_stream()
    for t, name in enumerate(("ll", "of", "ml")):
        c["z4_repeat_" + name] = _z4_repeat_each(t)
    c["z4_three_sources"] = _z4_three_sources()
    c["z4_rle_and_predefined_repeated"] = _z4_rle_and_predefined_repeated()
    c["z4_max_accuracy"] = _z4_max_accuracy()
    c["z4_less_than_one"] = _z4_less_than_one()
    for n in NSEQ:
        c["z5_nseq_%d_tail" % n] = _z5_count(n, 3)
        c["z5_nseq_%d_no_tail" % n] = _z5_count(n, 0)
    c.update(_z6_positions())
    c["z6_group_boundary"] = _z6_boundaries(130, 64)        # per = 1: also a slice boundary at every sequence
    c["z6_slice_boundary_per2"] = _z6_boundaries(300, 150)  # per = 2: sequences 149 | 150 lie in different slices
    c["z6_slice_inside_per2"] = _z6_boundaries(300, 151)    # ... and 150 | 151 in the same one
    c["z6_group_boundary_per2"] = _z6_boundaries(300, 128)
    c["z6_only_repeats"] = _z6_only_repeats()
    c["z7_longest_codes"] = _z7_longest_codes()
    for lead in range(4):
        c["z7_fat_sequences_%d" % lead] = _z7_fat_sequences(lead)
    c.update(_z8_headers())
    _valid = c
    return c


def libzstd_all_quarters():
    """The one frame of the corpus libzstd writes (through pyarrow): 60000 literals over all 256 byte values, geometrically
    skewed -- FSE-compressed Huffman weights (the one coverage counter the builder cannot reach) and symbols in all four
    quarters 0..63 / 64..127 / 128..191 / 192..255 of the kernel's table fill."""
    import pyarrow as pa
    rng = np.random.default_rng(7)
    p = 0.985 ** ((np.arange(256) * 37) % 256)
    want = rng.choice(256, 60000, p=p / p.sum()).astype(np.uint8).tobytes()
    return dict(dtype="uint8", frame=pa.Codec("zstd", compression_level=3).compress(want, asbytes=True), want=want)


# ------------------------------------------------------------------------------------ the corpus: refused by the walk
def refused_cases():
    """name -> case: valid frames WalkZstdFrame does not take; the host library decompresses the record batch."""
    import pyarrow as pa
    out = {}
    z = Z(200)
    z.comp([(20, 4, 3), (3, 5, ("r", 2))], tail=3).rle(40)
    base = case(z)
    # content checksum: the low 32 bits of XXH64(content), taken from a frame libzstd wrote for the same content
    import ctypes as C
    L = libzstd()
    cctx = L.ZSTD_createCCtx()
    assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(cctx, 201, 1))          # ZSTD_c_checksumFlag
    dst = C.create_string_buffer(1024)
    n = L.ZSTD_compress2(cctx, dst, 1024, base["want"], len(base["want"]))
    assert not L.ZSTD_isError(n)
    L.ZSTD_freeCCtx(cctx)
    theirs = dst.raw[:n]
    assert theirs[4] & 0x04
    out["content_checksum"] = dict(base, frame=z.frame(checksum=True) + theirs[-4:])
    out["trailing_skippable_frame"] = dict(base, frame=base["frame"] + skippable_frame())
    z2 = Z(201)
    z2.raw(30).comp([(2, 6, 11)], tail=1)
    # no content size in either: the reader compares a frame's content size, where it has one, with the buffer's length
    out["two_frames"] = dict(dtype="uint8", frame=z.frame(window=0x10) + z2.frame(window=0x10), want=z.want + z2.want)
    return out


# --------------------------------------------------------------------------------------------------- the corpus: invalid
def invalid_cases():
    """name -> (frame, declared length, on_device, why, want): frames that must end in an error.  on_device: whether the walk
    takes the frame (the kernels must refuse it) or refuses it itself (the host library then has the last word).  `why` cites
    the bound that stops the case on the device.  want: None, or what the blocks mean where only the frame around them is
    invalid (block_larger_than_the_window: libzstd's one-shot decoder does not look at the window, see the host test)."""
    out = {}

    def add(name, z, on_device=True, why="", want=False, **kw):
        out[name] = (z.frame(**kw), kw.get("declared") or len(z.out), on_device, why, z.want if want else None)

    z = Z(300)
    z.raw(100).comp([(4, 8, 105)], tail=4, tamper=dict(execute=False))
    add("offset_one_byte_in_front_of_the_buffer", z, why="k8_expand_local: an offset larger than the sequence's position in the buffer fails the batch")
    z = Z(301)
    z.raw(100).comp([(0, 8, ("r", 3))], tail=4, tamper=dict(execute=False))
    add("rep0_minus_1_is_zero", z, why="RepStep returns 0 for s0 = 1; group(): off == 0 -> bad")
    z = Z(302)
    z.raw(100).comp([(4, 8, 10), (5, 4, 3)], tail=0, lits=("raw", dict(declare=8)), tamper=dict(execute=False))
    add("literal_length_overruns_the_literals", z, declared=100 + 8 + 12, why="group(): ll > z.lit_regen - lit_i -> bad")
    z = Z(303)
    z.raw(100).comp([(4, 70000, 10), (5, 70000, 3)], tail=3, tamper=dict(execute=False))
    add("block_output_passes_128_kib", z, why="group(): ll + ml > kBlockMax - out_i -> bad")
    z = Z(304)
    z.raw(100).comp(_seqs(z.rng, 9, 100), tail=2, tamper=dict(bitstream=lambda b: b"\0" + b))
    add("bitstream_one_byte_too_many", z, why="zstd_entropy: after the last sequence q == floor must hold")
    z = Z(305)
    z.raw(100).comp(_seqs(z.rng, 9, 100), tail=2, tamper=dict(bitstream=lambda b: b[1:]))
    add("bitstream_runs_out", z, why="step(): p_of_b < floor -> false, before any word below the stream is used")
    z = Z(306)
    z.raw(100).comp(_seqs(z.rng, 9, 100), tail=2, tamper=dict(bitstream=lambda b: b + b"\0"))
    add("bitstream_last_byte_zero", z, why="zstd_entropy: last_u != 0, else no head position is formed")
    z = Z(307)
    # the listed weights 2, 2, 1 stand for 2 + 2 + 1 = 5 cells: the rest to 8 is 3, no power of two
    z.raw(100).comp([(30, 4, 9)], tail=10, lits=("huf", [2, 1, 1, 3], 1, dict(description=bytes([127 + 3, (2 << 4) | 2, 1 << 4]))),
                    tamper=dict(execute=False))
    add("huffman_weights_do_not_complete_a_power_of_two", z, why="ReadHuffmanWeights: rest & (rest - 1) -> 0; s_fail, no stream is decoded")
    z = Z(308)
    desc = bytearray(fse_description(FSE_OF5[1], 5))
    desc[0] = (desc[0] & 0xF0) | 4        # accuracy log 9 for offsets (maximum: 8)
    z.raw(100).comp(_seqs(z.rng, 9, 100), tail=2, tables={OF: ("fse", FSE_OF5[1], 5, bytes(desc))}, tamper=dict(execute=False))
    add("fse_accuracy_log_above_the_maximum", z, why="ReadNCount: al > MaxLog(type) -> 0; s_fail before any table cell is written")
    z = Z(309)
    z.raw(100).comp(_seqs(z.rng, 9, 100), tail=2)
    add("eight_bytes_fewer_than_declared", z, declared=len(z.out) + 8, why="zstd_layout: at - out_off == out_len")
    z = Z(310)
    z.comp([(20, 4, 3)], tail=3).raw(2000)
    add("block_larger_than_the_window", z, on_device=False, want=True, window=0x00, why="WalkZstdFrame: size > block_max")
    z = Z(311)
    z.valid = False
    z.raw(100).comp([(30, 4, 9)], tail=10, lits=("treeless", 1), tamper=dict(execute=False))
    add("treeless_without_a_table", z, on_device=False, why="WalkZstdFrame: last_huf == none")
    z = Z(312)
    z.valid = False
    z.raw(100).comp(_seqs(z.rng, 9, 100), tail=2, tables={ML: "repeat"}, tamper=dict(execute=False))
    add("repeat_mode_without_a_table", z, on_device=False, why="WalkZstdFrame: last_tbl[t] == none")
    return out


# ---------------------------------------------------------------------------------------------------------------- libzstd
_lib = None


def libzstd():
    global _lib
    if _lib is None:
        import ctypes as C
        L = C.CDLL("libzstd.so.1")
        L.ZSTD_decompress.restype = C.c_size_t
        L.ZSTD_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        L.ZSTD_isError.restype = C.c_uint
        L.ZSTD_isError.argtypes = [C.c_size_t]
        L.ZSTD_getErrorName.restype = C.c_char_p
        L.ZSTD_getErrorName.argtypes = [C.c_size_t]
        L.ZSTD_createCCtx.restype = C.c_void_p
        L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
        L.ZSTD_CCtx_setParameter.restype = C.c_size_t
        L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.ZSTD_compress2.restype = C.c_size_t
        L.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
        _lib = L
    return _lib


def libzstd_decompress(frame, capacity):
    """ZSTD_decompress (what host_codec.cpp calls) into `capacity` bytes -> the bytes; ValueError with libzstd's error name."""
    import ctypes as C
    L = libzstd()
    dst = C.create_string_buffer(capacity + 1)
    n = L.ZSTD_decompress(dst, capacity, bytes(frame), len(frame))
    if L.ZSTD_isError(n):
        raise ValueError(L.ZSTD_getErrorName(n).decode())
    return dst.raw[:n]
