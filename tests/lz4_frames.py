"""LZ4 frames for tests, built byte by byte (lz4_Frame_format.md, lz4_Block_format.md): the flavours pyarrow never writes.

seq() / frame() assemble sequences, blocks and frames; decode_blocks() is a naive decoder that says what a hand-built frame
means; liblz4_frame() asks liblz4 (the library host_codec.cpp loads) for the flavours LZ4F_compressFrame can write.  The
corpus of hand-built frames (hand_built_cases / invalid_cases / refused_cases) is shared by tests/test_lz4_frames_host.py,
which proves it against liblz4 on the CPU, and tests/test_gpu_lz4_frames.py, which feeds it to the kernels.  No GPU here."""
import ctypes as C
import struct

import numpy as np

MAGIC = 0x184D2204
CHUNK = 8192          # kChunkBytes of kernels_lz4.hip: the unit of k8_expand_local / k8_emit
DP_MAX = 51200        # kDpMaxComp: the largest compressed block lz4_parse_dp takes
LDS_MAX = 59360       # the largest compressed block lz4_parse<true> takes (max_block_comp + 32 + 6144 <= 65536)


# ------------------------------------------------------------------------------------------------------------ xxh32
_P1, _P2, _P3, _P4, _P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
_M = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M


def xxh32(data, seed=0):
    """XXH32 of `data` (xxhash specification), pure Python: ~25 ms for 57 KiB."""
    data = bytes(data)
    n = len(data)
    i = 0
    if n >= 16:
        v1, v2, v3, v4 = (seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed & _M, (seed - _P1) & _M
        words = struct.unpack_from("<%dI" % (n // 16 * 4), data)
        for k in range(0, len(words), 4):
            v1 = (_rotl((v1 + words[k] * _P2) & _M, 13) * _P1) & _M
            v2 = (_rotl((v2 + words[k + 1] * _P2) & _M, 13) * _P1) & _M
            v3 = (_rotl((v3 + words[k + 2] * _P2) & _M, 13) * _P1) & _M
            v4 = (_rotl((v4 + words[k + 3] * _P2) & _M, 13) * _P1) & _M
        i = n // 16 * 16
        h = (_rotl(v1, 1) + _rotl(v2, 7) + _rotl(v3, 12) + _rotl(v4, 18)) & _M
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 4 <= n:
        h = (_rotl((h + struct.unpack_from("<I", data, i)[0] * _P3) & _M, 17) * _P4) & _M
        i += 4
    while i < n:
        h = (_rotl((h + data[i] * _P5) & _M, 11) * _P1) & _M
        i += 1
    h ^= h >> 15
    h = (h * _P2) & _M
    h ^= h >> 13
    h = (h * _P3) & _M
    h ^= h >> 16
    return h


# ------------------------------------------------------------------------------------------------- sequences, frames
def _extension(v):
    """The bytes that follow a nibble of 15: 255s, then the rest (which may be 0)."""
    v -= 15
    return b"\xff" * (v // 255) + bytes([v % 255])


def seq(ll, literals, offset=None, ml=None):
    """One LZ4 sequence: token, literal-length extension, literals and -- when `ml` (the real match length, >= 4) is given --
    the 2-byte offset and the match-length extension.  Without `ml`: a block's last sequence, literals only."""
    literals = bytes(literals)
    assert ll == len(literals)
    if ml is None:
        assert offset is None
        return bytes([min(ll, 15) << 4]) + (_extension(ll) if ll >= 15 else b"") + literals
    assert ml >= 4 and 0 <= offset <= 0xFFFF
    m = ml - 4
    return (bytes([(min(ll, 15) << 4) | min(m, 15)]) + (_extension(ll) if ll >= 15 else b"") + literals + struct.pack("<H", offset)
            + (_extension(m) if m >= 15 else b""))


def frame(blocks, bsid=4, independent=False, content_size=None, block_checksum=False, content_checksum=None, stored=(),
          dict_id=None):
    """An LZ4 frame around `blocks` (the block data as it is: compressed, or for indices in `stored` the bytes themselves).
    content_size / content_checksum / dict_id: the VALUE to write, or None to leave the field (and its FLG bit) out."""
    flg = 0x40 | (0x20 if independent else 0) | (0x10 if block_checksum else 0) | (0x08 if content_size is not None else 0) \
        | (0x04 if content_checksum is not None else 0) | (0x01 if dict_id is not None else 0)
    descriptor = bytes([flg, bsid << 4])
    if content_size is not None:
        descriptor += struct.pack("<Q", content_size)
    if dict_id is not None:
        descriptor += struct.pack("<I", dict_id)
    out = [struct.pack("<I", MAGIC), descriptor, bytes([(xxh32(descriptor) >> 8) & 0xFF])]
    for i, b in enumerate(blocks):
        out.append(struct.pack("<I", len(b) | (0x80000000 if i in stored else 0)))
        out.append(bytes(b))
        if block_checksum:
            out.append(struct.pack("<I", xxh32(b)))
    out.append(struct.pack("<I", 0))
    if content_checksum is not None:
        out.append(struct.pack("<I", content_checksum))
    return b"".join(out)


def decode_blocks(blocks, stored=(), independent=False):
    """What the blocks decompress to: a naive decoder, a byte at a time wherever a match overlaps its own output (a match
    that does not is the slice it names).  Raises ValueError on offset 0, on an offset that reaches in front of what the
    block may see (the buffer's first byte with linked blocks, the block's own with independent ones) and on a block that
    ends inside a sequence."""
    out = bytearray()
    for bi, b in enumerate(blocks):
        b = bytes(b)
        if bi in stored:
            out += b
            continue
        floor = len(out) if independent else 0
        ip, end = 0, len(b)
        while True:
            if ip >= end:
                raise ValueError("block %d ends without a last sequence" % bi)
            token = b[ip]
            ip += 1
            ll = token >> 4
            if ll == 15:
                while True:
                    if ip >= end:
                        raise ValueError("block %d: literal length runs past the block" % bi)
                    x = b[ip]
                    ip += 1
                    ll += x
                    if x != 255:
                        break
            if ll > end - ip:
                raise ValueError("block %d: literals run past the block" % bi)
            out += b[ip: ip + ll]
            ip += ll
            if ip == end:
                break
            if end - ip < 2:
                raise ValueError("block %d: no room for an offset" % bi)
            offset = b[ip] | (b[ip + 1] << 8)
            ip += 2
            ml = token & 15
            if ml == 15:
                while True:
                    if ip >= end:
                        raise ValueError("block %d: match length runs past the block" % bi)
                    x = b[ip]
                    ip += 1
                    ml += x
                    if x != 255:
                        break
            ml += 4
            if offset == 0:
                raise ValueError("block %d: offset 0" % bi)
            src = len(out) - offset
            if src < floor:
                raise ValueError("block %d: offset %d reaches %d bytes in front of what the block may see" % (bi, offset, floor - src))
            if offset >= ml:
                out += out[src: src + ml]
            else:
                for k in range(ml):
                    out.append(out[src + k])
    return bytes(out)


# --------------------------------------------------------------------------------------------------------- liblz4
class _FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int), ("frameType", C.c_int),
                ("contentSize", C.c_ulonglong), ("dictID", C.c_uint), ("blockChecksumFlag", C.c_int)]


class _Preferences(C.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint), ("favorDecSpeed", C.c_uint),
                ("reserved", C.c_uint * 3)]


_lib = None


def _liblz4():
    global _lib
    if _lib is None:
        L = C.CDLL("liblz4.so.1")
        L.LZ4F_compressFrameBound.restype = C.c_size_t
        L.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.POINTER(_Preferences)]
        L.LZ4F_compressFrame.restype = C.c_size_t
        L.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(_Preferences)]
        L.LZ4F_isError.restype = C.c_uint
        L.LZ4F_isError.argtypes = [C.c_size_t]
        L.LZ4F_getErrorName.restype = C.c_char_p
        L.LZ4F_getErrorName.argtypes = [C.c_size_t]
        L.LZ4F_createDecompressionContext.restype = C.c_size_t
        L.LZ4F_createDecompressionContext.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        L.LZ4F_freeDecompressionContext.restype = C.c_size_t
        L.LZ4F_freeDecompressionContext.argtypes = [C.c_void_p]
        L.LZ4F_decompress.restype = C.c_size_t
        L.LZ4F_decompress.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p]
        _lib = L
    return _lib


def liblz4_frame(data, bsid=4, independent=False, content_checksum=False, block_checksum=False, content_size=False, level=0):
    """LZ4F_compressFrame(data) with these preferences -> (frame bytes, FLG, BD).  LZ4F_compressFrame lowers the block size
    for small inputs and turns to independent blocks when the input fits one block: FLG and BD are those of the frame it
    WROTE, for the caller to assert on."""
    L = _liblz4()
    data = bytes(data)
    p = _Preferences()
    p.frameInfo.blockSizeID = bsid
    p.frameInfo.blockMode = 1 if independent else 0
    p.frameInfo.contentChecksumFlag = 1 if content_checksum else 0
    p.frameInfo.blockChecksumFlag = 1 if block_checksum else 0
    p.frameInfo.contentSize = len(data) if content_size else 0
    p.compressionLevel = level
    cap = L.LZ4F_compressFrameBound(len(data), C.byref(p))
    dst = C.create_string_buffer(cap)
    n = L.LZ4F_compressFrame(dst, cap, data, len(data), C.byref(p))
    if L.LZ4F_isError(n):
        raise RuntimeError(L.LZ4F_getErrorName(n).decode())
    out = dst.raw[:n]
    assert struct.unpack_from("<I", out)[0] == MAGIC
    return out, out[4], out[5]


def liblz4_decompress(frame_bytes, capacity):
    """LZ4F_decompress of one whole frame into `capacity` bytes -> the bytes it produced.  Raises ValueError with liblz4's
    error name when it rejects the frame, or when the frame does not end inside `frame_bytes` / `capacity`."""
    L = _liblz4()
    ctx = C.c_void_p()
    rc = L.LZ4F_createDecompressionContext(C.byref(ctx), 100)
    assert not L.LZ4F_isError(rc)
    try:
        src = C.create_string_buffer(bytes(frame_bytes), len(frame_bytes))
        dst = C.create_string_buffer(capacity + 1)
        s_at = d_at = 0
        while True:
            d_n, s_n = C.c_size_t(capacity - d_at), C.c_size_t(len(frame_bytes) - s_at)
            rc = L.LZ4F_decompress(ctx, C.byref(dst, d_at), C.byref(d_n), C.byref(src, s_at), C.byref(s_n), None)
            if L.LZ4F_isError(rc):
                raise ValueError(L.LZ4F_getErrorName(rc).decode())
            d_at += d_n.value
            s_at += s_n.value
            if rc == 0:
                return dst.raw[:d_at]
            if d_n.value == 0 and s_n.value == 0:
                raise ValueError("frame does not end: %d of %d input bytes, %d of %d output bytes" % (s_at, len(frame_bytes), d_at, capacity))
    finally:
        L.LZ4F_freeDecompressionContext(ctx)


# ----------------------------------------------------------------------------------------------- building blocks
class Blocks:
    """Blocks under construction.  Literals are random bytes; lit() / match() append to the open block, end() closes it with
    its last, literals-only sequence.  Every closed block obeys liblz4's end-of-block rules: the last sequence has >= 5
    literals and the last match ends >= 12 bytes before the block's end (end() tops the pending literals up to 12)."""

    def __init__(self, seed, bsid=4):
        self.rng = np.random.default_rng(seed)
        self.bsid = bsid
        self.block_max = 1 << (8 + 2 * bsid)
        self.blocks, self.stored = [], set()
        self.parts, self.pending = [], b""
        self.pos = 0            # output bytes so far, all blocks
        self.block_start = 0    # ... when the open block began

    @property
    def bpos(self):
        return self.pos - self.block_start

    def comp(self):
        """Compressed bytes of the open block so far (the pending literals not counted)."""
        return sum(len(p) for p in self.parts)

    def lit(self, n):
        self.pending += self.rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        self.pos += n

    def lit_to(self, bpos):
        assert bpos >= self.bpos
        self.lit(bpos - self.bpos)

    def match(self, offset, ml):
        self.parts.append(seq(len(self.pending), self.pending, offset, ml))
        self.pending = b""
        self.pos += ml

    def end(self, tail=12):
        if self.parts and len(self.pending) < tail:
            self.lit(tail - len(self.pending))
        self.parts.append(seq(len(self.pending), self.pending))
        assert self.bpos <= self.block_max, (self.bpos, self.block_max)
        self.blocks.append(b"".join(self.parts))
        self.parts, self.pending, self.block_start = [], b"", self.pos

    def stored_block(self, n):
        assert not self.parts and not self.pending and n <= self.block_max
        self.stored.add(len(self.blocks))
        self.blocks.append(self.rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        self.pos += n
        self.block_start = self.pos

    def finish(self, multiple=8, remainder=0):
        """Close the last block so that the total length is `remainder` modulo `multiple`."""
        short = max(12 - len(self.pending), 0) if self.parts else 0
        self.lit(short + (remainder - self.pos - short) % multiple)
        self.end()
        assert self.pos % multiple == remainder
        return self

    def random_block(self, out_len, max_ll=40, max_ml=300, overlap=True):
        """A block of exactly out_len output bytes: random literal runs and matches at random offsets into everything
        before them (earlier blocks included), some overlapping their own output."""
        assert not self.parts and not self.pending
        target = self.block_start + out_len
        if self.pos == 0:
            self.lit(min(out_len, 16))
        while target - self.pos > 12 + max_ll + max_ml:
            self.lit(int(self.rng.integers(0, max_ll + 1)))
            ml = int(self.rng.integers(4, max_ml + 1))
            reach = min(self.pos, 65535)
            offset = int(self.rng.integers(1, reach + 1))
            if overlap and self.rng.random() < 0.2:
                offset = int(self.rng.integers(1, min(reach, 16) + 1))
            self.match(offset, ml)
        self.lit(target - self.pos)
        self.end(tail=0)
        assert self.pos == target


def column(b, dtype="int64", independent=False, **flags):
    """A column of a case: the frame's blocks and flavour, and the bytes it stands for (decode_blocks)."""
    want = decode_blocks(b.blocks, b.stored, independent)
    assert len(want) == b.pos and len(want) % np.dtype(dtype).itemsize == 0
    return dict(dtype=dtype, blocks=b.blocks, stored=frozenset(b.stored), bsid=b.bsid, independent=independent, flags=flags, want=want)


def column_frame(col, want=None):
    """The frame bytes of a column (checksums and content size computed from its bytes where its flags ask for them)."""
    want = col["want"] if want is None else want
    f = col["flags"]
    return frame(col["blocks"], bsid=col["bsid"], independent=col["independent"], stored=col["stored"],
                 content_size=len(want) if f.get("content_size") else None, block_checksum=bool(f.get("block_checksum")),
                 content_checksum=xxh32(want) if f.get("content_checksum") else None, dict_id=f.get("dict_id"))


# ------------------------------------------------------------------------------------------------- the corpus: valid
def _h1_chain(chunks, offset=CHUNK, bsid=4):
    """H1: 8192 random bytes, then nothing but non-overlapping matches of 8192 bytes at `offset`: every chunk links one hop
    back into the chunk before it, so the last chunk's chain crosses `chunks - 1` chunk boundaries one at a time (the 16
    literals that must end a block restart the chain for 16 positions out of 65536)."""
    b = Blocks(100 + chunks + offset, bsid)
    total = chunks * CHUNK
    while b.pos < total:
        stop = min(b.block_start + b.block_max, total) - 16
        if b.pos == 0:
            b.lit(CHUNK if offset <= CHUNK else CHUNK + 8)
        while b.pos < stop:
            b.match(offset, min(CHUNK, stop - b.pos))
        b.lit(16)
        b.end()
    assert b.pos == total
    return column(b)


def _h2_odd_blocks(total, dtype):
    """H2: blocks of 65533, 8191, 8193 and 1 output bytes, then more: later blocks begin at positions that are no multiple
    of 4 (the (lo & 3) != 0 branches of k8_expand_local and k8_emit), chunks end in 1 to 3 odd bytes, matches reach back
    across all of it.  `total` output bytes in all."""
    b = Blocks(200 + total % 97)
    for n in (65533, 8191, 8193):
        b.random_block(n)
    b.lit(1)
    b.end(tail=0)          # one byte: a block without a match needs no 12-byte tail
    for n in (20001, 8194, 3):
        b.random_block(n)
    while total - b.pos > b.block_max:
        b.random_block(65531)
    b.lit(40)
    b.match(30000, 500)
    b.match(9, 77)
    b.lit_to(total - b.block_start)
    b.end()
    assert b.pos == total
    return column(b, dtype)


H2_ROWS = 110749           # rows of the H2 table: the uint8 column's bytes, 5 modulo 8


_EXT = (14, 15, 16, 269, 270, 271, 524, 525, 15 + 255 * 20)


def _h3_extensions():
    """H3: literal length and match length - 4 each take 14, 15 (15 + 0), 16, 269, 270 (15 + 255 + 0), 271, 524, 525
    (15 + 255 + 255 + 0) and 15 + 255 * 20, in every combination."""
    b = Blocks(300)
    for ll in _EXT:
        for m in _EXT:
            if b.bpos + ll + m + 4 + 12 > b.block_max:
                b.end()
            b.lit(ll)
            b.match(int(b.rng.integers(1, min(b.pos, 65535) + 1)), m + 4)
    b.finish()
    return column(b)


def _h4_overlaps():
    """H4: overlapping matches (offset < length) at offsets 1, 2, 3, 4, 7: lengths around the offset, around kLongSeq (128:
    with one literal in front, sequence lengths 127 to 130) and 20000; each placed across a chunk boundary (20000 spans
    three)."""
    b = Blocks(400)
    for offset in (1, 2, 3, 4, 7):
        for ml in sorted({max(4, offset - 1), max(4, offset + 1), 126, 127, 128, 129, 20000}):
            boundary = (b.bpos // CHUNK + 1) * CHUNK
            if boundary - b.bpos < ml // 2 + 8:
                boundary += CHUNK
            if boundary + ml + 12 > b.block_max:
                b.end()
                boundary = CHUNK
            b.lit_to(boundary - min(ml // 2, 3000) - 1)
            b.lit(1)
            b.match(offset, ml)
    b.finish()
    return column(b)


def _h5_offsets():
    """H5: offset 65535; an offset that names the buffer's first byte, in the first block and in the second; a linked match
    whose source begins in the previous block and ends in its own."""
    b = Blocks(500)
    b.lit(5000)
    b.match(5000, 100)          # source: byte 0
    b.lit(3)
    b.match(b.pos, 64)          # again, from an odd position
    b.lit_to(60000)
    b.end()
    assert b.pos == 60000
    b.lit(50)
    b.match(150, 120)           # source: the last 100 bytes of block 0 and the first 20 of this one
    b.lit_to(5535)
    assert b.pos == 65535
    b.match(65535, 1000)        # the largest offset there is, and it names byte 0
    b.lit(7)
    b.match(65535, 19)
    b.finish()
    return column(b)


def _h6_literal_run():
    """H6: a block that is one 60000-byte literal run (many parse lanes' segments hold no token at all), a match, the tail."""
    b = Blocks(600)
    b.lit(60000)
    b.match(59999, 300)
    b.finish()
    return column(b)


def _h6_dense(bsid):
    """H6: the densest block there is, ll = 0 / ml = 4 sequences of 3 bytes: as many as Lz4SeqCapacity has room for per lane.
    bsid 4: the 64 KiB of OUTPUT are the limit (16380 sequences, 49 KiB compressed: lz4_parse_dp); bsid 5: 21841 sequences
    fill 64 KiB of compressed size exactly (lz4_parse<false>)."""
    b = Blocks(610 + bsid, bsid)
    b.lit(4096)
    b.end()
    n = 16380 if bsid == 4 else 21841
    for _ in range(n):
        b.match(int(b.rng.integers(1, 4097)), 4)
    b.end()
    assert len(b.blocks[1]) == 3 * n + 13 and (bsid == 4 or len(b.blocks[1]) == 65536)
    b.lit(20)
    b.finish()
    return column(b)


def _h6_tiny_blocks():
    """H6: blocks of 1, 2, 13 and 255 compressed bytes (fewer bytes than parse lanes) between ordinary ones."""
    b = Blocks(620)
    b.random_block(3000)
    b.end(tail=0)               # 1 byte: the token alone, no output
    b.lit(1)
    b.end(tail=0)               # 2 bytes
    b.lit(12)
    b.end(tail=0)               # 13 bytes
    b.lit(99)
    b.match(2000, 18)
    b.lit(150)
    b.end()                     # 1 + 1 + 99 + 2, then 1 + 1 + 150: 255 bytes
    assert [len(x) for x in b.blocks[1:]] == [1, 2, 13, 255]
    b.random_block(5000)
    b.lit(3)
    b.finish()
    return column(b)


def _sized_block(b, comp_size):
    """Appends a block of exactly comp_size compressed bytes to `b`: literal-heavy sequences, then short ones to the byte."""
    assert not b.parts and not b.pending
    if b.pos == 0:
        b.lit(16)
    tail = 1 + 1 + 100                                  # the last sequence: 100 literals
    while comp_size - b.comp() - len(b.pending) - tail > 1200:
        b.lit(1000)
        b.match(int(b.rng.integers(1, min(b.pos, 65535) + 1)), int(b.rng.integers(4, 12)))   # 1 + 4 + 1000 + 2 bytes
    if b.pending:                                       # the 16 bytes that open a buffer
        b.match(int(b.rng.integers(1, b.pos + 1)), 4)
    while True:                                         # sequences of 3 + ll bytes, ll <= 14: any remainder >= 3 can be met
        left = comp_size - b.comp() - tail
        if left == 0:
            break
        ll = 14 if left >= 20 else left - 3 if left <= 17 else 0
        b.lit(ll)
        b.match(int(b.rng.integers(1, min(b.pos, 65535) + 1)), int(b.rng.integers(4, 19)))
    b.lit(100)
    b.end()
    assert len(b.blocks[-1]) == comp_size, (len(b.blocks[-1]), comp_size)


def _h7_selection(sizes, seed):
    """H7: blocks of exactly these compressed sizes in one frame of one record batch (see H7_LAUNCHES)."""
    b = Blocks(seed)
    for n in sizes:
        _sized_block(b, n)
    if b.pos % 8:
        b.stored_block(8 - b.pos % 8)   # a stored block has no token walk: it does not take part in the choice of kernels
    return column(b)


# the five launch combinations of LaunchLz4Decompress: name -> compressed block sizes
H7_LAUNCHES = {
    "h7_dp_only": (DP_MAX, 40000, DP_MAX),                           # lz4_parse_dp alone
    "h7_dp_and_lds": (DP_MAX, LDS_MAX, 300, DP_MAX + 1),             # lz4_parse_dp + lz4_parse<true>, blocks shared through _pad
    "h7_dp_and_global": (DP_MAX, LDS_MAX + 1, 1000),                 # lz4_parse_dp + lz4_parse<false>
    "h7_lds_only": (DP_MAX + 1, LDS_MAX, 55000, DP_MAX + 1),         # lz4_parse<true> alone
    "h7_global_only": (LDS_MAX + 1, 61000, LDS_MAX + 1),             # lz4_parse<false> alone
}


def _h8_stored(**flags):
    """H8: stored blocks (bit 31 of the size word) of odd sizes between compressed ones in a linked frame; matches copy from
    the stored bytes, one from a source that begins in a stored block and ends in the compressed block behind it."""
    b = Blocks(800)
    b.random_block(9001)
    b.stored_block(4099)
    b.lit(30)
    b.match(2000, 900)          # all of it inside the stored block
    b.match(4099 + 30 + 900 + 50, 300)   # begins in block 0, ends in the stored block
    b.end()
    b.stored_block(1)
    b.stored_block(8193)
    b.lit(10)
    b.match(25, 15)             # source: the stored block's last 15 bytes
    b.lit(9)
    b.match(8193 + 10 + 15 + 9 + 1 + 5, 40)   # begins in the compressed block in front of the stored ones
    b.finish()
    return column(b, **flags)


def hand_built_cases():
    """name -> columns.  Every frame is valid: tests/test_lz4_frames_host.py holds liblz4 to that."""
    cases = {}
    for chunks in (24, 26, 27, 630):    # around kSkelHops + 1 = 25 hops, and just over 25 * 25
        cases["h1_chain_%d" % chunks] = [_h1_chain(chunks)]
    cases["h1_chain_26_offset_8191"] = [_h1_chain(26, CHUNK - 1)]
    cases["h1_chain_26_offset_8193"] = [_h1_chain(26, CHUNK + 1)]
    cases["h1_chain_26_one_block"] = [_h1_chain(26, bsid=6)]
    cases["h2_odd_blocks"] = [_h2_odd_blocks(8 * H2_ROWS, "int64"), _h2_odd_blocks(H2_ROWS, "uint8")]
    cases["h3_extensions"] = [_h3_extensions()]
    cases["h4_overlaps"] = [_h4_overlaps()]
    cases["h5_offsets"] = [_h5_offsets()]
    cases["h6_literal_run"] = [_h6_literal_run()]
    cases["h6_dense"] = [_h6_dense(4)]
    cases["h6_dense_64k"] = [_h6_dense(5)]
    cases["h6_tiny_blocks"] = [_h6_tiny_blocks()]
    for i, (name, sizes) in enumerate(H7_LAUNCHES.items()):
        cases[name] = [_h7_selection(sizes, 700 + i)]
    cases["h8_stored"] = [_h8_stored()]
    cases["h8_stored_checksums"] = [_h8_stored(block_checksum=True, content_checksum=True, content_size=True)]
    return cases


SMALL_CASES = ("h2_odd_blocks", "h3_extensions", "h4_overlaps", "h5_offsets", "h6_literal_run", "h6_dense", "h6_dense_64k",
               "h6_tiny_blocks", "h8_stored")      # H9: run once more under each forced parse kernel


# ----------------------------------------------------------------------------------------------- the corpus: invalid
def invalid_cases():
    """name -> (frame bytes, declared uncompressed length): frames liblz4 rejects, or whose blocks do not add up to the
    declared length.  The declared length is a multiple of 8: the frame stands in for an int64 column's data."""
    out = {}
    # block-independent, but the second block's match reaches into the first (as linked blocks it would be valid)
    b = Blocks(900)
    b.random_block(4000)
    b.lit(20)
    b.match(500, 100)
    b.finish()
    assert len(decode_blocks(b.blocks)) == b.pos
    out["independent_match_into_previous_block"] = (frame(b.blocks, independent=True), b.pos)
    b = Blocks(901)
    b.lit(100)
    b.match(0, 40)
    b.finish()
    out["offset_zero"] = (frame(b.blocks), b.pos)
    b = Blocks(902)
    b.lit(100)
    b.match(101, 40)
    b.finish()
    out["offset_one_past_the_buffer_start"] = (frame(b.blocks), b.pos)
    b = Blocks(903, bsid=5)      # built with room, written as bsid 4: 65536 + 8 output bytes
    b.lit(100)
    b.match(50, 65536 + 8 - 100 - 12)
    b.finish()
    assert b.pos == 65536 + 8
    out["block_larger_than_block_max"] = (frame(b.blocks, bsid=4), b.pos)
    b = Blocks(904)
    b.random_block(3000)
    b.random_block(1000)
    out["eight_bytes_short_of_the_declared_length"] = (frame(b.blocks), b.pos + 8)
    return out


def refused_cases():
    """name -> column: frames WalkLz4Frame does not take (the record batch is decompressed by the host library)."""
    b = Blocks(950)
    b.random_block(5000)
    b.lit(4)
    b.finish()
    return {"dictionary_id": column(b, dict_id=7)}


def bsid3_frame():
    """A frame whose BD byte names block size id 3, which lz4_Frame_format.md reserves: (frame, declared length)."""
    b = Blocks(951)
    b.random_block(800)
    return frame(b.blocks, bsid=3), b.pos


# ------------------------------------------------------------------------------------------------- frames in a stream
def ipc_stream(columns, frames, codec="lz4"):
    """An Arrow IPC stream of ONE record batch, written with compression=`codec` ("lz4" or "zstd"), whose column i holds
    columns[i]["want"] as values of columns[i]["dtype"] and whose data buffer i is frames[i] (None: the frame pyarrow wrote)
    behind the length prefix pyarrow wrote.  -> (stream bytes, the pyarrow table)."""
    import pyarrow as pa
    import pyarrow.ipc as ipc
    from helpers import rewrite_buffers
    table = pa.table({"c%d" % i: pa.array(np.frombuffer(c["want"], c["dtype"])) for i, c in enumerate(columns)})
    sink = pa.BufferOutputStream()
    with ipc.new_stream(sink, table.schema, options=ipc.IpcWriteOptions(compression=codec)) as w:
        w.write_table(table, max_chunksize=max(table.num_rows, 1))
    seen = []

    def encode(bi, k, plain):
        ci, data = divmod(k, 2)      # a primitive column: validity (empty here, no nulls), data
        assert bi == 0 and data == 1 and plain == columns[ci]["want"]
        seen.append(ci)
        return frames[ci]

    out = rewrite_buffers(sink.getvalue().to_pybytes(), encode)
    assert seen == list(range(len(columns)))
    return out, table
