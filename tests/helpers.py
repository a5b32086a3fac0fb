"""Shared test helpers: DuckDB-layout vectors -> canonical logical values (the same canonical form
tests/golden/make_golden.py computes with pyarrow), used for both the oracle and the HIP path."""
import hashlib
import json
import os

import numpy as np

from oracle import pyoracle as po

# The host sources of the IPC reader (duckdb-arrow_amd/csrc), for the g++ builds of tests/sanitize/*.cpp: metadata decode,
# the I/O pool, libzstd / liblz4, the frame walks, the batch slicing and the reader classes.  Link with -ldl -lpthread.
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "duckdb-arrow_amd", "csrc")
READER_HOST_SOURCES = [os.path.join(_CSRC, name + ".cpp")
                       for name in ("ipc_format", "io_pool", "host_codec", "frame_walk", "batch_slice", "ipc_stream_reader")]

# Arrow type ids (Schema.fbs Type union)
T_INT, T_FLOAT, T_BINARY, T_UTF8, T_BOOL, T_DECIMAL, T_DATE, T_TIME, T_TIMESTAMP = 2, 3, 4, 5, 6, 7, 8, 9, 10
T_FIXED_BINARY, T_DURATION, T_LARGE_BINARY, T_LARGE_UTF8 = 15, 18, 19, 20


def column_digest(values):
    return hashlib.sha256(json.dumps(values, separators=(",", ":")).encode()).hexdigest()


def canon_python(v):
    """Python values as the host mirror returns them (lists / dicts / (key, value) tuples / bytes / floats) -> the
    canonical JSON-able form of tests/golden/expected.json."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, (list, tuple)):
        return [canon_python(x) for x in v]
    if isinstance(v, dict):
        return {k: canon_python(x) for k, x in v.items()}
    if isinstance(v, float):
        return "nan" if v != v else repr(v)
    if isinstance(v, (bytes, bytearray)):
        return "b:" + bytes(v).hex()
    raise TypeError(type(v))


def _fixed(data, ok, dtype):
    vals = data.view(dtype)
    return [vals[i].item() if ok[i] else None for i in range(len(ok))]


def canon_flat(field, kind, param, width, data, validity, n, heap, heap_base=0):
    """One decoded flat vector -> canonical logical list.  `heap_base` = pointer value of heap[0]; with
    pyoracle.decode_stream's default pointer bases the heap is the whole stream and heap_base is 0."""
    ok = po.valid_bits(validity, n) if n else np.zeros(0, bool)
    t = field["type"]
    if kind in (po.K_STR32, po.K_STR64, po.K_FIXED_BINARY):
        as_bytes = t in (T_BINARY, T_LARGE_BINARY, T_FIXED_BINARY)
        vals = po.strings_to_pylist(data, validity, n, heap, heap_base, as_bytes=as_bytes)
        return [("b:" + v.hex()) if (as_bytes and v is not None) else v for v in vals]
    if kind == po.K_BOOL:
        return [bool(data[i]) if ok[i] else None for i in range(n)]
    if kind == po.K_NULL:
        return [None] * n
    if t == T_FLOAT:
        vals = data.view(np.float32 if width == 4 else np.float64)
        return [("nan" if vals[i] != vals[i] else repr(float(vals[i]))) if ok[i] else None for i in range(n)]
    if t == T_INT:
        dt = np.dtype("%s%d" % ("i" if field["is_signed"] else "u", width))
        return _fixed(data, ok, dt)
    if t == T_DECIMAL and width == 16:
        lo = data.view(np.uint64)[0::2]
        hi = data.view(np.int64)[1::2]
        return [(int(hi[i]) << 64) + int(lo[i]) if ok[i] else None for i in range(n)]
    if kind == po.K_DURATION:
        return [int(data.view(np.int64)[2 * i + 1]) if ok[i] else None for i in range(n)]
    if kind in (po.K_INTERVAL_MONTHS, po.K_INTERVAL_MDN):
        md, us = data.view(np.int32), data.view(np.int64)
        return [[int(md[4 * i]), int(md[4 * i + 1]), int(us[2 * i + 1])] if ok[i] else None for i in range(n)]
    dt = {2: np.int16, 4: np.int32, 8: np.int64}[width]
    return _fixed(data, ok, dt)


def canon_node(node, heap, heap_base=0):
    """A decoded node (flat or nested) -> canonical logical values for ALL its rows (batch level)."""
    f = node["field"] if "field" in node else None
    n = node["nrows"]
    kind = node["kind"]
    ok = po.valid_bits(node["validity"], n) if n else np.zeros(0, bool)
    if kind in (po.K_LIST32, po.K_LIST64):
        child = canon_node(node["children"][0], heap, heap_base)
        ent = node["data"].view(np.uint64).reshape(-1, 2) if n else np.zeros((0, 2), np.uint64)
        win, cwin = node["win"], node["children"][0]["win"]
        out = []
        k = 0
        is_map = f is not None and f["type"] == 17
        for r in range(n):
            while r >= win[k + 1]:
                k += 1
            if not ok[r]:
                out.append(None)
                continue
            start = cwin[k] + int(ent[r, 0])
            vals = child[start: start + int(ent[r, 1])]
            out.append([[v["key"], v["value"]] for v in vals] if is_map else vals)
        return out
    if kind == po.K_STRUCT:
        kids = [canon_node(c, heap, heap_base) for c in node["children"]]
        if f is not None and f["type"] == 16:  # fixed_size_list
            size = int(node["param"])
            return [kids[0][r * size: (r + 1) * size] if ok[r] else None for r in range(n)]
        names = [c["name"] for c in node["children"]]
        return [{nm: kid[r] for nm, kid in zip(names, kids)} if ok[r] else None for r in range(n)]
    if kind == po.K_STRVIEW:
        as_bytes = f["type"] == 23
        vals = po.strings_to_pylist(node["data"], node["validity"], n, heap, heap_base, as_bytes=as_bytes)
        return [("b:" + v.hex()) if (as_bytes and v is not None) else v for v in vals]
    if kind == po.K_DICT:
        d = node["dictionary"]
        vf = dict(f, has_dict=0)
        base = canon_flat(vf, d["kind"], d["param"], d["width"], d["data"], d["validity"], d["nrows"], heap, heap_base) + [None]
        sel = node["data"].view(np.uint32)
        return [base[int(sel[i])] for i in range(n)]
    return canon_flat(f, kind, node["param"], node["width"], node["data"], node["validity"], n, heap, heap_base)


def canon_oracle_column(field, col, n, heap, heap_base=0):
    """A column node from pyoracle.decode_stream (or the GPU equivalent) -> canonical logical list."""
    if "field" not in col:
        col = dict(col, field=field)
    if "nrows" not in col:
        col = dict(col, nrows=n)
    return canon_node(col, heap, heap_base)


def canon_stream(fields, batches, heap, heap_base=0):
    """-> {column name: canonical list over all batches}"""
    out = {f["name"]: [] for f in fields}
    by_name = {f["name"]: f for f in fields}
    for b in batches:
        for c in b["columns"]:
            out[c["name"]].extend(canon_oracle_column(by_name[c["name"]], c, b["nrows"], heap, heap_base))
    return out


# ------------------------------------------------------------------------------------------ pyarrow as the value oracle
def pyarrow_value(t, v):
    """A pyarrow python value in the form the package's host mirror returns (stored integers for DATE / DECIMAL, tuples for
    map entries): pyarrow is the oracle of the reference's own python tests (test/python/test_integration.py:32-61)."""
    import datetime
    import pyarrow as pa
    if v is None:
        return None
    if pa.types.is_dictionary(t):
        return pyarrow_value(t.value_type, v)
    if pa.types.is_date32(t):
        return (v - datetime.date(1970, 1, 1)).days if not isinstance(v, int) else v
    if pa.types.is_decimal(t):
        return int(v.scaleb(t.scale).to_integral_value())
    if pa.types.is_floating(t):
        return "nan" if v != v else float(v)
    if pa.types.is_map(t):
        return [(k, pyarrow_value(t.item_type, x)) for k, x in v]
    if pa.types.is_fixed_size_list(t) or pa.types.is_list(t) or pa.types.is_large_list(t):
        return [pyarrow_value(t.value_type, x) for x in v]
    if pa.types.is_struct(t):
        return {t.field(i).name: pyarrow_value(t.field(i).type, v[t.field(i).name]) for i in range(t.num_fields)}
    return v


def pyarrow_columns(table):
    """Every column of a pyarrow table as canonical values (canon_python form)."""
    import pyarrow as pa
    out = []
    for i, f in enumerate(table.schema):
        col, t = table.column(i), f.type
        if pa.types.is_timestamp(t):   # stored int64 in DuckDB's unit: microseconds (nanoseconds stay TIMESTAMP_NS)
            if t.unit in ("s", "ms"):
                col = col.cast(pa.timestamp("us", tz=t.tz))
            col, t = col.cast(pa.int64()), pa.int64()
        out.append(canon_python([pyarrow_value(t, v) for v in col.to_pylist()]))
    return out


# ------------------------------------------------------------------------------------------ raw (-1) compressed buffers
def rewrite_buffers(stream_bytes, encode, prefix=None, select=None):
    """A compressed IPC stream with some of its buffers' frames replaced: bodies re-laid out, RecordBatch.buffers and
    Message.bodyLength patched in place in the flatbuffer (same metadata size).  encode(batch_index, buffer_index,
    uncompressed_bytes) is asked about every non-empty buffer: the frame bytes to write behind the buffer's unchanged 8-byte
    length prefix, or None to keep the buffer as it is.  `prefix`: a length prefix to write in front of the replaced
    buffers instead; select(batch_index, buffer_index, length in the stream): the buffers `encode` is asked about at all
    (default: every one).  Returns the new stream as bytes."""
    import struct
    import pyarrow as pa
    a = np.frombuffer(stream_bytes, dtype=np.uint8)
    out = bytearray()
    at = 0
    bi = 0
    for m in po.walk_stream(a):
        out += a[at: m["prefix_off"]].tobytes()
        head = bytearray(a[m["prefix_off"]: m["body_off"]].tobytes())
        body = a[m["body_off"]: m["body_off"] + m["body_len"]].tobytes()
        at = m["body_off"] + m["body_len"]
        if m["type"] != po.MSG_RECORD_BATCH or m["body_len"] == 0:
            out += head + body
            continue
        rb = po.decode_record_batch(a[m["meta_off"]: m["meta_off"] + m["meta_len"]])
        assert rb["compression"] in (0, 1)
        codec = pa.Codec("lz4" if rb["compression"] == 0 else "zstd")
        new_body, new_bufs = bytearray(), []
        for k, (off, ln) in enumerate(rb["buffers"]):
            piece = body[off: off + ln]
            if ln > 8 and (select is None or select(bi, k, ln)):
                (ulen,) = struct.unpack("<q", piece[:8])
                plain = piece[8:] if ulen == -1 else codec.decompress(piece[8:], decompressed_size=ulen).to_pybytes()
                new = encode(bi, k, plain)
                if new is not None:
                    piece = (piece[:8] if prefix is None else struct.pack("<q", prefix)) + bytes(new)
            new_bufs.append((len(new_body), len(piece)))
            new_body += piece + b"\0" * ((-len(piece)) % 8)
        old_vec = b"".join(struct.pack("<qq", o, l) for o, l in rb["buffers"])
        new_vec = b"".join(struct.pack("<qq", o, l) for o, l in new_bufs)
        where = bytes(head).find(old_vec)
        assert where >= 0 and bytes(head).find(old_vec, where + 1) < 0, "RecordBatch.buffers not found exactly once"
        head[where: where + len(old_vec)] = new_vec
        old_len = struct.pack("<q", m["body_len"])
        hits = [i for i in range(0, len(head) - 7) if bytes(head[i: i + 8]) == old_len and not (where <= i < where + len(old_vec))]
        assert len(hits) == 1, "Message.bodyLength not found exactly once"
        head[hits[0]: hits[0] + 8] = struct.pack("<q", len(new_body))
        out += head + new_body
        bi += 1
    out += a[at:].tobytes()
    return bytes(out)


def rewrite_buffers_raw(stream_bytes, pick):
    """A compressed IPC stream with some of its buffers stored RAW: length prefix -1 followed by the uncompressed bytes, what
    Arrow C++ (IpcWriteOptions::min_space_savings), arrow-rs and Arrow Java write for incompressible buffers.  pyarrow's
    Python writer never emits them, so the stream is rewritten here (rewrite_buffers).  pick(batch_index, buffer_index,
    length) chooses the buffers, `length` being the buffer's length in the stream, prefix included.  Returns the new stream
    as bytes."""
    return rewrite_buffers(stream_bytes, lambda bi, k, plain: plain, prefix=-1, select=pick)


# ------------------------------------------------------------------------------------------ late materialisation (gather)
# The reference of the gather kernel (kernels_gather.hip): the oracle decodes the WHOLE column with its per-kind functions,
# numpy then takes the selected rows.  There is no gather entry point in the oracle, on purpose: the compacted vectors must
# be what slicing the flat vectors with the selection gives.
ST_BAD_OFFSETS, ST_STRING_TOO_LARGE, ST_MUL_OVERFLOW, ST_INDEX_RANGE, ST_DECIMAL_RANGE, ST_DICT_INDEX = 1, 2, 4, 8, 16, 64  # mi_arrow_ipc.h

_orc_ready = False


def _orc():
    """The oracle with the prototypes of the per-kind functions pyoracle.lib() leaves undeclared."""
    global _orc_ready
    import ctypes as C
    L = po.lib()
    if not _orc_ready:
        P, I64, I32, U64, U32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_uint32
        for name, args in (("orc_bool", [P, I64, I64, P]), ("orc_decimal128_narrow", [P, P, I64, I64, I32, P]),
                           ("orc_date64_to_date32", [P, I64, I64, P]), ("orc_div_i64", [P, I64, I64, I64, P]),
                           ("orc_fixed_binary", [P, I32, P, I64, I64, U64, P]), ("orc_dict_sel", [P, I32, I32, P, I64, I64, U32, P]),
                           ("orc_duration_to_interval", [P, P, I64, I64, I64, P]), ("orc_interval_months", [P, I64, I64, P]),
                           ("orc_interval_mdn", [P, I64, I64, P]), ("orc_narrow", [P, I32, P, I64, I64, I32, P]),
                           ("orc_half_to_float", [P, I64, I64, P]), ("orc_string_view", [P, P, I64, I64, P, I64, P]),
                           ("orc_list_entries", [P, I32, I64, I64, I64, I64, P])):
            getattr(L, name).argtypes = args
        _orc_ready = True
    return L


def _words_of(ok):
    """bool per row -> validity_t words, pad bits ones."""
    n = len(ok)
    return np.packbits(np.concatenate([ok.astype(bool), np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()


def decode_column_reference(kind, nrows, buf1, *, param=0, param2=0, validity=None, null_count=-1, row_offset=0, buf2=None,
                            buf2_len=None, ptr_base=0, window_starts=None, parent=None):
    """Rows [row_offset, row_offset + nrows) of one Arrow column as the flat decode path hands them to DuckDB, from the
    oracle's per-kind functions (each takes the array offset `o`): (data uint8[nrows, width], valid bool[nrows],
    err uint32[nrows]).  Every decode kind (the gather reference below refuses the ones a selection vector cannot take).

    parent = (validity words of the struct / fixed_size_list vector that owns the column, rows per parent row): the
    combined validity own & parent[r // max(div, 1)] is what the per-kind functions receive as `valid` and what comes back.
    COPY, BOOL, DATE64, DIV_I64, the interval kinds and a dividing DURATION keep their source-derived values under NULL, as
    the oracle does; NULL (the Arrow type) is zero bytes with every row NULL; STRUCT has no data (width 0).
    STRVIEW: buf2 = the table of variadic buffers as uint64 {address, length} pairs, buf2_len = their number.
    LIST32 / LIST64: param = child length, window_starts = the rows (of this column) where the top-level 2048-row windows
    start (None: every 2048-row tile is one); orc_list_entries is called once per window with its win_row.

    err[r] = the MI_ST_* bits row r raises when it is decoded.  The oracle reports errors per call, not per row, so its
    conditions are restated per row: FULL offset validation (first >= 0, non-decreasing, end <= data length) and "Strings
    over 4GB" (an end offset past UINT32_MAX) for every row, NULL or not, as the whole-array validation is, and likewise
    the list offsets (a < 0, b < a, b > child length, a < the window's base); multiply overflow (MUL_I64, a multiplying
    DURATION), an index that does not fit uint32 or points past the dictionary, a decimal that is not the sign extension
    of its narrowed value (Hugeint::TryCast / NARROW; the oracle only truncates), and a long string view whose buffer
    index or offset + length leaves the table, for valid rows.  A row with damaged offsets decodes to the canonical 16
    zero bytes (the oracle is not asked to follow them)."""
    L = _orc()
    n, o = int(nrows), int(row_offset)
    w = po.out_width(kind, param)
    b1 = np.ascontiguousarray(buf1).view(np.uint8).reshape(-1) if buf1 is not None else np.zeros(16, np.uint8)
    bm = np.ascontiguousarray(validity).view(np.uint8).reshape(-1) if validity is not None else None
    words = np.full(max((n + 63) // 64, 1), np.uint64(0xFFFFFFFFFFFFFFFF))
    if n:
        L.orc_validity(bm.ctypes.data if bm is not None else None, null_count, o, n, words.ctypes.data)
    ok = po.valid_bits(words, n)
    if parent is not None and n:
        pbits = np.unpackbits(np.ascontiguousarray(parent[0]).view(np.uint8), bitorder="little").astype(bool)
        ok = ok & pbits[np.arange(n) // max(int(parent[1]), 1)]
        words = _words_of(ok)
    if kind == po.K_NULL:
        ok = np.zeros(n, bool)
    err = np.zeros(n, np.uint32)
    out = np.zeros(max(n * w, 1), np.uint8)
    rows = slice(o, o + n)
    if n == 0:
        return out[:0].reshape(0, max(w, 1)), ok, err
    if kind == po.K_COPY:
        out[: n * w] = b1[o * w: (o + n) * w]
    elif kind == po.K_BOOL:
        L.orc_bool(b1.ctypes.data, o, n, out.ctypes.data)
    elif kind == po.K_DEC128:
        L.orc_decimal128_narrow(b1.ctypes.data, words.ctypes.data, o, n, w, out.ctypes.data)
        halves = b1[: (o + n) * 16].view(np.int64).reshape(-1, 2)[rows]
        sext = halves[:, 0].astype({2: np.int16, 4: np.int32, 8: np.int64}[w]).astype(np.int64)
        err[ok & ((sext != halves[:, 0]) | (halves[:, 1] != (sext >> 63)))] = ST_DECIMAL_RANGE
    elif kind == po.K_DATE64:
        L.orc_date64_to_date32(b1.ctypes.data, o, n, out.ctypes.data)
    elif kind == po.K_MUL_I32:
        assert 0 < param < 2**31      # an int32 times this cannot leave int64: no per-row condition
        assert L.orc_mul_i32_to_i64(b1.ctypes.data, words.ctypes.data, o, n, param, out.ctypes.data) == 0
    elif kind == po.K_MUL_I64:
        L.orc_mul_i64(b1.ctypes.data, words.ctypes.data, o, n, param, out.ctypes.data)
        src = b1[: (o + n) * 8].view(np.int64)[rows]
        err[ok & ((src > (2**63 - 1) // param) | (src < -(2**63 // param)))] = ST_MUL_OVERFLOW
    elif kind == po.K_DIV_I64:
        L.orc_div_i64(b1.ctypes.data, o, n, param, out.ctypes.data)
    elif kind in (po.K_STR32, po.K_STR64):
        off = b1.view(np.int32 if kind == po.K_STR32 else np.int64)[o: o + n + 1].astype(np.int64)
        b2 = np.ascontiguousarray(buf2).view(np.uint8).reshape(-1) if buf2 is not None and len(buf2) else np.zeros(16, np.uint8)
        data_len = (len(np.ascontiguousarray(buf2).view(np.uint8).reshape(-1)) if buf2 is not None else 0) if buf2_len is None else buf2_len
        a, b = off[:-1], off[1:]
        bad = ~((a >= 0) & (b >= a) & (b <= data_len))
        big = ~bad & (b > 0xFFFFFFFF) if kind == po.K_STR64 else np.zeros(n, bool)
        err[bad] = ST_BAD_OFFSETS
        err[big] = ST_STRING_TOO_LARGE
        follow = _words_of(ok & ~bad & ~big)
        fn = L.orc_string32 if kind == po.K_STR32 else L.orc_string64
        fn(b1.ctypes.data, b2.ctypes.data, follow.ctypes.data, o, n, ptr_base, out.ctypes.data)
    elif kind == po.K_FIXED_BINARY:
        L.orc_fixed_binary(b1.ctypes.data, int(param), words.ctypes.data, o, n, ptr_base, out.ctypes.data)
    elif kind == po.K_DICT:
        iw, signed = int(param & 0xFF), int((param >> 8) & 1)
        L.orc_dict_sel(b1.ctypes.data, iw, signed, words.ctypes.data, o, n, param2, out.ctypes.data)
        idx = b1[: (o + n) * iw].view(np.dtype("%s%d" % ("i" if signed and iw < 8 else "u", iw)))[rows]
        wide = (idx.astype(np.int64).view(np.uint64) if iw < 8 else idx) > np.uint64(0xFFFFFFFF)
        past = ~wide & (idx.astype(np.uint64) >= np.uint64(param2))
        err[ok & wide] = ST_INDEX_RANGE
        err[ok & past] = ST_DICT_INDEX
    elif kind == po.K_DURATION:
        L.orc_duration_to_interval(b1.ctypes.data, words.ctypes.data, o, n, param, out.ctypes.data)
        if param > 0:
            src = b1[: (o + n) * 8].view(np.int64)[rows]
            err[ok & ((src > (2**63 - 1) // param) | (src < -(2**63 // param)))] = ST_MUL_OVERFLOW
    elif kind == po.K_INTERVAL_MONTHS:
        L.orc_interval_months(b1.ctypes.data, o, n, out.ctypes.data)
    elif kind == po.K_INTERVAL_MDN:
        L.orc_interval_mdn(b1.ctypes.data, o, n, out.ctypes.data)
    elif kind == po.K_NARROW:
        sw, dw = int(param & 0xFF), int((param >> 8) & 0xFF)
        L.orc_narrow(b1.ctypes.data, sw, words.ctypes.data, o, n, dw, out.ctypes.data)
        src = b1[: (o + n) * sw].view(np.int32 if sw == 4 else np.int64)[rows].astype(np.int64)
        err[ok & (src.astype({2: np.int16, 4: np.int32}[dw]).astype(np.int64) != src)] = ST_DECIMAL_RANGE
    elif kind == po.K_HALF_FLOAT:
        L.orc_half_to_float(b1.ctypes.data, o, n, out.ctypes.data)
    elif kind in (po.K_NULL, po.K_STRUCT):
        pass
    elif kind == po.K_STRVIEW:
        nbuf = int(buf2_len or 0)
        table = np.ascontiguousarray(buf2).view(np.uint64).reshape(-1) if nbuf else np.zeros(2, np.uint64)
        L.orc_string_view(b1.ctypes.data, words.ctypes.data, o, n, table.ctypes.data, nbuf, out.ctypes.data)
        v = b1[: (o + n) * 16].view(np.int32).reshape(-1, 4)[rows].astype(np.int64)
        ln, bi, bo = v[:, 0] & 0xFFFFFFFF, v[:, 2], v[:, 3]
        size = table[1::2].astype(np.int64)[np.clip(bi, 0, max(nbuf - 1, 0))]
        err[ok & (ln > 12) & ((bi < 0) | (bi >= nbuf) | (bo < 0) | (bo + ln > size))] = ST_BAD_OFFSETS
    elif kind in (po.K_LIST32, po.K_LIST64):
        offw = 4 if kind == po.K_LIST32 else 8
        off = b1.view(np.int32 if offw == 4 else np.int64)
        wins = list(range(0, n, 2048)) if window_starts is None else [int(x) for x in window_starts]
        base = np.zeros(n, np.int64)
        for k, r0 in enumerate(wins):
            r1 = min(wins[k + 1] if k + 1 < len(wins) else n, n)
            if k == 0:
                r0 = 0      # rows in front of the first start (there are none in a well-formed table) belong to it
            if r1 > r0:
                L.orc_list_entries(b1.ctypes.data, offw, o + r0, r1 - r0, o + wins[k], int(param), out[16 * r0:].ctypes.data)
                base[r0: r1] = off[o + wins[k]]
        a, b = off[o: o + n].astype(np.int64), off[o + 1: o + n + 1].astype(np.int64)
        err[(a < 0) | (b < a) | (b > param) | (a < base)] = ST_BAD_OFFSETS
    else:
        raise NotImplementedError("kind %d" % kind)
    return out[: n * w].reshape(n, w), ok, err


GATHER_KINDS = (po.K_COPY, po.K_DEC128, po.K_STR32, po.K_STR64, po.K_FIXED_BINARY, po.K_BOOL, po.K_DATE64, po.K_MUL_I32, po.K_MUL_I64,
                po.K_DIV_I64, po.K_DICT)      # KindCanGather (kernels_gather.hip)


def gather_take(data, ok, err, sel):
    """The take-and-pack half of the gather reference.  `sel` = one ascending list of window-relative row indices per
    2048-row window.  -> (rows 2048 * w + sel[w][i] of `data` in window order, densely packed, as uint8[total * width];
    their validity bits as uint64 words with every bit past the total set; the OR of their err bits)."""
    parts = [2048 * w + np.asarray(s, np.int64) for w, s in enumerate(sel)]
    rows = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    status = int(np.bitwise_or.reduce(err[rows])) if len(rows) else 0
    return np.ascontiguousarray(data[rows]).reshape(-1), _words_of(ok[rows]), status


def gather_reference(kind, nrows, buf1, sel, **column):
    """Expected output bytes, validity words and status of one gather task (a column decoded through a selection vector)."""
    if kind not in GATHER_KINDS:
        raise NotImplementedError("kind %d is not decoded through a selection vector" % kind)
    return gather_take(*decode_column_reference(kind, nrows, buf1, **column), sel)
