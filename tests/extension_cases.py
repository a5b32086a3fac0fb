"""The Arrow canonical extension types (arrow.uuid, arrow.bool8, arrow.json) restated in numpy, and the columns and plans
the extension suites share (test_extension_reference_host.py, test_extension_schema_host.py, test_gpu_extension_*.py).

The restatement calls neither the package nor the oracle; test_extension_reference_host.py holds it against Python's uuid
module and against pyarrow's buffers.  The rules (csrc/extension_format.hpp):

  arrow.uuid   16 bytes in the order of the canonical text -> hugeint_t{uint64 lower; int64 upper}: upper = bytes 0..7 read
               big-endian with bit 63 flipped, lower = bytes 8..15 read big-endian.  Every row is converted, NULL rows too.
  arrow.bool8  int8 -> one byte, v != 0.  Every row is converted.
  UUID text    hugeint_t rows -> utf8: 36 bytes of lower-case 8-4-4-4-12 hex per valid row, none per NULL row."""
import io
import uuid

import numpy as np

K_UUID, K_BOOL8, K_ENC_UUID_TEXT = 25, 26, 39
WIN = 2048
SENTINEL = 0xA5
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
ROWS = [0, 1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 17]
BOOL8_BYTES = [0, 1, 2, 0x7F, 0x80, 0xFF]
UUID_EDGES = [bytes(16), b"\xff" * 16, b"\x7f" + b"\xff" * 15, b"\x80" + bytes(15), bytes(8) + b"\xff" * 8, b"\xff" * 8 + bytes(8),
              bytes(range(16)), bytes(range(240, 256))]      # first bit 0 and 1, all zero, all ones, every byte distinct


# ------------------------------------------------------------------------------------------------ the restatement
def uuid_from_arrow(raw):
    """(n, 16) uint8, text order -> (n, 16) uint8: the hugeint_t rows, little-endian {lower, upper}"""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1, 16)
    upper = raw[:, 0:8].copy().view(">u8").reshape(-1).astype(np.uint64) ^ np.uint64(1 << 63)
    lower = raw[:, 8:16].copy().view(">u8").reshape(-1).astype(np.uint64)
    return np.stack([lower, upper], axis=1).astype("<u8").view(np.uint8).reshape(-1, 16)


def hugeint_of(rows):
    """(n, 16) uint8 hugeint_t rows -> signed Python ints"""
    w = np.ascontiguousarray(rows, np.uint8).reshape(-1, 16).view("<u8")
    out = []
    for lo, hi in w.tolist():
        v = (hi << 64) | lo
        out.append(v - (1 << 128) if v >= (1 << 127) else v)
    return out


def uuid_text(rows):
    """(n, 16) uint8 hugeint_t rows -> (n, 36) uint8: the text of every row"""
    w = np.ascontiguousarray(rows, np.uint8).reshape(-1, 16).view("<u8")
    hi, lo = w[:, 1] ^ np.uint64(1 << 63), w[:, 0]
    shifts = np.arange(60, -4, -4).astype(np.uint64)
    nib = np.concatenate([(hi[:, None] >> shifts) & np.uint64(15), (lo[:, None] >> shifts) & np.uint64(15)], axis=1).astype(np.uint8)   # (n, 32)
    chars = np.where(nib < 10, nib + ord("0"), nib + (ord("a") - 10)).astype(np.uint8)
    out = np.full((len(w), 36), ord("-"), np.uint8)
    out[:, [i for i in range(36) if i not in (8, 13, 18, 23)]] = chars
    return out


def bool8(raw):
    return (np.ascontiguousarray(raw).view(np.uint8) != 0).astype(np.uint8)


def words_of(ok):
    """row validity -> validity words, pad bits ones"""
    ok = np.asarray(ok, bool)
    return np.packbits(np.concatenate([ok, np.ones(-len(ok) % 64, bool)]), bitorder="little").view(np.uint64).copy()


def uuid_text_reference(rows, ok, large):
    """-> (offset bytes, text bytes, bitmap bytes, NULL count) of MI_K_ENC_UUID_TEXT over n hugeint_t rows; ok None = no
    validity words.  A NULL row adds no bytes and repeats the offset (ArrowVarcharData::Append)."""
    n = len(rows)
    valid = np.ones(n, bool) if ok is None else np.asarray(ok, bool)
    off = np.concatenate([[0], np.cumsum(np.where(valid, 36, 0), dtype=np.int64)])
    text = uuid_text(rows)[valid].reshape(-1)
    bitmap = np.packbits(np.concatenate([valid, np.ones(-n % 8, bool)]), bitorder="little")
    return off.astype("<i8" if large else "<i4").view(np.uint8), text, bitmap, n - int(valid.sum())


# ------------------------------------------------------------------------------------------------ decode tasks
def parent_bits(parent, n):
    """validity of child rows [0, n) under parent = (words, child rows per parent row; 0 and 1: a struct)"""
    bits = np.unpackbits(np.ascontiguousarray(parent[0]).view(np.uint8), bitorder="little").astype(bool)
    return bits[np.arange(n) // max(parent[1], 1)]


def make_column(kind, n, row_offset, nulls, rng, parent=None, edges=True):
    """One source column: `n` rows at Arrow array offset `row_offset`, generated 2048 + 64 rows longer than that, so that a
    kernel that read past the last row would show as a wrong value.  nulls: "none" (no bitmap), "all_valid", "all_null",
    "random".  The special values sit on valid and on NULL rows alike: every row is converted."""
    total = row_offset + n + WIN + 64
    col = dict(kind=kind, n=n, row_offset=row_offset, name="k%d/%s/n%d/o%d" % (kind, nulls, n, row_offset))
    if kind == K_UUID:
        raw = rng.integers(0, 256, (total, 16), dtype=np.uint8)
        if edges and n:
            at = row_offset + rng.integers(0, n, 4 * len(UUID_EDGES))
            raw[at] = np.frombuffer(b"".join(UUID_EDGES * 4), np.uint8).reshape(-1, 16)
        col.update(buf1=raw.reshape(-1), width=16, want=uuid_from_arrow(raw[row_offset: row_offset + n]).reshape(-1))
    else:
        raw = rng.integers(0, 256, total, dtype=np.uint8)
        raw[rng.integers(0, total, total // 2)] = rng.choice(BOOL8_BYTES, total // 2)
        col.update(buf1=raw, width=1, want=bool8(raw[row_offset: row_offset + n]))
    ok = np.ones(n, bool)
    if nulls != "none":
        bitmap = rng.integers(0, 256, (total + 63) // 64 * 8 + 8, dtype=np.uint8)
        if nulls in ("all_valid", "all_null"):
            bitmap[:] = 0xFF if nulls == "all_valid" else 0
        col["validity"] = bitmap
        ok = np.unpackbits(bitmap, bitorder="little")[row_offset: row_offset + n].astype(bool)
    if parent is not None:
        col.update(out_aux=np.ascontiguousarray(parent[0]), parent_div=parent[1], depth=1, name=col["name"] + "/div%d" % parent[1])
        ok = ok & parent_bits(parent, n)
    col.update(ok=ok, want_words=words_of(ok))
    return col


def _dev(torch, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([b, np.zeros(16 - len(b) % 8, np.uint8)])).cuda()


def run_decode(ctx, torch, cols, sels=None):
    """One Plan of the columns, one launch; sels[i] = index lists per 2048-row window (a gather task) or None.
    -> [(data bytes with the sentinel tail, validity words with the guard word)], status"""
    import duckdb_arrow_amd as da
    keep, tasks, outs = [], [], []
    for i, col in enumerate(cols):
        sel = sels[i] if sels else None
        total = col["n"] if sel is None else sum(len(s) for s in sel)
        w = col["width"]
        d1 = _dev(torch, col["buf1"])
        dv = _dev(torch, col["validity"]) if "validity" in col else None
        daux = _dev(torch, col["out_aux"]) if "out_aux" in col else None
        dsel = dcnt = None
        if sel is not None:
            flat = np.full(max(len(sel), 1) * WIN, WIN, np.uint32)
            for k, s in enumerate(sel):
                flat[k * WIN: k * WIN + len(s)] = s
            dsel = torch.from_numpy(flat.view(np.int32)).cuda()
            dcnt = torch.from_numpy(np.array([len(s) for s in sel] + [0], np.uint32).view(np.int32)).cuda()
        out = torch.full((total * w + 64 + (-total * w) % 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        outv = torch.full(((total + 63) // 64 * 8 + 8,), 0xFF, dtype=torch.uint8, device="cuda")
        keep += [d1, dv, daux, dsel, dcnt]
        outs.append((out, outv))
        tasks.append(da.make_task(col["kind"], col["n"], d1.data_ptr(), out.data_ptr(), validity=dv.data_ptr() if dv is not None else 0,
                                  out_validity=outv.data_ptr(), out_aux=daux.data_ptr() if daux is not None else 0,
                                  parent_div=col.get("parent_div", 0), depth=col.get("depth", 0), row_offset=col["row_offset"], param=col["width"],
                                  null_count=-1, sel=dsel.data_ptr() if dsel is not None else 0, sel_count=dcnt.data_ptr() if dcnt is not None else 0))
    plan = da.Plan(ctx, tasks)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    status = plan.status()
    got = [(o.cpu().numpy(), v.cpu().numpy().view(np.uint64)) for o, v in outs]
    plan.close()
    return got, status


def check_decode(col, got, sel=None):
    """Every data row equals the restatement, NULL slots included; the bytes behind the last row are the sentinel; the validity
    words equal the reference, pad bits ones; the guard word is intact.  With `sel`: the selected rows, packed."""
    data, words = got
    w = col["width"]
    want, ok = col["want"].reshape(-1, w), col["ok"]
    if sel is not None:
        rows = np.concatenate([k * WIN + np.asarray(s, np.int64) for k, s in enumerate(sel)] + [np.zeros(0, np.int64)])
        want, ok = want[rows], ok[rows]
    total = len(want)
    got_rows = data[: total * w].reshape(-1, w)
    if not np.array_equal(got_rows, want):
        bad = np.nonzero(np.any(got_rows != want, axis=1))[0]
        raise AssertionError("%s: %d of %d rows differ, first %d: got %s want %s" % (col["name"], len(bad), total, bad[0], got_rows[bad[0]].tolist(), want[bad[0]].tolist()))
    assert (data[total * w:] == SENTINEL).all(), (col["name"], "bytes behind the last output row were written")
    want_words = words_of(ok)
    assert len(words) == len(want_words) + 1
    if not np.array_equal(words[:-1], want_words):
        bad = np.nonzero(words[:-1] != want_words)[0]
        raise AssertionError("%s: validity word %d: got %016x want %016x" % (col["name"], bad[0], int(words[bad[0]]), int(want_words[bad[0]])))
    assert words[-1] == ONES, (col["name"], "the guard word behind the validity words lost bits")


# ------------------------------------------------------------------------------------------------ encode tasks
def text_column(n, ok, rng, name, large=False, vpos=0):
    """A column of encode_tasks.run_plan's shape: n random hugeint_t rows (the edge UUIDs among them), validity `ok` (None: no
    validity words; the bits behind row n are random), and its reference in encode_tasks.encode_reference's shape."""
    raw = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if n:
        raw[rng.integers(0, n, len(UUID_EDGES))] = np.frombuffer(b"".join(UUID_EDGES), np.uint8).reshape(-1, 16)
    rows = uuid_from_arrow(raw)
    words = None
    if ok is not None:
        words = np.packbits(np.concatenate([ok, rng.random(-n % 64) < 0.5]), bitorder="little").view(np.uint64).copy()
    col = dict(kind=K_ENC_UUID_TEXT, n=n, large=large, ok=ok, words=words, heap=None, ptr_base=0, width=16, bitmap=True, vpos=vpos, name=name,
               src=rows.reshape(-1), arrow=raw)
    off, text, bitmap, nulls = uuid_text_reference(rows, ok, large)
    empty = np.zeros(0, np.uint8)
    ref = dict(bitmap=bitmap, data=off if n else empty, aux=text, loose=0, nulls=nulls, status=0)
    return col, ref


# ------------------------------------------------------------------------------------------------ files
def ipc_stream(table_or_batches, schema=None, **options):
    """pyarrow table / record batches -> the bytes of an IPC stream"""
    import pyarrow as pa
    sink = io.BytesIO()
    batches = table_or_batches.to_batches() if isinstance(table_or_batches, pa.Table) else table_or_batches
    schema = schema or (table_or_batches.schema if isinstance(table_or_batches, pa.Table) else batches[0].schema)
    with pa.ipc.new_stream(sink, schema, options=pa.ipc.IpcWriteOptions(**options)) as w:
        for b in batches:
            w.write_batch(b)
    return sink.getvalue()


def random_uuids(n, rng):
    """n uuid.UUID values with the edges among them"""
    raw = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    if n >= len(UUID_EDGES):
        raw[: len(UUID_EDGES)] = np.frombuffer(b"".join(UUID_EDGES), np.uint8).reshape(-1, 16)
    return [uuid.UUID(bytes=r.tobytes()) for r in raw]
