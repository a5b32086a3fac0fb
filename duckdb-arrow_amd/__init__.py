"""duckdb-arrow_amd -- MI355X-native Arrow IPC scan / encode path of the DuckDB `nanoarrow` extension.

Host-side mirror (Python flavour) of the reference's operator surface for this path, over the C ABI of
libmi_arrow_ipc.so (include/mi_arrow_ipc.h):

    read_arrow(...)        src/scanner/read_arrow.cpp:43-86            -> Connection.read_arrow
    scan_arrow_ipc(...)    src/scanner/scan_arrow_ipc.cpp:20-64        -> Connection.scan_arrow_ipc / from_arrow
    to_arrow_ipc(...)      src/writer/to_arrow_ipc.cpp:52-182          -> Connection.to_arrow_ipc
    COPY ... (FORMAT ARROWS)  src/writer/write_arrow_stream.cpp:54-272 -> Connection.copy_to
    nanoarrow_version()    src/nanoarrow_extension.cpp:20-31           -> nanoarrow_version()

The package directory name carries a hyphen (it is the name the build contract asks for); import it through the
`duckdb_arrow_amd` shim module at the repository root.  Nothing here falls back to the CPU: without the built
library or without a HIP device every scan / encode call raises.
"""
import ctypes as C
import decimal
import os
import re
import struct
import uuid

import numpy as np

from . import _ffi
from ._ffi import MiError, VECTOR_SIZE  # noqa: F401

__all__ = ["Connection", "Reader", "Context", "Plan", "Table", "UnionValue", "MiError", "nanoarrow_version", "version", "build",
           "synth_lineitem_stream", "VECTOR_SIZE"]


def build(verbose=False):
    """Compiles libmi_arrow_ipc.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.run(["make", "-j8", "-C", os.path.join(here, "csrc")] + ([] if verbose else ["-s"]), check=True)


def version():
    return _ffi.lib().mi_version().decode()


def nanoarrow_version():
    """SELECT nanoarrow_version() (test/sql/nanoarrow.test:15-18)."""
    return _ffi.lib().mi_nanoarrow_version().decode()


def device_count():
    return _ffi.lib().mi_device_count()


def _field_dict(f):
    # names come from the file: a damaged stream may carry bytes that are not UTF-8
    return dict(name=f.name.decode("utf-8", "replace"), duck_type=f.duck_type.decode("utf-8", "replace"),
                format=f.format.decode("utf-8", "replace"), arrow_type=f.arrow_type,
                kind=f.kind, out_width=f.out_width, param=f.param, n_buffers=f.n_buffers, flat_index=f.flat_index,
                bit_width=f.bit_width, is_signed=f.is_signed, precision=f.precision, scale=f.scale, unit=f.unit,
                byte_width=f.byte_width, nullable=f.nullable, timezone=f.timezone.decode("utf-8", "replace"),
                has_dictionary=f.has_dictionary, dict_id=f.dict_id, dict_index_bit_width=f.dict_index_bit_width,
                dict_index_signed=f.dict_index_signed)


def _as_u8(buf):
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(buf, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- host reader
class Reader:
    """IPCFileStreamReader / IPCBufferStreamReader (host only, no GPU needed)."""

    def __init__(self, path=None, buffers=None):
        self._h = C.c_void_p()
        self._keep = []
        L = _ffi.lib()
        if path is not None:
            _ffi.check(L.mi_reader_open_file(os.fsencode(path), C.byref(self._h)))
        else:
            arr = (_ffi.IpcBuffer * len(buffers))()
            for i, b in enumerate(buffers):
                if isinstance(b, tuple):
                    arr[i].ptr, arr[i].size = b
                else:
                    a = _as_u8(b)
                    self._keep.append(a)
                    arr[i].ptr, arr[i].size = a.ctypes.data, a.size
            _ffi.check(L.mi_reader_open_buffers(arr, len(buffers), C.byref(self._h)))

    def close(self):
        if self._h:
            _ffi.lib().mi_reader_close(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def schema(self):
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().mi_reader_schema(self._h, None, 0, C.byref(n)))
        fields = (_ffi.Field * max(n.value, 1))()
        _ffi.check(_ffi.lib().mi_reader_schema(self._h, fields, n.value, C.byref(n)))
        return [_field_dict(f) for f in fields[: n.value]]

    def schema_metadata(self):
        cnt = C.c_int32(0)
        _ffi.check(_ffi.lib().mi_reader_schema_metadata(self._h, -1, None, None, None, None, C.byref(cnt)))
        out = []
        for i in range(cnt.value):
            k, kl, v, vl = C.c_char_p(), C.c_int32(), C.c_void_p(), C.c_int32()
            _ffi.check(_ffi.lib().mi_reader_schema_metadata(self._h, i, C.byref(k), C.byref(kl), C.byref(v), C.byref(vl),
                                                            C.byref(cnt)))
            out.append((k.value[: kl.value].decode(), C.string_at(v.value, vl.value)))
        return out

    def set_projection(self, names):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        _ffi.check(_ffi.lib().mi_reader_set_projection(self._h, arr, len(names)))

    def next_batch(self, accept_dictionaries=False):
        b = _ffi.Batch()
        rc = _ffi.lib().mi_reader_next_batch(self._h, 1 if accept_dictionaries else 0, C.byref(b))
        if rc == _ffi.MI_ENODATA:
            return None
        _ffi.check(rc)
        nc = b.n_columns
        body = np.ctypeslib.as_array(C.cast(b.body, C.POINTER(C.c_uint8)), shape=(b.body_size,)) if b.body_size else \
            np.zeros(0, np.uint8)
        return dict(length=b.length, body=body, body_ptr=b.body or 0, body_size=b.body_size,
                    body_file_offset=b.body_file_offset, is_dictionary=bool(b.is_dictionary), dict_id=b.dict_id,
                    is_delta=bool(b.is_delta), compression=b.compression,
                    column_field=[b.column_field[i] for i in range(nc)],
                    null_count=[b.null_count[i] for i in range(nc)],
                    buffers=[(b.buffers[i].offset, b.buffers[i].length) for i in range(3 * nc)],
                    column_node=[b.column_node[i] for i in range(nc)],
                    nodes=[dict(name=b.nodes[i].name.decode("utf-8", "replace"), arrow_type=b.nodes[i].arrow_type, kind=b.nodes[i].kind,
                                out_width=b.nodes[i].out_width, parent=b.nodes[i].parent, depth=b.nodes[i].depth,
                                n_children=b.nodes[i].n_children, param=b.nodes[i].param, length=b.nodes[i].length,
                                null_count=b.nodes[i].null_count,
                                spans=[(b.node_spans[j].offset, b.node_spans[j].length)
                                       for j in range(b.nodes[i].first_span, b.nodes[i].first_span + b.nodes[i].n_spans)])
                           for i in range(b.n_nodes)])

    def export_stream(self, accept_dictionaries=False):
        """The reader (with its projection) as an Arrow C stream (mi_reader_export_stream), imported into pyarrow: what
        DuckDB's arrow scan would consume in place of the reference's IpcArrayStream.  The reader is consumed."""
        import pyarrow as pa
        stream = _ffi.ArrowArrayStream()
        _ffi.check(_ffi.lib().mi_reader_export_stream(self._h, 1 if accept_dictionaries else 0, C.byref(stream)))
        self._keep.append(stream)
        return pa.RecordBatchReader._import_from_c(C.addressof(stream))

    def index(self):
        ent = C.POINTER(_ffi.BatchIndexEntry)()
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().mi_reader_index(self._h, C.byref(ent), C.byref(n)))
        return [dict(prefix_offset=ent[i].prefix_offset, meta_len=ent[i].meta_len, type=ent[i].type,
                     body_offset=ent[i].body_offset, body_len=ent[i].body_len, n_rows=ent[i].n_rows)
                for i in range(n.value)]

    def progress(self):
        return _ffi.lib().mi_reader_progress(self._h)


# ---------------------------------------------------------------------------------------------------- device
class Context:
    """mi_ctx: one per (GPU, worker).  Raises MiError(ENODEV) without a HIP device -- there is no CPU fallback."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        self._users = 0          # open relations that scan on this context
        self._orphaned = False
        _ffi.check(_ffi.lib().mi_ctx_create(device, C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            _ffi.lib().mi_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        # A relation holds its context, so reference counting frees the relation first.  The cycle collector finalises a group
        # of objects in any order (a traceback that holds a frame with both is such a group): a context finalised before a
        # relation that is still open stays alive, and the last such relation to close destroys it.
        if self._users:
            self._orphaned = True
        else:
            self.close()

    def _retain(self):
        self._users += 1

    def _release(self):
        self._users -= 1
        if self._orphaned and not self._users:
            self.close()

    def numa(self):
        """(NUMA node of the GPU or -1, the node's CPUs as a set) -- mi_ctx_numa."""
        node = C.c_int32(-1)
        buf = C.create_string_buffer(4096)
        _ffi.check(_ffi.lib().mi_ctx_numa(self._h, C.byref(node), buf, len(buf)))
        cpus = set()
        for part in buf.value.decode().split(","):
            if part:
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        return node.value, cpus

    def bind_this_thread(self):
        """Pins the CALLING thread (threads it starts afterwards inherit) to the CPUs of the GPU's NUMA node, within what it may
        use: for the threads of a host program that write the files a scan reads or consume its chunks.  Returns the node, or
        -1 when nothing was bound."""
        import os
        node, cpus = self.numa()
        allowed = os.sched_getaffinity(0)
        if node < 0 or not (cpus & allowed):
            return -1
        os.sched_setaffinity(0, cpus & allowed)
        return node


def make_task(kind, nrows, buf1, out_data, *, validity=0, buf2=0, out_validity=0, out_aux=0, ptr_base=0, row_offset=0,
              buf2_len=0, param=0, param2=0, null_count=-1, depth=0, parent_div=0, sel=0, sel_count=0):
    """mi_col_task from raw device addresses (decode: out_aux = parent validity words, parent_div = rows per parent row;
    sel / sel_count: gather mode, only the selected rows are decoded, densely packed)."""
    return _ffi.ColTask(validity=validity or None, buf1=buf1 or None, buf2=buf2 or None, out_data=out_data or None,
                        out_validity=out_validity or None, out_aux=out_aux or None, ptr_base=ptr_base, nrows=nrows,
                        row_offset=row_offset, buf2_len=buf2_len, param=param, param2=param2, null_count=null_count,
                        kind=kind, flags=parent_div, depth=depth, sel=sel or None, sel_count=sel_count or None)


class Plan:
    """mi_plan: a device-resident task table; launch() = one kernel per kernel class for ALL tasks."""

    def __init__(self, ctx, tasks):
        self._h = C.c_void_p()
        self.ctx = ctx
        self.n_tasks = len(tasks)
        arr = (_ffi.ColTask * max(len(tasks), 1))(*tasks)
        _ffi.check(_ffi.lib().mi_plan_create(ctx._h, arr, len(tasks), C.byref(self._h)))

    def launch(self, stream=0):
        _ffi.check(_ffi.lib().mi_plan_launch(self._h, C.c_void_p(stream or None)))

    def status(self):
        bits = C.c_uint32(0)
        _ffi.check(_ffi.lib().mi_plan_status(self._h, C.byref(bits)))
        return bits.value

    def raise_for_status(self):
        bits = self.status()
        if bits:
            _ffi.check(_ffi.lib().mi_status_to_error(bits))
        return bits

    def stats(self):
        r, w, rows, tiles = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().mi_plan_stats(self._h, C.byref(r), C.byref(w), C.byref(rows), C.byref(tiles)))
        return dict(bytes_read=r.value, bytes_written=w.value, rows=rows.value, tiles=tiles.value)

    def class_stats(self):
        """Per kernel class: algorithmic bytes read / written, rows, tiles and the kernel's name."""
        out = []
        for cls in range(_ffi.NUM_KERNEL_CLASSES):
            r, w, rows, tiles, name = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_char_p()
            _ffi.check(_ffi.lib().mi_plan_class_stats(self._h, cls, C.byref(r), C.byref(w), C.byref(rows), C.byref(tiles),
                                                      C.byref(name)))
            out.append(dict(kernel=name.value.decode(), bytes_read=r.value, bytes_written=w.value, rows=rows.value,
                            tiles=tiles.value))
        return out

    def launch_timed(self, stream=0):
        """One launch with HIP events around every kernel class; returns [ms per class] after synchronising."""
        ms = (C.c_float * _ffi.NUM_KERNEL_CLASSES)()
        _ffi.check(_ffi.lib().mi_plan_launch_timed(self._h, C.c_void_p(stream or None), ms))
        return list(ms)

    def null_counts(self):
        out = (C.c_int64 * max(self.n_tasks, 1))()
        _ffi.check(_ffi.lib().mi_plan_null_counts(self._h, out, self.n_tasks))
        return list(out[: self.n_tasks])

    def close(self):
        if self._h:
            _ffi.lib().mi_plan_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close


def filter_range(ctx, values_ptr, width, validity_ptr, nrows, lo, hi, sel_ptr, count_ptr, stream=0):
    _ffi.check(_ffi.lib().mi_filter_range(ctx._h, values_ptr, width, validity_ptr or None, nrows, lo, hi, sel_ptr, count_ptr,
                                          C.c_void_p(stream or None)))


def filter_between(ctx, values_ptr, width, validity_ptr, nrows, lo, hi, sel_ptr, count_ptr, stream=0):
    """lo <= v <= hi on a resident vector (mi_filter_between): Python floats on FLOAT / DOUBLE vectors (width 4 / 8, DuckDB's
    total order), ints on hugeint vectors (width 16)."""
    if width == 16:
        signed = lambda w: w - (1 << 64) if w >= (1 << 63) else w
        words = [signed((v >> s) & ((1 << 64) - 1)) for v in (int(lo), int(hi)) for s in (0, 64)]
        kind = _ffi.FV_INT128
    else:
        words = [struct.unpack("<q", struct.pack("<d", float(v)))[0] for v in (lo, hi)]
        kind = _ffi.FV_DOUBLE
    bounds = (C.c_int64 * len(words))(*words)
    _ffi.check(_ffi.lib().mi_filter_between(ctx._h, values_ptr, width, validity_ptr or None, nrows, kind, bounds, sel_ptr, count_ptr,
                                            C.c_void_p(stream or None)))


_AGG_OPS = {"count_star": _ffi.AGG_COUNT_STAR, "count": _ffi.AGG_COUNT, "sum": _ffi.AGG_SUM, "sum_product": _ffi.AGG_SUM_PRODUCT,
            "min": _ffi.AGG_MIN, "max": _ffi.AGG_MAX, "sum_expr": _ffi.AGG_SUM_EXPR}
_AGG_ARITY = {"count_star": 0, "count": 1, "sum": 1, "sum_product": 2, "min": 1, "max": 1}   # (sum_expr: 1 .. 4 factors)


def _agg_check_specs(specs):
    """What needs no library: 1 .. 8 specs, known operations, the right number of arguments -> [(name, args)]"""
    specs = [tuple(sp) if isinstance(sp, (tuple, list)) else (sp,) for sp in specs]
    if not 1 <= len(specs) <= _ffi.MAX_AGGREGATES:
        raise MiError(_ffi.MI_EINVAL, "aggregate takes 1 to %d aggregates, not %d" % (_ffi.MAX_AGGREGATES, len(specs)))
    out = []
    for sp in specs:
        name = str(sp[0]).lower() if sp else ""
        if name not in _AGG_OPS:
            raise MiError(_ffi.MI_EINVAL, "aggregate: unknown operation %r (one of %s)" % (sp[0] if sp else None, ", ".join(sorted(_AGG_OPS))))
        if name == "sum_expr":
            if not 1 <= len(sp) - 1 <= _ffi.MAX_EXPR_FACTORS:
                raise MiError(_ffi.MI_EINVAL, "aggregate: sum_expr takes 1 to %d factors, not %d" % (_ffi.MAX_EXPR_FACTORS, len(sp) - 1))
            factors = [_agg_factor(f) for f in sp[1:]]
            if all(f[0] is None for f in factors):
                raise MiError(_ffi.MI_EINVAL, "aggregate: sum_expr needs at least one factor with a column")
            out.append((name, tuple(factors)))
            continue
        if len(sp) - 1 != _AGG_ARITY[name]:
            raise MiError(_ffi.MI_EINVAL, "aggregate: %s takes %d argument(s), not %d" % (name, _AGG_ARITY[name], len(sp) - 1))
        out.append((name, sp[1:]))
    return out


def _is_number(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _agg_factor(f):
    """One factor of a sum_expr -> (column or None, mul, add).  The forms: a column; (column, mul, add); (None, add) or a
    bare number for a constant.  What a column is -- a name for a scan, a (data, validity, width, class) tuple for the
    *_vectors calls -- is the caller's business: anything that is neither a number nor a 2- / 3-tuple of one of these
    forms is taken as a column."""
    def int64(*constants):
        for v in constants:
            if isinstance(v, int) and not -(1 << 63) <= v < (1 << 63):
                raise MiError(_ffi.MI_EINVAL, "aggregate: the sum_expr constant %d does not fit an int64" % v)

    if _is_number(f):
        int64(f)
        return (None, 1, f)
    if isinstance(f, (tuple, list)):
        if len(f) == 2 and f[0] is None and _is_number(f[1]):
            int64(f[1])
            return (None, 1, f[1])
        if len(f) == 3 and f[0] is not None and _is_number(f[1]) and _is_number(f[2]):
            int64(f[1], f[2])
            return (f[0], f[1], f[2])
        if len(f) in (2, 3) and f[0] is None:
            raise MiError(_ffi.MI_EINVAL, "aggregate: a constant sum_expr factor is (None, number) or a number, not %r" % (f,))
    if f is None or isinstance(f, bool):
        raise MiError(_ffi.MI_EINVAL, "aggregate: a sum_expr factor is a column, (column, mul, add), (None, add) or a number, not %r" % (f,))
    return (f, 1, 0)


def _agg_fill_constants(slot, mul, add):
    """mul / add into a mi_agg_factor or mi_agg_vector_factor: Python ints are MI_AGG_CONST_INT, a float makes both doubles"""
    if isinstance(mul, float) or isinstance(add, float):
        slot.constants, slot.fmul, slot.fadd = _ffi.AGG_CONST_DOUBLE, float(mul), float(add)
        slot.mul, slot.add = 1, 0
        return
    slot.constants, slot.mul, slot.add, slot.fmul, slot.fadd = _ffi.AGG_CONST_INT, mul, add, 1.0, 0.0


def _agg_scan_specs(checked):
    """[(name, args)] -> (mi_agg_spec array, what must stay alive while it is used)"""
    arr = (_ffi.AggSpec * len(checked))()
    keep = []
    for i, (name, cols) in enumerate(checked):
        arr[i].op = _AGG_OPS[name]
        if name == "sum_expr":
            expr = _ffi.AggExpr()
            expr.n_factors = len(cols)
            for slot, (col, mul, add) in zip(expr.factors, cols):
                if col is not None:
                    keep.append(col.encode() if isinstance(col, str) else col)
                    slot.column = keep[-1]
                _agg_fill_constants(slot, mul, add)
            keep.append(expr)
            arr[i].expr = C.pointer(expr)
            continue
        names = [c.encode() if isinstance(c, str) else c for c in cols]
        keep.append(names)
        if names:
            arr[i].column_a = names[0]
        if len(names) > 1:
            arr[i].column_b = names[1]
    return arr, keep


def _agg_vector_specs(checked, classes):
    """[(name, args)] -> (mi_agg_vector_spec array, what must stay alive while it is used)"""
    def fill(slot, col):
        data, validity, width, cls = col
        slot.data, slot.validity, slot.width, slot.value_class = data or None, validity or None, width, classes[cls]

    arr = (_ffi.AggVectorSpec * len(checked))()
    keep = []
    for i, (name, cols) in enumerate(checked):
        arr[i].op = _AGG_OPS[name]
        if name == "sum_expr":
            expr = _ffi.AggVectorExpr()
            expr.n_factors = len(cols)
            for slot, (col, mul, add) in zip(expr.factors, cols):
                if col is not None:
                    fill(slot.column, col)
                _agg_fill_constants(slot, mul, add)
            keep.append(expr)
            arr[i].expr = C.pointer(expr)
            continue
        for slot, col in zip((arr[i].a, arr[i].b), cols):
            fill(slot, col)
    return arr, keep


def _agg_value(v):
    """mi_agg_value -> int / float / None"""
    if v.is_null:
        return None
    if v.kind == _ffi.AGG_VALUE_DOUBLE:
        return struct.unpack("<d", struct.pack("<Q", v.lo))[0]
    return (v.hi << 64) + v.lo


def aggregate_vectors(ctx, specs, nrows, sel_ptr=0, count_ptr=0, stream=0, detail=False):
    """Aggregates over resident vectors (mi_aggregate_vectors).  `specs` as Relation.aggregate takes them, a column being
    (data_ptr, validity_ptr or 0, width, value_class) with value_class one of "signed", "unsigned", "float", "wide", "any";
    sel_ptr / count_ptr: a selection vector in the filter's layout, or 0 for every row.  Returns ints / floats / None per
    spec; with `detail` (value, contributing rows) pairs."""
    classes = {"any": _ffi.AGG_CLASS_ANY, "signed": _ffi.AGG_CLASS_SIGNED, "unsigned": _ffi.AGG_CLASS_UNSIGNED,
               "float": _ffi.AGG_CLASS_FLOAT, "wide": _ffi.AGG_CLASS_WIDE}
    checked = _agg_check_specs(specs)
    arr, _keep = _agg_vector_specs(checked, classes)
    out = (_ffi.AggValue * len(checked))()
    _ffi.check(_ffi.lib().mi_aggregate_vectors(ctx._h, arr, len(checked), sel_ptr or None, count_ptr or None, nrows, out,
                                               C.c_void_p(stream or None)))
    return [(_agg_value(v), v.count) if detail else _agg_value(v) for v in out]


def aggregate_counters():
    """(agg_windows launches, agg_combine launches, agg_windows ms, agg_combine ms) of this process; the times are summed
    over the mi_scan_aggregate calls that ran with MI_AGG_TIMING=1 in the environment."""
    a, b, c, d = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    _ffi.check(_ffi.lib().mi_aggregate_counters(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return a.value, b.value, c.value, d.value


def _group_check_keys(keys):
    """What needs no library: 1 .. 4 keys -> list"""
    keys = [keys] if isinstance(keys, (str, bytes)) else list(keys)
    if not 1 <= len(keys) <= _ffi.MAX_GROUP_KEYS:
        raise MiError(_ffi.MI_EINVAL, "group_aggregate takes 1 to %d key columns, not %d" % (_ffi.MAX_GROUP_KEYS, len(keys)))
    return keys


def _group_key_value(v, as_text):
    """mi_group_key_value -> int / str (as_text) / bytes / None"""
    if v.is_null:
        return None
    raw = bytes(v.bytes)
    if v.kind == _ffi.GROUP_KEY_STRING:
        body = raw[4: 4 + int.from_bytes(raw[:4], "little")]
        return body.decode("utf-8", "surrogateescape") if as_text else body
    return int.from_bytes(raw, "little", signed=True)


def _group_rows(out_keys, out_values, n_groups, n_keys, n_aggs, text, detail):
    rows = []
    for g in range(n_groups):
        key = tuple(_group_key_value(out_keys[g * n_keys + k], text[k]) for k in range(n_keys))
        vals = [out_values[g * n_aggs + a] for a in range(n_aggs)]
        rows.append((key, [(_agg_value(v), v.count) if detail else _agg_value(v) for v in vals]))
    return rows


def group_aggregate_vectors(ctx, keys, specs, nrows, sel_ptr=0, count_ptr=0, capacity=_ffi.MAX_GROUPS, stream=0, detail=False):
    """GROUP BY over resident vectors (mi_group_aggregate_vectors).  `keys`: 1 .. 4 columns (data_ptr, validity_ptr or 0,
    width, key_class) with key_class one of "signed", "unsigned", "wide", "string" (16-byte string_t rows; they come back as
    bytes) ; `specs`, sel_ptr / count_ptr as aggregate_vectors takes them.  Returns [(key_tuple, [values...]), ...] sorted
    ascending by key, NULLS LAST; with `detail` every value is a (value, contributing rows) pair."""
    classes = {"signed": _ffi.GROUP_KEY_CLASS_SIGNED, "unsigned": _ffi.GROUP_KEY_CLASS_UNSIGNED, "wide": _ffi.GROUP_KEY_CLASS_WIDE,
               "string": _ffi.GROUP_KEY_CLASS_STRING}
    agg_classes = {"any": _ffi.AGG_CLASS_ANY, "signed": _ffi.AGG_CLASS_SIGNED, "unsigned": _ffi.AGG_CLASS_UNSIGNED,
                   "float": _ffi.AGG_CLASS_FLOAT, "wide": _ffi.AGG_CLASS_WIDE}
    keys = _group_check_keys(keys)
    checked = _agg_check_specs(specs)
    karr = (_ffi.GroupKeyColumn * len(keys))()
    for i, (data, validity, width, cls) in enumerate(keys):
        if cls not in classes:
            raise MiError(_ffi.MI_EINVAL, "group_aggregate_vectors: unknown key class %r (one of %s)" % (cls, ", ".join(sorted(classes))))
        karr[i].data, karr[i].validity, karr[i].width, karr[i].key_class = data or None, validity or None, width, classes[cls]
    arr, _keep = _agg_vector_specs(checked, agg_classes)
    capacity = max(int(capacity), 0)
    out_keys = (_ffi.GroupKeyValue * max(capacity * len(keys), 1))()
    out_values = (_ffi.AggValue * max(capacity * len(checked), 1))()
    n_groups = C.c_int32()
    _ffi.check(_ffi.lib().mi_group_aggregate_vectors(ctx._h, karr, len(keys), arr, len(checked), sel_ptr or None, count_ptr or None, nrows,
                                                     out_keys, out_values, capacity, C.byref(n_groups), C.c_void_p(stream or None)))
    return _group_rows(out_keys, out_values, n_groups.value, len(keys), len(checked), [False] * len(keys), detail)


def group_aggregate_counters():
    """(group_windows launches, group_combine launches, group_windows ms, group_combine ms) of this process; the times are
    summed over the mi_scan_group_aggregate calls that ran with MI_AGG_TIMING=1 in the environment."""
    a, b, c, d = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    _ffi.check(_ffi.lib().mi_group_aggregate_counters(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return a.value, b.value, c.value, d.value


def _hash_check_args(key, max_groups, capacity):
    """What needs no library: ONE key, 1 <= max_groups <= 2^24 -> (key, max_groups, capacity); capacity None = max_groups"""
    if isinstance(key, list) or (isinstance(key, tuple) and all(isinstance(k, (str, bytes, tuple, list)) for k in key)):
        if len(key) != 1:
            raise MiError(_ffi.MI_ENOTSUP, "hash_aggregate takes ONE key column, not %d: a key of several columns is not one 64-bit word; "
                                           "group_aggregate takes up to %d key columns for few groups" % (len(key), _ffi.MAX_GROUP_KEYS))
        key = key[0]
    if isinstance(max_groups, bool) or not isinstance(max_groups, int) or not 1 <= max_groups <= _ffi.MAX_HASH_GROUPS:
        raise MiError(_ffi.MI_EINVAL, "hash_aggregate: max_groups must be an int of 1 to %d (MI_MAX_HASH_GROUPS), not %r" % (_ffi.MAX_HASH_GROUPS, max_groups))
    capacity = max_groups if capacity is None else max(int(capacity), 0)
    return key, max_groups, capacity


def hash_aggregate_vectors(ctx, key, specs, nrows, max_groups, sel_ptr=0, count_ptr=0, capacity=None, stream=0, detail=False):
    """Hash GROUP BY over resident vectors for many groups (mi_hash_aggregate_vectors).  `key`: ONE column (data_ptr,
    validity_ptr or 0, width, key_class) with key_class "signed" or "unsigned" ("wide" and "string" are MI_ENOTSUP:
    group_aggregate_vectors takes them for few groups); `specs`, sel_ptr / count_ptr as aggregate_vectors takes them, without
    floating-point sums and 16-byte MIN / MAX; `max_groups`: 1 .. 2^24 distinct keys, more is MI_ENOTSUP.  Returns
    [((key,), [values...]), ...] sorted ascending by key, NULLS LAST; with `detail` every value is a (value, contributing
    rows) pair.  `capacity` (default max_groups): the groups the result arrays hold."""
    classes = {"signed": _ffi.GROUP_KEY_CLASS_SIGNED, "unsigned": _ffi.GROUP_KEY_CLASS_UNSIGNED, "wide": _ffi.GROUP_KEY_CLASS_WIDE,
               "string": _ffi.GROUP_KEY_CLASS_STRING}
    agg_classes = {"any": _ffi.AGG_CLASS_ANY, "signed": _ffi.AGG_CLASS_SIGNED, "unsigned": _ffi.AGG_CLASS_UNSIGNED,
                   "float": _ffi.AGG_CLASS_FLOAT, "wide": _ffi.AGG_CLASS_WIDE}
    key, max_groups, capacity = _hash_check_args(key, max_groups, capacity)
    checked = _agg_check_specs(specs)
    data, validity, width, cls = key
    if cls not in classes:
        raise MiError(_ffi.MI_EINVAL, "hash_aggregate_vectors: unknown key class %r (one of %s)" % (cls, ", ".join(sorted(classes))))
    kcol = _ffi.GroupKeyColumn()
    kcol.data, kcol.validity, kcol.width, kcol.key_class = data or None, validity or None, width, classes[cls]
    arr, _keep = _agg_vector_specs(checked, agg_classes)
    out_keys = (_ffi.GroupKeyValue * max(capacity, 1))()
    out_values = (_ffi.AggValue * max(capacity * len(checked), 1))()
    n_groups = C.c_int32()
    _ffi.check(_ffi.lib().mi_hash_aggregate_vectors(ctx._h, C.byref(kcol), arr, len(checked), sel_ptr or None, count_ptr or None, nrows, max_groups,
                                                    out_keys, out_values, capacity, C.byref(n_groups), C.c_void_p(stream or None)))
    return _group_rows(out_keys, out_values, n_groups.value, 1, len(checked), [False], detail)


def hash_aggregate_counters():
    """(hash_group_rows launches, hash_group_collect launches, hash_group_rows ms, hash_group_collect ms) of this process; the
    times are summed over the mi_scan_hash_aggregate / mi_hash_aggregate_vectors calls that ran with MI_AGG_TIMING=1."""
    a, b, c, d = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
    _ffi.check(_ffi.lib().mi_hash_aggregate_counters(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return a.value, b.value, c.value, d.value


def filter_float_key(value, width):
    """The order-preserving integer key the filter kernel compares a FLOAT (width 4) / DOUBLE (width 8) value by."""
    key = C.c_int64()
    _ffi.check(_ffi.lib().mi_filter_float_key(float(value), width, C.byref(key)))
    return key.value


def filter_launch_counts():
    """(launches of the filter kernel's base instance, launches of its FLOAT / DOUBLE / 128-bit instance) by this process."""
    base, ext = C.c_int64(), C.c_int64()
    _ffi.check(_ffi.lib().mi_filter_launch_counts(C.byref(base), C.byref(ext)))
    return base.value, ext.value


def filter_string(ctx, rows_ptr, validity_ptr, nrows, heap_ptr, ptr_base, op, constant, sel_ptr, count_ptr, launches=1):
    """One string leaf ("=", "<", "starts_with", "contains", "ends_with", "like", "not like", ...) over a resident string_t vector
    (mi_filter_string): uploads the constant, launches the filter kernel `launches` times and waits.  Returns the mean kernel
    time in ms, from device events."""
    codes = {"=": _ffi.F_EQ, "<>": _ffi.F_NE, "<": _ffi.F_LT, "<=": _ffi.F_LE, ">": _ffi.F_GT, ">=": _ffi.F_GE, "starts_with": _ffi.F_STARTS_WITH,
             "contains": _ffi.F_CONTAINS, "ends_with": _ffi.F_ENDS_WITH, "like": _ffi.F_LIKE, "not like": _ffi.F_NOT_LIKE}
    constant = constant.encode() if isinstance(constant, str) else bytes(constant)
    ms = C.c_float()
    _ffi.check(_ffi.lib().mi_filter_string(ctx._h, rows_ptr, validity_ptr or None, nrows, heap_ptr or None, ptr_base, codes[op.lower()], constant,
                                           len(constant), sel_ptr, count_ptr, launches, C.byref(ms)))
    return ms.value


def filter_like_match(op, pattern, row):
    """Does the byte string `row` pass `op` ("contains", "ends_with", "like", "not like") with this needle / suffix / pattern:
    the matcher the filter kernel compiles, on the host (mi_filter_like_match).  Raises MiError where Relation.filter would."""
    as_bytes = lambda v: v.encode() if isinstance(v, str) else bytes(v)
    code = op if isinstance(op, int) else {"contains": _ffi.F_CONTAINS, "ends_with": _ffi.F_ENDS_WITH, "like": _ffi.F_LIKE,
                                           "not like": _ffi.F_NOT_LIKE}[op.lower()]
    pattern, row, result = as_bytes(pattern), as_bytes(row), C.c_int32()
    _ffi.check(_ffi.lib().mi_filter_like_match(code, pattern, len(pattern), row, len(row), C.byref(result)))
    return bool(result.value)


def filter_pattern_launches():
    """Launches of the filter kernel's contains / ends_with / LIKE instance by this process (mi_filter_pattern_launches)."""
    n = C.c_int64()
    _ffi.check(_ffi.lib().mi_filter_pattern_launches(C.byref(n)))
    return n.value


_FILTER_LEAF_FIELDS = ("data", "validity", "in_values", "lo", "hi", "op", "width", "flags", "n_in")


def filter_program(ctx, leaves, nrows, sel_ptr, count_ptr, stream=0):
    """A hand-built program of the filter kernel's own leaves over resident vectors (mi_filter_program_vectors): `leaves` are
    dicts (missing fields are 0) or tuples in the order data, validity, in_values, lo, hi, op, width, flags, n_in, every
    address a device address.  Nothing is normalised, uploaded or waited for; _ffi.FL_* / FLF_* name the ops and flag bits."""
    arr = (_ffi.FilterVectorLeaf * max(len(leaves), 1))()
    for slot, leaf in zip(arr, leaves):
        if not isinstance(leaf, dict):
            leaf = dict(zip(_FILTER_LEAF_FIELDS, leaf))
        unknown = set(leaf) - set(_FILTER_LEAF_FIELDS)
        if unknown:
            raise ValueError("filter_program: unknown leaf field %s" % sorted(unknown))
        for name in _FILTER_LEAF_FIELDS:
            v = int(leaf.get(name, 0) or 0)
            if name in ("lo", "hi") and v >= 1 << 63:   # an address above 2^63 in a signed field
                v -= 1 << 64
            setattr(slot, name, v or None if name in ("data", "validity", "in_values") else v)
    _ffi.check(_ffi.lib().mi_filter_program_vectors(ctx._h, arr, len(leaves), nrows, sel_ptr or None, count_ptr or None, C.c_void_p(stream or None)))


def writer_fused_counts():
    """(row groups the fused COPY pump encoded where the scan decoded them, string-view columns among them) by this process."""
    groups, views = C.c_int64(), C.c_int64()
    _ffi.check(_ffi.lib().mi_writer_fused_counts(C.byref(groups), C.byref(views)))
    return groups.value, views.value


# ---------------------------------------------------------------------------------------------------- logical views
def _valid_bits(validity_ptr, n, shift=0):
    """`shift`: bit of the first word that belongs to row 0 (mi_vector.validity_shift, nested children only)."""
    if not validity_ptr:
        return np.ones(n, bool)
    words = np.ctypeslib.as_array(C.cast(validity_ptr, C.POINTER(C.c_uint64)), shape=((n + shift + 63) // 64 or 1,))
    return np.unpackbits(words.view(np.uint8), bitorder="little")[shift: shift + n].astype(bool)


def uuid_to_hugeint(u):
    """uuid.UUID (or its text) -> the signed 128-bit integer DuckDB stores for it: the UUID's bits with the top bit flipped, so
    that signed order is the order of the canonical text (extension_format.hpp: UuidFromArrow)."""
    u = u if isinstance(u, uuid.UUID) else uuid.UUID(str(u))
    v = u.int ^ (1 << 127)
    return v - (1 << 128) if v >= (1 << 127) else v


def uuid_from_hugeint(v):
    """the inverse of uuid_to_hugeint"""
    return uuid.UUID(int=(int(v) & ((1 << 128) - 1)) ^ (1 << 127))


def _string_values(data_ptr, n, ok, as_bytes):
    raw = np.ctypeslib.as_array(C.cast(data_ptr, C.POINTER(C.c_uint8)), shape=(n * 16,)).reshape(n, 16)
    lens = raw[:, 0:4].copy().view(np.uint32).reshape(-1)
    ptrs = raw[:, 8:16].copy().view(np.uint64).reshape(-1)
    out = []
    for i in range(n):
        if not ok[i]:
            out.append(None)
            continue
        ln = int(lens[i])
        b = raw[i, 4: 4 + ln].tobytes() if ln <= 12 else C.string_at(int(ptrs[i]), ln)
        out.append(b if as_bytes else b.decode("utf-8", "replace"))   # damaged payloads are not ours to reject
    return out


_INT_TYPES = {"TINYINT": np.int8, "UTINYINT": np.uint8, "SMALLINT": np.int16, "USMALLINT": np.uint16,
              "INTEGER": np.int32, "UINTEGER": np.uint32, "BIGINT": np.int64, "UBIGINT": np.uint64,
              "DATE": np.int32, "TIME": np.int64, "TIMESTAMP": np.int64, "TIMESTAMP_S": np.int64,
              "TIMESTAMP_MS": np.int64, "TIMESTAMP_NS": np.int64, "TIMESTAMP WITH TIME ZONE": np.int64}


def _flat_values(duck_type, width, data_ptr, validity_ptr, n, shift=0):
    """One host DuckDB flat vector -> python list of the raw stored values (ints for temporal / decimal types)."""
    ok = _valid_bits(validity_ptr, n, shift)
    if n == 0:
        return []
    if duck_type in ("VARCHAR", "BLOB", "JSON"):
        return _string_values(data_ptr, n, ok, as_bytes=(duck_type == "BLOB"))
    raw = np.ctypeslib.as_array(C.cast(data_ptr, C.POINTER(C.c_uint8)), shape=(n * width,))
    if duck_type == "BOOLEAN":
        return [bool(raw[i]) if ok[i] else None for i in range(n)]
    if duck_type in ("FLOAT", "DOUBLE"):
        vals = raw.view(np.float32 if width == 4 else np.float64)
        return [float(vals[i]) if ok[i] else None for i in range(n)]
    if duck_type == '"NULL"':
        return [None] * n
    if duck_type == "INTERVAL":
        md, us = raw.view(np.int32), raw.view(np.int64)
        return [(int(md[4 * i]), int(md[4 * i + 1]), int(us[2 * i + 1])) if ok[i] else None for i in range(n)]
    if duck_type == "UUID":
        lo, hi = raw.view(np.uint64)[0::2], raw.view(np.int64)[1::2]
        return [uuid_from_hugeint((int(hi[i]) << 64) + int(lo[i])) if ok[i] else None for i in range(n)]
    if duck_type.startswith("DECIMAL") and width == 16:
        lo, hi = raw.view(np.uint64)[0::2], raw.view(np.int64)[1::2]
        return [(int(hi[i]) << 64) + int(lo[i]) if ok[i] else None for i in range(n)]
    if duck_type.startswith("DECIMAL"):
        vals = raw.view({2: np.int16, 4: np.int32, 8: np.int64}[width])
    else:
        vals = raw.view(_INT_TYPES[duck_type])
    return [vals[i].item() if ok[i] else None for i in range(n)]


def _split_top(text, sep=","):
    """Split on `sep` outside parentheses / quotes."""
    parts, depth, cur, quoted = [], 0, [], False
    for ch in text:
        if ch == '"':
            quoted = not quoted
        if not quoted:
            depth += ch == "("
            depth -= ch == ")"
            if ch == sep and depth == 0:
                parts.append("".join(cur).strip())
                cur = []
                continue
        cur.append(ch)
    if cur or parts:
        parts.append("".join(cur).strip())
    return parts


def parse_duck_type(text):
    """'STRUCT(a INTEGER, b VARCHAR)[]' -> ('list', ('struct', [('a', ('leaf', 'INTEGER')), ...])).  Mirrors the
    LogicalType the reference binds for the column (ArrowType::GetDuckType)."""
    text = text.strip()
    if text.endswith("]"):
        i = text.rindex("[")
        inner, size = parse_duck_type(text[:i]), text[i + 1: -1]
        return ("list", inner) if size == "" else ("array", inner, int(size))
    if text.startswith("STRUCT(") and text.endswith(")"):
        kids = []
        for part in _split_top(text[7:-1]):
            if part.startswith('"'):
                j = part.index('"', 1)
                name, rest = part[1:j], part[j + 1:]
            else:
                name, _, rest = part.partition(" ")
            kids.append((name, parse_duck_type(rest)))
        return ("struct", kids)
    if text.startswith("UNION(") and text.endswith(")"):
        kids = []
        for part in _split_top(text[6:-1]):
            if part.startswith('"'):
                j = part.index('"', 1)
                name, rest = part[1:j], part[j + 1:]
            else:
                name, _, rest = part.partition(" ")
            kids.append((name, parse_duck_type(rest)))
        return ("union", kids)
    if text.startswith("MAP(") and text.endswith(")"):
        k, v = _split_top(text[4:-1])
        return ("map", parse_duck_type(k), parse_duck_type(v))
    return ("leaf", text)


def _vector_values(v, ty, n):
    """One host mi_vector (flat, dictionary or nested) of n rows -> python values."""
    shift = v.validity_shift
    if v.kind == _ffi.K_DICT:
        dt = ty[1]
        base = _flat_values(dt, {"VARCHAR": 16, "BLOB": 16, "JSON": 16}.get(dt, _dict_width(dt)), v.dictionary, v.dictionary_validity,
                            v.dict_len + 1)
        sel = np.ctypeslib.as_array(C.cast(v.data, C.POINTER(C.c_uint32)), shape=(max(n, 1),))[:n]
        return [base[int(x)] for x in sel]
    if ty[0] == "leaf":
        return _flat_values(ty[1], v.out_width, v.data, v.validity, n, shift)
    ok = _valid_bits(v.validity, n, shift)
    if ty[0] in ("list", "map"):
        child = v.children[0]
        cty = ty[1] if ty[0] == "list" else ("struct", [("key", ty[1]), ("value", ty[2])])
        cvals = _vector_values(child, cty, child.count)
        ent = np.ctypeslib.as_array(C.cast(v.data, C.POINTER(C.c_uint64)), shape=(max(n, 1) * 2,))[: n * 2].reshape(-1, 2)
        out = []
        for r in range(n):
            if not ok[r]:
                out.append(None)
                continue
            vals = cvals[int(ent[r, 0]): int(ent[r, 0]) + int(ent[r, 1])]
            out.append([(e["key"], e["value"]) for e in vals] if ty[0] == "map" else vals)
        return out
    if ty[0] == "array":
        child = v.children[0]
        cvals = _vector_values(child, ty[1], child.count)
        return [cvals[r * ty[2]: (r + 1) * ty[2]] if ok[r] else None for r in range(n)]
    if ty[0] == "union":
        if v.n_children == 0:      # a column absent from this file (union_by_name): an all-NULL vector without a tree
            return [None] * n
        # children: the tag vector (UTINYINT member index), then one vector per member; a row is its selected member's value
        tags = _flat_values("UTINYINT", 1, v.children[0].data, None, n)
        kids = [_vector_values(v.children[1 + i], kt, n) for i, (_, kt) in enumerate(ty[1])]
        return [kids[tags[r]][r] if ok[r] else None for r in range(n)]
    kids = [_vector_values(v.children[i], kt, n) for i, (_, kt) in enumerate(ty[1])]
    return [{nm: kid[r] for (nm, _), kid in zip(ty[1], kids)} if ok[r] else None for r in range(n)]


def chunk_to_columns(chunk, fields):
    """mi_data_chunk (host vectors) -> list of python value lists; dictionary vectors flattened, nested vectors as
    python lists / dicts / (key, value) tuples."""
    return [_vector_values(chunk.columns[ci], parse_duck_type(f["duck_type"]), chunk.size) for ci, f in enumerate(fields)]


def _dict_width(duck_type):
    if duck_type in _INT_TYPES:
        return np.dtype(_INT_TYPES[duck_type]).itemsize
    return {"BOOLEAN": 1, "FLOAT": 4, "DOUBLE": 8, "INTERVAL": 16, "UUID": 16}.get(duck_type, 8)


# ---------------------------------------------------------------------------------------------------- scan operator
class Relation:
    """Result of read_arrow / scan_arrow_ipc: bind info + a pull loop of <= 2048-row DataChunks."""

    def __init__(self, conn, handle, keep=None):
        self._conn = conn
        self._h = handle
        self._keep = keep
        self._contexts = [c for c in [conn.ctx] + (keep if isinstance(keep, list) else []) if isinstance(c, Context)]
        for c in self._contexts:
            c._retain()
        n = C.c_int32(0)
        _ffi.check(_ffi.lib().mi_scan_bind(self._h, None, 0, C.byref(n)))
        fields = (_ffi.Field * max(n.value, 1))()
        _ffi.check(_ffi.lib().mi_scan_bind(self._h, fields, n.value, C.byref(n)))
        self.fields = [_field_dict(f) for f in fields[: n.value]]
        self._out_fields = self.fields
        self._projection = None
        self._initialised = False

    @property
    def columns(self):
        return [f["name"] for f in self._out_fields]

    @property
    def types(self):
        return [f["duck_type"] for f in self._out_fields]

    def project(self, names):
        """projection_pushdown = true (read_arrow.cpp:46).  Applied lazily at the first pull, like init_global."""
        by_name = {f["name"]: f for f in self.fields}
        missing = [n for n in names if n not in by_name]
        if missing:
            raise MiError(_ffi.MI_EINVAL, "Field '%s' does not exist in IPC file schema" % missing[0])
        self._projection = list(names)
        self._out_fields = [by_name[n] for n in names]
        return self

    def filter_range(self, column, lo, hi):
        _ffi.check(_ffi.lib().mi_scan_set_filter_range(self._h, column.encode(), lo, hi))
        return self

    def filter(self, expr):
        """Pushed-down predicate tree (mi_scan_set_filter).  `expr` is nested tuples:
            ("and", e1, e2, ...) | ("or", e1, e2, ...) | (column, op, value) with op in = <> != < <= > >= |
            (column, "in", [values]) | (column, "is null") | (column, "is not null") | (column, "starts_with", prefix) |
            (column, "contains", needle) | (column, "ends_with", suffix) | (column, "like", pattern) | (column, "not like", pattern)
        Constants are the stored integers, or str / bytes for VARCHAR / BLOB columns (byte-wise order).  The column's DuckDB
        type picks what a number is sent as: FLOAT / DOUBLE columns take Python floats (float('nan'), inf; ints are converted)
        in DuckDB's total order -- NaN = NaN, NaN greatest, -0.0 = +0.0; HUGEINT / DECIMAL(19..38) columns take ints of up to
        128 bits; UUID columns take uuid.UUID values or their text; a decimal.Decimal on any DECIMAL column is scaled to the
        stored integer.  A float against an integer column
        is refused.  NULL semantics are SQL's: a comparison with NULL is not true.  Needles and suffixes are literal bytes; in a
        LIKE pattern `%` is the only wildcard (`_` and more than 8 literal segments are refused with MI_ENOTSUP, there is no
        escape character), and a NULL row passes neither "like" nor "not like"."""
        ops = {"=": _ffi.F_EQ, "==": _ffi.F_EQ, "<>": _ffi.F_NE, "!=": _ffi.F_NE, "<": _ffi.F_LT, "<=": _ffi.F_LE,
               ">": _ffi.F_GT, ">=": _ffi.F_GE, "is null": _ffi.F_IS_NULL, "is not null": _ffi.F_IS_NOT_NULL, "in": _ffi.F_IN,
               "starts_with": _ffi.F_STARTS_WITH, "contains": _ffi.F_CONTAINS, "ends_with": _ffi.F_ENDS_WITH, "like": _ffi.F_LIKE,
               "not like": _ffi.F_NOT_LIKE}
        nodes, keep = [None], []
        duck = {f["name"]: f["duck_type"] for f in self.fields}

        def numbers(col, vals):
            """-> (value_kind, low words, high words or None) of the constants of one leaf"""
            ty = duck.get(col, "")
            if ty == "UUID" and vals and all(isinstance(v, (uuid.UUID, str, bytes)) for v in vals):
                # the hugeint_t image, always as 128 bits: an image that happens to fit 64 bits is still no int64 constant
                stored = [uuid_to_hugeint(v.decode() if isinstance(v, bytes) else v) for v in vals]
                signed = lambda w: w - (1 << 64) if w >= (1 << 63) else w
                return _ffi.FV_INT128, [signed(v & ((1 << 64) - 1)) for v in stored], [signed((v >> 64) & ((1 << 64) - 1)) for v in stored]
            if ty in ("FLOAT", "DOUBLE") and all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in vals):
                return _ffi.FV_DOUBLE, [struct.unpack("<q", struct.pack("<d", float(v)))[0] for v in vals], None
            m = re.match(r"DECIMAL\((\d+),(\d+)\)$", ty)
            stored = []
            for v in vals:
                if isinstance(v, decimal.Decimal):
                    if not m:
                        raise MiError(_ffi.MI_EINVAL, "filter on column '%s' (%s): a Decimal constant needs a DECIMAL column" % (col, ty))
                    scaled = decimal.Context(prec=120).scaleb(v, int(m.group(2)))
                    if scaled != scaled.to_integral_value():
                        raise MiError(_ffi.MI_EINVAL, "filter on column '%s' (%s): %s has more digits behind the point than the column" % (col, ty, v))
                    v = int(scaled)
                stored.append(v)
            if any(isinstance(v, float) for v in stored):   # the library names the column it does not fit
                return _ffi.FV_DOUBLE, [struct.unpack("<q", struct.pack("<d", v))[0] for v in stored], None
            stored = [int(v) for v in stored]
            if all(-(1 << 63) <= v < (1 << 63) for v in stored):
                return _ffi.FV_INT64, stored, None
            if not all(-(1 << 127) <= v < (1 << 127) for v in stored):
                raise MiError(_ffi.MI_EINVAL, "filter on column '%s': constant beyond 128 bits" % col)
            signed = lambda w: w - (1 << 64) if w >= (1 << 63) else w
            return _ffi.FV_INT128, [signed(v & ((1 << 64) - 1)) for v in stored], [signed((v >> 64) & ((1 << 64) - 1)) for v in stored]

        def emit(at, e):
            if e[0] in ("and", "or") and len(e) > 1 and isinstance(e[1], tuple):
                kids = list(e[1:])
                first = len(nodes)
                nodes.extend([None] * len(kids))
                nodes[at] = _ffi.FilterNode(op=_ffi.F_AND if e[0] == "and" else _ffi.F_OR, first_child=first, n_children=len(kids))
                for k, kid in enumerate(kids):
                    emit(first + k, kid)
                return
            col, op = e[0], e[1].lower()
            n = _ffi.FilterNode(op=ops[op], column=col.encode())
            as_bytes = lambda v: v.encode() if isinstance(v, str) else bytes(v)
            is_uuid = duck.get(col) == "UUID"   # its text is a 128-bit constant, not a byte string
            if op == "in" and len(e[2]) > 0 and isinstance(e[2][0], (str, bytes)) and not is_uuid:
                vals = [as_bytes(v) for v in e[2]]
                ptrs = (C.c_char_p * len(vals))(*vals)
                lens = (C.c_int32 * len(vals))(*[len(v) for v in vals])
                keep.extend([vals, ptrs, lens])
                n.str_values, n.str_lens, n.n_values = ptrs, lens, len(vals)
            elif op == "in":
                n.value_kind, lows, highs = numbers(col, list(e[2]))
                arr = (C.c_int64 * max(len(lows), 1))(*lows)
                keep.append(arr)
                n.values, n.n_values = arr, len(lows)
                if highs is not None:
                    arr_hi = (C.c_int64 * max(len(highs), 1))(*highs)
                    keep.append(arr_hi)
                    n.values_hi = arr_hi
            elif op not in ("is null", "is not null") and isinstance(e[2], (str, bytes)) and not is_uuid:
                v = as_bytes(e[2])
                keep.append(v)
                n.str_value, n.str_len = v, len(v)
            elif op not in ("is null", "is not null"):
                n.value_kind, lows, highs = numbers(col, [e[2]])
                n.value = lows[0]
                if highs is not None:
                    n.value_hi = highs[0]
            nodes[at] = n

        emit(0, expr)
        arr = (_ffi.FilterNode * len(nodes))(*nodes)
        _ffi.check(_ffi.lib().mi_scan_set_filter(self._h, arr, len(nodes), 0))
        return self

    def chunks(self):
        self._init()
        ch = _ffi.DataChunk()
        while True:
            _ffi.check(_ffi.lib().mi_scan_next(self._h, C.byref(ch)))
            if ch.size == 0:
                return
            yield ch

    def fetch_columns(self, apply_filter=True):
        """All rows as python value lists per column (stored integer values for temporal / decimal types)."""
        out = [[] for _ in self._out_fields]
        for ch in self.chunks():
            cols = chunk_to_columns(ch, self._out_fields)
            if apply_filter and ch.sel:
                sel = [ch.sel[i] for i in range(ch.sel_count)]
                cols = [[c[i] for i in sel] for c in cols]   # (compacted chunks carry no sel: their rows are the selected ones)
            for o, c in zip(out, cols):
                o.extend(c)
        return out

    def fetchall(self):
        cols = self.fetch_columns()
        return list(zip(*cols)) if cols and cols[0] is not None else []

    def _init(self):
        if not self._initialised:
            if self._projection:
                arr = (C.c_char_p * len(self._projection))(*[n.encode() for n in self._projection])
                _ffi.check(_ffi.lib().mi_scan_init(self._h, arr, len(self._projection)))
            else:
                _ffi.check(_ffi.lib().mi_scan_init(self._h, None, 0))
            self._initialised = True

    def count(self, detail=False):
        """SELECT count(*) (rows passing the pushed-down filter, if any); the pull loop runs natively."""
        self._init()
        rows, sel, chunks = C.c_int64(), C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().mi_scan_count(self._h, C.byref(rows), C.byref(sel), C.byref(chunks)))
        return dict(rows=rows.value, selected=sel.value, chunks=chunks.value) if detail else sel.value

    def sum_product(self, a, b, filters=()):
        """SELECT sum(a * b), count(*) WHERE lo <= f < hi ... evaluated on the GPU (mi_scan_sum_product); `filters` =
        [(column, lo, hi), ...] on stored integers.  Returns (sum as python int, rows selected, rows scanned)."""
        arr = (_ffi.RangeFilter * max(len(filters), 1))()
        for i, (c, lo, hi) in enumerate(filters):
            arr[i].column, arr[i].lo, arr[i].hi = c.encode(), lo, hi
        r = _ffi.SumProductResult()
        _ffi.check(_ffi.lib().mi_scan_sum_product(self._h, a.encode(), b.encode(), arr, len(filters), C.byref(r)))
        self._initialised = True
        return (r.sum_hi << 64) + r.sum_lo, r.rows_selected, r.rows_scanned

    def aggregate(self, specs, detail=False):
        """SELECT agg_1, ..., agg_n (n <= 8) over the rows the pushed-down filter keeps, on the GPU in one pass
        (mi_scan_aggregate); call it in place of chunks() / count().  `specs`: ("count_star",), ("count", c), ("sum", c),
        ("sum_product", a, b), ("min", c), ("max", c), ("sum_expr", factor, ...) -- the sum of a product of 1 .. 4 factors,
        a factor being a column name, (column, mul, add) for add + mul * column, or (None, add) / a bare number for a
        constant; Python ints are exact int64 constants, floats doubles (floating-point columns only).  Returns one Python value per spec -- an int (counts; sums, minima and
        maxima of integer-like columns as the stored integers, exact in 128 bits), a float (FLOAT / DOUBLE columns) or None
        (SUM / MIN / MAX over no row that is not NULL); with `detail` also the rows scanned and selected:
        (values, rows_scanned, rows_selected)."""
        checked = _agg_check_specs(specs)
        arr, _keep = _agg_scan_specs(checked)
        out = (_ffi.AggValue * len(checked))()
        scanned, selected = C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().mi_scan_aggregate(self._h, arr, len(checked), out, C.byref(scanned), C.byref(selected)))
        self._initialised = True
        values = self._typed_aggregates(checked, [_agg_value(v) for v in out])
        return (values, scanned.value, selected.value) if detail else values

    def _typed_aggregates(self, checked, values):
        """MIN / MAX of a UUID column come back as uuid.UUID, not as the stored 128-bit integer"""
        types = {f["name"]: f["duck_type"] for f in self.fields}
        as_uuid = [name in ("min", "max") and types.get(cols[0] if isinstance(cols[0], str) else cols[0].decode()) == "UUID" for name, cols in checked]
        return [uuid_from_hugeint(v) if u and v is not None else v for u, v in zip(as_uuid, values)]

    def group_aggregate(self, keys, specs, detail=False, capacity=_ffi.MAX_GROUPS):
        """SELECT k_1 .. k_m, agg_1 .. agg_n ... GROUP BY k_1 .. k_m (m <= 4, n <= 8) over the rows the pushed-down filter
        keeps, on the GPU (mi_scan_group_aggregate), for few groups: at most 256 distinct keys per 2048-row window and 4096
        in the scan.  `keys`: column names; `specs` as aggregate() takes them.  Returns [(key_tuple, [values...]), ...]
        sorted ascending by key, NULLS LAST; a key comes back as an int (the stored integer), a str (VARCHAR / JSON), bytes (BLOB),
        a uuid.UUID, a bool or None.  With `detail`: (rows, rows_scanned, rows_selected)."""
        keys = _group_check_keys(keys)
        checked = _agg_check_specs(specs)
        arr, _keep = _agg_scan_specs(checked)
        karr = (C.c_char_p * len(keys))(*[k.encode() if isinstance(k, str) else k for k in keys])
        capacity = max(int(capacity), 0)
        out_keys = (_ffi.GroupKeyValue * max(capacity * len(keys), 1))()
        out_values = (_ffi.AggValue * max(capacity * len(checked), 1))()
        n_groups, scanned, selected = C.c_int32(), C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().mi_scan_group_aggregate(self._h, karr, len(keys), arr, len(checked), out_keys, out_values, capacity,
                                                      C.byref(n_groups), C.byref(scanned), C.byref(selected)))
        self._initialised = True
        types = {f["name"]: f["duck_type"] for f in self.fields}
        text = [str(types.get(k if isinstance(k, str) else k.decode(), "")).upper().startswith(("VARCHAR", "JSON")) for k in keys]
        rows = _group_rows(out_keys, out_values, n_groups.value, len(keys), len(checked), text, False)
        # UUID keys as uuid.UUID, BOOLEAN keys as bool (the stored integers otherwise); the order is the stored one either way
        key_types = [str(types.get(k if isinstance(k, str) else k.decode(), "")).upper() for k in keys]
        typed = {"UUID": uuid_from_hugeint, "BOOLEAN": bool}
        if any(t in typed for t in key_types):
            rows = [(tuple(typed[t](v) if t in typed and v is not None else v for t, v in zip(key_types, key)), vals) for key, vals in rows]
        rows = [(key, self._typed_aggregates(checked, vals)) for key, vals in rows]
        return (rows, scanned.value, selected.value) if detail else rows

    def hash_aggregate(self, key, specs, max_groups, detail=False, capacity=None):
        """SELECT k, agg_1 .. agg_n ... GROUP BY k over the rows the pushed-down filter keeps, on the GPU, for MANY groups
        (mi_scan_hash_aggregate): ONE integer-like key column (integers, BOOLEAN, DATE, TIME / TIMESTAMP, DECIMAL(<=18)) and up
        to `max_groups` (1 .. 2^24) distinct keys; more is MI_ENOTSUP, naming max_groups.  `specs` as aggregate() takes them,
        without floating-point sums and MIN / MAX of 16-byte columns (MI_ENOTSUP: group_aggregate takes those, several keys,
        16-byte and string keys, for few groups).  Returns [((key,), [values...]), ...] sorted ascending by key, NULLS LAST.
        With `detail`: (rows, rows_scanned, rows_selected).  `capacity` (default max_groups): the groups the result arrays hold."""
        key, max_groups, capacity = _hash_check_args(key, max_groups, capacity)
        checked = _agg_check_specs(specs)
        arr, _keep = _agg_scan_specs(checked)
        out_keys = (_ffi.GroupKeyValue * max(capacity, 1))()
        out_values = (_ffi.AggValue * max(capacity * len(checked), 1))()
        n_groups, scanned, selected = C.c_int32(), C.c_int64(), C.c_int64()
        _ffi.check(_ffi.lib().mi_scan_hash_aggregate(self._h, key.encode() if isinstance(key, str) else key, arr, len(checked), max_groups, out_keys,
                                                     out_values, capacity, C.byref(n_groups), C.byref(scanned), C.byref(selected)))
        self._initialised = True
        rows = _group_rows(out_keys, out_values, n_groups.value, 1, len(checked), [False], False)
        types = {f["name"]: f["duck_type"] for f in self.fields}
        if str(types.get(key if isinstance(key, str) else key.decode(), "")).upper() == "BOOLEAN":
            rows = [(tuple(bool(v) if v is not None else v for v in k), vals) for k, vals in rows]
        rows = [(k, self._typed_aggregates(checked, vals)) for k, vals in rows]
        return (rows, scanned.value, selected.value) if detail else rows

    def progress(self):
        return _ffi.lib().mi_scan_progress(self._h)

    def stats(self):
        """mi_scan_get_stats: record batches submitted, LZ4 bodies decompressed in HBM, bytes over PCIe, bytes decompressed."""
        st = _ffi.ScanStats()
        _ffi.check(_ffi.lib().mi_scan_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in _ffi.ScanStats._fields_}

    def close(self):
        if self._h:
            _ffi.lib().mi_scan_close(self._h)
            self._h = C.c_void_p()
            for c in self._contexts:
                c._release()

    __del__ = close


# ---------------------------------------------------------------------------------------------------- tables (write side)
class Table:
    """A python-side stand-in for a DuckDB table: names, DuckDB types and python values per column."""

    def __init__(self, names, types, columns):
        self.names, self.types, self.columns = list(names), list(types), [list(c) for c in columns]
        assert len(self.names) == len(self.types) == len(self.columns)

    @property
    def num_rows(self):
        return len(self.columns[0]) if self.columns else 0


def _vector_from_python(values, duck_type, keep):
    """python values -> (data ndarray, validity ndarray|None) in DuckDB flat-vector layout."""
    n = len(values)
    ok = np.array([v is not None for v in values], dtype=bool)
    validity = None
    if not ok.all():
        validity = np.packbits(np.concatenate([ok, np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()
    t = duck_type.upper()
    if t in ("VARCHAR", "BLOB", "JSON"):
        data = np.zeros((n, 16), np.uint8)
        for i, v in enumerate(values):
            if v is None:
                continue
            b = v.encode() if isinstance(v, str) else bytes(v)
            data[i, 0:4] = np.frombuffer(np.uint32(len(b)).tobytes(), np.uint8)
            if len(b) <= 12:
                data[i, 4: 4 + len(b)] = np.frombuffer(b, np.uint8)
            else:
                heap = np.frombuffer(b, np.uint8).copy()
                keep.append(heap)
                data[i, 4:8] = heap[:4]
                data[i, 8:16] = np.frombuffer(np.uint64(heap.ctypes.data).tobytes(), np.uint8)
        return data.reshape(-1), validity
    if t == "BOOLEAN":
        return np.array([1 if v else 0 for v in values], np.uint8), validity
    if t in ("FLOAT", "DOUBLE"):
        return np.array([0.0 if v is None else v for v in values], np.float32 if t == "FLOAT" else np.float64), validity
    if t.startswith("DECIMAL"):
        p = int(t[t.index("(") + 1: t.index(",")])
        if p > 18:
            data = np.zeros((n, 2), np.uint64)
            for i, v in enumerate(values):
                if v is not None:
                    data[i, 0] = v & 0xFFFFFFFFFFFFFFFF
                    data[i, 1] = (v >> 64) & 0xFFFFFFFFFFFFFFFF
            return data.reshape(-1), validity
        dt = np.int16 if p <= 4 else np.int32 if p <= 9 else np.int64
        return np.array([0 if v is None else v for v in values], dt), validity
    if t == "UUID":   # uuid.UUID values (or their text) as DuckDB stores them
        data = np.zeros((n, 2), np.uint64)
        for i, v in enumerate(values):
            if v is not None:
                h = uuid_to_hugeint(v)
                data[i, 0] = h & 0xFFFFFFFFFFFFFFFF
                data[i, 1] = (h >> 64) & 0xFFFFFFFFFFFFFFFF
        return data.reshape(-1), validity
    if t == "HUGEINT":
        data = np.zeros((n, 2), np.uint64)
        for i, v in enumerate(values):
            if v is not None:
                data[i, 0] = v & 0xFFFFFFFFFFFFFFFF
                data[i, 1] = (v >> 64) & 0xFFFFFFFFFFFFFFFF
        return data.reshape(-1), validity
    if t == "INTERVAL":   # (months, days, micros), as fetch_columns returns them -> interval_t rows
        data = np.zeros(n, np.dtype([("months", np.int32), ("days", np.int32), ("micros", np.int64)]))
        for i, v in enumerate(values):
            if v is not None:
                data[i] = tuple(int(x) for x in v)
        return data.view(np.uint8).reshape(-1), validity
    if t in ('"NULL"', "NULL"):   # every value must be None; one byte per row, as the scan's vector of this type has
        if ok.any():
            raise MiError(_ffi.MI_EINVAL, 'a "NULL" column holds only None')
        return np.zeros(max(n, 1), np.uint8), validity
    return np.array([0 if v is None else v for v in values], _INT_TYPES[t]), validity


class UnionValue:
    """A value of a UNION column with its member named: UnionValue("s", "text").  A bare python value goes to the first
    member whose type takes it (what fetch_columns returns for a union column is bare values)."""

    def __init__(self, member, value):
        self.member, self.value = member, value

    def __repr__(self):
        return "UnionValue(%r, %r)" % (self.member, self.value)


def _python_value_fits(v, ty):
    if ty[0] == "leaf":
        t = ty[1].upper()
        if t in ("VARCHAR", "JSON"):
            return isinstance(v, str)
        if t == "BLOB":
            return isinstance(v, (bytes, bytearray))
        if t == "BOOLEAN":
            return isinstance(v, (bool, np.bool_))
        if t in ("FLOAT", "DOUBLE"):
            return isinstance(v, (float, np.floating))
        if t == "INTERVAL":
            return isinstance(v, tuple) and len(v) == 3
        if t in ('"NULL"', "NULL"):
            return False
        if t == "UUID":
            import uuid as _uuid
            return isinstance(v, _uuid.UUID)
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    if ty[0] == "struct":
        return isinstance(v, dict)
    if ty[0] == "map":
        return isinstance(v, dict) or (isinstance(v, list) and all(isinstance(e, tuple) and len(e) == 2 for e in v))
    return isinstance(v, list)   # list / array


def _union_member(v, members):
    """-> (member index, the member's value) of one non-None python value of a UNION(members) column."""
    if isinstance(v, UnionValue):
        for k, (nm, _) in enumerate(members):
            if nm == v.member:
                return k, v.value
        raise MiError(_ffi.MI_EINVAL, "UNION has no member '%s'" % v.member)
    for k, (_, kt) in enumerate(members):
        if _python_value_fits(v, kt):
            return k, v
    raise MiError(_ffi.MI_EINVAL, "no member of the UNION takes the value %r" % (v,))


def _fill_vector(vec, values, ty, keep):
    """python values -> one mi_vector (flat, or nested with child vectors) in DuckDB layout; `ty` from parse_duck_type."""
    n = len(values)
    vec.count = n
    if ty[0] == "leaf":
        data, validity = _vector_from_python(values, ty[1], keep)
        keep.append(data)
        vec.data = data.ctypes.data
    else:
        ok = np.array([v is not None for v in values], dtype=bool)
        validity = None
        if not ok.all():
            validity = np.packbits(np.concatenate([ok, np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()
        if ty[0] in ("list", "map"):
            ent = np.zeros((max(n, 1), 2), np.uint64)
            flat = []
            for i, v in enumerate(values):
                if v is None:
                    continue
                items = list(v.items()) if isinstance(v, dict) else list(v)
                ent[i] = (len(flat), len(items))
                flat.extend(items)
            keep.append(ent)
            vec.data = ent.ctypes.data
            kids = (_ffi.Vector * 1)()
            if ty[0] == "map":
                cty = ("struct", [("key", ty[1]), ("value", ty[2])])
                flat = [None if e is None else {"key": e[0], "value": e[1]} for e in flat]
            else:
                cty = ty[1]
            _fill_vector(kids[0], flat, cty, keep)
        elif ty[0] == "array":
            flat = []
            for v in values:
                flat.extend([None] * ty[2] if v is None else list(v))
            kids = (_ffi.Vector * 1)()
            _fill_vector(kids[0], flat, ty[1], keep)
        elif ty[0] == "union":
            # child 0 the tags (UTINYINT member index, 0 for a NULL row; also this vector's data), then one vector per member
            # with a slot per row, NULL wherever another member is selected
            members = ty[1]
            tags = np.zeros(max(n, 1), np.uint8)
            per_member = [[None] * n for _ in members]
            for i, v in enumerate(values):
                if v is None:
                    continue
                k, inner = _union_member(v, members)
                tags[i] = k
                per_member[k][i] = inner
                if inner is None:   # a NULL of member k is a NULL union row in DuckDB's vector (the tag is kept)
                    ok[i] = False
            if not ok.all():
                validity = np.packbits(np.concatenate([ok, np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()
            keep.append(tags)
            vec.data = tags.ctypes.data
            kids = (_ffi.Vector * (len(members) + 1))()
            kids[0].data, kids[0].count = tags.ctypes.data, n
            for k, (_, kt) in enumerate(members):
                _fill_vector(kids[1 + k], per_member[k], kt, keep)
        else:  # struct
            kids = (_ffi.Vector * len(ty[1]))()
            for k, (nm, kt) in enumerate(ty[1]):
                _fill_vector(kids[k], [None if v is None else v.get(nm) for v in values], kt, keep)
        keep.append(kids)
        vec.children = kids
        vec.n_children = len(kids)
    if validity is not None:
        keep.append(validity)
        vec.validity = validity.ctypes.data


def _chunks_from_table(table, keep, chunk_rows=VECTOR_SIZE):
    """Table -> list of mi_data_chunk (host vectors, <= 2048 rows each) the way DuckDB feeds a sink."""
    chunks = []
    trees = [parse_duck_type(t) for t in table.types]
    for r0 in range(0, max(table.num_rows, 0), chunk_rows):
        r1 = min(table.num_rows, r0 + chunk_rows)
        vecs = (_ffi.Vector * len(table.names))()
        for ci, (ty, col) in enumerate(zip(trees, table.columns)):
            _fill_vector(vecs[ci], col[r0:r1], ty, keep)
        keep.append(vecs)
        ch = _ffi.DataChunk(size=r1 - r0, n_columns=len(table.names), columns=vecs)
        chunks.append(ch)
    return chunks


def encode_schema(names, types):
    """The Arrow IPC Schema message the writer emits for these DuckDB columns (host only)."""
    fields = _c_fields(names, types)
    size = C.c_int64(0)
    _ffi.check(_ffi.lib().mi_encode_schema(fields, len(names), None, 0, C.byref(size)))
    buf = np.zeros(size.value, np.uint8)
    _ffi.check(_ffi.lib().mi_encode_schema(fields, len(names), buf.ctypes.data, buf.size, C.byref(size)))
    return buf.tobytes()


def _c_fields(names, types):
    arr = (_ffi.Field * len(names))()
    for i, (n, t) in enumerate(zip(names, types)):
        arr[i].name = n.encode()
        arr[i].duck_type = t.encode()
    return arr


# ---------------------------------------------------------------------------------------------------- connection
class Connection:
    """The extension's function surface for this path, bound to one GPU."""

    def __init__(self, device=0):
        import weakref
        self.ctx = Context(device)
        self._relations = weakref.WeakSet()   # scans hold streams / buffers of the context: they go first

    def close(self):
        for rel in list(self._relations):
            rel.close()
        self.ctx.close()

    def _relation(self, handle, keep=None):
        rel = Relation(self, handle, keep)
        self._relations.add(rel)
        return rel

    # -- scan ------------------------------------------------------------------------------------------
    @staticmethod
    def _options(union_by_name=False, filename=False, hive_partitioning=False, rank=0, world=1, device_resident=False,
                 accept_dictionaries=False, zero_copy_direct=None, unset_all_valid=False, filter_compact=False,
                 pipeline_depth=0, host_decompress=False, **unknown):
        for k in unknown:
            # MultiFileFunction rejects unknown named parameters (test/sql/read_arrow.test:40-43)
            raise MiError(_ffi.MI_EINVAL, 'Invalid named parameter "%s" for function read_arrow' % k)
        return _ffi.ScanOptions(union_by_name=int(union_by_name), filename=int(filename),
                                hive_partitioning=int(hive_partitioning), rank=rank, world=world,
                                device_resident=int(device_resident), accept_dictionaries=int(accept_dictionaries),
                                # None = the library's default (on for device-resident consumers), False = never
                                zero_copy_direct=0 if zero_copy_direct is None else (1 if zero_copy_direct else -1),
                                unset_all_valid=int(unset_all_valid), filter_compact=int(filter_compact),
                                pipeline_depth=int(pipeline_depth), host_decompress=(-1 if host_decompress == "gpu" else int(bool(host_decompress))))

    def read_arrow(self, paths, contexts=None, **options):
        """FROM read_arrow('file') / read_arrow(['a', 'b']) / read_arrow('dir/*.arrow') (globs expanded here).
        `contexts`: a list of Context objects (one per GPU, or several on one GPU) = the in-library multi-device scan
        (mi_scan_open_files_multi): record batches are dealt over them and chunks come back in record-batch order."""
        import glob as _glob
        if isinstance(paths, (str, bytes, os.PathLike)):
            paths = [paths]
        expanded = []
        for p in paths:
            p = os.fspath(p)
            if any(ch in p for ch in "*?["):
                hits = sorted(_glob.glob(p))
                if not hits:
                    raise MiError(_ffi.MI_EIO, 'No files found that match the pattern "%s"' % p)
                expanded.extend(hits)
            else:
                expanded.append(p)
        opts = self._options(**options)
        arr = (C.c_char_p * len(expanded))(*[os.fsencode(p) for p in expanded])
        h = C.c_void_p()
        if contexts:
            cs = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
            _ffi.check(_ffi.lib().mi_scan_open_files_multi(cs, len(contexts), arr, len(expanded), C.byref(opts), C.byref(h)))
            return self._relation(h, keep=list(contexts))
        _ffi.check(_ffi.lib().mi_scan_open_files(self.ctx._h, arr, len(expanded), C.byref(opts), C.byref(h)))
        return self._relation(h)

    def scan_arrow_ipc(self, buffers, **options):
        """FROM scan_arrow_ipc([{ptr, size}, ...]); buffers may be bytes-like objects or (ptr, size) tuples."""
        keep, arr = [], (_ffi.IpcBuffer * len(buffers))()
        for i, b in enumerate(buffers):
            if isinstance(b, tuple):
                arr[i].ptr, arr[i].size = b
            else:
                a = _as_u8(b)
                keep.append(a)
                arr[i].ptr, arr[i].size = a.ctypes.data, a.size
        opts = self._options(**options)
        h = C.c_void_p()
        _ffi.check(_ffi.lib().mi_scan_open_buffers(self.ctx._h, arr, len(buffers), C.byref(opts), C.byref(h)))
        return self._relation(h, keep=(keep, buffers))

    def from_arrow(self, message_reader, **options):
        """con.from_arrow(pyarrow.ipc.MessageReader): serialises each message back to its IPC bytes and scans the
        buffers, which is what the DuckDB python client does for this extension (test/python/test_arrow_ipc_scan.py:22-31)."""
        bufs = []
        while True:
            try:
                msg = message_reader.read_next_message()
            except StopIteration:
                break
            if msg is None:
                break
            bufs.append(msg.serialize().to_pybytes())
        return self.scan_arrow_ipc([b"".join(bufs)], **options)

    # -- write -----------------------------------------------------------------------------------------
    def to_arrow_ipc(self, table, chunk_size=120 * VECTOR_SIZE):
        """FROM to_arrow_ipc((FROM T)) -> [(ipc BLOB, header BOOL), ...]: first the schema message (header = True),
        then one record-batch message per 120 x 2048 rows (src/include/writer/to_arrow_ipc.hpp:28)."""
        L = _ffi.lib()
        w = C.c_void_p()
        _ffi.check(L.mi_ipc_serializer_create(self.ctx._h, _c_fields(table.names, table.types), len(table.names), C.byref(w)))
        try:
            blob, size = C.c_void_p(), C.c_int64()
            _ffi.check(L.mi_ipc_serialize_schema(w, C.byref(blob), C.byref(size)))
            rows = [(C.string_at(blob.value, size.value), True)]
            keep = []
            chunks = _chunks_from_table(table, keep)
            per_msg = max(1, chunk_size // VECTOR_SIZE)
            for i in range(0, len(chunks), per_msg):
                group = chunks[i: i + per_msg]
                arr = (_ffi.DataChunk * len(group))(*group)
                _ffi.check(L.mi_ipc_serialize_chunks(w, arr, len(group), C.byref(blob), C.byref(size)))
                rows.append((C.string_at(blob.value, size.value), False))
            return rows
        finally:
            L.mi_writer_close(w)

    def copy_to(self, table, path, preserve_insertion_order=True, file_size_bytes=None, arrow_large_buffer_size=False,
                produce_arrow_string_view=False, **options):
        """COPY table TO 'path' (FORMAT ARROWS, row_group_size ..., chunk_size ..., row_group_size_bytes ...,
        row_groups_per_file ..., kv_metadata {...}, compression ...).  With row_groups_per_file / file_size_bytes `path`
        becomes a directory of data_<i>.arrows files, like DuckDB's file rotation.  compression (or codec) = "lz4" /
        "lz4_frame" writes record batches with BodyCompression LZ4_FRAME, compressed on the GPU -- any Arrow reader takes
        them, and a device-resident read_arrow expands them in HBM; "none" / "uncompressed" is the default; "zstd" is
        refused (ZSTD bodies are read, not written).  File sizes that rotation counts are compressed sizes.  Returns the
        list of files written.  produce_arrow_string_view is DuckDB's setting of that name: VARCHAR fields at any depth are
        written as Arrow string views (Utf8View), whatever arrow_large_buffer_size says, which BLOB and LIST keep following."""
        L = _ffi.lib()
        o = _ffi.WriteOptions()
        _ffi.check(L.mi_write_options_init(C.byref(o)))
        o.preserve_insertion_order = int(preserve_insertion_order)
        o.arrow_large_buffer_size = int(arrow_large_buffer_size)   # SET arrow_large_buffer_size=true
        o.produce_arrow_string_view = int(produce_arrow_string_view)   # SET produce_arrow_string_view=true
        for k, v in options.items():
            if k.lower() == "kv_metadata":
                if not isinstance(v, dict):
                    raise MiError(_ffi.MI_EINVAL, "Expected kv_metadata argument to be a STRUCT")
                for kk, vv in v.items():
                    vb = vv if isinstance(vv, bytes) else str(vv).encode()
                    _ffi.check(L.mi_write_options_add_kv(C.byref(o), kk.encode(), vb, len(vb)))
            elif k.lower() == "format":
                continue
            else:
                _ffi.check(L.mi_write_options_set(C.byref(o), k.encode(), None if v is None else str(v).encode()))
        _ffi.check(L.mi_write_options_finalize(C.byref(o)))
        rotate = o.row_groups_per_file > 0 or file_size_bytes is not None
        files, keep = [], []
        if isinstance(table, Relation):   # COPY (FROM read_arrow(...)) TO ...: the scan's chunks go straight into the sink
            names, types, source = table.columns, table.types, table.chunks()
        else:
            names, types, source = table.names, table.types, _chunks_from_table(table, keep)
        fields = _c_fields(names, types)

        def open_writer():
            if rotate:
                os.makedirs(path, exist_ok=True)
                p = os.path.join(path, "data_%d.arrows" % len(files))
            else:
                p = path
            w = C.c_void_p()
            _ffi.check(L.mi_writer_open(self.ctx._h, os.fsencode(p), fields, len(names), C.byref(o), C.byref(w)))
            files.append(p)
            return w

        w = open_writer()
        try:
            if isinstance(table, Relation) and not rotate:   # native pump: scan -> sink without a Python loop
                table._init()
                _ffi.check(L.mi_writer_sink_scan(w, table._h, None))
                source = ()
            for ch in source:
                _ffi.check(L.mi_writer_sink(w, C.byref(ch)))
                if rotate and L.mi_writer_rotate_next_file(w, -1 if file_size_bytes is None else file_size_bytes):
                    _ffi.check(L.mi_writer_finalize(w))
                    L.mi_writer_close(w)
                    w = open_writer()
            _ffi.check(L.mi_writer_finalize(w))
        finally:
            L.mi_writer_close(w)
        return files


# ---------------------------------------------------------------------------------------------------- synthetic input
def synth_lineitem_stream(scale_factor=1.0, seed=42, n_rows=0, rows_per_batch=0, with_validity=True, n_threads=0, out=None,
                          first_row=0):
    """Seeded TPC-H-shaped lineitem as an Arrow IPC stream (include/mi_synth.h).  Returns (uint8 ndarray, info)."""
    L = _ffi.lib()
    o = _ffi.SynthOptions(scale_factor=scale_factor, seed=seed, rows_per_batch=rows_per_batch, n_rows=n_rows,
                          first_row=first_row, with_validity=int(with_validity), n_threads=n_threads)
    rows, nb, size = C.c_int64(), C.c_int64(), C.c_int64()
    _ffi.check(L.mi_synth_lineitem_layout(C.byref(o), C.byref(rows), C.byref(nb), C.byref(size), None, 0))
    offs = (C.c_int64 * (nb.value + 1))()
    _ffi.check(L.mi_synth_lineitem_layout(C.byref(o), C.byref(rows), C.byref(nb), C.byref(size), offs, nb.value + 1))
    if out is None:
        out = np.empty(size.value, dtype=np.uint8)
    assert out.size >= size.value
    _ffi.check(L.mi_synth_lineitem_fill(C.byref(o), out.ctypes.data, out.size))
    return out[: size.value], dict(n_rows=rows.value, n_batches=nb.value, stream_size=size.value,
                                   batch_offsets=list(offs))
