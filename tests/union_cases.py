"""Arrow union columns (MI_K_UNION / MI_K_UNION_DENSE, kernels_union.hip) for test_union_reference_host.py,
test_gpu_union_tasks.py and test_gpu_union_scan.py: the reference, the union table of a task, the columns the files share
and the runner of hand-built plans.

The reference is numpy and Python ints only.  test_union_reference_host.py holds it to pyarrow (UnionArray.to_pylist() and
.field(k)); the GPU files hold the kernels to it.  The oracle knows unions as a type id only, so they are pinned the way
run-end encoded columns are.

The rule restated (union_format.hpp, mi_arrow_ipc.h): the tag of a row is the member index of its type id; a row is NULL
when the id is negative or no member (ST_BAD_UNION_TAG), when it is dense and its offset lies outside the member array
(ST_BAD_UNION_OFFSET), when the selected member's value is NULL, or when the struct parent is NULL; a NULL row has tag 0
and is NULL in every member; a valid row holds its member's value (sparse: row r, dense: row offsets[r]) in that member
alone."""
import numpy as np

WIN = 2048
SENTINEL = 0xA5
POISON = 0xEE
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
ST_BAD_UNION_TAG, ST_BAD_UNION_OFFSET = 8192, 16384     # restated: test_union_reference_host.py holds them to _ffi
MAX_MEMBERS = 32
TABLE_WORDS, MEMBER_WORDS = 16, 4


# ------------------------------------------------------------------------------------------------ reference
def words_of(ok):
    """bool per row -> validity words, pad bits of the last word ones"""
    n = len(ok)
    return np.packbits(np.concatenate([np.asarray(ok, bool), np.ones((-n) % 64, bool)]), bitorder="little").view(np.uint64).copy()


def bits_of(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def id_map_of(type_codes):
    """the 128-entry id -> member table of Union.typeIds (None: id = index is the caller's to pass as range(m))"""
    codes = [int(c) for c in type_codes]
    assert 1 <= len(codes) <= MAX_MEMBERS and len(set(codes)) == len(codes) and all(0 <= c < 128 for c in codes)
    table = np.full(128, -1, np.int8)
    for k, c in enumerate(codes):
        table[c] = k
    return table


def union_reference(mode, type_ids, offsets, id_map, members, parent=None):
    """mode "sparse" / "dense"; type_ids: int8 per row; offsets: int32 per row (dense) or None; id_map: id_map_of(...);
    members: per member (length in rows, bool per member row or None = every value valid, null_type); parent: bool per row
    (the struct parent's validity) or None.
    -> dict(tags uint8[n], valid bool[n], member_ok [m] of bool[n], member_src [m] of int64[n]: the member row a valid row
       takes its value from, -1 where the member is NULL, status)"""
    ids = np.asarray(type_ids).astype(np.int64)
    n, m = len(ids), len(members)
    dense = mode == "dense"
    offs = np.asarray(offsets).astype(np.int64) if dense else np.arange(n, dtype=np.int64)
    tags, valid = np.zeros(n, np.uint8), np.zeros(n, bool)
    src = [np.full(n, -1, np.int64) for _ in range(m)]
    status = 0
    for r in range(n):
        mem = int(id_map[ids[r]]) if 0 <= ids[r] < 128 else -1
        if mem < 0 or mem >= m:
            status |= ST_BAD_UNION_TAG
            continue
        length, ok, null_type = members[mem]
        if dense and not 0 <= offs[r] < length:
            status |= ST_BAD_UNION_OFFSET
            continue
        if null_type or (ok is not None and not ok[offs[r]]) or (parent is not None and not parent[r]):
            continue
        tags[r], valid[r] = mem, True
        src[mem][r] = offs[r]
    return dict(tags=tags, valid=valid, member_ok=[s >= 0 for s in src], member_src=src, status=status)


def member_rows(values, src):
    """the member vector the reference expects: values[src] where src >= 0, zero rows elsewhere; values = (rows, w) bytes"""
    values = np.ascontiguousarray(values)
    out = np.zeros((len(src), values.shape[1]), np.uint8)
    out[src >= 0] = values[src[src >= 0]]
    return out


# ------------------------------------------------------------------------------------------------ the union table of a task
def union_table(id_map, member_records):
    """buf2 of a K_UNION task: 16 words of id -> member table, then {bitmap address, length, null_count, flags} per member"""
    words = [np.asarray(id_map, np.int8).view(np.uint64)]
    for rec in member_records:
        words.append(np.array([int(x) & (2**64 - 1) for x in rec], np.uint64))
    return np.concatenate(words)


# ------------------------------------------------------------------------------------------------ columns for the task tests
def make_member(length, w, rng, *, nulls=False, null_type=False, null_count=-1):
    """One member array of `length` rows of w bytes, POISON rows behind it; a bitmap with random bits (some NULL) or none"""
    v = rng.integers(0, 256, (length + 64, w), dtype=np.uint8)
    v[v[:, 0] == POISON, 0] = POISON ^ 0xFF
    v[length:] = POISON
    bits = None
    if nulls:
        bits = rng.integers(0, 256, (length + 64 + 63) // 64 * 8 + 8, dtype=np.uint8)
    return dict(length=length, w=w, values=v, bits=bits, null_type=null_type, null_count=null_count)


def member_ok(mem, bit_offset=0):
    """bool per member row as the kernel sees it (null_count == 0: the bitmap is ignored), None = all valid"""
    if mem["bits"] is None or mem["null_count"] == 0:
        return None
    return np.unpackbits(mem["bits"], bitorder="little")[bit_offset: bit_offset + mem["length"]].astype(bool)


def make_union_case(mode, type_codes, members, ids, offsets, *, row_offset=0, parent=None, name=""):
    """ids / offsets: the rows of the task (row_offset rows of padding are put in front of them here)"""
    n = len(ids)
    pad_ids = np.full(row_offset, -7, np.int8)
    dev_ids = np.concatenate([pad_ids, np.asarray(ids, np.int8), np.full(64, -9, np.int8)])
    dev_offs = None
    if mode == "dense":
        dev_offs = np.concatenate([np.full(row_offset, -1, np.int32), np.asarray(offsets, np.int32), np.full(64, 2**31 - 1, np.int32)])
    return dict(mode=mode, codes=list(type_codes), members=members, ids=np.asarray(ids, np.int8), offsets=None if offsets is None else np.asarray(offsets, np.int32),
                dev_ids=dev_ids, dev_offs=dev_offs, row_offset=row_offset, nrows=n, parent=parent,
                name="%s/%s/m%d/n%d/o%d" % (name, mode, len(members), n, row_offset))


def case_reference(case):
    """sparse member bitmaps are read at bit row_offset + r: the reference sees them from there"""
    sparse = case["mode"] == "sparse"
    recs = [(m["length"], member_ok(m, case["row_offset"] if sparse else 0), m["null_type"]) for m in case["members"]]
    parent = None if case["parent"] is None else bits_of(case["parent"], case["nrows"])
    return union_reference(case["mode"], case["ids"], case["offsets"], id_map_of(case["codes"]), recs, parent)


def parent_words(rows, rng):
    """random validity words of a struct parent of `rows` rows, pad bits included, and one word more"""
    return rng.integers(0, 256, ((rows + 63) // 64 + 1) * 8, dtype=np.uint8).view(np.uint64)


def random_rows(mode, codes, members, n, rng, absent=()):
    """n rows: random members (none of `absent`), dense offsets random inside the member (shared and skipped rows both happen)"""
    m = len(codes)
    pick = [k for k in range(m) if k not in absent and (mode == "sparse" or members[k]["length"] > 0)]
    tag = rng.choice(pick, n)
    ids = np.asarray(codes, np.int8)[tag]
    offs = None
    if mode == "dense":
        offs = np.array([rng.integers(0, members[k]["length"]) for k in tag], np.int32)
    return ids, offs


# ------------------------------------------------------------------------------------------------ running a plan
class Uploads:
    """numpy array -> device bytes, once per array (padded to 8 bytes and never empty, as IPC buffers are)"""

    def __init__(self, torch):
        self.torch, self.dev, self.keep = torch, {}, []

    def __call__(self, a):
        if id(a) not in self.dev:
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            self.dev[id(a)] = self.torch.from_numpy(np.concatenate([b, np.zeros(16 - len(b) % 8, np.uint8)])).cuda()
            self.keep.append(a)
        return self.dev[id(a)]


def run_union_plan(ctx, torch, cases, out_validity=True, dense_member_task="after"):
    """One plan: per case a K_UNION task and, for dense cases, per member a K_COPY task that decodes the member array into a
    scratch vector preset to POISON (standing before or after the union tasks in the task array) and a K_UNION_DENSE task.
    Layout per case, all in one arena preset to SENTINEL (words: ones): tags + 64 sentinel bytes; a guard word, the union's
    words, a guard word; per member a mask of ceil(n / 64) words and a guard word (the mask stride); per dense member the
    vector + 64 sentinel bytes and words + guard.
    -> ([dict(tags, words, masks [m], member_data [m], member_words [m]) per case], status)"""
    import duckdb_arrow_amd as da
    from duckdb_arrow_amd import _ffi
    up = Uploads(torch)
    plans, at = [], 0

    def take(nbytes):
        nonlocal at
        a = at
        at += (nbytes + 15) // 16 * 16
        return a
    for c in cases:
        n, m, W = c["nrows"], len(c["members"]), (c["nrows"] + 63) // 64
        p = dict(tags=take(n + 64), words=take(8 * (W + 2)), masks=take(8 * (W + 1) * m + 8), dense=[])
        for mem in c["members"]:
            if c["mode"] == "dense":
                p["dense"].append((take(n * mem["w"] + 64), take(8 * (W + 1))))
        plans.append(p)
    arena = torch.full((at + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    base = arena.data_ptr()
    assert base % 16 == 0
    for c, p in zip(cases, plans):       # validity words and masks start as ones
        n, m, W = c["nrows"], len(c["members"]), (c["nrows"] + 63) // 64
        arena[p["words"]: p["words"] + 8 * (W + 2)] = 0xFF
        arena[p["masks"]: p["masks"] + 8 * (W + 1) * m + 8] = 0xFF
        for _, wa in p["dense"]:
            arena[wa: wa + 8 * (W + 1)] = 0xFF
    union_tasks, copy_tasks, keep = [], [], []
    for c, p in zip(cases, plans):
        n, m, W = c["nrows"], len(c["members"]), (c["nrows"] + 63) // 64
        dense = c["mode"] == "dense"
        recs = []
        for mem in c["members"]:
            recs.append((up(mem["bits"]).data_ptr() if mem["bits"] is not None else 0, mem["length"], mem["null_count"] if mem["bits"] is not None else 0,
                         1 if mem["null_type"] else 0))
        table = union_table(id_map_of(c["codes"]), recs)
        stride = 8 * (W + 1)
        mask0 = p["masks"] + 8                       # a guard word in front of mask 0, one behind every mask
        has_parent = c["parent"] is not None
        udepth = 1 if has_parent else 0
        union_tasks.append(da.make_task(_ffi.K_UNION, n, up(c["dev_ids"]).data_ptr(), base + p["tags"], buf2=up(table).data_ptr(),
                                        ptr_base=up(c["dev_offs"]).data_ptr() if dense else 0,
                                        out_validity=base + p["words"] + 8 if out_validity else 0,
                                        out_aux=up(c["parent"]).data_ptr() if has_parent else 0, parent_div=1 if has_parent else 0,
                                        depth=udepth, row_offset=c["row_offset"], param=m, param2=mask0 - p["tags"],
                                        buf2_len=stride))
        if dense:
            for k, (mem, (da_, wa)) in enumerate(zip(c["members"], p["dense"])):
                w = mem["w"]
                scratch = torch.full((mem["values"].size + 16,), POISON, dtype=torch.uint8, device="cuda")
                sw = torch.full((8 * ((mem["length"] + 64 + 63) // 64 + 1),), 0xFF, dtype=torch.uint8, device="cuda")
                keep += [scratch, sw]
                nulls = mem["bits"] is not None and mem["null_count"] != 0
                if mem["length"] > 0:
                    copy_tasks.append(da.make_task(_ffi.K_COPY, mem["length"], up(mem["values"]).data_ptr(), scratch.data_ptr(),
                                                   validity=up(mem["bits"]).data_ptr() if nulls else 0, out_validity=sw.data_ptr(), param=w,
                                                   null_count=mem["null_count"] if nulls else 0, depth=udepth + 1))
                union_tasks.append(da.make_task(_ffi.K_UNION_DENSE, n, up(c["dev_offs"]).data_ptr(), base + da_, buf2=scratch.data_ptr(),
                                                buf2_len=mem["length"], validity=sw.data_ptr() if nulls else 0,
                                                null_count=mem["null_count"] if nulls else 0, out_validity=base + wa,
                                                out_aux=base + mask0 + k * stride, parent_div=1, depth=udepth + 1,
                                                row_offset=c["row_offset"], param=w))
    tasks = copy_tasks + union_tasks if dense_member_task == "before" else union_tasks + copy_tasks
    plan = da.Plan(ctx, tasks)
    plan.launch(torch.cuda.current_stream().cuda_stream)
    status = plan.status()
    h = arena.cpu().numpy()
    plan.close()
    out = []
    for c, p in zip(cases, plans):
        n, m, W = c["nrows"], len(c["members"]), (c["nrows"] + 63) // 64
        g = dict(tags=h[p["tags"]: p["tags"] + n + 64], words=h[p["words"]: p["words"] + 8 * (W + 2)].view(np.uint64),
                 masks=h[p["masks"]: p["masks"] + 8 * (W + 1) * m + 8].view(np.uint64), member_data=[], member_words=[])
        for mem, (da_, wa) in zip(c["members"], p["dense"]):
            g["member_data"].append(h[da_: da_ + n * mem["w"] + 64])
            g["member_words"].append(h[wa: wa + 8 * (W + 1)].view(np.uint64))
        out.append(g)
    return out, status


def check_union_case(case, got, want=None, out_validity=True, damaged_rows=()):
    """Tags, sentinel tail, the union's words between their guard words, every mask and its guard word, and for a dense case
    every member vector (values where the mask selects, zero elsewhere), its sentinel tail, words and guard word."""
    want = want if want is not None else case_reference(case)
    n, m, W, where = case["nrows"], len(case["members"]), (case["nrows"] + 63) // 64, case["name"]
    if not np.array_equal(got["tags"][:n], want["tags"]):
        bad = np.nonzero(got["tags"][:n] != want["tags"])[0]
        raise AssertionError("%s: %d of %d tags differ, first at row %d: got %d want %d" % (where, len(bad), n, bad[0], got["tags"][bad[0]], want["tags"][bad[0]]))
    assert (got["tags"][n:] == SENTINEL).all(), (where, "bytes behind the last tag were written")
    words = got["words"]
    assert words[0] == ONES and words[-1] == ONES, (where, "a guard word beside the union's validity lost bits")
    if out_validity:
        ww = words_of(want["valid"])
        if not np.array_equal(words[1:-1], ww):
            bad = np.nonzero(words[1:-1] != ww)[0]
            raise AssertionError("%s: %d validity words differ, first %d of %d: got %016x want %016x" % (where, len(bad), bad[0], W, int(words[1 + bad[0]]), int(ww[bad[0]])))
    else:
        assert (words == ONES).all(), (where, "validity words were written without out_validity")
    masks = got["masks"]
    assert masks[0] == ONES, (where, "the guard word in front of mask 0 lost bits")
    for k in range(m):
        mk = masks[1 + k * (W + 1): 1 + (k + 1) * (W + 1)]
        wk = words_of(want["member_ok"][k])
        if not np.array_equal(mk[:-1], wk):
            bad = np.nonzero(mk[:-1] != wk)[0]
            raise AssertionError("%s: mask %d: %d words differ, first %d: got %016x want %016x" % (where, k, len(bad), bad[0], int(mk[bad[0]]), int(wk[bad[0]])))
        assert mk[-1] == ONES, (where, "the guard word behind mask %d lost bits" % k)
    for r in damaged_rows:
        assert want["tags"][r] == 0 and not want["valid"][r] and not any(ok[r] for ok in want["member_ok"]), (where, r)
    if case["mode"] != "dense":
        return
    for k, mem in enumerate(case["members"]):
        w = mem["w"]
        data, mw = got["member_data"][k], got["member_words"][k]
        src = want["member_src"][k]
        expect = member_rows(mem["values"][: max(mem["length"], 1)], np.where(src >= 0, src, -1) if mem["length"] else np.full(n, -1))
        if not np.array_equal(data[: n * w].reshape(n, w), expect):
            bad = np.nonzero(np.any(data[: n * w].reshape(n, w) != expect, axis=1))[0]
            raise AssertionError("%s: member %d: %d of %d rows differ, first %d: got %s want %s" % (
                where, k, len(bad), n, bad[0], data[bad[0] * w: bad[0] * w + w].tolist(), expect[bad[0]].tolist()))
        assert (data[n * w:] == SENTINEL).all(), (where, "bytes behind member %d's last row were written" % k)
        wk = words_of(want["member_ok"][k])
        assert np.array_equal(mw[:-1], wk), (where, "member %d validity" % k)
        assert mw[-1] == ONES, (where, "the guard word behind member %d's words lost bits" % k)
