"""MI_K_ENC_UNION and MI_K_ENC_INTERVAL at the task level, for test_union_encode_reference_host.py and
test_gpu_encode_union_tasks.py: DuckDB-layout union vectors (tags, union validity words, member vectors with validity words
of their own, a struct parent's words) and interval_t rows, a plain numpy restatement of what the writer makes of them
(union_reference, interval_reference: they call neither the package nor the oracle; the members' buffers are
encode_tasks.encode_reference under the member's EFFECTIVE mask), one Plan per list of items (run_plan) and the assertions
on its output (check_plan).

The rule (mi_arrow_ipc.h, union_format.hpp: EncodeRow): a union row is valid when its own bit and its struct parent's are
set; a valid row whose tag names no member (tag >= m) is damaged: status bit, type id 0, NULL in every mask.  Type id =
the tag of a valid row, 0 otherwise.  Bit r of mask k = row r is valid AND tag[r] == k AND member k's own bit r; pad bits
ones.  Member k is encoded under mask k whatever its kind.  A union is an item dict: n, m, tags, words / pwords (uint64
words or None), members (encode_tasks columns whose `words` are the member's OWN validity words), name."""
import zlib

import numpy as np

import encode_tasks as et

K_ENC_INTERVAL, K_ENC_UNION = 41, 42
ST_BAD_UNION_TAG = 8192
MAX_MEMBERS = 32
ROWS = [1, 63, 64, 65, 2047, 2048, 2049, 2 * 2048 + 1]
INTERVAL = np.dtype([("months", "<i4"), ("days", "<i4"), ("micros", "<i8")])
I32_MIN, I32_MAX, I64_MIN, I64_MAX = -2**31, 2**31 - 1, -2**63, 2**63 - 1
# micros whose product with 1000 leaves int64: the result is the low 64 bits (ArrowIntervalConverter does not check)
WRAPPING_MICROS = [I64_MAX, I64_MIN, I64_MAX // 1000 + 1, I64_MIN // 1000 - 1, 2**62, -2**62 - 1]


def _bits(words, n):
    if words is None:
        return np.ones(n, bool)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def mask_words(bits):
    """the words of a mask over len(bits) rows, pad bits ones"""
    return np.packbits(np.concatenate([bits, np.ones(-len(bits) % 64, bool)]), bitorder="little").view(np.uint64).copy()


# ------------------------------------------------------------------------------------------------ interval
def interval_column(rows, ok, rng, name, vpos=0):
    """rows: a structured INTERVAL array (interval_t rows as DuckDB holds them)"""
    rows = np.asarray(rows, INTERVAL)
    return et._column(K_ENC_INTERVAL, len(rows), ok, rng, name, src=rows.view(np.uint8).reshape(-1).copy(), width=16, vpos=vpos,
                      values=lambda: et._null_to_none([tuple(int(x) for x in r) for r in rows.tolist()], ok))


def random_intervals(n, rng, extremes=True):
    rows = np.zeros(n, INTERVAL)
    rows["months"] = rng.integers(-5000, 5000, n)
    rows["days"] = rng.integers(-40000, 40000, n)
    rows["micros"] = rng.integers(-2**52, 2**52, n)
    if extremes:
        edge = [(I32_MIN, I32_MAX, 0), (I32_MAX, I32_MIN, -1), (0, 0, I64_MAX // 1000), (-1, -1, I64_MIN // 1000), (0, 0, 0)] + \
               [(1, -1, m) for m in WRAPPING_MICROS]
        at = rng.permutation(n)[: len(edge)]
        for r, e in zip(at, edge):
            rows[r] = e
    return rows


def interval_reference(col):
    """-> the dict encode_tasks.encode_reference returns: bitmap + {int32 months, int32 days, int64 micros * 1000 (two's
    complement, wrapping)} per row, 16 zero bytes under a NULL"""
    out = et.encode_reference(dict(col, kind=et.K_ENC_VALIDITY))
    n = col["n"]
    if n == 0:
        return out
    rows = col["src"][: 16 * n].view(INTERVAL)
    data = np.zeros(n, INTERVAL)
    data["months"], data["days"] = rows["months"], rows["days"]
    nanos = [((int(m) * 1000 + 2**63) % 2**64) - 2**63 for m in rows["micros"].tolist()]      # Python integers: exact, then wrapped
    data["micros"] = np.array(nanos, np.int64)
    data[~et._row_bits(col)] = (0, 0, 0)
    out["data"] = data.view(np.uint8).reshape(-1).copy()
    return out


def reference(col):
    return interval_reference(col) if col["kind"] == K_ENC_INTERVAL else et.encode_reference(col)


# ------------------------------------------------------------------------------------------------ unions
def union_reference(u):
    """-> dict(type_ids int8[n], masks [uint64 words per member], effective [bool[n] per member], members [reference dict per
    member, under its mask], status, valid bool[n] (the rows that are valid and not damaged))"""
    n, m = u["n"], u["m"]
    tags = u["tags"][:n].astype(np.int64)
    valid = _bits(u["words"], n) & _bits(u["pwords"], n)
    bad = valid & (tags >= m)
    valid = valid & ~bad
    type_ids = np.where(valid, tags, 0).astype(np.int8)
    effective, masks, members = [], [], []
    for k, mem in enumerate(u["members"]):
        eff = valid & (tags == k) & _bits(mem["words"], n)
        effective.append(eff)
        masks.append(mask_words(eff))
        members.append(reference(dict(mem, words=masks[-1])))
    return dict(type_ids=type_ids, masks=masks, effective=effective, members=members, status=ST_BAD_UNION_TAG if bad.any() else 0, valid=valid)


def logical_values(u, ref):
    """what the union column holds row by row: None, or (member index, the member's value)"""
    vals = [mem["values"]() for mem in u["members"]]     # built from the effective rows: None elsewhere
    out = []
    for r in range(u["n"]):
        k = int(ref["type_ids"][r])
        out.append((k, vals[k][r]) if ref["effective"][k][r] else None)
    return out


def _union_bits(form, n, rng):
    if form == "none":
        return None
    ok = np.ones(n, bool)
    if form == "random":
        ok = rng.random(n) < 0.8
    elif form == "seams":        # NULL rows on both sides of a word seam and of a tile seam
        for lo, hi in ((62, 66), (126, 129), (2040, 2060), (4090, 4097)):
            ok[lo:hi] = False
    elif form == "all_null":
        ok[:] = False
    else:
        assert form == "all_valid", form
    return ok


def _member(spec, own, eff, rng, name):
    """one member vector of n rows: its content is built for the rows it will own (`eff`: everything else holds what a NULL slot
    holds -- junk lengths, far pointers), its validity words are `own` (None: no words), which say more than `eff`"""
    n = len(eff)
    if spec.startswith("copy") or spec.startswith("dec") or spec == "bool" or spec == "validity":
        col = et.fixed_column(spec, n, eff, rng, name)
    elif spec in ("str32", "str64"):
        col = et.string_column(rng.choice([0, 1, 5, 12, 13, 30], n), eff, rng, name, large=spec == "str64")
    elif spec in ("list32", "list64"):
        col = et.list_column([int(x) for x in rng.integers(0, 5, n)], eff, rng, name, large=spec == "list64")
    else:
        assert spec == "interval", spec
        col = interval_column(random_intervals(n, rng, extremes=False), eff, rng, name)
    col["words"] = None if own is None else et._words(own, rng)
    return col


def make_union(n, specs, rng, name, tags="random", form="random", parent=False, own="random", bad_rows=()):
    """specs: one member spec per member.  tags: "random", ("all", k) every row member k, ("never", k) member k never selected.
    form: the union's validity (_union_bits).  parent: a struct parent's words.  own: the members' validity words -- "random",
    "none", "mixed" (every other member has none).  bad_rows: rows whose tag is set to a value >= m (made valid)."""
    m = len(specs)
    if tags == "random":
        tg = rng.integers(0, m, n)
    elif tags[0] == "all":
        tg = np.full(n, tags[1])
    else:
        tg = rng.integers(0, max(m - 1, 1), n)
        tg = (tg + (tg >= tags[1])) % m if m > 1 else tg
    tg = tg.astype(np.uint8)
    ubits = _union_bits(form, n, rng)
    pbits = (rng.random(n) < 0.9) if parent else None
    for r in bad_rows:
        tg[r] = (m, 255, 128, m + 1)[r % 4]
        if ubits is not None:
            ubits[r] = True
        if pbits is not None:
            pbits[r] = True
    u = dict(kind=K_ENC_UNION, n=n, m=m, tags=tg, words=et._words(ubits, rng), pwords=et._words(pbits, rng), name=name, members=[])
    valid = _bits(u["words"], n) & _bits(u["pwords"], n) & (tg < m)
    for k, spec in enumerate(specs):
        has_own = own == "random" or (own == "mixed" and k % 2 == 0)
        # a member's own words say "valid" on most rows, those of other members included: only the mask keeps them out
        own_bits = (rng.random(n) < 0.85) if has_own else None
        eff = valid & (tg == k) & (own_bits if own_bits is not None else True)
        u["members"].append(_member(spec, own_bits, eff, rng, "%s/m%d_%s" % (name, k, spec)))
    return u


def _rows_cases(rng):
    """every row count with 1, 2 and 32 members, the union's validity absent / random / at the seams"""
    out = []
    for i, n in enumerate(ROWS):
        out.append(make_union(n, ["copy4"], rng, "rows/n%d/m1" % n, form=("random", "none")[i % 2], own=("none", "random")[i % 2]))
        out.append(make_union(n, ["copy8", "str32"], rng, "rows/n%d/m2" % n, form=("seams", "random", "none")[i % 3], own="mixed"))
        out.append(make_union(n, ["copy4", "copy1"] * 16, rng, "rows/n%d/m32" % n, form=("none", "seams")[i % 2], own="mixed", parent=i % 3 == 0))
    return out


def _shape_cases(rng):
    n = 2 * 2048 + 1
    return [
        make_union(n, ["copy4", "str32", "copy2"], rng, "never_selected", tags=("never", 1)),
        make_union(n, ["copy4", "str32", "copy2"], rng, "all_one_member", tags=("all", 2), form="none"),
        make_union(n, ["copy4", "copy8"], rng, "null_rows_at_the_seams", form="seams", own="none"),
        make_union(n, ["copy4", "copy8"], rng, "all_null", form="all_null"),
        make_union(n, ["copy4", "copy8"], rng, "no_member_words", own="none"),
        make_union(2049, ["copy4", "interval"], rng, "struct_parent", parent=True),
        make_union(2049, ["copy4", "interval"], rng, "struct_parent_alone", parent=True, form="none", own="none"),
        make_union(n, ["str32", "str64"], rng, "string_members"),
        make_union(2049, ["list32", "list64", "copy4"], rng, "list_members"),
        make_union(65, ["validity", "bool", "dec4", "copy16"], rng, "other_fixed_members"),
    ]


def _bad_tag_cases(rng):
    """a damaged union beside a clean twin built from the same generator state: the twin's bytes must not change"""
    out = []
    for bad in ((), (0, 63, 64, 2047, 2048, 4096)):
        twin = np.random.default_rng(99)
        out.append(make_union(2 * 2048 + 1, ["copy4", "str32"], twin, "bad_tag/%s" % ("damaged" if bad else "clean"), bad_rows=bad))
    out.append(make_union(2049, ["copy4", "str32"], rng, "bad_tag/under_null_rows_only", form="random"))
    u = out[-1]
    gone = np.nonzero(~_bits(u["words"], u["n"]))[0]
    u["tags"][gone[:20]] = 200          # a tag >= m under a NULL row is not looked at
    return out


CASES = {"rows": _rows_cases, "shapes": _shape_cases, "bad_tags": _bad_tag_cases}
EXPECTED_STATUS = {"bad_tags": ST_BAD_UNION_TAG}
_built = {}


def case_items(name):
    """the unions of a case and their references, built once and shared (nobody writes to them)"""
    if name not in _built:
        items = CASES[name](np.random.default_rng(zlib.crc32(name.encode())))
        _built[name] = (items, [union_reference(u) for u in items])
    return _built[name]


def interval_columns():
    if "interval" not in _built:
        rng = np.random.default_rng(41)
        cols = []
        for i, n in enumerate(ROWS):
            for form in ("none", "random", "all_null"):
                cols.append(interval_column(random_intervals(n, rng, extremes=n >= 63), et.validity_form(form, n, rng), rng,
                                            "interval/n%d/%s" % (n, form), vpos=et.VPOS[i % 4]))
        n = 2 * 2048 + 1
        ok = np.ones(n, bool)
        ok[2000:2100] = False
        ok[4090:] = False
        cols.append(interval_column(random_intervals(n, rng), ok, rng, "interval/null_runs_over_the_tile_seams"))
        _built["interval"] = (cols, [interval_reference(c) for c in cols])
    return _built["interval"]


# ------------------------------------------------------------------------------------------------ running a plan
def run_plan(ctx, torch, unions, urefs, cols=(), refs=(), launches=1):
    """One Plan: per union its member tasks FIRST and its own task behind them (the launch order is the plan's business, not
    the caller's), then the plain columns.  Outputs lie in one arena filled with the sentinel, as in encode_tasks.run_plan.
    -> (arena bytes, [dict(ids=, masks=[...], members=[where dicts])] per union, [where dict] per column, [(status, NULL counts)])"""
    import duckdb_arrow_amd as da
    src, dst = et._Arena(), et._Arena()

    def put_col(col, ref):
        at = {}
        for key, phase in (("bitmap", col["vpos"]), ("data", 0), ("aux", 0)):
            if ref[key] is not None:
                loose = ref["loose"] if key == "data" else 0
                at[key] = (dst.add(len(ref[key]) + loose, phase), len(ref[key]), loose)
        t = dict(src=src.add(len(col["src"]), content=col["src"]),
                 words=src.add(8 * len(col["words"]), content=col["words"].view(np.uint8)) if col["words"] is not None else None,
                 heap=src.add(len(col["heap"]), et.HEAP_PHASE, col["heap"]) if col["heap"] is not None else None)
        return at, t

    def put_words(words):
        return src.add(8 * len(words), content=words.view(np.uint8)) if words is not None else None

    laid = []
    for u, ur in zip(unions, urefs):
        nw = (u["n"] + 63) // 64
        stride = 8 * nw + 8 * (len(laid) % 3)          # the masks lie a multiple of 8 apart, not always back to back
        e = dict(tags=src.add(u["n"], content=u["tags"]), words=put_words(u["words"]), pwords=put_words(u["pwords"]), table=src.add(8 * u["m"]),
                 ids=dst.add(u["n"]), masks=dst.add(stride * (u["m"] - 1) + 8 * nw), stride=stride, members=[put_col(c, r) for c, r in zip(u["members"], ur["members"])])
        laid.append(e)
    plain = [put_col(c, r) for c, r in zip(cols, refs)]
    host = np.zeros(src.size, np.uint8)
    for at, content in src.parts:
        host[at: at + len(content)] = content
    d_src = torch.from_numpy(host).cuda()
    spare = 4096 + sum(len(r["aux"]) for ur in urefs for r in ur["members"] if r["aux"] is not None) + sum(len(r["aux"]) for r in refs if r["aux"] is not None)
    d_dst = torch.full((dst.size + spare,), et.SENTINEL, dtype=torch.uint8, device="cuda")
    s0, d0 = d_src.data_ptr(), d_dst.data_ptr()
    assert s0 % 256 == 0 and d0 % 256 == 0
    # the members' own validity addresses: known only now
    for u, e in zip(unions, laid):
        table = np.array([s0 + t["words"] if t["words"] is not None else 0 for _, t in e["members"]], np.uint64)
        d_src[e["table"]: e["table"] + 8 * u["m"]] = torch.from_numpy(table.view(np.uint8)).cuda()

    def task(col, at, t, validity):
        return da.make_task(col["kind"], col["n"], s0 + t["src"], d0 + at["data"][0] if "data" in at else 0, validity=validity,
                            out_validity=d0 + at["bitmap"][0] if "bitmap" in at else 0, out_aux=d0 + at["aux"][0] if "aux" in at else 0,
                            buf2=s0 + t["heap"] if t["heap"] is not None else 0, ptr_base=col["ptr_base"],
                            buf2_len=len(col["heap"]) if col["heap"] is not None else 0, param=col["width"], parent_div=int(col["large"]))

    made, order = [], []
    for ui, (u, e) in enumerate(zip(unions, laid)):
        for k, (col, (at, t)) in enumerate(zip(u["members"], e["members"])):
            made.append(task(col, at, t, d0 + e["masks"] + k * e["stride"]))      # under mask k, whatever the member's own words say
            order.append(("member", ui, k))
        made.append(da.make_task(K_ENC_UNION, u["n"], s0 + e["tags"], d0 + e["ids"], validity=s0 + e["words"] if e["words"] is not None else 0,
                                 buf2=s0 + e["table"], buf2_len=e["stride"], out_aux=d0 + e["masks"], param=u["m"],
                                 ptr_base=s0 + e["pwords"] if e["pwords"] is not None else 0))
        order.append(("union", ui, -1))
    for col, (at, t) in zip(cols, plain):
        made.append(task(col, at, t, s0 + t["words"] if t["words"] is not None else 0))
        order.append(("plain", len(order), -1))
    plan = da.Plan(ctx, made)
    runs = []
    for _ in range(launches):
        plan.launch(torch.cuda.current_stream().cuda_stream)
        runs.append((plan.status(), plan.null_counts()))
    got = d_dst.cpu().numpy()
    assert (got[dst.size:] == et.SENTINEL).all(), "bytes behind the last buffer were written"
    plan.close()
    return got, laid, [at for at, _ in plain], runs, order


def check_plan(unions, urefs, cols, refs, result):
    """type ids and masks equal the restatement bit for bit, every member's buffers equal its reference under its mask, the
    bytes around every buffer are still the sentinel; per launch the status is the OR of the unions' and the NULL counts are
    the members' (0 for the unions themselves), in the caller's order"""
    got, laid, plain, runs, order = result
    want_status, want_nulls = 0, []
    for u, ur, e in zip(unions, urefs, laid):
        nw = (u["n"] + 63) // 64
        ids = got[e["ids"]: e["ids"] + u["n"]].view(np.int8)
        assert np.array_equal(ids, ur["type_ids"]), (u["name"], "type ids", np.nonzero(ids != ur["type_ids"])[0][:8])
        assert (got[e["ids"] - 64: e["ids"]] == et.SENTINEL).all() and (got[e["ids"] + u["n"]: e["ids"] + u["n"] + 64] == et.SENTINEL).all(), u["name"]
        for k in range(u["m"]):
            at = e["masks"] + k * e["stride"]
            words = got[at: at + 8 * nw].view(np.uint64)
            assert np.array_equal(words, ur["masks"][k]), (u["name"], "mask", k, np.nonzero(words != ur["masks"][k])[0][:8])
            assert (got[at + 8 * nw: at + e["stride"]] == et.SENTINEL).all() or k == u["m"] - 1, (u["name"], "bytes between the masks")
        end = e["masks"] + (u["m"] - 1) * e["stride"] + 8 * nw
        assert (got[e["masks"] - 64: e["masks"]] == et.SENTINEL).all() and (got[end: end + 64] == et.SENTINEL).all(), u["name"]
        for col, ref, (at, _) in zip(u["members"], ur["members"], e["members"]):
            et.check_task(col, ref, got, at)
            want_nulls.append(ref["nulls"])
        want_nulls.append(0)
        want_status |= ur["status"]
    for col, ref, at in zip(cols, refs, plain):
        et.check_task(col, ref, got, at)
        want_nulls.append(ref["nulls"])
        want_status |= ref["status"]
    for status, nulls in runs:
        assert status == want_status, (status, want_status)
        assert nulls == want_nulls
    return want_status
