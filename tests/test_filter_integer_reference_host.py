"""The evaluator behind tests/test_gpu_filter_integers.py against the project's oracle (oracle_transcode.c leaf_true /
orc_filter_cnf) on the fixture's stored integers and validity words: what makes the expected rows trustworthy before a kernel
is involved.  No GPU and no library: the oracle is plain C."""
import numpy as np
import pytest

import filter_integer_cases as fc
from oracle import pyoracle as po

I64_MIN, I64_MAX, P63 = fc.I64_MIN, fc.I64_MAX, fc.P63


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


def _oracle_rows(fx, clauses):
    names = sorted({leaf[0] for clause in clauses for leaf in clause})
    return po.filter_cnf(clauses, fx.oracle_columns(names), fc.N_ROWS).tolist()


def _check(fx, expr):
    clauses = fc.cnf_of(expr)
    assert clauses is not None, expr
    want = _oracle_rows(fx, clauses)
    got = np.flatnonzero(fc.evaluate(fx, expr)).tolist()
    assert got == want, "%r: the evaluator keeps %d rows, the oracle %d" % (expr, len(got), len(want))
    return len(got)


def test_the_fixture_holds_the_rows_the_cases_are_about(fx):
    """the batches, the edge values at the seams, NULLs in every nullable column and none in the twins"""
    assert fc.BATCH_ROWS == (8197, 2047, 0, 1, 4096, 2049, 63) and len(fx.batch) == fc.N_ROWS
    for name in fx.filter_columns():
        col, pool = fx.columns[name], fx.pool(name)
        stored, ok = fx.stored[name], fx.valid[name]
        for i, r in enumerate(fc.EDGE_ROWS):
            assert int(stored[r]) == pool[i] and ok[r], (name, r)
        for b, rows in enumerate(fc.BATCH_ROWS):
            if rows:
                last = fx.batch_offsets[b] + rows - 1
                assert int(stored[last]) == pool[6 - b % 7] and ok[last], (name, b)
        nulls = int((~ok).sum())
        assert (0.10 * fc.N_ROWS < nulls < 0.20 * fc.N_ROWS) if col.nullable else nulls == 0, name
        # = and IN keep many rows: every pool value occurs often
        assert min(int(((stored == stored.dtype.type(v)) & ok).sum()) for v in set(pool)) > 300, name
    u64 = [int(v) for v in fx.stored["u64"][list(fc.EDGE_ROWS)]]
    assert u64 == [0, 1, P63 - 1, P63, P63 + 1, 2 ** 64 - 2, 2 ** 64 - 1]
    # the scaled kinds: the stored integers are the decode kernels' (C division truncates towards zero)
    assert fx.pool("date64") == fc._edges(-2 ** 31, 2 ** 31 - 1) and fx.pool("time64_ns")[:5] == [-(P63 // 1000), -(P63 // 1000), -1, 0, 1]
    assert fx.pool("ts_s_tz")[0] == -(I64_MAX // 1000000) * 1000000 and fx.pool("time32_s")[6] == (2 ** 31 - 1) * 1000000


def test_cnf_size_counts_what_distribution_produces():
    leaf = ("a", "=", 1)
    assert fc.cnf_size(leaf) == (1, 1)
    assert fc.cnf_size(("and", leaf, leaf, leaf)) == (3, 3)
    assert fc.cnf_size(("or", leaf, leaf)) == (1, 2)
    # (A1 & A2) | (B1 & B2) = (A1|B1) & (A1|B2) & (A2|B1) & (A2|B2)
    assert fc.cnf_size(("or", ("and", leaf, leaf), ("and", leaf, leaf))) == (4, 8)
    # 3 x 1 x 2 clauses; each takes one leaf of the first child, the second, and a clause of one or of two leaves of the third
    assert fc.cnf_size(("or", ("and", leaf, leaf, leaf), leaf, ("and", leaf, ("or", leaf, leaf)))) == (6, 3 * (1 + 1 + 1) + 3 * (1 + 1 + 2))
    assert [fc.cnf_size(t)[1] > 96 for t in fc.refused_trees()] == [True] * 3
    assert fc.needs_distribution(("and", leaf, ("or", leaf, ("and", leaf, leaf)))) and not fc.needs_distribution(("and", ("or", leaf, leaf), leaf))


@pytest.mark.parametrize("name", fc.filter_column_names())
def test_single_leaves_equal_the_oracle(fx, name):
    """every op at every edge constant, IS NULL, IS NOT NULL"""
    kept = [_check(fx, leaf) for leaf in fc.single_leaf_cases(fx, name)]
    assert 0 in kept and max(kept) > fc.N_ROWS // 2   # the cases reach both ends


def test_in_lists_equal_the_oracle(fx):
    for leaf in fc.in_list_cases(fx):
        _check(fx, leaf)


def test_trees_in_conjunctive_form_equal_the_oracle(fx):
    checked = 0
    for expr in fc.merge_cases(fx) + fc.generated_trees(fx) + fc.delivery_cases(fx):
        if fc.cnf_of(expr) is not None:
            _check(fx, expr)
            checked += 1
    assert checked > 100


def test_uint64_against_constants_it_cannot_hold(fx):
    """the oracle is the arbiter: `> INT64_MAX` keeps the values >= 2^63, a negative constant is below every value and no
    member of the column, so IN never matches it"""
    for name in ("u64", "u64_nn"):
        v, ok = fx.stored[name], fx.valid[name]
        big = np.flatnonzero((v >= np.uint64(P63)) & ok).tolist()
        assert len(big) > 1000
        assert _oracle_rows(fx, [[(name, ">", I64_MAX)]]) == big == np.flatnonzero(fc.evaluate(fx, (name, ">", I64_MAX))).tolist()
        five = np.flatnonzero((v == np.uint64(5)) & ok).tolist()
        assert len(five) > 100 and int(((v == np.uint64(2 ** 64 - 1)) & ok).sum()) > 300 and int(((v == np.uint64(2 ** 64 - 2)) & ok).sum()) > 300
        assert _oracle_rows(fx, [[(name, "in", [-1, 5])]]) == five == np.flatnonzero(fc.evaluate(fx, (name, "in", [-1, 5]))).tolist()
        assert _oracle_rows(fx, [[(name, "in", [-1, -2])]]) == [] == np.flatnonzero(fc.evaluate(fx, (name, "in", [-1, -2]))).tolist()
        for c in (-1, -5, I64_MIN):
            assert _oracle_rows(fx, [[(name, ">", c)]]) == np.flatnonzero(ok).tolist() and _oracle_rows(fx, [[(name, "<=", c)]]) == []
    # on a signed column nothing is above INT64_MAX
    assert _oracle_rows(fx, [[("i64", ">", I64_MAX)]]) == [] and not fc.evaluate(fx, ("i64", ">", I64_MAX)).any()
