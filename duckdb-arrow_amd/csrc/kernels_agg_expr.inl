// kernels_agg_expr.inl -- the fold of one selected row into a lane's partial for kOpSumExpr, SUM(f_0 * ... * f_{F-1}) with a
// factor add + mul * column or a constant.  Included by kernels_aggregate.hip and kernels_group.hip inside their unnamed
// namespace, behind their row_is_valid / load_integer / load_double, so K9 and K10 fold a row by the same text.  The
// arithmetic of a factor and of the product is agg_merge.hpp (ExprStepInt, ExprStepDouble), shared with the host.
//
// A row contributes when every column a factor names is not NULL in it: the factors are walked left to right and the row
// is left at the first NULL, before that column's bytes are read.  The descriptors are kernel arguments indexed by a
// uniform loop counter (scalar loads); the only addresses formed are column[row], with `row` a row of the window.
// The sum takes the finished product exactly as SUM takes a value: one Add128, or `partial + product` rounded once with the
// first contributor copied -- so SUM_EXPR[a] is SUM(a) and SUM_EXPR[a, b] is SUM_PRODUCT(a, b) bit for bit.
__device__ __forceinline__ void fold_expr_row(const AggExprDev& e, int cls, int64_t row, Partial* p) {
  const int n_factors = e.n_factors;
  if (cls == aggmerge::kClassFloat) {
    double product = 0.0;
#pragma clang loop unroll(disable)
    for (int f = 0; f < n_factors; f++) {
      const AggFactorDev& fc = e.factors[f];
      const bool has_column = fc.col.cls != aggmerge::kClassAny;
      double v = 0.0;
      if (has_column) {
        if (!row_is_valid(fc.col.validity, row)) return;
        v = load_double(fc.col, row);
      }
      product = aggmerge::ExprStepDouble(f == 0, has_column, aggmerge::DoubleOf(fc.mul), aggmerge::DoubleOf(fc.add), v, product);
    }
    p->lo = aggmerge::BitsOf(p->count ? __dadd_rn(aggmerge::DoubleOf(p->lo), product) : product);
    p->count++;
    return;
  }
  uint64_t lo = 0, hi = 0;
#pragma clang loop unroll(disable)
  for (int f = 0; f < n_factors; f++) {
    const AggFactorDev& fc = e.factors[f];
    const bool has_column = fc.col.cls != aggmerge::kClassAny;
    uint64_t vlo = 0, vhi = 0;
    if (has_column) {
      if (!row_is_valid(fc.col.validity, row)) return;
      load_integer(fc.col, row, &vlo, &vhi);
    }
    aggmerge::ExprStepInt(f == 0, has_column, static_cast<int64_t>(fc.mul), static_cast<int64_t>(fc.add), vlo, vhi, &lo, &hi);
  }
  aggmerge::Add128(&p->lo, &p->hi, lo, hi);
  p->count++;
}
