// kernels_agg_fold.inl -- the one place where K9 (kernels_aggregate.hip) and K10 (kernels_group.hip) read a row and fold it:
// how a validity bit, an integer of any class, a float and a Partial are loaded, the fold of one selected row into a lane's
// partial (fold_row; fold_expr_row for kOpSumExpr) and the shuffle of a partial for the reduction over a wave.  K11
// (kernels_hash_group.hip) reads a row through the same text: it folds the row into an empty partial and sends that to its
// table by atomics.  Included by these files inside their unnamed namespace, behind device_common.hpp, agg_merge.hpp and `using aggmerge::Partial`.  The
// arithmetic of a merge, of a factor and of the product is agg_merge.hpp, shared with the host.

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
typedef u64x2 u64x2_a8 __attribute__((aligned(8)));   // a zero-copy alias of the Arrow body is 8-byte aligned only (leaf_wide)

__device__ __forceinline__ bool row_is_valid(const uint64_t* validity, int64_t row) {
  return validity == nullptr || ((GC<uint64_t>(validity)[row >> 6] >> (row & 63)) & 1ull) != 0;
}

// one integer of any class as a 128-bit two's-complement integer
__device__ __forceinline__ void load_integer(const AggColumnDev& c, int64_t row, uint64_t* lo, uint64_t* hi) {
  if (c.cls == aggmerge::kClassWide) {
    const u64x2 v = GC<u64x2_a8>(c.data)[row];
    *lo = v.x;
    *hi = v.y;
    return;
  }
  uint64_t u;
  int64_t s;
  switch (c.width) {
    case 1: u = GC<uint8_t>(c.data)[row]; s = static_cast<int8_t>(u); break;
    case 2: u = GC<uint16_t>(c.data)[row]; s = static_cast<int16_t>(u); break;
    case 4: u = GC<uint32_t>(c.data)[row]; s = static_cast<int32_t>(u); break;
    default: u = GC<uint64_t>(c.data)[row]; s = static_cast<int64_t>(u); break;
  }
  if (c.cls == aggmerge::kClassUnsigned) {
    *lo = u;
    *hi = 0;
  } else {
    *lo = static_cast<uint64_t>(s);
    *hi = s < 0 ? ~0ull : 0ull;
  }
}

__device__ __forceinline__ double load_double(const AggColumnDev& c, int64_t row) {
  return c.width == 4 ? static_cast<double>(GC<float>(c.data)[row]) : GC<double>(c.data)[row];
}

__device__ __forceinline__ Partial load_partial(gptr<const Partial> p) {
  const u64x2 x = ((gptr<const u64x2_a8>)p)[0], y = ((gptr<const u64x2_a8>)p)[1];
  return Partial{x.x, x.y, y.x, y.y};
}
__device__ __forceinline__ void store_partial(gptr<Partial> p, const Partial& v) {
  const u64x2 x = {v.lo, v.hi}, y = {v.count, v.flags};
  ((gptr<u64x2_a8>)p)[0] = x;
  ((gptr<u64x2_a8>)p)[1] = y;
}

// one selected row folded into a lane's partial, for every operation but kOpSumExpr: 128-bit wrapping sums, doubles without fma
__device__ __forceinline__ void fold_row(const AggDescDev& d, int op, int cls, int64_t row, Partial* p) {
  if (op == aggmerge::kOpCountStar) {
    p->count++;
    return;
  }
  bool valid = row_is_valid(d.a.validity, row);
  if (op == aggmerge::kOpSumProduct) valid = valid && row_is_valid(d.b.validity, row);
  if (!valid) return;
  const bool is_sum = op == aggmerge::kOpSum || op == aggmerge::kOpSumProduct;
  if (op == aggmerge::kOpCount) {
    p->count++;
  } else if (cls == aggmerge::kClassFloat) {
    double v = load_double(d.a, row);
    if (op == aggmerge::kOpSumProduct) v = __dmul_rn(v, load_double(d.b, row));   // rounded product, then the sum: no fma
    if (is_sum) {
      p->lo = aggmerge::BitsOf(p->count ? __dadd_rn(aggmerge::DoubleOf(p->lo), v) : v);
      p->count++;
    } else {
      aggmerge::Fold<false>(op, cls, p, aggmerge::CanonicalBits(v), 0ull);
    }
  } else {
    uint64_t lo, hi;
    load_integer(d.a, row, &lo, &hi);
    if (op == aggmerge::kOpSumProduct) {
      uint64_t blo, bhi;
      load_integer(d.b, row, &blo, &bhi);
      const unsigned __int128 x = (static_cast<unsigned __int128>(hi) << 64) | lo, y = (static_cast<unsigned __int128>(bhi) << 64) | blo;
      const unsigned __int128 prod = x * y;   // modulo 2^128: the two's-complement product
      lo = static_cast<uint64_t>(prod);
      hi = static_cast<uint64_t>(prod >> 64);
    }
    if (is_sum) {
      aggmerge::Add128(&p->lo, &p->hi, lo, hi);
      p->count++;
    } else {
      aggmerge::Fold<false>(op, cls, p, lo, hi);
    }
  }
}

// The same for kOpSumExpr, SUM(f_0 * ... * f_{F-1}) with a factor add + mul * column or a constant.
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

// One step of the wave reduction: the partial of lane l + dist.  The caller merges it while that lane exists,
//   for (dist = 32; dist >= 1; dist >>= 1) { o = shfl_down_partial(p, dist); if (lane + dist < 64) Merge(op, cls, &p, o); }
// (a lane whose partner would lie past the wave keeps its partial as it is: __shfl_down hands such a lane its own value
// back, which must not be folded in a second time).  The loop and the Merge stay in the kernels: with aggmerge::Merge called
// from an include function the compiler inlines it there first, and group_windows then costs two more VGPRs.
__device__ __forceinline__ Partial shfl_down_partial(const Partial& p, int dist) {
  Partial o;
  o.lo = __shfl_down(p.lo, dist, 64);
  o.hi = __shfl_down(p.hi, dist, 64);
  o.count = __shfl_down(p.count, dist, 64);
  o.flags = __shfl_down(p.flags, dist, 64);
  return o;
}
