// knnx_rot_shape.h -- the shape rules of the OPQ rotation in front of IVF-PQ (A f32 [d_out][d_in], y = A x), as plain host arithmetic:
// no HIP in here, so that tools/rot_shape_check.cpp can drive it under the sanitizers (like knnx_pq_plan.h).
#pragma once
#include <cmath>
#include <cstddef>

namespace knnx {

// the widths an index may be given: both multiples of 256, 256 <= d_in <= d_out <= 1024 (d_out == d_in: the square rotation)
inline bool rot_width_ok(int d) { return d == 256 || d == 512 || d == 768 || d == 1024; }
inline bool rot_shape_supported(int d_in, int d_out) { return rot_width_ok(d_in) && rot_width_ok(d_out) && d_in <= d_out; }

// max |A A^T - I_rows| of A f32 [rows][cols] in double precision: the orthonormality of a SQUARE rotation's rows.  A NaN anywhere gives
// a NaN result (never a small number): callers test !(worst <= tol).
inline double rot_row_gram_error(const float* A, int rows, int cols) {
  double worst = 0.0;
  for (int i = 0; i < rows; ++i)
    for (int j = i; j < rows; ++j) {
      const float *a = A + (size_t)i * cols, *b = A + (size_t)j * cols;
      double s = 0.0;
      for (int c = 0; c < cols; ++c) s += (double)a[c] * (double)b[c];
      const double e = fabs(s - (i == j ? 1.0 : 0.0));
      if (e != e) return e;  // a NaN stays: a later finite entry must not paper over it
      if (e > worst) worst = e;
    }
  return worst;
}

// max |A^T A - I_cols| of A f32 [rows][cols] in double precision: the orthonormality of the COLUMNS, what a rectangular rotation
// (rows > cols) must have for <A q, A x> = <q, x>.  G (cols x cols doubles, caller's scratch) is accumulated row by row, so A is read
// once, in order.  NaN rule as above.
inline double rot_col_gram_error(const float* A, int rows, int cols, double* G) {
  for (size_t e = 0; e < (size_t)cols * cols; ++e) G[e] = 0.0;
  for (int r = 0; r < rows; ++r) {
    const float* a = A + (size_t)r * cols;
    for (int i = 0; i < cols; ++i) {
      const double ai = (double)a[i];
      double* g = G + (size_t)i * cols;
      for (int j = i; j < cols; ++j) g[j] += ai * (double)a[j];
    }
  }
  double worst = 0.0;
  for (int i = 0; i < cols; ++i)
    for (int j = i; j < cols; ++j) {
      const double e = fabs(G[(size_t)i * cols + j] - (i == j ? 1.0 : 0.0));
      if (e != e) return e;
      if (e > worst) worst = e;
    }
  return worst;
}

}  // namespace knnx
