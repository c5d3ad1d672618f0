// rot_shape_check.cpp -- drives csrc/knnx_rot_shape.h (the width rule of an IVF-PQ index with d_out >= d_in and the double-precision
// orthonormality checks of its rotation) on the CPU.  Its own main, only that header: built with -fsanitize=address,undefined by
// tests/test_opq_rect_cpu.py and run as a child process.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I clip-retrieval_amd/csrc tools/rot_shape_check.cpp -o rot_shape_check
// Prints one line per case and "rot shape ok" at the end; a failed check prints FAILED and the exit status is 1.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "knnx_rot_shape.h"

using namespace knnx;

static int failures = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                              \
    }                                                          \
  } while (0)

// a seeded generator (no <random>: the same numbers with every library)
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(rng_state >> 11) / 9007199254740992.0 - 0.5;
}

// A f32 [rows][cols] with orthonormal columns: modified Gram-Schmidt, twice, in double
static std::vector<float> orthonormal_columns(int rows, int cols) {
  std::vector<double> a((size_t)rows * cols);
  for (auto& v : a) v = uniform();
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < cols; ++c) {
      for (int p = 0; p < c; ++p) {
        double dot = 0;
        for (int r = 0; r < rows; ++r) dot += a[(size_t)r * cols + c] * a[(size_t)r * cols + p];
        for (int r = 0; r < rows; ++r) a[(size_t)r * cols + c] -= dot * a[(size_t)r * cols + p];
      }
      double nn = 0;
      for (int r = 0; r < rows; ++r) nn += a[(size_t)r * cols + c] * a[(size_t)r * cols + c];
      nn = sqrt(nn);
      for (int r = 0; r < rows; ++r) a[(size_t)r * cols + c] /= nn;
    }
  return std::vector<float>(a.begin(), a.end());
}

int main() {
  const int widths[] = {0, 64, 128, 255, 256, 257, 384, 512, 640, 768, 1000, 1024, 1280, 2048, -256};
  int supported = 0, refused = 0;
  for (int di : widths)
    for (int dout : widths) {
      const bool want = di >= 256 && di <= 1024 && dout <= 1024 && di % 256 == 0 && dout % 256 == 0 && di <= dout;
      const bool got = rot_shape_supported(di, dout);
      if (want || (di > 0 && dout > 0 && di % 256 == 0 && dout % 256 == 0))
        printf("shape d_in %5d d_out %5d -> %s\n", di, dout, got ? "supported" : "refused");
      CHECK(got == want);
      supported += got;
      refused += !got;
    }
  printf("shapes: %d supported, %d refused\n", supported, refused);
  CHECK(supported == 10);  // four square widths and the six pairs d_in < d_out

  // every rectangular pair: orthonormal columns pass the column check (and fail a row check: A A^T is a projector, not I)
  const int pairs[][2] = {{256, 512}, {256, 768}, {256, 1024}, {512, 768}, {512, 1024}, {768, 1024}};
  for (auto& pr : pairs) {
    const int di = pr[0], dout = pr[1];
    std::vector<float> A = orthonormal_columns(dout, di);
    std::vector<double> G((size_t)di * di);
    const double e = rot_col_gram_error(A.data(), dout, di, G.data());
    printf("gram rect %4d x %4d orthonormal columns: max |A^T A - I| = %.3g\n", dout, di, e);
    CHECK(e <= 1e-5);
    if (di == 256) {
      const double er = rot_row_gram_error(A.data(), dout, di);
      printf("gram rect %4d x %4d the same by rows:     max |A A^T - I| = %.3g\n", dout, di, er);
      CHECK(er > 0.1);
    }
  }
  {  // one column scaled by 1.01: off by 0.0201 on its diagonal entry
    const int di = 256, dout = 512;
    std::vector<float> A = orthonormal_columns(dout, di);
    for (int r = 0; r < dout; ++r) A[(size_t)r * di + 7] *= 1.01f;
    std::vector<double> G((size_t)di * di);
    const double e = rot_col_gram_error(A.data(), dout, di, G.data());
    printf("gram rect scaled column: %.5f\n", e);
    CHECK(e > 1e-3 && fabs(e - 0.0201) < 1e-4);
    CHECK(!(e <= 1e-3));
  }
  {  // a NaN anywhere is never "orthonormal"
    const int di = 256, dout = 768;
    std::vector<float> A = orthonormal_columns(dout, di);
    A[(size_t)300 * di + 11] = NAN;
    std::vector<double> G((size_t)di * di);
    const double e = rot_col_gram_error(A.data(), dout, di, G.data());
    printf("gram rect NaN: %g\n", e);
    CHECK(!(e <= 1e-3));
    A = orthonormal_columns(di, di);
    A[5] = NAN;
    CHECK(!(rot_row_gram_error(A.data(), di, di) <= 1e-3));
  }
  {  // a square matrix: rows and columns agree, and a scaled ROW is seen by the row check
    const int d = 256;
    std::vector<float> A = orthonormal_columns(d, d);
    std::vector<double> G((size_t)d * d);
    const double er = rot_row_gram_error(A.data(), d, d), ec = rot_col_gram_error(A.data(), d, d, G.data());
    printf("gram square %d: rows %.3g columns %.3g\n", d, er, ec);
    CHECK(er <= 1e-5 && ec <= 1e-5);
    for (int c = 0; c < d; ++c) A[(size_t)9 * d + c] *= 1.01f;
    const double es = rot_row_gram_error(A.data(), d, d);
    printf("gram square scaled row: %.5f\n", es);
    CHECK(es > 1e-3 && fabs(es - 0.0201) < 1e-4);
  }
  if (failures) {
    printf("%d checks FAILED\n", failures);
    return 1;
  }
  printf("rot shape ok\n");
  return 0;
}
