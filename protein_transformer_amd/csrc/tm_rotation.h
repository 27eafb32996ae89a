// The least-squares superposition behind csrc/tmscore.hip: from the 16 moments of a set of (p, q) pairs - n, sum p, sum q,
// sum p q^T - the PROPER rotation R (det = +1) and translation t that minimise sum |R p + t - q|^2.
//
// Route: Horn, "Closed-form solution of absolute orientation using unit quaternions", J. Opt. Soc. Am. A 4(4):629-642 (1987).
// With S = sum (p - pbar)(q - qbar)^T the unit quaternion of the best rotation is the eigenvector of the largest eigenvalue of a
// symmetric 4x4 matrix built from S; a quaternion is a proper rotation by construction, so the mirror-image case (det S < 0)
// needs no correction step.  The eigenvectors come from cyclic Jacobi rotations in fp64, the pattern of sym3_eigenvalues in
// csrc/kabsch.hip with the rotations accumulated.  Every loop over matrix indices is unrolled: the matrices live in registers.
// __host__ __device__, so a CPU program can check it against an SVD.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace tm_rotation {

constexpr int NMOM = 15;   // sum p (3), sum q (3), sum p q^T (9, row = p's axis); the count travels beside them as an integer

// x[0..8] = R row-major, x[9..11] = t
__host__ __device__ inline void solve(const double (&m)[NMOM], int n, double (&x)[12]) {
  const double inv = 1.0 / (double)n;
  const double pb[3] = {m[0] * inv, m[1] * inv, m[2] * inv}, qb[3] = {m[3] * inv, m[4] * inv, m[5] * inv};
  double S[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) S[i][j] = m[6 + 3 * i + j] - (double)n * pb[i] * qb[j];
  double a[4][4], v[4][4];
  a[0][0] = S[0][0] + S[1][1] + S[2][2];
  a[1][1] = S[0][0] - S[1][1] - S[2][2];
  a[2][2] = -S[0][0] + S[1][1] - S[2][2];
  a[3][3] = -S[0][0] - S[1][1] + S[2][2];
  a[0][1] = a[1][0] = S[1][2] - S[2][1];
  a[0][2] = a[2][0] = S[2][0] - S[0][2];
  a[0][3] = a[3][0] = S[0][1] - S[1][0];
  a[1][2] = a[2][1] = S[0][1] + S[1][0];
  a[1][3] = a[3][1] = S[2][0] + S[0][2];
  a[2][3] = a[3][2] = S[1][2] + S[2][1];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  // Jacobi converges quadratically; the sweep that finds the off-diagonal below 1e-20 of the diagonal is the last one (an
  // eigenvector is then exact to rounding unless the two largest eigenvalues agree to ~1e-16, where no rotation is defined)
  for (int sweep = 0; sweep < 30; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
    const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]);
    if (off <= 1e-20 * diag) break;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = a[p][q];
        if (apq != 0.0) {
          const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          a[p][p] -= t * apq;
          a[q][q] += t * apq;
          a[p][q] = a[q][p] = 0.0;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (r != p && r != q) {
              const double arp = a[r][p], arq = a[r][q];
              a[r][p] = a[p][r] = c * arp - s * arq;
              a[r][q] = a[q][r] = s * arp + c * arq;
            }
            const double vrp = v[r][p], vrq = v[r][q];
            v[r][p] = c * vrp - s * vrq;
            v[r][q] = s * vrp + c * vrq;
          }
        }
      }
  }
  // the column of the largest eigenvalue, picked with selects: no indexed access to the register arrays.  A later column wins
  // only by more than Jacobi's own rounding (64 eps of the diagonal): eigenvalues that close are a tie, every column of a tie is
  // optimal to that rounding, and the FIRST one is taken.  It matters for a set fitted on itself: S is then symmetric to the bit,
  // row 0 of Horn's matrix is exactly zero and stays so, and column 0 remains the identity quaternion with eigenvalue trace S
  // untouched.  For collinear atoms (sigma2 = sigma3 = 0) the half turn about the line has that same eigenvalue, and a plain `>`
  // let the rounding of the sweeps choose between the two: the half turn leaves residuals of 1e-15 where the identity leaves 0.
  const double tie = 64.0 * 2.220446049250313e-16 * (fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]));
  double ev = a[0][0], qw = v[0][0], qx = v[1][0], qy = v[2][0], qz = v[3][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = a[k][k] > ev + tie;
    ev = up ? a[k][k] : ev;
    qw = up ? v[0][k] : qw;
    qx = up ? v[1][k] : qx;
    qy = up ? v[2][k] : qy;
    qz = up ? v[3][k] : qz;
  }
  const double nq = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);   // (a product of rotations: 1 up to rounding)
  qw *= nq; qx *= nq; qy *= nq; qz *= nq;
  x[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  x[1] = 2.0 * (qx * qy - qw * qz);
  x[2] = 2.0 * (qx * qz + qw * qy);
  x[3] = 2.0 * (qx * qy + qw * qz);
  x[4] = 1.0 - 2.0 * (qx * qx + qz * qz);
  x[5] = 2.0 * (qy * qz - qw * qx);
  x[6] = 2.0 * (qx * qz - qw * qy);
  x[7] = 2.0 * (qy * qz + qw * qx);
  x[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
#pragma unroll
  for (int i = 0; i < 3; ++i) x[9 + i] = qb[i] - (x[3 * i] * pb[0] + x[3 * i + 1] * pb[1] + x[3 * i + 2] * pb[2]);
}

}  // namespace tm_rotation
