// The backbone frame of a residue - AlphaFold's algorithm 21 (Jumper et al., Nature 596:583-589 (2021), supplementary) from its
// N, CA, C - and a point in that frame's coordinates.  csrc/fape.hip (the FAPE training loss) and csrc/sidechain.hip (the
// local-frame side-chain RMSD) express atoms in these frames: which residues span a frame, and how a point is rounded on its
// way into one, is decided here and nowhere else.
#pragma once
#include <math.h>

#include "common.h"

namespace backbone_frame {

constexpr double DEGENERATE = 1.0e-8;   // A^2: |v1|^2 or |u2|^2 at or below this spans no frame

struct __attribute__((aligned(16))) Frame {   // x_local = (e1 . r, e2 . r, e3 . r), r = x - t
  float e[9];                                 // e1, e2, e3
  float t[3];
};

// Algorithm 21 from the points N, CA, C (nine consecutive floats): fp64 on the fp32 coordinates, rounded once.  False when the
// points span no frame (a NaN fails both tests); the record is then not to be used.  Not inlined: prediction and truth run the
// same instructions, whatever the compiler contracts.
static __device__ __noinline__ bool build_frame(const float *__restrict__ nca_c, Frame &f) {
  const double nx = nca_c[0], ny = nca_c[1], nz = nca_c[2], ax = nca_c[3], ay = nca_c[4], az = nca_c[5];
  const double cx = nca_c[6], cy = nca_c[7], cz = nca_c[8];
  const double v1x = cx - ax, v1y = cy - ay, v1z = cz - az, v2x = nx - ax, v2y = ny - ay, v2z = nz - az;
  const double q1 = v1x * v1x + v1y * v1y + v1z * v1z;
  const double i1 = 1.0 / sqrt(q1);
  const double e1x = v1x * i1, e1y = v1y * i1, e1z = v1z * i1;
  const double s = e1x * v2x + e1y * v2y + e1z * v2z;
  const double ux = v2x - e1x * s, uy = v2y - e1y * s, uz = v2z - e1z * s;
  const double q2 = ux * ux + uy * uy + uz * uz;
  const double i2 = 1.0 / sqrt(q2);
  const double e2x = ux * i2, e2y = uy * i2, e2z = uz * i2;
  f.e[0] = (float)e1x; f.e[1] = (float)e1y; f.e[2] = (float)e1z;
  f.e[3] = (float)e2x; f.e[4] = (float)e2y; f.e[5] = (float)e2z;
  f.e[6] = (float)(e1y * e2z - e1z * e2y); f.e[7] = (float)(e1z * e2x - e1x * e2z); f.e[8] = (float)(e1x * e2y - e1y * e2x);
  f.t[0] = nca_c[3]; f.t[1] = nca_c[4]; f.t[2] = nca_c[5];
  return q1 > DEGENERATE && q2 > DEGENERATE;
}
// r = x - t and the point in the frame's coordinates; explicit multiply-adds, so both callers round alike
__device__ __forceinline__ void local_coords(const Frame &f, float x, float y, float z, float &rx, float &ry, float &rz, float &lx,
                                             float &ly, float &lz) {
  rx = x - f.t[0]; ry = y - f.t[1]; rz = z - f.t[2];
  lx = fmaf(f.e[2], rz, fmaf(f.e[1], ry, __fmul_rn(f.e[0], rx)));
  ly = fmaf(f.e[5], rz, fmaf(f.e[4], ry, __fmul_rn(f.e[3], rx)));
  lz = fmaf(f.e[8], rz, fmaf(f.e[7], ry, __fmul_rn(f.e[6], rx)));
}

}  // namespace backbone_frame
