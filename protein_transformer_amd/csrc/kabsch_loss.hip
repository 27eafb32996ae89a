// RMSD after optimal superposition as a TRAINING loss for gfx950: `train.py -l kabsch`, forward and analytic backward.
//
// Stands beside
//   rmsd(a, b)            /root/reference/protein_transformer/losses.py:281-286
// which the reference only evaluates (ProDy), and beside csrc/kabsch.hip, which reports it as `rmsd-full` from a trace formula
// without ever forming the rotation.  A gradient needs the rotation: with R the optimal PROPER rotation and r_k = R (a_k - abar)
// - (b_k - bbar), d(loss)/d(a_k) = R^T r_k / (n loss) - R is optimal and sum r_k = 0, so neither contributes a term.  The
// definition, its edges and the place where it is not differentiable are in include/ptamd.h.
//
// One workgroup per protein, one launch, no workspace:
//   origin   the protein's first present slot (block-wide vote, normally one round): every coordinate below is taken relative to
//            that (pred, true) pair in fp64, as csrc/tmscore.hip does, so a structure 1e3 A from the origin loses nothing to
//            cancellation.
//   sweep 1  the 15 moments of csrc/tm_rotation.h, the count and sum |a|^2 + |b|^2 (a NaN / infinite coordinate reaches it and
//            cannot cancel) in fp64: wave_sum_d, one LDS step in wavefront order.  One lane centres them - S = M - (sum a)(sum
//            b)^T / n, symmetric to the bit when a == b - calls tm_rotation::solve on the centred moments and broadcasts R, t
//            through LDS.
//   sweep 2  re-reads the atoms and sums |r_k|^2 in fp64 in the same fixed order: the loss comes from the residuals of the R
//            that the gradient uses, not from a trace formula.
//   sweep 3  (dcrd != NULL) re-reads them once more and writes R^T r_k / (n loss), and 0.0f into every other slot.
// Nothing is kept in registers across sweeps (L goes to 4096); the re-reads come from L2 (172 KB per protein at L = 512).
// No atomics, no order that depends on scheduling: two runs give the same bits, and a protein's bits do not depend on its batch.
// Algorithmic traffic: 24 B per atom slot per sweep read (x 3 with the gradient, x 2 without) + 12 B written with the gradient.
#include <math.h>

#include "common.h"
#include "tm_rotation.h"

namespace {

using tm_rotation::NMOM;

constexpr int KL = 256;             // threads per protein
constexpr int KW = KL / 64;         // wavefronts per protein
constexpr int NSUM = NMOM + 1;      // the 15 moments, then sum |a|^2 + |b|^2

struct Atom {
  double p[3], q[3];
};

// slot s of a protein: present = residue not padded (collate pads the truth with zeros, not NaN) and no NaN in the true
// coordinate (losses.py:70-72), the rule of kabsch_rmsd_kernel; what the prediction holds never decides presence
__device__ __forceinline__ bool load_atom(const float *__restrict__ pred, const float *__restrict__ truth,
                                          const int64_t *__restrict__ seq, int s, const Atom &org, Atom &a) {
  if (seq[s / PTAMD_NUM_SLOTS] == PTAMD_PAD_ID) return false;
  const size_t at = (size_t)s * 3;
  const float tx = truth[at], ty = truth[at + 1], tz = truth[at + 2];
  if (isnan(tx) || isnan(ty) || isnan(tz)) return false;
  a.p[0] = (double)pred[at] - org.p[0];
  a.p[1] = (double)pred[at + 1] - org.p[1];
  a.p[2] = (double)pred[at + 2] - org.p[2];
  a.q[0] = (double)tx - org.q[0];
  a.q[1] = (double)ty - org.q[1];
  a.q[2] = (double)tz - org.q[2];
  return true;
}

// r = R p + t - q, x = (R row-major, t)
__device__ __forceinline__ void residual(const double (&x)[12], const Atom &a, double (&r)[3]) {
#pragma unroll
  for (int u = 0; u < 3; ++u)
    r[u] = fma(x[3 * u], a.p[0], fma(x[3 * u + 1], a.p[1], fma(x[3 * u + 2], a.p[2], x[9 + u]))) - a.q[u];
}

__global__ __launch_bounds__(KL) void kabsch_loss_kernel(const float *__restrict__ pred, const float *__restrict__ truth,
                                                         const int64_t *__restrict__ seq, int L, float *__restrict__ stats,
                                                         float *__restrict__ dcrd) {
  __shared__ int s_first[KW], s_cnt[KW], s_n, s_ok;
  __shared__ double s_part[KW][NSUM], s_x[12], s_sq[KW];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nslot = L * PTAMD_NUM_SLOTS;
  pred += (size_t)b * nslot * 3;
  truth += (size_t)b * nslot * 3;
  seq += (size_t)b * L;
  if (dcrd) dcrd += (size_t)b * nslot * 3;

  // ---- the origin: the first present slot.  Every branch on `first` is uniform over the workgroup.
  const Atom zero = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  Atom a;
  int first = -1;
  for (int base = 0; base < nslot && first < 0; base += KL) {
    const int s = base + tid;
    const unsigned long long m = __ballot(s < nslot && load_atom(pred, truth, seq, s, zero, a));
    if (lane == 0) s_first[wave] = m ? base + wave * 64 + __ffsll((long long)m) - 1 : -1;
    __syncthreads();
#pragma unroll
    for (int w = KW - 1; w >= 0; --w) first = s_first[w] >= 0 ? s_first[w] : first;
    __syncthreads();
  }
  Atom org = zero;
  if (first >= 0) load_atom(pred, truth, seq, first, zero, org);

  // ---- sweep 1: moments
  double mom[NSUM];
#pragma unroll
  for (int k = 0; k < NSUM; ++k) mom[k] = 0.0;
  int cnt = 0;   // (wavefront-uniform)
  for (int base = 0; base < nslot; base += KL) {
    const int s = base + tid;
    const bool ok = s < nslot && load_atom(pred, truth, seq, s, org, a);
    cnt += __popcll(__ballot(ok));
    if (ok) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        mom[u] += a.p[u];
        mom[3 + u] += a.q[u];
#pragma unroll
        for (int v = 0; v < 3; ++v) mom[6 + 3 * u + v] = fma(a.p[u], a.q[v], mom[6 + 3 * u + v]);
        mom[NMOM] = fma(a.p[u], a.p[u], fma(a.q[u], a.q[u], mom[NMOM]));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NSUM; ++k) {
    const double v = wave_sum_d(mom[k]);
    if (lane == 0) s_part[wave][k] = v;
  }
  if (lane == 0) s_cnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    double m[NSUM];
    int n = 0;
    for (int k = 0; k < NSUM; ++k) {
      double v = 0.0;
      for (int w = 0; w < KW; ++w) v += s_part[w][k];
      m[k] = v;
    }
    for (int w = 0; w < KW; ++w) n += s_cnt[w];
    // fewer than 3 atoms leave the rotation undetermined; a NaN / infinite coordinate on a present atom reaches the sum of
    // squares, where nothing cancels (finite fp32 coordinates of any size keep it finite in fp64)
    const bool ok = n >= 3 && isfinite(m[NMOM]);
    if (ok) {
      // centred here, not in solve(): (sum a)_u (sum b)_v and (sum a)_v (sum b)_u are the same product when a == b, so S is
      // symmetric to the bit, Horn's matrix has an exactly zero first row, and a prediction that IS the truth gets R = 1, t = 0
      // and residuals that are exactly zero.  solve() sees sums of zero and subtracts nothing.
      const double inv = 1.0 / (double)n;
      double c[NMOM], x[12];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        c[u] = c[3 + u] = 0.0;
#pragma unroll
        for (int v = 0; v < 3; ++v) c[6 + 3 * u + v] = m[6 + 3 * u + v] - (m[u] * m[3 + v]) * inv;
      }
      tm_rotation::solve(c, n, x);
#pragma unroll
      for (int k = 0; k < 9; ++k) s_x[k] = x[k];
#pragma unroll
      for (int u = 0; u < 3; ++u)   // t = bbar - R abar, as (sum b - R sum a) / n: with R = 1 and equal sums the bracket is an
                                    // exact zero however the compiler fuses it (bbar - abar, fused, is the rounding of a mean)
        s_x[9 + u] = (m[3 + u] - (x[3 * u] * m[0] + x[3 * u + 1] * m[1] + x[3 * u + 2] * m[2])) * inv;
    }
    s_n = n;
    s_ok = ok ? 1 : 0;
  }
  __syncthreads();
  const int n = s_n;
  const bool usable = s_ok != 0;   // (uniform over the workgroup)

  // ---- sweep 2: the loss, from the residuals themselves
  double x[12], total = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) x[k] = usable ? s_x[k] : 0.0;
  if (usable) {
    double sq = 0.0;
    for (int base = 0; base < nslot; base += KL) {
      const int s = base + tid;
      if (s < nslot && load_atom(pred, truth, seq, s, org, a)) {
        double r[3];
        residual(x, a, r);
        sq = fma(r[0], r[0], fma(r[1], r[1], fma(r[2], r[2], sq)));
      }
    }
    sq = wave_sum_d(sq);
    if (lane == 0) s_sq[wave] = sq;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < KW; ++w) total += s_sq[w];   // the same bits in every thread
  }
  const double loss = usable ? sqrt(total / (double)n) : (double)__builtin_nanf("");
  if (tid == 0) {
    stats[(size_t)b * 2] = (float)loss;
    stats[(size_t)b * 2 + 1] = (float)n;
  }
  if (!dcrd) return;

  // ---- sweep 3: the gradient; every slot of the protein is written.  loss == 0 means every residual is zero: nothing is divided.
  const bool live = usable && total > 0.0;
  const double scale = live ? 1.0 / ((double)n * loss) : 0.0;
  for (int base = 0; base < nslot; base += KL) {
    const int s = base + tid;
    if (s >= nslot) break;
    float g[3] = {0.0f, 0.0f, 0.0f};
    if (live && load_atom(pred, truth, seq, s, org, a)) {
      double r[3];
      residual(x, a, r);
#pragma unroll
      for (int u = 0; u < 3; ++u) g[u] = (float)((x[u] * r[0] + x[3 + u] * r[1] + x[6 + u] * r[2]) * scale);   // R^T r
    }
    dcrd[(size_t)s * 3] = g[0];
    dcrd[(size_t)s * 3 + 1] = g[1];
    dcrd[(size_t)s * 3 + 2] = g[2];
  }
}

}  // namespace

extern "C" int ptamd_kabsch_loss_fwd_bwd(const float *crd, const float *true_crd, const int64_t *seq, int B, int L, float *stats,
                                         float *dcrd, void *stream) {
  if (B <= 0 || L <= 0 || L > INT_MAX / (2 * PTAMD_NUM_SLOTS)) return PTAMD_ERR_BAD_SHAPE;   // slot indices are ints
  if (!crd || !true_crd || !seq || !stats) return PTAMD_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(kabsch_loss_kernel, dim3(B), dim3(KL), 0, (hipStream_t)stream, crd, true_crd, seq, L, stats, dcrd);
  return pt_check_launch();
}
