// Smooth lDDT loss, forward + analytic backward, for a whole batch on gfx950: the training loss `train.py -l slddt`.
//
// The reference (protein_transformer) has no counterpart: every structural loss it trains on is a global all-pairs RMS of
// distance errors.  This is the differentiable lDDT of Abramson et al., "Accurate structure prediction of biomolecular
// interactions with AlphaFold 3", Nature 630:493-500 (2024), supplementary algorithm 27: the four threshold tests of lDDT
// (csrc/lddt.hip) replaced by logistic functions.  It departs from that algorithm in one point: a temperature tau divides the
// argument of the logistics (tau = 1 is AlphaFold 3's loss, tau -> 0 the hard lDDT).  Definition: include/ptamd.h.
//
// Three launches per batch behind the zero fill of `dcrd`:
//   compact   the present atoms of each protein, in slot order, into the workspace, and the bounding box of the TRUE
//             coordinates of every tile of 64 of them: csrc/atom_tiles.h, shared with csrc/lddt.hip.  This file's record keeps
//             the atom's slot, and a predicted coordinate that is not finite (or beyond 1e18: its squared differences would
//             not be) is replaced by 0 and the atom marked: its pairs are counted, score 0 and carry no gradient - nothing
//             non-finite enters the sweep.  (csrc/drmsd.hip packs differently: the backbone first, for its backbone-only loss.)
//   sweep     the strip-by-chunk sweep of csrc/pair_sweep.h over the upper triangle of tile pairs, shared with csrc/clash.hip;
//             this file owns the pair term (SlddtPair below: the four logistics and their derivative), and a tile pair goes
//             when the gap between its true boxes exceeds the cutoff.
//   finalize  per protein the work items' sums (pair_sweep::item_sums), loss and score, and per atom the gathered gradient
//             (pair_sweep::atom_gradient) scaled by 1 / (4 tau npairs) and scattered back to the slot layout.
// Two runs give the same bits; a protein's bits do not depend on the batch around it or on its padding.
#include <limits.h>
#include <math.h>

#include "pair_sweep.h"

namespace {

using namespace pair_sweep;

constexpr int NTHR = 4;           // thresholds 0.5, 1, 2, 4

// stage 1, atom_tiles::compact_kernel with atom_tiles::SlotRecord: code = residue << 1 | (predicted coordinate unusable), -1
// behind the last atom; aux = slot

// constants of a launch, computed on the host: exp((delta - t) / tau) = 2^(u - a_t) with u = delta kexp, a_t = t kexp split
// into an integer ia[t] and a fraction whose power of two is cfrac[t] - one exponential of the fraction of u serves all four
struct Consts {
  float cutoff, kexp;
  float cfrac[NTHR];
  int ia[NTHR];
};

struct Layout {
  TileLayout t;
  size_t total;
  SweepLayout s;
  Layout(int B, int L) : t(B, L), total(t.end), s(B, t.tiles, total) {}
};

// ---- stage 2: the pair term of the sweep.  An Item is the sum over the scored pairs of the four logistics, and the included
// pairs.  Per pair, with q the sums of squares: 6 subtractions, 6 multiply-adds, v_sqrt_f32 of both (the true distance is
// atom_tiles' true_dist, as in lddt_sweep_kernel; the predicted one is the same function of its q, so a prediction equal to the
// truth has delta == 0 exactly), v_rsq_f32 for 1 / dp (gradient only), one v_exp_f32 and four v_rcp_f32 for the
// logistics.  The clamp of csrc/drmsd.hip under the root is the 1e-30 added to the predicted squares - to their rounded SUM, not
// as the addend of the first multiply-add: there it breaks a rounding tie of dx^2 (differences of stored coordinates have few
// significant bits, so exact ties do occur) and leaves dp one ulp above dt for a prediction equal to the truth.
struct SlddtPair {
  using Atom = Atom8;
  static constexpr bool SPARSE = false;
  struct Row {};
  Consts k;
  static __device__ __forceinline__ Atom dead() { return Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1, 0}; }
  static __device__ __forceinline__ float4 position(const Atom &a) { return make_float4(a.px, a.py, a.pz, 0.f); }
  __device__ __forceinline__ float reach() const { return k.cutoff; }
  __device__ __forceinline__ Row row(const Atom &) const { return Row{}; }
  __device__ __forceinline__ Term term(const Atom &a, Row, const Atom &c, bool apart) const {
    const float dxt = a.tx - c.tx, dyt = a.ty - c.ty, dzt = a.tz - c.tz;
    const float dxp = a.px - c.px, dyp = a.py - c.py, dzp = a.pz - c.pz;
    const float qp = fmaf(dzp, dzp, fmaf(dyp, dyp, dxp * dxp)) + 1e-30f;   // (the sum itself above 1e-22)
    const float dt = true_dist(dxt, dyt, dzt);
    const float dp = __builtin_amdgcn_sqrtf(qp);
    const bool incl = dt < k.cutoff && apart;   // strict
    const bool scored = incl && ((a.code | c.code) & 1) == 0;
    const float sd = dp - dt, delta = fabsf(sd);
    const float u = fminf(delta * k.kexp, 1073741824.f);
    const float fl = floorf(u);
    const float ef = __builtin_amdgcn_exp2f(u - fl);   // in [1, 2)
    const int nu = (int)fl;
    float sig = 0.f, wgt = 0.f;
#pragma unroll
    for (int t = 0; t < NTHR; ++t) {
      const float s = __builtin_amdgcn_rcpf(1.f + ldexpf(ef * k.cfrac[t], nu - k.ia[t]));
      sig += s;
      wgt = fmaf(s, 1.f - s, wgt);   // sigma' as sigma (1 - sigma): a saturated exponential gives 0
    }
    const float wi = wgt * __builtin_amdgcn_rsqf(qp);
    const float cf = sd > 0.f ? wi : (sd < 0.f ? -wi : 0.f);   // sign(0) = 0
    return Term{scored ? sig : 0.f, incl, scored ? cf : 0.f, dxp, dyp, dzp};
  }
};

template <bool WITH_GRAD>
__global__ __launch_bounds__(TS) void slddt_sweep_kernel(const Atom8 *__restrict__ atoms, const Box8 *__restrict__ boxes,
                                                         const int *__restrict__ natoms, int nstride, Dims d, Consts k,
                                                         float4 *__restrict__ rowpart, float4 *__restrict__ colpart,
                                                         int *__restrict__ kept, Item *__restrict__ items) {
  sweep<WITH_GRAD>(SlddtPair{k}, atoms, boxes, natoms, nstride, d, rowpart, colpart, kept, items);
}

// ---- stage 3: grid (ceil(nstride / 256), B); dcrd was zeroed before.  Every workgroup of a protein sums the protein's work
// items (it needs npairs for the gradient scale).
__global__ __launch_bounds__(FIN_THREADS) void slddt_finalize_kernel(const Atom8 *__restrict__ atoms, const int *__restrict__ natoms,
                                                                     const float4 *__restrict__ rowpart,
                                                                     const float4 *__restrict__ colpart,
                                                                     const int *__restrict__ kept, const Item *__restrict__ items,
                                                                     int nstride, Dims d, float gscale, float *__restrict__ stats,
                                                                     long long *__restrict__ npairs, float *__restrict__ dcrd,
                                                                     int nslot) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  if ((int)blockIdx.x * FIN_THREADS >= max(n, 1)) return;
  const Item all = item_sums(items, d, b, nT);
  const double eps = all.sum;
  const long long np = all.count;
  if (blockIdx.x == 0 && tid == 0) {
    const float score = np > 0 ? (float)(eps / (4.0 * (double)np)) : __builtin_nanf("");
    stats[(size_t)b * 2] = np > 0 ? (float)(1.0 - eps / (4.0 * (double)np)) : __builtin_nanf("");
    stats[(size_t)b * 2 + 1] = score;
    npairs[b] = np;
  }
  if (dcrd == nullptr) return;
  const int j = blockIdx.x * FIN_THREADS + tid;
  if (j >= n) return;
  const float scale = np > 0 ? (float)((double)gscale / (double)np) : 0.f;
  const Atom8 a = atoms[(size_t)b * nstride + j];
  const float3 g = atom_gradient(rowpart, colpart, kept, d, b, j, nT, SlddtPair::position(a));
  float *out = dcrd + ((size_t)b * nslot + a.aux) * 3;
  const bool bad = a.code & 1;   // (its coefficients are all zero: written as a plain 0)
  out[0] = bad ? 0.f : scale * g.x;
  out[1] = bad ? 0.f : scale * g.y;
  out[2] = bad ? 0.f : scale * g.z;
}

}  // namespace

extern "C" {

size_t ptamd_slddt_workspace_bytes(int B, int L) {
  if (!tile_shape_ok(B, L)) return 0;
  return Layout(B, L).total;
}

int ptamd_slddt_fwd_bwd(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float cutoff,
                        float temperature, float *stats, int64_t *npairs, float *dcrd, void *workspace, size_t workspace_bytes,
                        void *stream) {
  if (!tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !stats || !npairs) return PTAMD_ERR_BAD_SHAPE;
  if (!(cutoff > 0.f) || !isfinite(cutoff) || !(temperature > 0.f) || !isfinite(temperature)) return PTAMD_ERR_BAD_SHAPE;
  const Layout l(B, L);
  const Dims d = l.s.d;
  if (!workspace || workspace_bytes < l.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  if ((size_t)d.strips * d.chunks > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;   // (a grid dimension; its workspace is beyond any device)
  char *ws = static_cast<char *>(workspace);
  Atom8 *atoms = reinterpret_cast<Atom8 *>(ws + l.t.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.t.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.t.natoms);
  float4 *rowpart = reinterpret_cast<float4 *>(ws + l.s.rowpart), *colpart = reinterpret_cast<float4 *>(ws + l.s.colpart);
  int *kept = reinterpret_cast<int *>(ws + l.s.kept);
  Item *items = reinterpret_cast<Item *>(ws + l.s.items);
  // the scale constants of the launch
  Consts k;
  k.cutoff = cutoff;
  const double kexp = 1.4426950408889634 / (double)temperature;   // log2(e) / tau
  k.kexp = (float)kexp;
  const double thr[NTHR] = {0.5, 1.0, 2.0, 4.0};
  for (int t = 0; t < NTHR; ++t) {
    const double a = fmin(thr[t] * kexp, 1073741824.0), ai = floor(a);
    k.ia[t] = (int)ai;
    k.cfrac[t] = (float)exp2(-(a - ai));
  }
  const float gscale = (float)(0.25 / (double)temperature);
  hipStream_t st = (hipStream_t)stream;
  const int nslot = L * PTAMD_NUM_SLOTS;
  if (dcrd) PT_HIP_TRY(hipMemsetAsync(dcrd, 0, (size_t)B * nslot * 3 * sizeof(float), st));   // slots of absent atoms stay 0
  hipLaunchKernelGGL(compact_kernel<SlotRecord>, dim3(B), dim3(COMPACT_THREADS), 0, st, pred_crd, true_crd, seq, L, l.t.nstride, l.t.tiles,
                     atoms, boxes, natoms);
  int rc = pt_check_launch();
  if (rc) return rc;
  auto sweep = dcrd ? slddt_sweep_kernel<true> : slddt_sweep_kernel<false>;
  hipLaunchKernelGGL(sweep, dim3((unsigned)(d.strips * d.chunks), B), dim3(TS), 0, st, atoms, boxes, natoms, l.t.nstride, d, k,
                     rowpart, colpart, kept, items);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(slddt_finalize_kernel, dim3(dcrd ? (unsigned)((l.t.nstride + FIN_THREADS - 1) / FIN_THREADS) : 1u, B),
                     dim3(FIN_THREADS), 0, st, atoms, natoms, rowpart, colpart, kept, items, l.t.nstride, d, gscale, stats,
                     reinterpret_cast<long long *>(npairs), dcrd, nslot);
  return pt_check_launch();
}

}  // extern "C"
