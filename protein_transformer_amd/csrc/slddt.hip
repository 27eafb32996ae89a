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
//   sweep     the UPPER TRIANGLE of tile pairs, every unordered pair of atoms once.  A work item is one wavefront: a STRIP of 4
//             row tiles (one atom per lane and tile, in registers) against a CHUNK of 8 column tiles.  Per column tile J the
//             wavefront stages the tile in LDS and visits the row tiles I <= J of its strip whose true bounding box lies within
//             the cutoff of J's (no pair of two farther tiles can be included).  16 columns at a time:
//               phase 1  lane = row atom, column atom broadcast from LDS: the pair's logistics, its share of the row atom's
//                        gradient, and its coefficient cf_ij left in LDS (row-major, 17-word rows);
//               phase 2  that 64 x 16 tile re-read TRANSPOSED (lane = column, a quarter of the rows): S_j = sum_i cf_ij and
//                        V_j = sum_i cf_ij x_i, the quarters folded by two lane exchanges - the column atom's share is
//                        x_j S_j - V_j (the scheme of csrc/drmsd.hip, without its DPP operands).
//             The (S, V) of a column tile are summed over the strip's row tiles in tile order and written once per (strip,
//             column tile) with a flag "this strip touched the tile"; row gradients once per (row tile, chunk); the sum of the
//             logistics (fp32 inside a tile pair, fp64 across them) and the pair count once per work item.  Wavefronts share
//             nothing: no barrier, no atomics.
//   finalize  per protein the work items' sums in an order that depends on the protein's atom count alone (not on B, not on
//             L), loss and score, and per atom row partials (chunk order) + column partials (strip order), scaled by
//             1 / (4 tau npairs) and scattered back to the slot layout.
// Two runs give the same bits; a protein's bits do not depend on the batch around it or on its padding.
#include <limits.h>
#include <math.h>

#include "atom_tiles.h"

namespace {

using namespace atom_tiles;

constexpr int STRIP_TILES = 4;    // row tiles of a work item
constexpr int CHUNK_TILES = 8;    // column tiles of a work item (<= 64: a lane tests one column tile's box)
constexpr int SUB = 16, CF_LD = SUB + 1;   // the coefficient tile is kept for 16 columns at a time: 4.3 KB
constexpr int FIN_THREADS = 256;
constexpr int NTHR = 4;           // thresholds 0.5, 1, 2, 4

// stage 1, atom_tiles::compact_kernel with atom_tiles::SlotRecord: code = residue << 1 | (predicted coordinate unusable), -1
// behind the last atom; aux = slot
struct __attribute__((aligned(16))) Item {   // what one work item of the sweep leaves for the finalize kernel
  double eps;        // sum over its scored pairs of the four logistics
  long long pairs;   // its included pairs
};
// constants of a launch, computed on the host: exp((delta - t) / tau) = 2^(u - a_t) with u = delta kexp, a_t = t kexp split
// into an integer ia[t] and a fraction whose power of two is cfrac[t] - one exponential of the fraction of u serves all four
struct Consts {
  float cutoff, kexp;
  float cfrac[NTHR];
  int ia[NTHR];
};

struct Layout {
  TileLayout t;
  size_t rowpart, colpart, kept, items, total;
  int strips, chunks;
  Layout(int B, int L) : t(B, L) {
    strips = (t.tiles + STRIP_TILES - 1) / STRIP_TILES;
    chunks = (t.tiles + CHUNK_TILES - 1) / CHUNK_TILES;
    total = t.end;
    rowpart = take(total, (size_t)B * t.tiles * chunks * TS * sizeof(float4));   // [b][row tile][chunk][lane]
    colpart = take(total, (size_t)B * strips * t.tiles * TS * sizeof(float4));   // [b][strip][column tile][lane]
    kept = take(total, (size_t)B * strips * t.tiles * sizeof(int));              // [b][strip][column tile]
    items = take(total, (size_t)B * strips * chunks * sizeof(Item));             // [b][strip][chunk]
  }
};

// ---- stage 2: the pair sweep.  grid (strips * chunks, B), one wavefront per workgroup = one work item.
// Per pair (phase 1), with q the sums of squares: 6 subtractions, 6 multiply-adds, v_sqrt_f32 of both (the true distance is
// atom_tiles' true_dist, as in lddt_sweep_kernel; the predicted one is the same function of its q, so a prediction equal to the
// truth has delta == 0 exactly), v_rsq_f32 for 1 / dp (gradient only), one v_exp_f32 and four v_rcp_f32 for the
// logistics.  The clamp of csrc/drmsd.hip under the root is the 1e-30 added to the predicted squares - to their rounded SUM, not
// as the addend of the first multiply-add: there it breaks a rounding tie of dx^2 (differences of stored coordinates have few
// significant bits, so exact ties do occur) and leaves dp one ulp above dt for a prediction equal to the truth.
template <bool WITH_GRAD>
__global__ __launch_bounds__(TS) void slddt_sweep_kernel(const Atom8 *__restrict__ atoms, const Box8 *__restrict__ boxes,
                                                         const int *__restrict__ natoms, int nstride, int tiles, int strips,
                                                         int chunks, Consts k, float4 *__restrict__ rowpart,
                                                         float4 *__restrict__ colpart, int *__restrict__ kept,
                                                         Item *__restrict__ items) {
  __shared__ Atom8 s_col[TS];
  __shared__ float s_cf[TS * CF_LD];
  __shared__ float4 s_row[TS];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int strip = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  const int I0 = strip * STRIP_TILES;
  const int J0 = max(I0, chunk * CHUNK_TILES), J1 = min(nT, (chunk + 1) * CHUNK_TILES);
  if (I0 >= nT || J0 >= J1) return;   // below the diagonal or behind the protein: the finalize kernel skips these items too
  atoms += (size_t)b * nstride;
  boxes += (size_t)b * tiles;

  // near[r]: bit l = column tile J0 + l can hold an included pair with row tile I0 + r
  unsigned long long near[STRIP_TILES];
  {
    Box8 c = Box8{0, 0, 0, 0, 0, 0, 0, 0};
    const bool have = J0 + lane < J1;
    if (have) c = boxes[J0 + lane];
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) {
      near[r] = 0ull;
      if (I0 + r < nT) near[r] = __ballot(have && I0 + r <= J0 + lane && boxes_near(boxes[I0 + r], c, k.cutoff));
    }
  }

  Atom8 me[STRIP_TILES];
  float gx[STRIP_TILES], gy[STRIP_TILES], gz[STRIP_TILES];
#pragma unroll
  for (int r = 0; r < STRIP_TILES; ++r) {
    me[r] = Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
    const int i = (I0 + r) * TS + lane;
    if (i < n) me[r] = atoms[i];
    gx[r] = gy[r] = gz[r] = 0.f;
  }
  double eps_sum = 0.0;
  int pairs = 0;

  for (int J = J0; J < J1; ++J) {
    const int jb = J - J0;
    const bool any = ((near[0] | near[1] | near[2] | near[3]) >> jb) & 1ull;
    if (lane == 0) kept[((size_t)b * strips + strip) * tiles + J] = any;
    if (!any) continue;   // wavefront-uniform
    const int cnt = min(TS, n - J * TS);   // live columns of the tile
    {
      const int j = J * TS + lane;
      s_col[lane] = j < n ? atoms[j] : Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
    }
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);   // (S, Vx, Vy, Vz) of column `lane` of the tile
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) {
      if (!((near[r] >> jb) & 1ull)) continue;   // wavefront-uniform
      const Atom8 a = me[r];
      const bool a_live = a.code >= 0;
      const bool diag = I0 + r == J;   // the diagonal tile: pairs i < j only
      if (WITH_GRAD) s_row[lane] = make_float4(a.px, a.py, a.pz, 0.f);
      float eps_t = 0.f;
      for (int j0 = 0; j0 < cnt; j0 += SUB) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll 4
        for (int jj = 0; jj < SUB; ++jj) {
          const int j = j0 + jj;
          const Atom8 c = s_col[j];   // broadcast
          const float dxt = a.tx - c.tx, dyt = a.ty - c.ty, dzt = a.tz - c.tz;
          const float dxp = a.px - c.px, dyp = a.py - c.py, dzp = a.pz - c.pz;
          const float qp = fmaf(dzp, dzp, fmaf(dyp, dyp, dxp * dxp)) + 1e-30f;   // (the sum itself above 1e-22)
          const float dt = true_dist(dxt, dyt, dzt);
          const float dp = __builtin_amdgcn_sqrtf(qp);
          // strict; different residues; a column behind the last atom has code -1 (and a dead row is excluded by a_live)
          const bool incl = dt < k.cutoff && (unsigned)(a.code ^ c.code) > 1u && c.code >= 0 && a_live && (!diag || lane < j);
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
          eps_t += scored ? sig : 0.f;
          pairs += incl ? 1 : 0;
          if (WITH_GRAD) {
            const float wi = wgt * __builtin_amdgcn_rsqf(qp);
            float cf = sd > 0.f ? wi : (sd < 0.f ? -wi : 0.f);   // sign(0) = 0
            cf = scored ? cf : 0.f;
            gx[r] = fmaf(cf, dxp, gx[r]);
            gy[r] = fmaf(cf, dyp, gy[r]);
            gz[r] = fmaf(cf, dzp, gz[r]);
            s_cf[lane * CF_LD + jj] = cf;
          }
        }
        if (WITH_GRAD) {
          // phase 2 for these 16 columns: lane = (column j0 + (lane & 15), quarter lane >> 4 of the rows)
          __builtin_amdgcn_wave_barrier();
          const int col = lane & (SUB - 1), r0 = (lane >> 4) * SUB;
          float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int rr = 0; rr < SUB; ++rr) {
            const float c = s_cf[(r0 + rr) * CF_LD + col];
            const float4 x = s_row[r0 + rr];
            q.x += c;
            q.y = fmaf(c, x.x, q.y);
            q.z = fmaf(c, x.y, q.z);
            q.w = fmaf(c, x.z, q.w);
          }
          // fold the four row quarters (lanes l, l ^ 16, l ^ 32, l ^ 48) in a fixed order: every lane ends with the sum
          q.x += __shfl_xor(q.x, 16, 64); q.y += __shfl_xor(q.y, 16, 64); q.z += __shfl_xor(q.z, 16, 64); q.w += __shfl_xor(q.w, 16, 64);
          q.x += __shfl_xor(q.x, 32, 64); q.y += __shfl_xor(q.y, 32, 64); q.z += __shfl_xor(q.z, 32, 64); q.w += __shfl_xor(q.w, 32, 64);
          if ((lane >> 4) == (j0 >> 4)) {   // lane l keeps column l of the tile
            cs.x += q.x; cs.y += q.y; cs.z += q.z; cs.w += q.w;
          }
        }
      }
      eps_sum += (double)eps_t;
      __builtin_amdgcn_wave_barrier();   // s_row is rewritten for the next row tile
    }
    if (WITH_GRAD) colpart[(((size_t)b * strips + strip) * tiles + J) * TS + lane] = cs;
    __builtin_amdgcn_wave_barrier();     // s_col is rewritten for the next column tile
  }
  if (WITH_GRAD) {
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r)
      if (I0 + r < nT) rowpart[(((size_t)b * tiles + I0 + r) * chunks + chunk) * TS + lane] = make_float4(gx[r], gy[r], gz[r], 0.f);
  }
  eps_sum = wave_sum_d(eps_sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) pairs += __shfl_xor(pairs, o, 64);   // (<= 4 * 8 * 64 * 64: an int)
  if (lane == 0) items[((size_t)b * strips + strip) * chunks + chunk] = Item{eps_sum, (long long)pairs};
}

// ---- stage 3: grid (ceil(nstride / 256), B); dcrd was zeroed before.  Every workgroup of a protein sums the protein's work
// items (it needs npairs for the gradient scale): thread t takes the items t, t + 256, ... of the protein's OWN triangle
// (strips and chunks of its atom count, whatever L is), then a fixed tree.
__global__ __launch_bounds__(FIN_THREADS) void slddt_finalize_kernel(const Atom8 *__restrict__ atoms, const int *__restrict__ natoms,
                                                                     const float4 *__restrict__ rowpart,
                                                                     const float4 *__restrict__ colpart,
                                                                     const int *__restrict__ kept, const Item *__restrict__ items,
                                                                     int nstride, int tiles, int strips, int chunks, float gscale,
                                                                     float *__restrict__ stats, long long *__restrict__ npairs,
                                                                     float *__restrict__ dcrd, int nslot) {
  __shared__ double s_eps[FIN_THREADS];
  __shared__ long long s_cnt[FIN_THREADS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  if ((int)blockIdx.x * FIN_THREADS >= max(n, 1)) return;
  {
    const int sN = (nT + STRIP_TILES - 1) / STRIP_TILES, cN = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
    double e = 0.0;
    long long c = 0;
    for (int r = tid; r < sN * cN; r += FIN_THREADS) {
      const int s = r / cN, ch = r % cN;
      if ((ch + 1) * CHUNK_TILES <= s * STRIP_TILES) continue;   // below the diagonal: never written
      const Item it = items[((size_t)b * strips + s) * chunks + ch];
      e += it.eps;
      c += it.pairs;
    }
    s_eps[tid] = e;
    s_cnt[tid] = c;
    __syncthreads();
    for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
      if (tid < o) {
        s_eps[tid] += s_eps[tid + o];
        s_cnt[tid] += s_cnt[tid + o];
      }
      __syncthreads();
    }
  }
  const double eps = s_eps[0];
  const long long np = s_cnt[0];
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
  const int J = j / TS, lane = j & (TS - 1), sJ = J / STRIP_TILES;
  float rx = 0.f, ry = 0.f, rz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  {  // row side: the chunks of the atom's strip that had work, in chunk order
    const int c0 = (STRIP_TILES * sJ) / CHUNK_TILES, c1 = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
    const float4 *rp = rowpart + ((size_t)b * tiles + J) * chunks * TS + lane;
    for (int c = c0; c < c1; ++c) {
      const float4 r = rp[(size_t)c * TS];
      rx += r.x; ry += r.y; rz += r.z;
    }
  }
  for (int s = 0; s <= sJ; ++s) {  // column side: the strips at or above the atom's tile that touched it, in strip order
    const size_t at = ((size_t)b * strips + s) * tiles + J;
    if (!kept[at]) continue;
    const float4 cp = colpart[at * TS + lane];
    cx += fmaf(a.px, cp.x, -cp.y);
    cy += fmaf(a.py, cp.x, -cp.z);
    cz += fmaf(a.pz, cp.x, -cp.w);
  }
  float *out = dcrd + ((size_t)b * nslot + a.aux) * 3;
  const bool bad = a.code & 1;   // (its coefficients are all zero: written as a plain 0)
  out[0] = bad ? 0.f : scale * (rx + cx);
  out[1] = bad ? 0.f : scale * (ry + cy);
  out[2] = bad ? 0.f : scale * (rz + cz);
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
  if (!workspace || workspace_bytes < l.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  if ((size_t)l.strips * l.chunks > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;   // (a grid dimension; its workspace is beyond any device)
  char *ws = static_cast<char *>(workspace);
  Atom8 *atoms = reinterpret_cast<Atom8 *>(ws + l.t.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.t.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.t.natoms);
  float4 *rowpart = reinterpret_cast<float4 *>(ws + l.rowpart), *colpart = reinterpret_cast<float4 *>(ws + l.colpart);
  int *kept = reinterpret_cast<int *>(ws + l.kept);
  Item *items = reinterpret_cast<Item *>(ws + l.items);
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
  hipLaunchKernelGGL(sweep, dim3((unsigned)(l.strips * l.chunks), B), dim3(TS), 0, st, atoms, boxes, natoms, l.t.nstride, l.t.tiles,
                     l.strips, l.chunks, k, rowpart, colpart, kept, items);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(slddt_finalize_kernel, dim3(dcrd ? (unsigned)((l.t.nstride + FIN_THREADS - 1) / FIN_THREADS) : 1u, B),
                     dim3(FIN_THREADS), 0, st, atoms, natoms, rowpart, colpart, kept, items, l.t.nstride, l.t.tiles, l.strips,
                     l.chunks, gscale, stats, reinterpret_cast<long long *>(npairs), dcrd, nslot);
  return pt_check_launch();
}

}  // extern "C"
