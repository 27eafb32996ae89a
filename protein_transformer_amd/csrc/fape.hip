// Frame aligned point error (FAPE), forward + analytic backward, for a whole batch on gfx950: the training loss
// `train.py -l fape`.
//
// The reference (protein_transformer) has no counterpart: every structural loss it trains on is a function of internal
// distances, so a structure and its mirror image score the same.  This is the loss of Jumper et al., "Highly accurate protein
// structure prediction with AlphaFold", Nature 596:583-589 (2021), supplementary algorithms 21 (a frame from three points) and
// 28 (FAPE): every atom expressed in the backbone frame (N, CA, C) of every residue, for prediction and truth, and the clamped
// deviation of the two.  Definition: include/ptamd.h.
//
// Five launches per batch behind the zero fill of `dcrd`:
//   compact   the present atoms of each protein, in slot order: csrc/atom_tiles.h with its SlotRecord, as csrc/slddt.hip (the
//             bounding boxes it also leaves are not used: FAPE has no inclusion radius, the whole rectangle is visited).
//   frames    one wavefront per protein: the residues whose true N, CA, C are present and span a frame, compacted in residue
//             order as records of predicted (R, t) and true (R, t) - 24 floats - with the residue index beside them, the
//             protein's frame count and its "unusable" flag (a present atom marked by the compaction, or a degenerate predicted
//             frame).  Algorithm 21 runs in fp64 on the fp32 points and is rounded once; prediction and truth go through the
//             same two device functions (build_frame, local_coords), so a prediction equal to the truth has Delta == 0 exactly.
//             The sweeps of an unusable protein return at once: nothing non-finite is ever swept.
//   frame sweep   a work item is one wavefront: a tile of 64 frames (lane = frame, its record in registers) against a chunk of 8
//             atom tiles, each staged in LDS and read as broadcasts.  Lane-private sums: the pair values (fp32 inside an atom
//             tile, fp64 across tiles), the clamped count, G = sum_j g_ij and M = sum_j g_ij (x) (x_j - t_i), with g_ij =
//             Delta_ij / d_ij in the frame's coordinates (0 for a clamped pair).  No cross-lane traffic but the two sums of the
//             work item's value and count at its end.
//   atom sweep    only when `dcrd` is wanted: the roles swapped - lane = atom of one atom tile, ALL frame tiles of the protein
//             in turn, their records broadcast from LDS, the pair recomputed - for the atom's own share sum_i R_i g_ij, scaled
//             and written to its slot.  See "the atom side" below.
//   finalize  per protein the work items' sums in an order that depends on the protein's own counts alone; per frame the (G, M)
//             of its chunks in chunk order, in fp64, through the backward of algorithm 21 into the predicted N, CA, C, scaled
//             by 1 / (Z npairs) and added to the three slots the atom sweep has written (every slot belongs to one frame).
// No atomics, wavefronts share nothing; two runs give the same bits, and a protein's bits depend neither on the batch around it
// nor on its padding.
//
// The atom side.  The recompute pass repeats the ~45 flops of the pair once more; the alternative is csrc/slddt.hip's LDS
// transpose with three values per pair (3 x 64 x 17 words written and re-read per 16 atoms, plus the fold across the row
// quarters).  The recompute pass was chosen for its shape - two kernels that are mirror images of each other, no cross-lane
// step, the atom's gradient written once by the lane that owns it with no partial sums in the workspace - and measured:
// profiles/fape/NOTES.md has the kernel times of both sweeps next to the dRMSD and smooth-lDDT sweeps of the same run.  The
// transpose variant was not built, so that file states the cost of the choice as the atom sweep's share, not as a difference.
#include <limits.h>
#include <math.h>

#include "atom_tiles.h"
#include "backbone_frame.h"

namespace {

using namespace atom_tiles;
using namespace backbone_frame;

constexpr int CHUNK_TILES = 8;          // atom tiles of a work item of the frame sweep
constexpr float D_EPS = 1.0e-4f;        // A^2, under the root
constexpr double Z_SCALE = 10.0;        // A: the length scale the pair values are divided by

struct __attribute__((aligned(16))) FramePair {
  Frame p, q;   // of the prediction, of the truth
};
struct __attribute__((aligned(16))) Item {   // what one work item of the frame sweep leaves for the finalize kernel
  double value;        // sum over its pairs of min(d, clamp)
  long long clamped;   // its clamped pairs
};

struct Layout {
  TileLayout t;
  size_t frames, fres, nframes, unusable, fpart, items, total;
  int ftiles, chunks;
  Layout(int B, int L) : t(B, L) {
    ftiles = (L + TS - 1) / TS;
    chunks = (t.tiles + CHUNK_TILES - 1) / CHUNK_TILES;
    total = t.end;
    frames = take(total, (size_t)B * L * sizeof(FramePair));                        // [b][frame]
    fres = take(total, (size_t)B * L * sizeof(int));                                // [b][frame]: its residue
    nframes = take(total, (size_t)B * sizeof(int));
    unusable = take(total, (size_t)B * sizeof(int));
    fpart = take(total, (size_t)B * ftiles * chunks * 3 * TS * sizeof(float4));     // [b][frame tile][chunk][3][lane]
    items = take(total, (size_t)B * ftiles * chunks * sizeof(Item));                // [b][frame tile][chunk]
  }
};

// ---- the two device functions that prediction and truth share, build_frame and local_coords: csrc/backbone_frame.h
// one pair: d, and (WITH_GRAD) g = Delta / d in the frame's coordinates, 0 for a clamped pair; r = x_pred - t_pred
template <bool WITH_GRAD>
__device__ __forceinline__ float pair_value(const FramePair &f, const Atom8 &a, float clamp, bool &open, float &rx, float &ry,
                                            float &rz, float &g0, float &g1, float &g2) {
  float px, py, pz, tx, ty, tz, ux, uy, uz;
  local_coords(f.p, a.px, a.py, a.pz, rx, ry, rz, px, py, pz);
  local_coords(f.q, a.tx, a.ty, a.tz, ux, uy, uz, tx, ty, tz);
  const float d0 = px - tx, d1 = py - ty, d2 = pz - tz;
  const float q = fmaf(d2, d2, fmaf(d1, d1, d0 * d0)) + D_EPS;
  const float d = __builtin_amdgcn_sqrtf(q);
  open = d < clamp;   // strict: a pair at the clamp is clamped
  if (WITH_GRAD) {
    const float w = open ? __builtin_amdgcn_rsqf(q) : 0.f;
    g0 = d0 * w; g1 = d1 * w; g2 = d2 * w;
  }
  return d;
}

// ---- stage 2: grid B, one wavefront per protein (behind the compaction: natoms and the marked atoms are read here)
__global__ __launch_bounds__(TS) void fape_frames_kernel(const float *__restrict__ pred, const float *__restrict__ truth,
                                                         const int64_t *__restrict__ seq, const Atom8 *__restrict__ atoms,
                                                         const int *__restrict__ natoms, int L, int nstride,
                                                         FramePair *__restrict__ frames, int *__restrict__ fres,
                                                         int *__restrict__ nframes, int *__restrict__ unusable) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t nslot = (size_t)L * PTAMD_NUM_SLOTS;
  pred += (size_t)b * nslot * 3;
  truth += (size_t)b * nslot * 3;
  seq += (size_t)b * L;
  frames += (size_t)b * L;
  fres += (size_t)b * L;
  atoms += (size_t)b * nstride;
  int bad = 0, pos0 = 0;
  for (int r0 = 0; r0 < L; r0 += TS) {
    const int r = r0 + lane;
    FramePair f;
    bool ok = r < L && seq[min(r, L - 1)] != PTAMD_PAD_ID;
    if (ok) {
      const float *tp = truth + (size_t)r * PTAMD_NUM_SLOTS * 3;
      ok = build_frame(tp, f.q);   // (an absent N, CA or C is a NaN: no frame)
    }
    const unsigned long long m = __ballot(ok);
    if (ok) {
      bad |= !build_frame(pred + (size_t)r * PTAMD_NUM_SLOTS * 3, f.p);
      const int pos = pos0 + __popcll(m & ((1ull << lane) - 1ull));
      frames[pos] = f;
      fres[pos] = r;
    }
    pos0 += __popcll(m);
  }
  const int n = natoms[b];
  for (int j = lane; j < n; j += TS) bad |= atoms[j].code & 1;
  const bool any_bad = __ballot(bad != 0) != 0ull;
  if (lane == 0) {
    nframes[b] = pos0;
    unusable[b] = any_bad;
  }
}

// ---- stage 3: the frame side.  grid (ftiles * chunks, B), one wavefront per workgroup = one work item.
template <bool WITH_GRAD>
__global__ __launch_bounds__(TS) void fape_frame_sweep_kernel(const Atom8 *__restrict__ atoms, const int *__restrict__ natoms,
                                                              const FramePair *__restrict__ frames,
                                                              const int *__restrict__ nframes, const int *__restrict__ unusable,
                                                              int nstride, int L, int ftiles, int chunks, float clamp,
                                                              float4 *__restrict__ fpart, Item *__restrict__ items) {
  __shared__ Atom8 s_atom[TS];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int ft = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int n = natoms[b], nf = nframes[b], nT = (n + TS - 1) / TS;
  const int J0 = ch * CHUNK_TILES, J1 = min(nT, J0 + CHUNK_TILES);
  if (unusable[b] || ft * TS >= nf || J0 >= J1) return;   // the finalize kernel skips these items too
  atoms += (size_t)b * nstride;
  const int i = ft * TS + lane;
  const bool live = i < nf;
  FramePair f = {};
  if (live) f = frames[(size_t)b * L + i];
  float G0 = 0.f, G1 = 0.f, G2 = 0.f;
  float M00 = 0.f, M01 = 0.f, M02 = 0.f, M10 = 0.f, M11 = 0.f, M12 = 0.f, M20 = 0.f, M21 = 0.f, M22 = 0.f;
  double value = 0.0;
  int clamped = 0;
  for (int J = J0; J < J1; ++J) {
    const int cnt = min(TS, n - J * TS);   // live atoms of the tile
    {
      const int j = J * TS + lane;
      s_atom[lane] = j < n ? atoms[j] : Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
    }
    __builtin_amdgcn_wave_barrier();
    float vt = 0.f;
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const Atom8 a = s_atom[j];   // broadcast
      bool open;
      float rx, ry, rz, g0 = 0.f, g1 = 0.f, g2 = 0.f;
      const float d = pair_value<WITH_GRAD>(f, a, clamp, open, rx, ry, rz, g0, g1, g2);
      vt += open ? d : clamp;
      clamped += open ? 0 : 1;
      if (WITH_GRAD) {
        G0 += g0; G1 += g1; G2 += g2;
        M00 = fmaf(g0, rx, M00); M01 = fmaf(g0, ry, M01); M02 = fmaf(g0, rz, M02);
        M10 = fmaf(g1, rx, M10); M11 = fmaf(g1, ry, M11); M12 = fmaf(g1, rz, M12);
        M20 = fmaf(g2, rx, M20); M21 = fmaf(g2, ry, M21); M22 = fmaf(g2, rz, M22);
      }
    }
    value += (double)vt;
    __builtin_amdgcn_wave_barrier();   // s_atom is rewritten for the next tile
  }
  const size_t item = ((size_t)b * ftiles + ft) * chunks + ch;
  if (WITH_GRAD) {   // (the lanes behind the last frame leave sums nobody reads)
    float4 *out = fpart + item * 3 * TS + lane;
    out[0] = make_float4(G0, G1, G2, M00);
    out[TS] = make_float4(M01, M02, M10, M11);
    out[2 * TS] = make_float4(M12, M20, M21, M22);
  }
  value = wave_sum_d(live ? value : 0.0);
  clamped = live ? clamped : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) clamped += __shfl_xor(clamped, o, 64);   // (<= 64 * 8 * 64: an int)
  if (lane == 0) items[item] = Item{value, (long long)clamped};
}

// ---- stage 4: the atom side.  grid (tiles, B), one wavefront per atom tile; every present atom's slot of dcrd is written here
__global__ __launch_bounds__(TS) void fape_atom_sweep_kernel(const Atom8 *__restrict__ atoms, const int *__restrict__ natoms,
                                                             const FramePair *__restrict__ frames,
                                                             const int *__restrict__ nframes, const int *__restrict__ unusable,
                                                             int nstride, int L, float clamp, float *__restrict__ dcrd) {
  __shared__ FramePair s_frame[TS];
  const int b = blockIdx.y, lane = threadIdx.x, J = blockIdx.x;
  const int n = natoms[b], nf = nframes[b];
  if (unusable[b] || nf == 0 || J * TS >= n) return;
  frames += (size_t)b * L;
  const int j = J * TS + lane;
  const bool live = j < n;
  Atom8 a = Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, -1, 0};
  if (live) a = atoms[(size_t)b * nstride + j];
  float gx = 0.f, gy = 0.f, gz = 0.f;
  for (int i0 = 0; i0 < nf; i0 += TS) {
    const int cnt = min(TS, nf - i0);
    if (lane < cnt) s_frame[lane] = frames[i0 + lane];
    __builtin_amdgcn_wave_barrier();
#pragma unroll 2
    for (int i = 0; i < cnt; ++i) {
      const FramePair &f = s_frame[i];   // broadcast
      bool open;
      float rx, ry, rz, g0 = 0.f, g1 = 0.f, g2 = 0.f;
      pair_value<true>(f, a, clamp, open, rx, ry, rz, g0, g1, g2);
      gx = fmaf(f.p.e[6], g2, fmaf(f.p.e[3], g1, fmaf(f.p.e[0], g0, gx)));   // R g
      gy = fmaf(f.p.e[7], g2, fmaf(f.p.e[4], g1, fmaf(f.p.e[1], g0, gy)));
      gz = fmaf(f.p.e[8], g2, fmaf(f.p.e[5], g1, fmaf(f.p.e[2], g0, gz)));
    }
    __builtin_amdgcn_wave_barrier();   // s_frame is rewritten for the next tile
  }
  if (!live) return;
  const float scale = (float)(1.0 / (Z_SCALE * (double)nf * (double)n));
  float *out = dcrd + ((size_t)b * L * PTAMD_NUM_SLOTS + a.aux) * 3;
  out[0] = scale * gx;
  out[1] = scale * gy;
  out[2] = scale * gz;
}

// ---- stage 5: grid (ftiles, B), one wavefront per tile of 64 frames.  The first of a protein also sums the protein's work
// items: lane l takes the items l, l + 64, ... of the protein's OWN rectangle (frame tiles and chunks of its own counts, whatever
// L is), then the fixed tree of wave_sum_d.
__global__ __launch_bounds__(TS) void fape_finalize_kernel(const float *__restrict__ pred, const int *__restrict__ natoms,
                                                           const int *__restrict__ nframes, const int *__restrict__ unusable,
                                                           const int *__restrict__ fres, const float4 *__restrict__ fpart,
                                                           const Item *__restrict__ items, int L, int ftiles, int chunks,
                                                           float *__restrict__ stats, long long *__restrict__ npairs,
                                                           long long *__restrict__ nclamped, float *__restrict__ dcrd) {
  const int b = blockIdx.y, lane = threadIdx.x, ft = blockIdx.x;
  const int n = natoms[b], nf = nframes[b], nT = (n + TS - 1) / TS;
  const int nFT = (nf + TS - 1) / TS, nCH = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
  const bool bad = unusable[b] != 0;
  const long long np = (long long)nf * (long long)n;
  if (ft == 0) {
    double v = 0.0;
    long long c = 0;
    if (!bad)
      for (int r = lane; r < nFT * nCH; r += TS) {
        const Item it = items[((size_t)b * ftiles + r / nCH) * chunks + r % nCH];
        v += it.value;
        c += it.clamped;
      }
    v = wave_sum_d(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) {
      const float nan = __builtin_nanf("");
      stats[(size_t)b * 2] = np > 0 && !bad ? (float)(v / (Z_SCALE * (double)np)) : nan;
      stats[(size_t)b * 2 + 1] = np > 0 ? (float)((double)c / (double)np) : nan;
      npairs[b] = np;
      nclamped[b] = c;
    }
  }
  const int i = ft * TS + lane;
  if (dcrd == nullptr || bad || np == 0 || i >= nf) return;
  double s[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) s[k] = 0.0;
  for (int ch = 0; ch < nCH; ++ch) {   // chunk order
    const float4 *in = fpart + (((size_t)b * ftiles + ft) * chunks + ch) * 3 * TS + lane;
    const float4 x = in[0], y = in[TS], z = in[2 * TS];
    s[0] += x.x; s[1] += x.y; s[2] += x.z; s[3] += x.w;
    s[4] += y.x; s[5] += y.y; s[6] += y.z; s[7] += y.w;
    s[8] += z.x; s[9] += z.y; s[10] += z.z; s[11] += z.w;
  }
  // G = s[0..3): d/d(x_local) summed over the atoms; rows of M = s[3..12): d/d(e1), d/d(e2), d/d(e3)
  const int res = fres[(size_t)b * L + i];
  float *out = dcrd + ((size_t)b * L + res) * PTAMD_NUM_SLOTS * 3;
  const float *p = pred + ((size_t)b * L + res) * PTAMD_NUM_SLOTS * 3;
  // algorithm 21 once more, keeping its intermediates
  const double v1x = (double)p[6] - p[3], v1y = (double)p[7] - p[4], v1z = (double)p[8] - p[5];
  const double v2x = (double)p[0] - p[3], v2y = (double)p[1] - p[4], v2z = (double)p[2] - p[5];
  const double i1 = 1.0 / sqrt(v1x * v1x + v1y * v1y + v1z * v1z);
  const double e1x = v1x * i1, e1y = v1y * i1, e1z = v1z * i1;
  const double sp = e1x * v2x + e1y * v2y + e1z * v2z;
  const double ux = v2x - e1x * sp, uy = v2y - e1y * sp, uz = v2z - e1z * sp;
  const double i2 = 1.0 / sqrt(ux * ux + uy * uy + uz * uz);
  const double e2x = ux * i2, e2y = uy * i2, e2z = uz * i2;
  const double e3x = e1y * e2z - e1z * e2y, e3y = e1z * e2x - e1x * e2z, e3z = e1x * e2y - e1y * e2x;
  // x_local = R^T (x - t): d/dt = -R G
  const double dtx = -(e1x * s[0] + e2x * s[1] + e3x * s[2]);
  const double dty = -(e1y * s[0] + e2y * s[1] + e3y * s[2]);
  const double dtz = -(e1z * s[0] + e2z * s[1] + e3z * s[2]);
  // e3 = e1 x e2: d/de1 += e2 x dE3, d/de2 += dE3 x e1
  double a1x = s[3] + (e2y * s[11] - e2z * s[10]), a1y = s[4] + (e2z * s[9] - e2x * s[11]), a1z = s[5] + (e2x * s[10] - e2y * s[9]);
  const double a2x = s[6] + (s[10] * e1z - s[11] * e1y), a2y = s[7] + (s[11] * e1x - s[9] * e1z), a2z = s[8] + (s[9] * e1y - s[10] * e1x);
  // e2 = u2 / |u2|
  const double k2 = e2x * a2x + e2y * a2y + e2z * a2z;
  const double dux = (a2x - e2x * k2) * i2, duy = (a2y - e2y * k2) * i2, duz = (a2z - e2z * k2) * i2;
  // u2 = v2 - e1 (e1 . v2)
  const double k1 = e1x * dux + e1y * duy + e1z * duz;
  const double dv2x = dux - e1x * k1, dv2y = duy - e1y * k1, dv2z = duz - e1z * k1;
  a1x -= sp * dux + k1 * v2x; a1y -= sp * duy + k1 * v2y; a1z -= sp * duz + k1 * v2z;
  // e1 = v1 / |v1|
  const double k0 = e1x * a1x + e1y * a1y + e1z * a1z;
  const double dv1x = (a1x - e1x * k0) * i1, dv1y = (a1y - e1y * k0) * i1, dv1z = (a1z - e1z * k0) * i1;
  // v1 = C - CA, v2 = N - CA, t = CA
  const double scale = 1.0 / (Z_SCALE * (double)np);
  out[0] += (float)(scale * dv2x); out[1] += (float)(scale * dv2y); out[2] += (float)(scale * dv2z);
  out[3] += (float)(scale * (dtx - dv1x - dv2x)); out[4] += (float)(scale * (dty - dv1y - dv2y)); out[5] += (float)(scale * (dtz - dv1z - dv2z));
  out[6] += (float)(scale * dv1x); out[7] += (float)(scale * dv1y); out[8] += (float)(scale * dv1z);
}

}  // namespace

extern "C" {

size_t ptamd_fape_workspace_bytes(int B, int L) {
  if (!tile_shape_ok(B, L)) return 0;
  return Layout(B, L).total;
}

int ptamd_fape_fwd_bwd(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float clamp, float *stats,
                       int64_t *npairs, int64_t *nclamped, float *dcrd, void *workspace, size_t workspace_bytes, void *stream) {
  if (!tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !stats || !npairs || !nclamped) return PTAMD_ERR_BAD_SHAPE;
  if (!(clamp > 0.f)) return PTAMD_ERR_BAD_SHAPE;   // (NaN fails; +inf = unclamped)
  const Layout l(B, L);
  if (!workspace || workspace_bytes < l.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  if ((size_t)l.ftiles * l.chunks > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;   // (a grid dimension; its workspace is beyond any device)
  char *ws = static_cast<char *>(workspace);
  Atom8 *atoms = reinterpret_cast<Atom8 *>(ws + l.t.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.t.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.t.natoms);
  FramePair *frames = reinterpret_cast<FramePair *>(ws + l.frames);
  int *fres = reinterpret_cast<int *>(ws + l.fres), *nframes = reinterpret_cast<int *>(ws + l.nframes);
  int *unusable = reinterpret_cast<int *>(ws + l.unusable);
  float4 *fpart = reinterpret_cast<float4 *>(ws + l.fpart);
  Item *items = reinterpret_cast<Item *>(ws + l.items);
  hipStream_t st = (hipStream_t)stream;
  if (dcrd) PT_HIP_TRY(hipMemsetAsync(dcrd, 0, (size_t)B * L * PTAMD_NUM_SLOTS * 3 * sizeof(float), st));   // absent slots stay 0
  hipLaunchKernelGGL(compact_kernel<SlotRecord>, dim3(B), dim3(COMPACT_THREADS), 0, st, pred_crd, true_crd, seq, L, l.t.nstride, l.t.tiles,
                     atoms, boxes, natoms);
  int rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(fape_frames_kernel, dim3(B), dim3(TS), 0, st, pred_crd, true_crd, seq, atoms, natoms, L, l.t.nstride, frames, fres,
                     nframes, unusable);
  rc = pt_check_launch();
  if (rc) return rc;
  auto sweep = dcrd ? fape_frame_sweep_kernel<true> : fape_frame_sweep_kernel<false>;
  hipLaunchKernelGGL(sweep, dim3((unsigned)(l.ftiles * l.chunks), B), dim3(TS), 0, st, atoms, natoms, frames, nframes, unusable,
                     l.t.nstride, L, l.ftiles, l.chunks, clamp, fpart, items);
  rc = pt_check_launch();
  if (rc) return rc;
  if (dcrd) {
    hipLaunchKernelGGL(fape_atom_sweep_kernel, dim3((unsigned)l.t.tiles, B), dim3(TS), 0, st, atoms, natoms, frames, nframes, unusable,
                       l.t.nstride, L, clamp, dcrd);
    rc = pt_check_launch();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(fape_finalize_kernel, dim3(dcrd ? (unsigned)l.ftiles : 1u, B), dim3(TS), 0, st, pred_crd, natoms, nframes, unusable,
                     fres, fpart, items, L, l.ftiles, l.chunks, stats, reinterpret_cast<long long *>(npairs),
                     reinterpret_cast<long long *>(nclamped), dcrd);
  return pt_check_launch();
}

}  // extern "C"
