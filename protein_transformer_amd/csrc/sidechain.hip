// Side-chain accuracy for a whole batch on gfx950: the share of correct rotamers (chi1, chi1+2), the mean chi error and the
// side-chain RMSD in each residue's own backbone frame - `eval_metrics.sidechain_batch` and the scorer
// `python -m protein_transformer_amd.score`.
//
// The reference (protein_transformer) has no counterpart.  The chi angles are those of the IUPAC-IUB Commission on Biochemical
// Nomenclature, "Abbreviations and symbols for the description of the conformation of polypeptide chains", Biochemistry
// 9:3471-3479 (1970); the frame is algorithm 21 of Jumper et al. (csrc/backbone_frame.h, shared with csrc/fape.hip).  The
// definition is in include/ptamd.h; this file restates only what the kernels do with it.
//
// Two launches per batch:
//   residues  one wavefront per 64 consecutive residues of one protein.  Their 64 x 42 floats are one contiguous piece of each
//             coordinate array: the wavefront copies both pieces to LDS with 8-byte loads, lane l taking the pair l, l + 64, ...
//             of the piece - every load instruction reads 512 consecutive bytes - where a lane per residue would read rows 168
//             bytes apart.  In LDS a residue's row is 43 words long, so lane = residue reads its atoms free of bank conflicts.
//             Then one lane per residue: the chain N, CA, CB, atoms 5 .. 8 gives chi1 .. chi4 through ONE device function for
//             prediction and truth (a prediction equal to the truth has Delta == 0 exactly); which chi are scored, and whether
//             the residue spans a frame, is decided in fp64 on the truth; the side-chain atoms go through local_coords of both
//             frames.  per_res is written by the lane; the tile's counts (popcounts of ballots, summed integers) and its two
//             fp64 sums (the fixed tree of wave_sum_d) go to the workspace.  Every tile of the grid writes its partial - a tile
//             of pad residues writes zeros - so nothing the workspace held before the call is ever read.
//   finalize  one wavefront per protein: lane l adds the partials of tiles l, l + 64, ... in that order, then the fixed tree;
//             a tile of pad residues adds +0.0 and 0, so the bits do not depend on how far the row is padded.
// No atomics, wavefronts share nothing: two runs give the same bits, and a protein's bits do not depend on the batch around it.
#include <math.h>

#include "atom_tiles.h"
#include "backbone_frame.h"

namespace {

using atom_tiles::take;
using namespace backbone_frame;

constexpr int TS = 64;                            // residues per tile = lanes of a wavefront
constexpr int ROW = PTAMD_NUM_SLOTS * 3;          // floats of a residue in memory
constexpr int ROW_LDS = ROW + 1;                  // ... and in LDS: an odd stride, lane = residue hits 32 different banks
constexpr int CHAIN = 7;                          // N, CA, CB, side-chain atoms 1 .. 4: slots 0, 1, 4 .. 8
constexpr float DEG = 57.29577951308232f;
constexpr float PI_F = 3.14159265358979323846f;

constexpr int NRES = 20;
// chi angles per residue type, ACDEFGHIKLMNPQRSTVWY; the chi whose far atoms are interchangeable (ASP chi2, GLU chi3, PHE chi2,
// TYR chi2; 0 = none)
const int h_nchi[NRES] = {0, 1, 2, 3, 2, 0, 2, 2, 4, 2, 3, 2, 2, 3, 4, 1, 1, 1, 2, 2};
const int h_sym_chi[NRES] = {0, 0, 2, 3, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2};
// per residue type one word for the kernel: bits 0..3 = side-chain atoms (csrc/nerf_tables.h through ptamd_sidechain_atoms),
// bits 4..6 = chi angles, bits 8..10 = the symmetric chi
struct ResidueTable {
  unsigned info[NRES];
};
// false if a type has a chi angle without the atom that closes it (chi_k ends on side-chain atom k + 1): a build error, not an input
bool make_table(ResidueTable &t) {
  for (int r = 0; r < NRES; ++r) {
    const int nsc = ptamd_sidechain_atoms(r);
    if (nsc < 0 || nsc > 15 || (h_nchi[r] > 0 && nsc < h_nchi[r] + 1)) return false;
    t.info[r] = (unsigned)nsc | (unsigned)h_nchi[r] << 4 | (unsigned)h_sym_chi[r] << 8;
  }
  return true;
}

// the slot that trades places with slot s in the other naming of a symmetric side chain (s itself elsewhere): ASP OD1/OD2,
// GLU OE1/OE2, PHE and TYR CD1/CD2 and CE1/CE2 - the pairs of losses.SYMMETRIC_SWAPS
__device__ __forceinline__ int swap_partner(int type, int s) {
  if (type == 2) return s == 6 || s == 7 ? 13 - s : s;
  if (type == 3) return s == 7 || s == 8 ? 15 - s : s;
  if (type == 4) return s == 6 || s == 7 || s == 9 || s == 10 ? 16 - s : s;
  if (type == 19) return s == 6 || s == 7 || s == 10 || s == 11 ? 17 - s : s;
  return s;
}

struct __attribute__((aligned(16))) Partial {   // what a tile leaves for the finalize kernel
  double sum_delta, sum_d2;                     // degrees over its scored chi; A^2 over its counted residues
  int c[12];                                    // the layout of `counts`
  int bad, pad[3];
};

struct ScLayout {
  size_t part, end;
  int words;   // tiles per protein
  ScLayout(int B, int L) {
    words = (L + TS - 1) / TS;
    end = 0;
    part = take(end, (size_t)B * words * sizeof(Partial));
  }
};

// chi1 .. chi4 of the chain N, CA, CB, atoms 5 .. 8 of one residue row: bonds v_i = P_i+1 - P_i, normals m_i = v_i x v_i+1,
// chi_k = atan2(|v_k| v_k-1 . m_k, m_k-1 . m_k) - the b1, b2, b3, n1, n2 of the definition with b2 = v_k.  fp32.  Not inlined:
// prediction and truth run the same instructions, whatever the compiler contracts.
__device__ __noinline__ float4 chain_chi(const float *__restrict__ row) {
  float p[CHAIN][3], v[CHAIN - 1][3], m[CHAIN - 2][3], chi[4];
#pragma unroll
  for (int i = 0; i < CHAIN; ++i) {
    const int s = i < 2 ? i : i + 2;
#pragma unroll
    for (int d = 0; d < 3; ++d) p[i][d] = row[s * 3 + d];
  }
#pragma unroll
  for (int i = 0; i < CHAIN - 1; ++i) {
#pragma unroll
    for (int d = 0; d < 3; ++d) v[i][d] = p[i + 1][d] - p[i][d];
  }
#pragma unroll
  for (int i = 0; i < CHAIN - 2; ++i) {
    m[i][0] = v[i][1] * v[i + 1][2] - v[i][2] * v[i + 1][1];
    m[i][1] = v[i][2] * v[i + 1][0] - v[i][0] * v[i + 1][2];
    m[i][2] = v[i][0] * v[i + 1][1] - v[i][1] * v[i + 1][0];
  }
#pragma unroll
  for (int k = 1; k <= 4; ++k) {
    const float len = sqrtf(v[k][0] * v[k][0] + v[k][1] * v[k][1] + v[k][2] * v[k][2]);
    const float y = len * (v[k - 1][0] * m[k][0] + v[k - 1][1] * m[k][1] + v[k - 1][2] * m[k][2]);
    const float x = m[k - 1][0] * m[k][0] + m[k - 1][1] * m[k][1] + m[k - 1][2] * m[k][2];
    chi[k - 1] = atan2f(y, x);
  }
  return make_float4(chi[0], chi[1], chi[2], chi[3]);
}

// |m_i|^2, i = 0 .. 4, of the same chain in fp64 on the fp32 coordinates: chi_k is scored when q[k-1] and q[k] both exceed 1e-8
// (an absent atom is a NaN and fails the test of both normals it enters)
__device__ __forceinline__ void chain_normals_d(const float *__restrict__ row, double q[CHAIN - 2]) {
  double v[CHAIN - 1][3];
#pragma unroll
  for (int i = 0; i < CHAIN - 1; ++i) {
    const int s0 = i < 2 ? i : i + 2, s1 = i + 1 < 2 ? i + 1 : i + 3;
#pragma unroll
    for (int d = 0; d < 3; ++d) v[i][d] = (double)row[s1 * 3 + d] - (double)row[s0 * 3 + d];
  }
#pragma unroll
  for (int i = 0; i < CHAIN - 2; ++i) {
    const double x = v[i][1] * v[i + 1][2] - v[i][2] * v[i + 1][1], y = v[i][2] * v[i + 1][0] - v[i][0] * v[i + 1][2],
                 z = v[i][0] * v[i + 1][1] - v[i][1] * v[i + 1][0];
    q[i] = x * x + y * y + z * z;
  }
}

__device__ __forceinline__ bool finite3(const float *__restrict__ a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

// ---- stage 1: one wavefront per tile of 64 residues; tile t = protein * words + tile of the protein
__global__ __launch_bounds__(TS) void sidechain_residues_kernel(const float *__restrict__ pred, const float *__restrict__ truth,
                                                                const int64_t *__restrict__ seq, int L, int words,
                                                                unsigned long long ntiles, float threshold, ResidueTable tab,
                                                                float *__restrict__ per_res, Partial *__restrict__ part) {
  __shared__ float s_crd[2][TS * ROW_LDS];
  __shared__ unsigned s_info[NRES];
  const int lane = threadIdx.x;
  if (lane < NRES) s_info[lane] = tab.info[lane];
  const float nan = __builtin_nanf("");
  for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t b = (size_t)(t / words);
    const int r0 = (int)(t % words) * TS, n = min(TS, L - r0);
    // the n rows of the tile are n * 42 consecutive floats, from an even float index: n * 21 aligned pairs
    const size_t base = (b * L + r0) * ROW;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float2 *src = reinterpret_cast<const float2 *>((s == 0 ? pred : truth) + base);
      for (int j = lane; j < n * (ROW / 2); j += TS) {
        const float2 x = src[j];
        const int f = 2 * j, res = f / ROW, k = f - res * ROW;   // (k is even: both floats belong to the same row)
        s_crd[s][res * ROW_LDS + k] = x.x;
        s_crd[s][res * ROW_LDS + k + 1] = x.y;
      }
    }
    __syncthreads();   // (a workgroup of one wavefront: the barrier is its fence on the LDS writes above)
    const int r = r0 + lane;
    int type = -1;
    if (lane < n) {
      const int64_t id = seq[b * L + r];
      if (id >= 0 && id < 20) type = (int)id;   // pad and unknown ids take no part
    }
    const float *rp = &s_crd[0][lane * ROW_LDS], *rt = &s_crd[1][lane * ROW_LDS];
    const unsigned info = type >= 0 ? s_info[type] : 0u;
    const int nsc = (int)(info & 15u), nchi = (int)(info >> 4 & 7u), sym = (int)(info >> 8 & 7u);
    bool bad = false;
    // ---- chi
    float delta[4] = {nan, nan, nan, nan};
    bool scored[4] = {false, false, false, false}, hit[4] = {false, false, false, false};
    if (nchi > 0) {
      double q[CHAIN - 2];
      chain_normals_d(rt, q);
      const float4 cp = chain_chi(rp), ct = chain_chi(rt);
      const float xp[4] = {cp.x, cp.y, cp.z, cp.w}, xt[4] = {ct.x, ct.y, ct.z, ct.w};
#pragma unroll
      for (int k = 1; k <= 4; ++k) {
        if (k <= nchi && q[k - 1] > DEGENERATE && q[k] > DEGENERATE) {
          scored[k - 1] = true;
          // its four predicted atoms: chain points k-1 .. k+2
          bool fin = true;
#pragma unroll
          for (int i = k - 1; i <= k + 2; ++i) fin = fin && finite3(rp + (i < 2 ? i : i + 2) * 3);
          bad = bad || !fin;
          float d = fabsf(xp[k - 1] - xt[k - 1]);
          d = d > PI_F ? 2.0f * PI_F - d : d;
          d *= DEG;
          if (k == sym) d = fminf(d, 180.0f - d);
          if (!fin) d = nan;   // (an infinite coordinate can leave atan2f a finite value)
          delta[k - 1] = d;
          hit[k - 1] = d <= threshold;   // (a NaN is no hit)
        }
      }
    }
    // ---- the side chain in the residue's own frame
    float rms = nan, d2 = 0.f;
    bool counted = false;
    if (nsc > 0) {
      Frame ft, fp;
      counted = build_frame(rt, ft);   // (an absent N, CA or C is a NaN: no frame)
      for (int k = 0; k < nsc; ++k) counted = counted && !(isnan(rt[(4 + k) * 3]) || isnan(rt[(4 + k) * 3 + 1]) || isnan(rt[(4 + k) * 3 + 2]));
      if (counted) {
        bool ok = build_frame(rp, fp);
        ok = ok && finite3(rp) && finite3(rp + 3) && finite3(rp + 6);
        float plain = 0.f, other = 0.f;
        for (int k = 0; k < nsc; ++k) {
          const int s = 4 + k, s2 = swap_partner(type, s);
          float ux, uy, uz, tx, ty, tz, px, py, pz, ox, oy, oz;
          ok = ok && finite3(rp + s * 3);
          local_coords(ft, rt[s * 3], rt[s * 3 + 1], rt[s * 3 + 2], ux, uy, uz, tx, ty, tz);
          local_coords(fp, rp[s * 3], rp[s * 3 + 1], rp[s * 3 + 2], ux, uy, uz, px, py, pz);
          local_coords(fp, rp[s2 * 3], rp[s2 * 3 + 1], rp[s2 * 3 + 2], ux, uy, uz, ox, oy, oz);
          const float a0 = px - tx, a1 = py - ty, a2 = pz - tz, b0 = ox - tx, b1 = oy - ty, b2 = oz - tz;
          plain += fmaf(a2, a2, fmaf(a1, a1, a0 * a0));
          other += fmaf(b2, b2, fmaf(b1, b1, b0 * b0));
        }
        bad = bad || !ok;
        d2 = ok ? fminf(plain, other) : nan;   // (non-symmetric types: other == plain)
        rms = ok ? sqrtf(d2 / (float)nsc) : nan;
      }
    }
    if (per_res && lane < n) {
      float *out = per_res + (b * L + r) * 5;
      out[0] = delta[0]; out[1] = delta[1]; out[2] = delta[2]; out[3] = delta[3];
      out[4] = rms;
    }
    // ---- the tile's partial
    double dsum = 0.0;   // every Delta enters the fp64 sum as it is
#pragma unroll
    for (int k = 0; k < 4; ++k) dsum += scored[k] ? (double)delta[k] : 0.0;   // (NaN only in a protein that has no scores)
    const double sum_delta = wave_sum_d(dsum);
    const double sum_d2 = wave_sum_d(counted ? (double)d2 : 0.0);
    int c[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      c[2 * k] = __popcll(__ballot(scored[k]));
      c[2 * k + 1] = __popcll(__ballot(hit[k]));
    }
    c[8] = __popcll(__ballot(scored[0] && scored[1]));
    c[9] = __popcll(__ballot(scored[0] && scored[1] && hit[0] && hit[1]));
    c[10] = __popcll(__ballot(counted));
    int atoms = counted ? nsc : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) atoms += __shfl_xor(atoms, o, 64);
    c[11] = atoms;
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) {
      Partial p;
      p.sum_delta = sum_delta;
      p.sum_d2 = sum_d2;
#pragma unroll
      for (int k = 0; k < 12; ++k) p.c[k] = c[k];
      p.bad = any_bad ? 1 : 0;
      p.pad[0] = p.pad[1] = p.pad[2] = 0;
      part[t] = p;
    }
    __syncthreads();   // s_crd is rewritten for the next tile
  }
}

// ---- stage 2: one wavefront per protein
__global__ __launch_bounds__(TS) void sidechain_finalize_kernel(const Partial *__restrict__ part, int words, float *__restrict__ score,
                                                                int32_t *__restrict__ counts) {
  const int b = blockIdx.x, lane = threadIdx.x;
  part += (size_t)b * words;
  double sd = 0.0, s2 = 0.0;
  int c[12], bad = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) c[k] = 0;
  for (int t = lane; t < words; t += TS) {   // tile order within the lane, then the fixed tree
    const Partial p = part[t];
    sd += p.sum_delta;
    s2 += p.sum_d2;
    bad |= p.bad;
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] += p.c[k];
  }
  sd = wave_sum_d(sd);
  s2 = wave_sum_d(s2);
#pragma unroll
  for (int k = 0; k < 12; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
  }
  const bool any_bad = __ballot(bad != 0) != 0ull;
  if (lane == 0) {
    const float nan = __builtin_nanf("");
    const int nscored = c[0] + c[2] + c[4] + c[6];
    float *s = score + (size_t)b * 4;
    s[0] = any_bad || c[0] == 0 ? nan : (float)((double)c[1] / (double)c[0]);
    s[1] = any_bad || c[8] == 0 ? nan : (float)((double)c[9] / (double)c[8]);
    s[2] = any_bad || nscored == 0 ? nan : (float)(sd / (double)nscored);
    s[3] = any_bad || c[11] == 0 ? nan : (float)sqrt(s2 / (double)c[11]);
#pragma unroll
    for (int k = 0; k < 12; ++k) counts[(size_t)b * 12 + k] = any_bad && (k == 9 || (k < 8 && (k & 1))) ? 0 : c[k];
  }
}

inline unsigned grid_for(unsigned long long items) {
  return (unsigned)(items < 0x7fffffffull ? items : 0x7fffffffull);   // the kernel strides over what a grid cannot hold
}

}  // namespace

extern "C" {

size_t ptamd_sidechain_workspace_bytes(int B, int L) {
  if (!atom_tiles::tile_shape_ok(B, L)) return 0;
  return ScLayout(B, L).end;
}

int ptamd_sidechain(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float threshold_deg, float *score,
                    int32_t *counts, float *per_res, void *workspace, size_t workspace_bytes, void *stream) {
  if (!atom_tiles::tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !score || !counts) return PTAMD_ERR_BAD_SHAPE;
  if (!(threshold_deg >= 0.f) || isinf(threshold_deg)) return PTAMD_ERR_BAD_SHAPE;   // (NaN fails the first test)
  ResidueTable tab;
  if (!make_table(tab)) return PTAMD_ERR_BAD_SHAPE;
  const ScLayout l(B, L);
  if (!workspace || workspace_bytes < l.end) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  // the staging loop reads the coordinates as pairs of floats
  if (((reinterpret_cast<uintptr_t>(pred_crd) | reinterpret_cast<uintptr_t>(true_crd)) & 7u) != 0) return PTAMD_ERR_ALIGN;
  Partial *part = reinterpret_cast<Partial *>(static_cast<char *>(workspace) + l.part);
  hipStream_t st = (hipStream_t)stream;
  const unsigned long long ntiles = (unsigned long long)B * l.words;
  hipLaunchKernelGGL(sidechain_residues_kernel, dim3(grid_for(ntiles)), dim3(TS), 0, st, pred_crd, true_crd, seq, L, l.words, ntiles,
                     threshold_deg, tab, per_res, part);
  const int rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(sidechain_finalize_kernel, dim3(B), dim3(TS), 0, st, part, l.words, score, counts);
  return pt_check_launch();
}

}  // extern "C"
