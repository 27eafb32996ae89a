// Superposed per-residue spread of K structures around a reference, for gfx950: what `ensemble.predict_ensemble` and
// `python -m protein_transformer_amd.predict` turn K dropout passes of a model into.
//
// The reference (protein_transformer) has no counterpart.  csrc/kabsch.hip returns one RMSD per pair and csrc/tmscore.hip fits by
// TM-score; this file returns what each residue does after the least-squares fit of every sample on the reference.  The
// definition - presence, usable samples, the two columns of rmsf, the NaN cases - is in include/ptamd.h; this file restates only
// what the kernels do with it.
//
// Two launches per batch:
//   fit    ONE WAVEFRONT PER (protein, sample).  Lane l owns residues l, l + 64, ...: it sums the 15 moments of the present
//          (sample, reference) C-alpha pairs in fp64, a butterfly (wave_sum_d) leaves the same bits in every lane, every lane
//          solves for the proper rotation (csrc/tm_rotation.h: a quaternion, so a mirror image is never fitted by a reflection),
//          (R, t) is rounded to fp32 once, and the same lanes walk the C-alphas again for the residual.  Leaves rmsd[b,k] and a
//          64-byte record (R, t, usable) in the workspace.  A C-alpha is 12 bytes of a 168-byte row: read where it lies, as
//          csrc/tmscore.hip reads it.
//   rmsf   ONE WAVEFRONT PER TILE OF 64 RESIDUES of a protein.  The tile's rows of the reference, then of one usable sample after
//          the other, are staged in LDS with coalesced reads (42 floats per residue, consecutive lanes on consecutive floats; an
//          odd row stride of 43 floats in LDS, so that lane = residue hits 32 different banks); lane = residue applies that
//          sample's (R, t) to its atoms in slot order and adds the sample's term to two fp64 sums.  The first tile of a protein
//          also writes usable[b].
// A sample's deviation is |R s + t - r|^2 in fp32 under the fp32 (R, t) of its record - the same device function in both
// launches, so rmsd and rmsf describe one fit -; sums over atoms are fp32 in slot order, sums over residues and over samples are
// fp64 in a fixed order.  No atomics, no order-dependent reduction: two runs give the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "tm_rotation.h"

namespace {

using tm_rotation::NMOM;

constexpr int CA_SLOT = 1;                        // the C-alpha of a residue (csrc/lddt.hip)
constexpr int TS = 64;                            // residues per tile = lanes of a wavefront
constexpr int ROW = PTAMD_NUM_SLOTS * 3;          // floats of a residue in memory
constexpr int ROW_LDS = ROW + 1;                  // ... and in LDS (csrc/sidechain.hip)
constexpr int NRES = 20;

struct __attribute__((aligned(16))) Fit {   // 64 bytes per (protein, sample)
  float x[12];                              // R row-major, then t: R s + t lies on the reference
  int usable, n;
  int pad[2];
};

// side-chain atoms per residue type (csrc/nerf_tables.h through ptamd_sidechain_atoms), four bits each: types 0..15 in lo,
// 16..19 in hi - a kernel argument that a lane indexes by its own residue type with a shift
struct NscBits {
  unsigned long long lo, hi;
};
// false if a type has more side-chain atoms than the slots hold: a build error, not an input
bool make_nsc(NscBits &t) {
  t.lo = t.hi = 0ull;
  for (int r = 0; r < NRES; ++r) {
    const int nsc = ptamd_sidechain_atoms(r);
    if (nsc < 0 || 4 + nsc > PTAMD_NUM_SLOTS) return false;
    (r < 16 ? t.lo : t.hi) |= (unsigned long long)nsc << (4 * (r & 15));
  }
  return true;
}

inline int tiles_of(int L) { return (L + TS - 1) / TS; }
inline bool ens_shape_ok(int B, int K, int L) {
  return B > 0 && K > 0 && L > 0 && L <= INT_MAX / 28 && (int64_t)B * K <= INT_MAX && (int64_t)B * tiles_of(L) <= INT_MAX;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// |R s + t - r|^2 in fp32
__device__ __forceinline__ float deviation2(const float (&x)[12], float sx, float sy, float sz, float rx, float ry, float rz) {
  const float ex = fmaf(x[0], sx, fmaf(x[1], sy, fmaf(x[2], sz, x[9]))) - rx;
  const float ey = fmaf(x[3], sx, fmaf(x[4], sy, fmaf(x[5], sz, x[10]))) - ry;
  const float ez = fmaf(x[6], sx, fmaf(x[7], sy, fmaf(x[8], sz, x[11]))) - rz;
  return fmaf(ex, ex, fmaf(ey, ey, ez * ez));
}

// ---- launch 1
__global__ __launch_bounds__(64) void ens_fit_kernel(const float *__restrict__ ref, const float *__restrict__ samples,
                                                     const int64_t *__restrict__ seq, int K, int L, Fit *__restrict__ fit,
                                                     float *__restrict__ rmsd) {
  const int bk = blockIdx.x, b = bk / K, lane = threadIdx.x;
  const size_t nslot = (size_t)L * PTAMD_NUM_SLOTS;
  ref += (size_t)b * nslot * 3;
  samples += (size_t)bk * nslot * 3;
  seq += (size_t)b * L;
  double m[NMOM];
#pragma unroll
  for (int k = 0; k < NMOM; ++k) m[k] = 0.0;
  int n = 0;   // (wavefront-uniform)
  bool bad = false;
  for (int r0 = 0; r0 < L; r0 += 64) {
    const int r = r0 + lane;
    bool present = false;
    if (r < L) {
      const int64_t type = seq[r];
      present = type >= 0 && type < NRES;
    }
    if (present) {
      const size_t at = ((size_t)r * PTAMD_NUM_SLOTS + CA_SLOT) * 3;
      const float p[3] = {samples[at], samples[at + 1], samples[at + 2]}, q[3] = {ref[at], ref[at + 1], ref[at + 2]};
      bad = bad || !(finite3(p[0], p[1], p[2]) && finite3(q[0], q[1], q[2]));
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        m[u] += (double)p[u];
        m[3 + u] += (double)q[u];
#pragma unroll
        for (int v = 0; v < 3; ++v) m[6 + 3 * u + v] = fma((double)p[u], (double)q[v], m[6 + 3 * u + v]);
      }
    }
    n += __popcll(__ballot(present));
  }
  const bool usable = n >= 3 && __ballot(bad) == 0ull;   // (wavefront-uniform)
  float xf[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) xf[k] = __builtin_nanf("");
  double ss = 0.0;
  if (usable) {
#pragma unroll
    for (int k = 0; k < NMOM; ++k) m[k] = wave_sum_d(m[k]);
    double x[12];
    tm_rotation::solve(m, n, x);
#pragma unroll
    for (int k = 0; k < 12; ++k) xf[k] = (float)x[k];
    for (int r = lane; r < L; r += 64) {
      const int64_t type = seq[r];
      if (type >= 0 && type < NRES) {
        const size_t at = ((size_t)r * PTAMD_NUM_SLOTS + CA_SLOT) * 3;
        ss += (double)deviation2(xf, samples[at], samples[at + 1], samples[at + 2], ref[at], ref[at + 1], ref[at + 2]);
      }
    }
    ss = wave_sum_d(ss);
  }
  if (lane == 0) {
    Fit out;
#pragma unroll
    for (int k = 0; k < 12; ++k) out.x[k] = xf[k];
    out.usable = usable ? 1 : 0;
    out.n = n;
    out.pad[0] = out.pad[1] = 0;
    fit[bk] = out;
    rmsd[bk] = usable ? (float)sqrt(ss / (double)n) : __builtin_nanf("");
  }
}

// ---- launch 2
// nfl floats of whole rows, from memory to LDS rows of ROW_LDS floats: element e of row e / ROW lands at e + e / ROW
__device__ __forceinline__ void stage_rows(float *__restrict__ dst, const float *__restrict__ src, int nfl, int lane) {
  for (int e = lane; e < nfl; e += 64) dst[e + e / ROW] = src[e];
}

__global__ __launch_bounds__(64) void ens_rmsf_kernel(const float *__restrict__ ref, const float *__restrict__ samples,
                                                      const int64_t *__restrict__ seq, NscBits nsc, int K, int L, int tiles,
                                                      const Fit *__restrict__ fit, float *__restrict__ rmsf,
                                                      int32_t *__restrict__ usable) {
  __shared__ float s_ref[TS * ROW_LDS], s_smp[TS * ROW_LDS];
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles, lane = threadIdx.x;
  const int r0 = tile * TS, rows = min(TS, L - r0), i = r0 + lane;
  stage_rows(s_ref, ref + ((size_t)b * L + r0) * ROW, rows * ROW, lane);
  int natoms = 0;   // 0: the residue is absent
  if (i < L) {
    const int64_t type = seq[(size_t)b * L + i];
    if (type >= 0 && type < NRES) natoms = 4 + (int)(((type < 16 ? nsc.lo : nsc.hi) >> (4 * ((int)type & 15))) & 15ull);
  }
  const float *mine = s_smp + lane * ROW_LDS, *mine_ref = s_ref + lane * ROW_LDS;
  double acc_ca = 0.0, acc_all = 0.0;
  int kused = 0;   // (uniform over the workgroup: a record is per (protein, sample))
  for (int k = 0; k < K; ++k) {
    const Fit *f = fit + (size_t)b * K + k;
    if (f->usable == 0) continue;
    ++kused;
    float x[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) x[j] = f->x[j];
    __syncthreads();   // the reference rows are staged; the previous sample's rows have been read
    stage_rows(s_smp, samples + (((size_t)b * K + k) * L + r0) * ROW, rows * ROW, lane);
    __syncthreads();
    if (natoms > 0) {
      float sum = 0.f, ca = 0.f;
      int cnt = 0;
#pragma unroll
      for (int a = 0; a < PTAMD_NUM_SLOTS; ++a) {
        if (a < natoms) {
          const float sx = mine[3 * a], sy = mine[3 * a + 1], sz = mine[3 * a + 2];
          const float rx = mine_ref[3 * a], ry = mine_ref[3 * a + 1], rz = mine_ref[3 * a + 2];
          const float d2 = deviation2(x, sx, sy, sz, rx, ry, rz);
          if (finite3(sx, sy, sz) && finite3(rx, ry, rz)) {
            sum += d2;
            ++cnt;
          }
          if (a == CA_SLOT) ca = d2;
        }
      }
      acc_ca += (double)ca;
      acc_all += (double)sum / (double)cnt;   // no atom left: 0 / 0, and the all-atom value is NaN (include/ptamd.h)
    }
  }
  if (i < L) {
    const bool defined = natoms > 0 && kused > 0;
    float *out = rmsf + ((size_t)b * L + i) * 2;
    out[0] = defined ? (float)sqrt(acc_ca / (double)kused) : __builtin_nanf("");
    out[1] = defined ? (float)sqrt(acc_all / (double)kused) : __builtin_nanf("");
  }
  if (tile == 0 && lane == 0) usable[b] = kused;
}

}  // namespace

extern "C" {

size_t ptamd_ensemble_workspace_bytes(int B, int K, int L) {
  if (!ens_shape_ok(B, K, L)) return 0;
  return (size_t)B * K * sizeof(Fit);
}

int ptamd_ensemble_spread(const float *ref_crd, const float *sample_crd, const int64_t *seq, int B, int K, int L, float *rmsd,
                          float *rmsf, int32_t *usable, void *workspace, size_t workspace_bytes, void *stream) {
  if (!ens_shape_ok(B, K, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!ref_crd || !sample_crd || !seq || !rmsd || !rmsf || !usable) return PTAMD_ERR_BAD_SHAPE;
  NscBits nsc;
  if (!make_nsc(nsc)) return PTAMD_ERR_BAD_SHAPE;
  if (!workspace || workspace_bytes < (size_t)B * K * sizeof(Fit)) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  Fit *fit = static_cast<Fit *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ens_fit_kernel, dim3((unsigned)(B * K)), dim3(64), 0, st, ref_crd, sample_crd, seq, K, L, fit, rmsd);
  const int rc = pt_check_launch();
  if (rc) return rc;
  const int tiles = tiles_of(L);
  hipLaunchKernelGGL(ens_rmsf_kernel, dim3((unsigned)(B * tiles)), dim3(64), 0, st, ref_crd, sample_crd, seq, nsc, K, L, tiles,
                     fit, rmsf, usable);
  return pt_check_launch();
}

}  // extern "C"
