// Binned-lDDT loss of the confidence head, for gfx950: softmax over nbins <= 64 bins of a token row, the expected bin centre as
// the row's pLDDT, the cross-entropy against the bin of the row's true lDDT-C-alpha, and its gradient
// (`protein_transformer_amd/confidence.py`).
//
// The reference (protein_transformer) has no counterpart; the head is the one of AlphaFold 2 (Jumper et al., Nature 596:583-589
// (2021), supplementary 1.9.6).  The definition - which rows count, the bin of a target, the NaN cases - is in include/ptamd.h;
// this file restates only what the kernels do with it.
//
// ONE WAVEFRONT PER WORKGROUP, ROWS rows one after the other, LANE = BIN.  Lanes at or beyond nbins hold -inf / 0 and take no part
// in the maximum or the sums; every row reduction is a butterfly over the 64 lanes (common.h: __shfl_xor), which leaves the same
// bits in every lane - no LDS, no barrier.  Two cancellations are written around instead of computed:
//   -log p_bin   when the target's bin holds the row maximum, log1p(sum of the OTHER lanes' exponentials): a confident, correct
//                row has a small positive loss instead of log(1 + 1e-30) = 0;
//   p_bin - 1    as -(sum of the other lanes) / (sum of all), in the gradient.
// The mean over the counted rows: every workgroup leaves {sum of ce, counted rows} of its ROWS rows as two doubles in the
// workspace - rows in index order -, and one further wavefront adds the workgroups' records in index order.  No atomics: two runs
// give the same bits.  The backward kernel reads the count from `sums` on the device.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int ROWS = 16;   // rows per workgroup = rows per workspace record

struct __attribute__((aligned(16))) Partial {
  double sum, count;
};

inline int64_t blocks_of(int64_t T) { return (T + ROWS - 1) / ROWS; }
inline bool plddt_shape_ok(int64_t T, int nbins, int ld) {
  return T > 0 && blocks_of(T) <= INT_MAX && nbins >= 2 && nbins <= PT_WAVE && ld >= nbins;
}

// the bin of a finite target: min(nbins - 1, max(0, floor(target * nbins))), clamped before the conversion to int
__device__ __forceinline__ int bin_of(float target, int nbins) {
  const float f = floorf(target * (float)nbins);
  return f <= 0.f ? 0 : f >= (float)(nbins - 1) ? nbins - 1 : (int)f;
}

// The softmax of one row, lane = bin: e = exp(x - max) (0 beyond nbins), s = its sum over the row; returns x - max of this lane.
// x - max is taken in fp64 (exact on fp32 inputs) and split into an fp32 head and tail, e = exp(head) (1 + tail): rounding the
// difference to fp32 alone costs half an ulp of it - 4e-6 of e at a difference of -80 - which a confident row's loss would show.
__device__ __forceinline__ float row_softmax(const float *__restrict__ row, int nbins, int lane, float &e, float &s) {
  const bool mine = lane < nbins;
  const float x = mine ? row[lane] : -INFINITY;
  const float m = wave_max(x);
  const double dd = (double)x - (double)m;
  const float d = (float)dd;
  const float tail = mine ? (float)(dd - (double)d) : 0.f;
  const float head = mine ? expf(d) : 0.f;
  e = fmaf(head, tail, head);
  s = wave_sum(e);
  return d;
}

__global__ __launch_bounds__(64) void plddt_fwd_kernel(const float *__restrict__ logits, int ld, const float *__restrict__ target,
                                                       int target_stride, int64_t T, int nbins, float *__restrict__ plddt,
                                                       float *__restrict__ ce, Partial *__restrict__ part) {
  const int lane = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * ROWS;
  const int rows = T - t0 < ROWS ? (int)(T - t0) : ROWS;
  const float centre = ((float)lane + 0.5f) / (float)nbins;
  double sum = 0.0, count = 0.0;   // (wavefront-uniform)
  for (int r = 0; r < rows; ++r) {
    const int64_t t = t0 + r;
    float e, s;
    const float d = row_softmax(logits + (size_t)t * ld, nbins, lane, e, s);
    const float expect = 100.f * wave_sum((e / s) * centre);
    // (every lane reads the same target word: the row's branch is uniform, and the reductions below sit outside it)
    const float y = target ? target[(size_t)t * target_stride] : __builtin_nanf("");
    const bool counted = isfinite(y);
    const int bin = counted ? bin_of(y, nbins) : 0;
    const float d_bin = __shfl(d, bin, 64);
    const float others = wave_sum(lane == bin ? 0.f : e);
    float loss = __builtin_nanf("");
    if (counted) {
      loss = d_bin == 0.f ? log1pf(others) : logf(s) - d_bin;
      sum += (double)loss;
      count += 1.0;
    }
    if (lane == 0) {
      plddt[t] = expect;
      if (target) ce[t] = loss;
    }
  }
  if (target && lane == 0) {
    Partial p;
    p.sum = sum;
    p.count = count;
    part[blockIdx.x] = p;
  }
}

// one wavefront: the records in index order (64 at a time are loaded, one per lane, and handed round in lane order)
__global__ __launch_bounds__(64) void plddt_finalize_kernel(const Partial *__restrict__ part, int nblocks, float *__restrict__ sums) {
  const int lane = threadIdx.x;
  double sum = 0.0, count = 0.0;
  for (int base = 0; base < nblocks; base += 64) {
    const bool have = base + lane < nblocks;
    const double s = have ? part[base + lane].sum : 0.0, c = have ? part[base + lane].count : 0.0;
    const int n = min(64, nblocks - base);
    for (int j = 0; j < n; ++j) {
      sum += __shfl(s, j, 64);
      count += __shfl(c, j, 64);
    }
  }
  if (lane == 0) {
    sums[0] = count > 0.0 ? (float)(sum / count) : __builtin_nanf("");
    sums[1] = (float)count;
  }
}

__global__ __launch_bounds__(64) void plddt_bwd_kernel(const float *__restrict__ logits, int ld, const float *__restrict__ target,
                                                       int target_stride, int64_t T, int nbins, const float *__restrict__ sums,
                                                       float coef, float *__restrict__ dlogits, int ldd) {
  const int lane = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * ROWS;
  const int rows = T - t0 < ROWS ? (int)(T - t0) : ROWS;
  const float n = sums[1];
  const float scale = n > 0.f ? coef / n : 0.f;
  for (int r = 0; r < rows; ++r) {
    const int64_t t = t0 + r;
    float *out = dlogits + (size_t)t * ldd;
    const float y = target[(size_t)t * target_stride];
    const bool counted = n > 0.f && isfinite(y);   // (uniform; the reductions sit outside the branch)
    float e, s;
    row_softmax(logits + (size_t)t * ld, nbins, lane, e, s);
    const int bin = counted ? bin_of(y, nbins) : 0;
    const float others = wave_sum(lane == bin ? 0.f : e);
    const float g = counted ? scale * (lane == bin ? -others / s : e / s) : 0.f;   // (0 beyond nbins: e is 0 there)
    if (lane < ldd) out[lane] = g;
    for (int c = 64 + lane; c < ldd; c += 64) out[c] = 0.f;
  }
}

}  // namespace

extern "C" {

int ptamd_plddt_rows_per_block(void) { return ROWS; }

size_t ptamd_plddt_workspace_bytes(int64_t T) {
  if (T <= 0 || blocks_of(T) > INT_MAX) return 0;
  return (size_t)blocks_of(T) * sizeof(Partial);
}

int ptamd_plddt_fwd(const float *logits, int ld, const float *target, int target_stride, int64_t T, int nbins, float *plddt,
                    float *ce, float *sums, void *workspace, size_t workspace_bytes, void *stream) {
  if (!plddt_shape_ok(T, nbins, ld) || !logits || !plddt) return PTAMD_ERR_BAD_SHAPE;
  if (target) {
    if (!ce || !sums || target_stride < 1) return PTAMD_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < ptamd_plddt_workspace_bytes(T)) return PTAMD_ERR_WORKSPACE;
    if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  }
  const int nblocks = (int)blocks_of(T);
  Partial *part = static_cast<Partial *>(workspace);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(plddt_fwd_kernel, dim3((unsigned)nblocks), dim3(64), 0, st, logits, ld, target, target_stride, T, nbins, plddt,
                     ce, part);
  const int rc = pt_check_launch();
  if (rc || !target) return rc;
  hipLaunchKernelGGL(plddt_finalize_kernel, dim3(1), dim3(64), 0, st, part, nblocks, sums);
  return pt_check_launch();
}

int ptamd_plddt_bwd(const float *logits, int ld, const float *target, int target_stride, int64_t T, int nbins, const float *sums,
                    float coef, float *dlogits, int ldd, void *stream) {
  if (!plddt_shape_ok(T, nbins, ld) || ldd < nbins || target_stride < 1) return PTAMD_ERR_BAD_SHAPE;
  if (!logits || !target || !sums || !dlogits) return PTAMD_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(plddt_bwd_kernel, dim3((unsigned)blocks_of(T)), dim3(64), 0, (hipStream_t)stream, logits, ld, target,
                     target_stride, T, nbins, sums, coef, dlogits, ldd);
  return pt_check_launch();
}

}  // extern "C"
