// What the three attention translation units share: attention.hip (the entry points and the exact-f32 kernels),
// attention_split.hip (bf16x3) and attention_f16x2.hip (f16x2).  The arguments of one call as plain structs - filled once by
// ptamd_attention_fwd / ptamd_attention_bwd and passed by reference down to the launch, so no launcher restates a positional
// list of look-alike pointers -, the prototypes of what one unit calls in another, the one way a kernel is launched, which
// arithmetic family serves a (dk, arith), and the device helpers all the kernels use: fast_exp, crow, and what every kernel does
// to its transposed 32 x 32 accumulators - acc_zero, acc_scale (the rescale by a running factor), acc_store_rows (a lane's row
// of the result) -, row_delta (delta[q] = sum_d dO O of a lane's query), max8 and f4_at.
#pragma once
#include <type_traits>

#include "split_bf16.h"

// ---- the arguments of one call
struct AttnArgs {  // both passes
  const float *qkv;
  const int64_t *seq;
  int B, L, H, dk;
  float p;  // dropout on the probabilities
  uint64_t seed;
  uint32_t sid;
  hipStream_t stream;
};
struct AttnFwd {
  float *out, *lse;
  uint32_t *keep_bits;  // f16x2 only: the dropout decisions for the backward pass, or null
};
struct AttnBwd {
  const float *o_fwd, *d_o, *lse;
  float *delta;  // workspace [B, H, L]
  float *dqkv;
  uint32_t *row_scale, *row_min;  // f16x2 only (or null): the f16x2 scale of every dqkv row, their minimum
  const uint32_t *keep_bits;      // f16x2 only (or null): the forward kernel's dropout decisions
  float *slabs;                   // f16x2 only: the workspace behind delta (the slabs of the split sweep)
  size_t slab_floats;
};
struct AttnKv {  // pre-split K / V (kv_format.h), f16x2 only; planes null: the kernels read them from qkv
  const char *planes;
  const float *inv;
};

// ---- across translation units
int pt_attention_fwd_split(const AttnArgs &a, const AttnFwd &f);  // dk = 64, 32 (attention_split.hip)
int pt_attention_bwd_split(const AttnArgs &a, const AttnBwd &b);
int pt_attention_fwd_f16x2(const AttnArgs &a, const AttnFwd &f, const AttnKv &kv);  // dk = 128, 64, 32 (attention_f16x2.hip)
int pt_attention_bwd_f16x2(const AttnArgs &a, const AttnBwd &b, const AttnKv &kv);
size_t pt_attention_bwd_f16x2_slab_floats(int B, int L, int H, int dk);  // floats the backward pass wants behind delta
bool pt_attention_f16x2_reads_kv_planes(int B, int L, int H, int dk);
namespace ptgemm {
int persistent_grid(int reserved_cus);  // CUs of the current device (gemm.hip: a table filled once, no per-launch query)
}

// ---- which kernels serve a head size under an `arith` (PTAMD_GEMM_*) in range: f16x2 where it exists and AUTO / F16X2 asks
// for it, bf16x3 where it exists unless F32 is asked for, exact f32 otherwise; ATTN_NONE: no kernel has this head size
enum AttnFamily { ATTN_NONE, ATTN_F32, ATTN_BF16X3, ATTN_F16X2 };
static inline AttnFamily attn_family(int dk, int arith) {
  const bool split = dk == 64 || dk == 32;
  if ((split || dk == 128) && (arith == PTAMD_GEMM_AUTO || arith == PTAMD_GEMM_F16X2)) return ATTN_F16X2;
  if (split && arith != PTAMD_GEMM_F32) return ATTN_BF16X3;
  return split || dk == 128 || dk == 16 || dk == 8 ? ATTN_F32 : ATTN_NONE;
}

// f(std::integral_constant<int, DK>) for the DK of the list that equals dk; PTAMD_ERR_BAD_SHAPE if none does
template <int... DKS, typename F>
int attn_by_dk(int dk, F &&f) {
  int rc = PTAMD_ERR_BAD_SHAPE;
  (void)((dk == DKS && ((rc = f(std::integral_constant<int, DKS>{})), true)) || ...);
  return rc;
}

// One launch: raise the kernel's dynamic-LDS limit where it uses any (idempotent, host-only: no state kept between calls),
// launch, read the launch status.  The arguments are converted to the kernel's parameter types as a direct call would.
template <typename... P, typename... A>
int attn_launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
  if (lds > 0)
    PT_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<P>(args)...);
  return pt_check_launch();
}

static inline size_t attn_delta_floats(int B, int L, int H) { return ((size_t)B * H * L + 3) & ~(size_t)3; }  // (what follows stays 16-byte aligned)

// ---- device helpers
using ptsplit::f32x16;  // a 32 x 32 MFMA C tile: 16 registers per lane
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
// row index inside a 32x32 MFMA C tile held by (register r, lane half lh)
__device__ __forceinline__ int crow(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// ---- accumulators acc[NT] of a TRANSPOSED result (O^T, dQ^T, dK^T, dV^T): tile t holds d = 32 t .. 32 t + 31 in its rows, a
// lane (l31, lh) the column of its query or key - registers 4 g .. 4 g + 3 are d = 32 t + 8 g + 4 lh + 0..3 (crow)
template <int NT>
__device__ __forceinline__ void acc_zero(f32x16 (&acc)[NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}
// acc *= f, for the rescale by a running maximum or scale inside a tile loop: scalar multiplies, kept apart by an empty asm
// (packed f32 VALU, which the compiler would form of them, stalls the matrix pipe)
template <int NT>
__device__ __forceinline__ void acc_scale(f32x16 (&acc)[NT], float f) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float v = acc[t][r] * f;
      asm volatile("" : "+v"(v));
      acc[t][r] = v;
    }
}
// the lane's half of row `row` (DK floats: the query's or key's row of the result) = its accumulator column times f, one float4
// per register quadruple; head sizes below 32 fill a part of the one accumulator
template <int DK, int NT>
__device__ __forceinline__ void acc_store_rows(float *__restrict__ row, const f32x16 (&acc)[NT], int lh, float f = 1.f) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d = t * 32 + 8 * g + 4 * lh;
      if (DK >= 32 || d < DK)
        *reinterpret_cast<float4 *>(row + d) =
            make_float4(acc[t][4 * g] * f, acc[t][4 * g + 1] * f, acc[t][4 * g + 2] * f, acc[t][4 * g + 3] * f);
    }
}
// sum_d g[d] o[d] over a row of 16 KS floats, in both lane halves: each holds d = 16 st + 8 lh + 0..7 of its query's row
template <int KS>
__device__ __forceinline__ float row_delta(const float *__restrict__ gp, const float *__restrict__ op, int lh) {
  float sum = 0.f;
#pragma unroll
  for (int st = 0; st < KS; ++st)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float4 g4 = *reinterpret_cast<const float4 *>(gp + 16 * st + 8 * lh + 4 * j);
      const float4 o4 = *reinterpret_cast<const float4 *>(op + 16 * st + 8 * lh + 4 * j);
      sum += g4.x * o4.x + g4.y * o4.y + g4.z * o4.z + g4.w * o4.w;
    }
  return sum + __shfl_xor(sum, 32, 64);
}
__device__ __forceinline__ float max8(const float4 &a, const float4 &b) {
  return fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
}
// component i & 3 of v (i a constant after unrolling: no select is left)
__device__ __forceinline__ float f4_at(const float4 &v, int i) {
  return (i & 3) == 0 ? v.x : (i & 3) == 1 ? v.y : (i & 3) == 2 ? v.z : v.w;
}
