// Pair sweep of the trained PAE head, for gfx950: for every (frame i, point j) of a protein the H-vector z = relu(u_i + v_j), its
// nbins logits W2 z + b2, their softmax, the expected aligned error, the pTM term and the cross-entropy against the bin of the
// true aligned error - and the gradient of that loss (`protein_transformer_amd/confidence.py`, class PaeHead).
//
// The reference (protein_transformer) has no counterpart; the head is the one of AlphaFold 2 (Jumper et al., Nature 596:583-589
// (2021), supplementary 1.9.7) without its relative-position features.  The definition - which pairs are defined, which count,
// the bin of a target, the NaN cases - is in include/ptamd.h; this file restates only what the kernels do with it.
//
// Nothing of size L x L x nbins or L x L x H exists anywhere: logits are formed, used and dropped pair by pair, and the backward
// pass forms them again.  ONE WAVEFRONT TAKES ONE PAIR AT A TIME, LANE = BIN: lane k holds row k of W2 in registers, u_i and the
// tile's v_j sit in LDS and every lane reads the same words of them (broadcast reads, 16 bytes at a time), the softmax is the
// butterfly of csrc/plddt.hip with its two cancellations written around (log1p of the other lanes for a confident pair,
// -(others) / (all) for p_bin - 1).  Lane jj keeps the expectation of point jj of the tile, so a row of pae leaves as one
// coalesced store per 64 points.
//
// FORWARD.  A workgroup is NW wavefronts = NW frames at a time, sweeping the protein's point tiles of 64.  Every frame's sums
// along j - expected error, pTM term, cross-entropy, counted pairs - are fp64 in the order j = 0 .. L-1.  With a target, the grid
// is (groups of NW frames, proteins); each frame leaves its four sums as one record in the workspace, one workgroup per protein
// adds the records (thread t the rows t, t + 256, .. in order, then the 256 threads in order) and takes the maximum, and one
// wavefront adds the proteins' cross-entropy in index order.  Without a target nothing but pae and stats may be written, so the
// workspace cannot carry the rows: the grid is one workgroup per protein - 16 wavefronts, 8 at H > 32 -, whose wavefronts keep
// their running sums and maximum and meet in LDS.  (A long single protein runs on one compute unit then;
// profiles/pae_head/NOTES.md has the figures.)
//
// BACKWARD.  The workspace may not grow with L^2 H, so a protein is cut into a FIXED number FS of frame slabs, grid (FS, proteins);
// a workgroup walks the point tiles and, inside a tile, its frames.  g_k = p_k - [k == bin] is carried WITHOUT the factor
// coef / n, which is applied once to every finished sum.  Lane k adds g_k z_h to its row of dW2 in registers; g goes through LDS
// once so that lane = h forms dz_h = sum_k W2[k][h] g_k from a register copy of W2's column, masks it by z_h > 0, adds
// it to du_i (a register, flushed into duv once per tile - the row belongs to this wavefront alone) and to the wavefront's own
// copy of the tile's dv in LDS.  At the end of a tile the copies are added in wavefront order and leave as the slab's partial; at
// the end of the sweep so do dW2 and db2.  A second launch adds the partials in index order in fp64 and writes the zeros of the
// spare columns.  No atomics anywhere: two calls give the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int NW = 4;    // wavefronts per forward workgroup
constexpr int TJ = 64;   // points per tile = lanes
constexpr int FS = 16;   // frame slabs per protein in the backward pass
constexpr int RT = 256;  // threads of the reducing kernels

struct __attribute__((aligned(16))) RowRec {
  double pae, tm, ce, count;
};
struct __attribute__((aligned(16))) CeRec {
  double sum, count;
};

inline int padded_h(int H) { return H <= 16 ? 16 : H <= 32 ? 32 : 64; }
inline size_t fwd_bytes(int B, int L) { return (size_t)B * L * sizeof(RowRec) + (size_t)B * sizeof(CeRec); }
inline size_t bwd_floats_dv(int B, int L, int H) { return (size_t)B * FS * L * H; }
inline size_t bwd_floats_dw(int B, int H, int nbins) { return (size_t)B * FS * nbins * (H + 1); }

inline bool pae_shape_ok(int B, int L, int H, int nbins, float bpa) {
  return B > 0 && L > 0 && B <= 65535 && (int64_t)B * L <= INT_MAX && H >= 4 && H <= 64 && H % 4 == 0 && nbins >= 2 &&
         nbins <= PT_WAVE && isfinite(bpa) && bpa > 0.f;
}

__device__ __forceinline__ bool present(int64_t r) { return r >= 0 && r < 20; }

// the bin of a finite target: min(nbins - 1, max(0, floor(target * bins_per_angstrom))), clamped before the conversion to int
__device__ __forceinline__ int bin_of(float target, float bpa, int nbins) {
  const float f = floorf(target * bpa);
  return f <= 0.f ? 0 : f >= (float)(nbins - 1) ? nbins - 1 : (int)f;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// present residues of a protein; every thread of the workgroup calls it and gets the same number (sh: one int per wavefront)
__device__ __forceinline__ int count_present(const int64_t *__restrict__ sq, int L, int *sh) {
  int c = 0;
  for (int j = threadIdx.x; j < L; j += blockDim.x) c += present(sq[j]) ? 1 : 0;
  c = wave_sum_i(c);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  int n = 0;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) n += sh[w];
  return n;
}

__device__ __forceinline__ float tm_d0(int nb) { return 1.24f * cbrtf((float)(max(nb, 19) - 15)) - 1.8f; }

// lane k's logit of one pair WITHOUT its bias: sum_h W2[k][h] relu(u[h] + v[h]); ur and vr are rows of LDS that every lane
// reads alike.  z keeps the pair's hidden vector (the same in every lane) for the backward pass.  The bias is added in fp64 by
// the caller: a bias of 80 would round every step of this chain to 2^-17 and the sum to 4e-6, and a pair that is confidently
// right has probabilities ~e^-80 whose RELATIVE error is the logit's absolute one.
template <int HP>
__device__ __forceinline__ float pair_logit(const float (&w)[HP], const float *ur, const float *vr, float (&z)[HP]) {
  float acc = 0.f;
#pragma unroll
  for (int h = 0; h < HP; h += 4) {
    const float4 a = *reinterpret_cast<const float4 *>(ur + h), c = *reinterpret_cast<const float4 *>(vr + h);
    z[h] = fmaxf(a.x + c.x, 0.f);
    z[h + 1] = fmaxf(a.y + c.y, 0.f);
    z[h + 2] = fmaxf(a.z + c.z, 0.f);
    z[h + 3] = fmaxf(a.w + c.w, 0.f);
    acc = fmaf(w[h], z[h], acc);
    acc = fmaf(w[h + 1], z[h + 1], acc);
    acc = fmaf(w[h + 2], z[h + 2], acc);
    acc = fmaf(w[h + 3], z[h + 3], acc);
  }
  return acc;
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// The softmax over the lanes (csrc/plddt.hip, row_softmax): e = exp(x - max) (0 beyond nbins), s = its sum; returns x - max.
// x = bias + acc and the difference are taken in fp64 (both exact on their fp32 inputs); the difference is split into an fp32
// head and tail, e = exp(head) (1 + tail).  The lane that holds the maximum has a difference of exactly 0.
__device__ __forceinline__ float lane_softmax(float bias, float acc, bool mine, float &e, float &s) {
  const double x = mine ? (double)bias + (double)acc : -(double)INFINITY;
  const double dd = x - wave_max_d(x);
  const float d = (float)dd;
  const float tail = mine ? (float)(dd - (double)d) : 0.f;
  const float head = mine ? expf(d) : 0.f;
  e = fmaf(head, tail, head);
  s = wave_sum(e);
  return d;
}

// lane k's row of W2 (zeros beyond nbins and beyond H: the padding of u and v in LDS is zero too)
template <int HP>
__device__ __forceinline__ void load_w_row(const float *__restrict__ w2, int H, int nbins, int lane, float (&w)[HP]) {
#pragma unroll
  for (int h = 0; h < HP; ++h) w[h] = (lane < nbins && h < H) ? w2[lane * H + h] : 0.f;
}

// the v rows of the points j0 .. j0 + 63 into LDS (zeros beyond L and beyond H), by the whole workgroup; returns nothing before
// the caller's barrier
template <int HP>
__device__ __forceinline__ void load_v_tile(const float *__restrict__ uv, int lduv, size_t row0, int j0, int L, int H,
                                            float (*vt)[HP]) {
  for (int e = threadIdx.x; e < TJ * HP; e += blockDim.x) {
    const int jj = e / HP, h = e % HP, j = j0 + jj;
    vt[jj][h] = (j < L && h < H) ? uv[(row0 + j) * lduv + H + h] : 0.f;
  }
}

template <int HP, int NWT>
__global__ __launch_bounds__(NWT * 64) void pae_fwd_kernel(const float *__restrict__ uv, int lduv, const float *__restrict__ w2,
                                                          const float *__restrict__ b2, const int64_t *__restrict__ seq,
                                                          const float *__restrict__ target, int L, int H, int nbins, float bpa,
                                                          float *__restrict__ pae, RowRec *__restrict__ rows,
                                                          float *__restrict__ stats) {
  __shared__ __attribute__((aligned(16))) float vt[TJ][HP];
  __shared__ __attribute__((aligned(16))) float ut[NWT][HP];
  __shared__ int cnt[NWT];
  __shared__ double red[NWT][2];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const size_t row0 = (size_t)b * L;
  const int64_t *sq = seq + row0;
  const int nb = count_present(sq, L, cnt);
  const bool mine = lane < nbins;
  const float centre = ((float)lane + 0.5f) / bpa;
  const float rel = centre / tm_d0(nb);
  const float tmw = 1.f / (1.f + rel * rel);
  float w[HP], z[HP];
  load_w_row<HP>(w2, H, nbins, lane, w);
  const float bias = mine ? b2[lane] : 0.f;
  const int ntile = (L + TJ - 1) / TJ;
  double tot = 0.0, best = 0.0;   // (one protein per workgroup: the running sum and maximum of this wavefront's frames)

  for (int i0 = blockIdx.x * NWT; i0 < L; i0 += gridDim.x * NWT) {
    const int i = i0 + wv;
    const bool row = i < L;
    const bool pi = row && present(sq[i]);
    __builtin_amdgcn_wave_barrier();
    if (lane < HP) ut[wv][lane] = (row && lane < H) ? uv[(row0 + i) * lduv + lane] : 0.f;   // (this wavefront's own row of ut)
    __builtin_amdgcn_wave_barrier();
    double sp = 0.0, st = 0.0, sc = 0.0, cn = 0.0;   // (wavefront-uniform)
    for (int jt = 0; jt < ntile; ++jt) {
      const int j0 = jt * TJ;
      __syncthreads();
      load_v_tile<HP>(uv, lduv, row0, j0, L, H, vt);
      __syncthreads();
      if (!row) continue;
      const int j = j0 + lane;
      const unsigned long long pm = __ballot(pi && j < L && present(sq[j]));   // the defined pairs of (frame i, this tile)
      const float tg = (target && j < L) ? target[(row0 + i) * L + j] : __builtin_nanf("");
      float value = __builtin_nanf("");
      for (int jj = 0; jj < TJ; ++jj) {
        if (!((pm >> jj) & 1ull)) continue;   // (uniform)
        const float acc = pair_logit<HP>(w, ut[wv], vt[jj], z);
        float e, s;
        const float d = lane_softmax(bias, acc, mine, e, s);
        const float ex = wave_sum(e * centre) / s;
        const float tm = wave_sum(e * tmw) / s;
        sp += (double)ex;
        st += (double)tm;
        if (lane == jj) value = ex;
        const float y = __shfl(tg, jj, 64);
        if (isfinite(y)) {   // (uniform; NaN without a target)
          const int bin = bin_of(y, bpa, nbins);
          const float d_bin = __shfl(d, bin, 64);
          const float others = wave_sum(lane == bin ? 0.f : e);
          sc += (double)(d_bin == 0.f ? log1pf(others) : logf(s) - d_bin);
          cn += 1.0;
        }
      }
      if (j < L) pae[(row0 + i) * L + j] = value;
    }
    if (!row) continue;
    if (rows) {
      if (lane == 0) {
        RowRec r;
        r.pae = sp, r.tm = st, r.ce = sc, r.count = cn;
        rows[row0 + i] = r;
      }
    } else if (pi) {
      tot += sp;
      best = fmax(best, st / (double)nb);
    }
  }
  if (rows) return;
  if (lane == 0) red[wv][0] = tot, red[wv][1] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0, m = 0.0;
    for (int k = 0; k < NWT; ++k) t += red[k][0], m = fmax(m, red[k][1]);
    stats[2 * b] = nb > 0 ? (float)(t / ((double)nb * (double)nb)) : __builtin_nanf("");
    stats[2 * b + 1] = nb > 0 ? (float)m : __builtin_nanf("");
  }
}

// one workgroup per protein: the rows' records -> stats[b] and the protein's {sum of ce, counted pairs}
__global__ __launch_bounds__(RT) void pae_stats_kernel(const RowRec *__restrict__ rows, const int64_t *__restrict__ seq, int L,
                                                       float *__restrict__ stats, CeRec *__restrict__ prot) {
  __shared__ double sh[4][RT];
  __shared__ int shn[RT];
  const int b = blockIdx.x, t = threadIdx.x;
  const size_t row0 = (size_t)b * L;
  double sp = 0.0, best = 0.0, sc = 0.0, cn = 0.0;
  int n = 0;
  for (int i = t; i < L; i += RT) {
    if (!present(seq[row0 + i])) continue;
    const RowRec r = rows[row0 + i];
    sp += r.pae, sc += r.ce, cn += r.count, ++n;
    best = fmax(best, r.tm);
  }
  sh[0][t] = sp, sh[1][t] = best, sh[2][t] = sc, sh[3][t] = cn, shn[t] = n;
  __syncthreads();
  if (t != 0) return;
  sp = best = sc = cn = 0.0, n = 0;
  for (int k = 0; k < RT; ++k) sp += sh[0][k], best = fmax(best, sh[1][k]), sc += sh[2][k], cn += sh[3][k], n += shn[k];
  stats[2 * b] = n > 0 ? (float)(sp / ((double)n * (double)n)) : __builtin_nanf("");
  stats[2 * b + 1] = n > 0 ? (float)(best / (double)n) : __builtin_nanf("");
  CeRec c;
  c.sum = sc, c.count = cn;
  prot[b] = c;
}

// one wavefront: the proteins' records in index order (csrc/plddt.hip, plddt_finalize_kernel)
__global__ __launch_bounds__(64) void pae_finalize_kernel(const CeRec *__restrict__ prot, int B, float *__restrict__ sums) {
  const int lane = threadIdx.x;
  double sum = 0.0, count = 0.0;
  for (int base = 0; base < B; base += 64) {
    const bool have = base + lane < B;
    const double s = have ? prot[base + lane].sum : 0.0, c = have ? prot[base + lane].count : 0.0;
    const int n = min(64, B - base);
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

template <int HP, int NWB>
__global__ __launch_bounds__(NWB * 64) void pae_bwd_kernel(const float *__restrict__ uv, int lduv, const float *__restrict__ w2,
                                                           const float *__restrict__ b2, const int64_t *__restrict__ seq,
                                                           const float *__restrict__ target, int L, int H, int nbins, float bpa,
                                                           const float *__restrict__ sums, float coef, float *__restrict__ duv,
                                                           int ldd, float *__restrict__ dvp, float *__restrict__ dwp) {
  __shared__ __attribute__((aligned(16))) float vt[TJ][HP];
  __shared__ __attribute__((aligned(16))) float ut[NWB][HP];
  __shared__ __attribute__((aligned(16))) float gs[NWB][64];
  __shared__ __attribute__((aligned(16))) float dvt[NWB][TJ][HP];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y, slab = blockIdx.x;
  const size_t row0 = (size_t)b * L;
  const int64_t *sq = seq + row0;
  const float n = sums[1];
  const bool live = n > 0.f;
  const float scale = live ? coef / n : 0.f;
  const bool mine = lane < nbins;
  float w[HP], z[HP], wt[64];
  double dw[HP];   // (fp64: a wavefront adds every pair of its frames into these, thousands of terms at L = 512)
  load_w_row<HP>(w2, H, nbins, lane, w);
#pragma unroll
  for (int h = 0; h < HP; ++h) dw[h] = 0.0;
#pragma unroll
  for (int k = 0; k < 64; ++k) wt[k] = (k < nbins && lane < H) ? w2[k * H + lane] : 0.f;   // lane h: column h of W2
  const float bias = mine ? b2[lane] : 0.f;
  double db = 0.0;
  const int ntile = (L + TJ - 1) / TJ;

  for (int jt = 0; jt < ntile; ++jt) {
    const int j0 = jt * TJ, j = j0 + lane;
    __syncthreads();
    load_v_tile<HP>(uv, lduv, row0, j0, L, H, vt);
    for (int jj = 0; jj < TJ; ++jj)
      if (lane < HP) dvt[wv][jj][lane] = 0.f;
    __syncthreads();
    const bool pj = j < L && present(sq[j]);
    for (int i = slab * NWB + wv; i < L; i += FS * NWB) {
      const bool pi = present(sq[i]);
      __builtin_amdgcn_wave_barrier();
      if (lane < HP) ut[wv][lane] = lane < H ? uv[(row0 + i) * lduv + lane] : 0.f;
      __builtin_amdgcn_wave_barrier();
      const float tg = j < L ? target[(row0 + i) * L + j] : __builtin_nanf("");
      const unsigned long long pm = __ballot(live && pi && pj && isfinite(tg));   // the counted pairs of (frame i, this tile)
      float du = 0.f;   // lane h: du_i[h] of this tile
      for (int jj = 0; jj < TJ; ++jj) {
        if (!((pm >> jj) & 1ull)) continue;   // (uniform)
        const float acc = pair_logit<HP>(w, ut[wv], vt[jj], z);
        float e, s;
        lane_softmax(bias, acc, mine, e, s);
        const int bin = bin_of(__shfl(tg, jj, 64), bpa, nbins);
        const float others = wave_sum(lane == bin ? 0.f : e);
        // p_k - [k == bin], WITHOUT coef / n: a pair that is confidently right has |g| ~ e^-80, which fp32 still holds as a
        // normal number; scaled first it would be a denormal and every sum made of such pairs alone would lose its digits.
        // The factor is applied once, to the finished sums (0 beyond nbins: e is 0 there)
        const float g = lane == bin ? -others / s : e / s;
        db += (double)g;
#pragma unroll
        for (int h = 0; h < HP; ++h) dw[h] = fma((double)g, (double)z[h], dw[h]);
        __builtin_amdgcn_wave_barrier();
        gs[wv][lane] = g;
        __builtin_amdgcn_wave_barrier();
        if (lane < HP) {
          float dz = 0.f;
#pragma unroll
          for (int k = 0; k < 64; k += 4) {
            const float4 g4 = *reinterpret_cast<const float4 *>(&gs[wv][k]);
            dz = fmaf(wt[k], g4.x, dz);
            dz = fmaf(wt[k + 1], g4.y, dz);
            dz = fmaf(wt[k + 2], g4.z, dz);
            dz = fmaf(wt[k + 3], g4.w, dz);
          }
          dz = ut[wv][lane] + vt[jj][lane] > 0.f ? dz : 0.f;   // the derivative of relu at exactly 0 is 0
          du += dz;
          dvt[wv][jj][lane] += dz;
        }
      }
      if (lane < H) {
        float *out = duv + (row0 + i) * ldd + lane;
        const float t = jt == 0 ? du : *out + du;   // (row i's u half belongs to this wavefront alone)
        *out = jt == ntile - 1 ? (t == 0.f ? 0.f : scale * t) : t;   // (+0 where nothing was summed, whatever coef's sign)
      }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TJ * HP; e += NWB * 64) {
      const int jj = e / HP, h = e % HP;
      if (j0 + jj >= L || h >= H) continue;
      float t = dvt[0][jj][h];
      for (int k = 1; k < NWB; ++k) t += dvt[k][jj][h];
      dvp[(((size_t)b * FS + slab) * L + j0 + jj) * H + h] = t;
    }
  }
  // dW2 and db2 of the slab: the wavefronts' registers meet in LDS (dvt is free now) and are added in wavefront order
  __syncthreads();
#pragma unroll
  for (int h = 0; h < HP; ++h) dvt[wv][lane][h] = (float)dw[h];
  gs[wv][lane] = (float)db;
  __syncthreads();
  float *out = dwp + ((size_t)b * FS + slab) * nbins * (H + 1);
  for (int e = threadIdx.x; e < TJ * HP; e += NWB * 64) {
    const int k = e / HP, h = e % HP;
    if (k >= nbins || h >= H) continue;
    float t = dvt[0][k][h];
    for (int q = 1; q < NWB; ++q) t += dvt[q][k][h];
    out[k * H + h] = t;
  }
  if ((int)threadIdx.x < nbins) {
    float t = gs[0][threadIdx.x];
    for (int q = 1; q < NWB; ++q) t += gs[q][threadIdx.x];
    out[nbins * H + threadIdx.x] = t;
  }
}

// the partials in index order, in fp64: the v half and the spare columns of duv, then dW2 and db2
__global__ __launch_bounds__(RT) void pae_bwd_reduce_kernel(const float *__restrict__ dvp, const float *__restrict__ dwp, int B, int L,
                                                            int H, int nbins, const float *__restrict__ sums, float coef,
                                                            float *__restrict__ duv, int ldd, float *__restrict__ dw2,
                                                            float *__restrict__ db2) {
  const float n = sums[1];
  const double scale = n > 0.f ? (double)(coef / n) : 0.0;
  const size_t cols = (size_t)(ldd - H), nduv = (size_t)B * L * cols, nw = (size_t)nbins * (H + 1);
  const size_t idx = (size_t)blockIdx.x * RT + threadIdx.x;
  if (idx < nduv) {
    const size_t r = idx / cols;
    const int c = H + (int)(idx % cols);
    double t = 0.0;
    if (c < 2 * H) {
      const size_t b = r / L, j = r % L;
      for (int s = 0; s < FS; ++s) t += (double)dvp[((b * FS + s) * L + j) * H + (c - H)];
    }
    duv[r * ldd + c] = t == 0.0 ? 0.f : (float)(scale * t);   // (+0 in the spare columns and where nothing was summed)
  } else if (idx < nduv + nw) {
    const size_t e = idx - nduv;
    double t = 0.0;
    for (int p = 0; p < B * FS; ++p) t += (double)dwp[(size_t)p * nw + e];
    if (e < (size_t)nbins * H)
      dw2[e] = t == 0.0 ? 0.f : (float)(scale * t);
    else
      db2[e - (size_t)nbins * H] = t == 0.0 ? 0.f : (float)(scale * t);
  }
}

}  // namespace

extern "C" {

size_t ptamd_pae_head_workspace_bytes(int B, int L, int H, int nbins) {
  if (!pae_shape_ok(B, L, H, nbins, 1.f)) return 0;
  const size_t f = fwd_bytes(B, L), g = (bwd_floats_dv(B, L, H) + bwd_floats_dw(B, H, nbins)) * sizeof(float);
  return ((f > g ? f : g) + 15) & ~(size_t)15;
}

int ptamd_pae_head_fwd(const float *uv, int lduv, const float *w2, const float *b2, const int64_t *seq, const float *target, int B,
                       int L, int H, int nbins, float bins_per_angstrom, float *pae, float *stats, float *sums, void *workspace,
                       size_t workspace_bytes, void *stream) {
  if (!pae_shape_ok(B, L, H, nbins, bins_per_angstrom) || lduv < 2 * H) return PTAMD_ERR_BAD_SHAPE;
  if (!uv || !w2 || !b2 || !seq || !pae || !stats || (target && !sums)) return PTAMD_ERR_BAD_SHAPE;
  if (target) {
    if (!workspace || workspace_bytes < ptamd_pae_head_workspace_bytes(B, L, H, nbins)) return PTAMD_ERR_WORKSPACE;
    if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  }
  RowRec *rows = target ? static_cast<RowRec *>(workspace) : nullptr;
  CeRec *prot = target ? reinterpret_cast<CeRec *>(rows + (size_t)B * L) : nullptr;
  hipStream_t st = (hipStream_t)stream;
  // with a target: groups of NW frames over the whole device; without one a protein is one workgroup, as wide as its registers allow
#define PAE_FWD(HP, NWT, GX)                                                                                              \
  hipLaunchKernelGGL((pae_fwd_kernel<HP, NWT>), dim3((unsigned)(GX), (unsigned)B), dim3(NWT * 64), 0, st, uv, lduv, w2, b2, seq, \
                     target, L, H, nbins, bins_per_angstrom, pae, rows, stats)
  const int groups = (L + NW - 1) / NW;
  switch (padded_h(H)) {
    case 16: if (target) PAE_FWD(16, NW, groups); else PAE_FWD(16, 16, 1); break;
    case 32: if (target) PAE_FWD(32, NW, groups); else PAE_FWD(32, 16, 1); break;
    default: if (target) PAE_FWD(64, NW, groups); else PAE_FWD(64, 8, 1); break;
  }
#undef PAE_FWD
  int rc = pt_check_launch();
  if (rc || !target) return rc;
  hipLaunchKernelGGL(pae_stats_kernel, dim3((unsigned)B), dim3(RT), 0, st, rows, seq, L, stats, prot);
  if ((rc = pt_check_launch())) return rc;
  hipLaunchKernelGGL(pae_finalize_kernel, dim3(1), dim3(64), 0, st, prot, B, sums);
  return pt_check_launch();
}

int ptamd_pae_head_bwd(const float *uv, int lduv, const float *w2, const float *b2, const int64_t *seq, const float *target, int B,
                       int L, int H, int nbins, float bins_per_angstrom, const float *sums, float coef, float *duv, int ldd,
                       float *dw2, float *db2, void *workspace, size_t workspace_bytes, void *stream) {
  if (!pae_shape_ok(B, L, H, nbins, bins_per_angstrom) || lduv < 2 * H || ldd < 2 * H) return PTAMD_ERR_BAD_SHAPE;
  if (!uv || !w2 || !b2 || !seq || !target || !sums || !duv || !dw2 || !db2) return PTAMD_ERR_BAD_SHAPE;
  const size_t total = (size_t)B * L * (size_t)(ldd - H) + (size_t)nbins * (H + 1);
  if ((total + RT - 1) / RT > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;
  if (!workspace || workspace_bytes < ptamd_pae_head_workspace_bytes(B, L, H, nbins)) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  float *dvp = static_cast<float *>(workspace), *dwp = dvp + bwd_floats_dv(B, L, H);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(FS, (unsigned)B);
#define PAE_BWD(HP, NWB)                                                                                                        \
  hipLaunchKernelGGL((pae_bwd_kernel<HP, NWB>), grid, dim3(NWB * 64), 0, st, uv, lduv, w2, b2, seq, target, L, H, nbins,        \
                     bins_per_angstrom, sums, coef, duv, ldd, dvp, dwp)
  switch (padded_h(H)) {
    case 16: PAE_BWD(16, 4); break;
    case 32: PAE_BWD(32, 4); break;
    default: PAE_BWD(64, 2); break;
  }
#undef PAE_BWD
  const int rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(pae_bwd_reduce_kernel, dim3((unsigned)((total + RT - 1) / RT)), dim3(RT), 0, st, dvp, dwp, B, L, H, nbins, sums,
                     coef, duv, ldd, dw2, db2);
  return pt_check_launch();
}

}  // extern "C"
