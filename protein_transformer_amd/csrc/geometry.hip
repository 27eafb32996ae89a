// Angle recovery (atan2) and the NeRF all-atom build, forward and adjoint, for gfx950.
//
// Replaces the per-atom Python/PyTorch op chain of
//   nerf                      /root/reference/protein_transformer/protein/Structure.py:23-65
//   StructureBuilder.build    .../protein/StructureBuilder.py:55-92
//   ResidueBuilder.build_bb   .../protein/StructureBuilder.py:147-191
//   ResidueBuilder.build_sc   .../protein/StructureBuilder.py:193-236
//   inverse_trig_transform    .../losses.py:26-36
// and the autograd graph the reference builds over them (losses.py:91-92).
//
// Structure of the work (one protein = one dependent chain of 3L backbone placements):
//   nerf_backbone_fwd  one wavefront per protein: the chain is a product of rigid transforms, evaluated as a
//                      parallel prefix scan (chunk per lane + 6 shuffle steps) instead of a 3L-step walk.
//   nerf_backbone_bwd  one wavefront per protein: gradients of all bond / torsion angles from suffix sums of
//                      force and torque over the chain atoms (fp64 accumulators), again chunk + wave scan.
//   nerf_sidechain_* one lane per residue: O plus up to 10 table-driven side-chain placements, per-lane
//                    atom arrays live in LDS ([slot][xyz][lane], conflict-free) because parent slots are
//                    data dependent.
#include "common.h"
#include "nerf_tables.h"

namespace {

constexpr float BL_N_CA = 1.442f, BL_CA_C = 1.498f, BL_C_N = 1.379f, BL_C_O = 1.229f, BA_CA_C_O = 2.0944f;
constexpr float PI_F = 3.141592653589793f;
constexpr int MAX_L_CHAIN = 2048;  // trig cache of the forward scan: 48 B of LDS per residue

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// torch.nn.functional.normalize: v / max(||v||, 1e-12)
__device__ __forceinline__ V3 unit(V3 v, float &nrm) {
  nrm = fmaxf(sqrtf(dot(v, v)), 1e-12f);
  return {v.x / nrm, v.y / nrm, v.z / nrm};
}

// Structure.py:44-65 with W_hat supplied (it equals the previous placement's x_hat on the backbone).
__device__ __forceinline__ V3 place_with_w(V3 W, V3 b, V3 c, float l, float st, float ct, float sx, float cx,
                                           V3 &x_out) {
  float nw, nn;
  V3 x = unit(c - b, nw);
  V3 z = unit(cross(W, x), nn);
  V3 y = cross(z, x);
  float d0 = -l * ct, d1 = l * st * cx, d2 = l * st * sx;
  x_out = x;
  return {c.x + (x.x * d0 + y.x * d1 + z.x * d2), c.y + (x.y * d0 + y.y * d1 + z.y * d2),
          c.z + (x.z * d0 + y.z * d1 + z.z * d2)};
}
__device__ __forceinline__ V3 place(V3 a, V3 b, V3 c, float l, float st, float ct, float sx, float cx) {
  float nu;
  V3 W = unit(b - a, nu), xo;
  return place_with_w(W, b, c, l, st, ct, sx, cx, xo);
}

// Adjoint of one placement.  g = dL/dd; accumulates into ga, gb, gc, gth, gchi.
__device__ __forceinline__ void place_bwd(V3 a, V3 b, V3 c, float l, float st, float ct, float sx, float cx, V3 g,
                                          V3 &ga, V3 &gb, V3 &gc, float &gth, float &gchi) {
  float nu, nw, nn;
  V3 u = b - a, w = c - b;
  float ru = sqrtf(dot(u, u)), rw = sqrtf(dot(w, w));
  V3 W = unit(u, nu), x = unit(w, nw);
  V3 n = cross(W, x);
  float rn = sqrtf(dot(n, n));
  V3 z = unit(n, nn);
  V3 y = cross(z, x);
  float v0 = -l * ct, v1 = l * st * cx, v2 = l * st * sx;
  gc = gc + g;
  V3 xb = v0 * g, yb = v1 * g, zb = v2 * g;
  float vb0 = dot(g, x), vb1 = dot(g, y), vb2 = dot(g, z);
  gth += l * (st * vb0 + ct * cx * vb1 + ct * sx * vb2);
  gchi += l * st * (-sx * vb1 + cx * vb2);
  zb = zb + cross(x, yb);
  xb = xb + cross(yb, z);
  V3 nb = (rn > 1e-12f) ? (1.f / nn) * (zb - dot(zb, z) * z) : (1.f / nn) * zb;
  V3 Wb = cross(x, nb);
  xb = xb + cross(nb, W);
  V3 wb = (rw > 1e-12f) ? (1.f / nw) * (xb - dot(xb, x) * x) : (1.f / nw) * xb;
  gc = gc + wb;
  gb = gb - wb;
  V3 ub = (ru > 1e-12f) ? (1.f / nu) * (Wb - dot(Wb, W) * W) : (1.f / nu) * Wb;
  gb = gb + ub;
  ga = ga - ub;
}

__device__ __forceinline__ V3 ld3(const float *p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float *p, V3 v) {
  p[0] = v.x;
  p[1] = v.y;
  p[2] = v.z;
}

// number of leading non-pad residues of one protein; flags ids outside 0..19 (wave-cooperative)
__device__ int protein_len(const int64_t *seq, int L, int lane, int32_t *status) {
  int cnt = 0, bad = 0;
  for (int i = lane; i < L; i += PT_WAVE) {
    int64_t r = seq[i];
    if (r != PTAMD_PAD_ID) {
      ++cnt;
      if (r < 0 || r > 19) bad = 1;
    }
  }
  cnt = (int)wave_sum((float)cnt);
  if (__any(bad) && lane == 0) atomicOr(status, PTAMD_ST_BAD_RESIDUE);
  return cnt;
}

// ------------------------------------------------------------------------------------------------
// angles
__global__ void angles_fwd_kernel(const float2 *__restrict__ sc, float *__restrict__ ang, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float2 v = sc[i];
    ang[i] = atan2f(v.y, v.x);
  }
}
__global__ void angles_bwd_kernel(const float2 *__restrict__ sc, const float *__restrict__ dang,
                                  float2 *__restrict__ dsc, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    float2 v = sc[i];
    float g = dang[i], r2 = v.x * v.x + v.y * v.y;
    float inv = r2 > 0.f ? 1.f / r2 : 0.f;
    dsc[i] = make_float2(-v.y * inv * g, v.x * inv * g);
  }
}

// ------------------------------------------------------------------------------------------------
// Backbone chain, forward, as a PARALLEL SCAN over rigid transforms.
//
// Placement k = 3i + a (a = 0: N_i, 1: CA_i, 2: C_i; i >= 1) builds P_k from (P_{k-3}, P_{k-2}, P_{k-1}) with
// the frame M_k = [x y z] of Structure.py:44-59.  In exact arithmetic the next frame is M_{k+1} = M_k R_k and
// P_k = P_{k-1} + M_k t_k, with R_k, t_k functions of (l_k, theta_k, chi_k) only:
//     x' = (-cos th, sin th cos chi, sin th sin chi)      (new bond direction in the old frame; t_k = l_k x')
//     z' = s (0, -sin chi, cos chi),  s = sign(sin th)    (normal of the plane b, c, d)
//     y' = z' x x' = s (-sin th, -cos th cos chi, -cos th sin chi)
// so the chain is a product of 4x4 affine matrices [[R_k, t_k], [0, 1]], which is associative: every lane
// composes a contiguous chunk of placements, one wave-wide Hillis-Steele scan (6 shuffle steps) combines the 64
// chunk products, and every lane re-walks its chunk from its prefix.  3L = 1536 dependent placements become
// ~2 * 24 + 6 dependent compositions.  The rounding differs from the reference's step-by-step fp32 walk (which
// itself drifts by up to 6e-3 A at L = 512 against fp64); it is covered by the stated coordinate tolerance.
struct Xf {
  float r[9];  // rotation, row-major: r[3 * row + col], columns = new x, y, z axes
  float t[3];
};
__device__ __forceinline__ Xf xf_identity() {
  Xf x;
#pragma unroll
  for (int i = 0; i < 9; ++i) x.r[i] = (i % 4 == 0) ? 1.f : 0.f;
  x.t[0] = x.t[1] = x.t[2] = 0.f;
  return x;
}
// a then b (b expressed in a's frame): R = Ra Rb, t = Ra tb + ta
__device__ __forceinline__ Xf xf_mul(const Xf &a, const Xf &b) {
  Xf o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o.r[3 * i + j] = a.r[3 * i] * b.r[j] + a.r[3 * i + 1] * b.r[3 + j] + a.r[3 * i + 2] * b.r[6 + j];
    o.t[i] = a.r[3 * i] * b.t[0] + a.r[3 * i + 1] * b.t[1] + a.r[3 * i + 2] * b.t[2] + a.t[i];
  }
  return o;
}
__device__ __forceinline__ Xf xf_shfl_up(const Xf &x, int d) {
  Xf o;
#pragma unroll
  for (int i = 0; i < 9; ++i) o.r[i] = __shfl_up(x.r[i], d, 64);
#pragma unroll
  for (int i = 0; i < 3; ++i) o.t[i] = __shfl_up(x.t[i], d, 64);
  return o;
}
__device__ __forceinline__ Xf xf_local(float l, float st, float ct, float sx, float cx) {
  const float s = st < 0.f ? -1.f : 1.f;
  Xf x;
  x.r[0] = -ct;      x.r[1] = -s * st;      x.r[2] = 0.f;
  x.r[3] = st * cx;  x.r[4] = -s * ct * cx; x.r[5] = -s * sx;
  x.r[6] = st * sx;  x.r[7] = -s * ct * sx; x.r[8] = s * cx;
  x.t[0] = l * x.r[0]; x.t[1] = l * x.r[3]; x.t[2] = l * x.r[6];
  return x;
}
// (bond length, theta column, chi column, residue offset) of placement p = k - 3
__device__ __forceinline__ void placement_params(int p, int &res, int &col_th, int &col_chi, float &l, int &slot) {
  const int i = 1 + p / 3, a = p - (i - 1) * 3;
  slot = a;
  if (a == 0) { res = i - 1; col_th = 4; col_chi = 1; l = BL_C_N; }
  else if (a == 1) { res = i - 1; col_th = 5; col_chi = 2; l = BL_N_CA; }
  else { res = i; col_th = 3; col_chi = 0; l = BL_CA_C; }
}

// grid = B, block = 64 NW (NW wavefronts per protein: round 6 - with one, 3 L = 1536 placements are 24 per lane and the
// kernel takes 24.5 us whatever the batch; with four, 6 per lane, the wave-wide scans joined through LDS by at most three more
// compositions).  dynamic LDS: chunk * 64 NW float4 of cached (sin th, cos th, sin chi, cos chi)
// BB: the backbone-only build (ptamd_nerf_bb_fwd) - the same scan, same composition order, same bits, written to the COMPACT
// array [B, 3 L, 3] (N, CA, C per residue: 9 floats instead of 42); no side-chain kernel follows, so the residues behind the
// protein's end (all of them for a protein that is too short) are zeroed here
template <int NW, bool BB>
__global__ __launch_bounds__(PT_WAVE * NW) void nerf_backbone_fwd_kernel(const float *__restrict__ ang,
                                                                         const int64_t *__restrict__ seq, int L,
                                                                         float *__restrict__ crd,
                                                                         int32_t *__restrict__ status) {
  constexpr int NT = PT_WAVE * NW;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float wave_total[NW][12];
  float4 *trig = reinterpret_cast<float4 *>(lds);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (PT_WAVE - 1), wave = tid / PT_WAVE;
  ang += (size_t)b * L * 12;
  seq += (size_t)b * L;
  constexpr int RES = BB ? 9 : 42;   // floats per residue of crd
  crd += (size_t)b * L * RES;
  const int len = protein_len(seq, L, lane, status);   // (every wavefront counts: the same number, idempotent flags)
  if (BB) {
    for (int k = (len < 2 ? 0 : len * RES) + tid; k < L * RES; k += NT) crd[k] = 0.f;
  }
  if (len < 2) {
    if (tid == 0) atomicOr(status, PTAMD_ST_TOO_SHORT);
    return;  // the side-chain kernel zero-fills (BB: zeroed above)
  }
  const int K = 3 * (len - 1), chunk = (K + NT - 1) / NT;
  const int p0 = min(K, tid * chunk), p1 = min(K, p0 + chunk);

  // pass 1: local transforms of my chunk, composed in order
  Xf q = xf_identity();
  int bad_theta = 0;
  for (int p = p0; p < p1; ++p) {
    int res, cth, cchi, slot;
    float l;
    placement_params(p, res, cth, cchi, l, slot);
    const float th = ang[res * 12 + cth], chi = ang[res * 12 + cchi];
    float st, ct, sx, cx;
    sincosf(th, &st, &ct);
    sincosf(chi, &sx, &cx);
    if (!(fabsf(th) <= PI_F)) bad_theta = 1;  // fp32 pi itself is accepted
    trig[(p - p0) * NT + tid] = make_float4(st, ct, sx, cx);
    q = xf_mul(q, xf_local(l, st, ct, sx, cx));
  }
  {
    const float a03 = ang[3];
    if (!(fabsf(a03) <= PI_F)) bad_theta = 1;
  }
  if (__any(bad_theta) && lane == 0) atomicOr(status, PTAMD_ST_BAD_THETA);

  // wave-wide inclusive scan of the chunk products, then shift to an exclusive prefix
#pragma unroll
  for (int d = 1; d < PT_WAVE; d <<= 1) {
    const Xf o = xf_shfl_up(q, d);
    if (lane >= d) q = xf_mul(o, q);
  }
  Xf ex = xf_shfl_up(q, 1);
  if (lane == 0) ex = xf_identity();
  if (NW > 1) {   // the wavefronts in front of mine: their products in order, then mine
    if (lane == PT_WAVE - 1) {
#pragma unroll
      for (int i = 0; i < 9; ++i) wave_total[wave][i] = q.r[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) wave_total[wave][9 + i] = q.t[i];
    }
    __syncthreads();
    if (wave > 0) {
      Xf pre;
#pragma unroll
      for (int i = 0; i < 9; ++i) pre.r[i] = wave_total[0][i];
#pragma unroll
      for (int i = 0; i < 3; ++i) pre.t[i] = wave_total[0][9 + i];
      for (int v = 1; v < wave; ++v) {
        Xf nx;
#pragma unroll
        for (int i = 0; i < 9; ++i) nx.r[i] = wave_total[v][i];
#pragma unroll
        for (int i = 0; i < 3; ++i) nx.t[i] = wave_total[v][9 + i];
        pre = xf_mul(pre, nx);
      }
      ex = xf_mul(pre, ex);
    }
  }

  // init_bb (StructureBuilder.py:181-191) and the frame of the first placement (N_1 from N_0, CA_0, C_0)
  const V3 pN = {0.f, 0.f, 0.001f};
  const V3 pCA = {pN.x + BL_N_CA, pN.y + 0.f, pN.z + 0.f};
  const float a03 = ang[3];
  const V3 pC = {pCA.x + cosf(PI_F - a03) * BL_CA_C, pCA.y + sinf(PI_F - a03) * BL_CA_C, pCA.z + 0.f};
  Xf g;
  {
    float n0, n1, n2;
    const V3 W = unit(pCA - pN, n0), x = unit(pC - pCA, n1);
    const V3 z = unit(cross(W, x), n2), y = cross(z, x);
    g.r[0] = x.x; g.r[1] = y.x; g.r[2] = z.x;
    g.r[3] = x.y; g.r[4] = y.y; g.r[5] = z.y;
    g.r[6] = x.z; g.r[7] = y.z; g.r[8] = z.z;
    g.t[0] = pC.x; g.t[1] = pC.y; g.t[2] = pC.z;
  }
  if (tid == 0) {
    st3(crd + 0, pN);
    st3(crd + 3, pCA);
    st3(crd + 6, pC);
  }
  g = xf_mul(g, ex);

  // pass 2: walk my chunk from its prefix, emitting the atoms
  for (int p = p0; p < p1; ++p) {
    int res, cth, cchi, slot;
    float l;
    placement_params(p, res, cth, cchi, l, slot);
    const float4 tr = trig[(p - p0) * NT + tid];
    g = xf_mul(g, xf_local(l, tr.x, tr.y, tr.z, tr.w));
    const int i = 1 + p / 3;
    float *o = crd + (size_t)i * RES + slot * 3;
    o[0] = g.t[0];
    o[1] = g.t[1];
    o[2] = g.t[2];
  }
}

// ------------------------------------------------------------------------------------------------
// O + side chain, forward. one lane per residue; grid.x = ceil(L/64), grid.y = B
constexpr int SC_BLOCK = 64;
#define PTS(slot, comp) pts[((slot) * 3 + (comp)) * SC_BLOCK + tid]
#define GRD(slot, comp) grd[((slot) * 3 + (comp)) * SC_BLOCK + tid]

__device__ __forceinline__ V3 lds_get(const float *pts, int slot, int tid) {
  return {PTS(slot, 0), PTS(slot, 1), PTS(slot, 2)};
}
__device__ __forceinline__ void lds_put(float *pts, int slot, int tid, V3 v) {
  PTS(slot, 0) = v.x;
  PTS(slot, 1) = v.y;
  PTS(slot, 2) = v.z;
}

__global__ __launch_bounds__(SC_BLOCK) void nerf_sidechain_fwd_kernel(const float *__restrict__ ang,
                                                                      const int64_t *__restrict__ seq, int L,
                                                                      float *__restrict__ crd) {
  __shared__ float pts[14 * 3 * SC_BLOCK];
  __shared__ int s_len;
  const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * SC_BLOCK + tid;
  ang += (size_t)b * L * 12;
  seq += (size_t)b * L;
  crd += (size_t)b * L * 42;
  {
    int32_t dummy = 0;
    int len = protein_len(seq, L, tid, &dummy);
    if (tid == 0) s_len = len;
  }
  __syncthreads();
  const int len = s_len;
  if (i >= L) return;
  float *out = crd + (size_t)i * 42;
  if (i >= len || len < 2) {
    for (int k = 0; k < 42; ++k) out[k] = 0.f;
    return;
  }
  int res = (int)seq[i];
  if (res < 0 || res > 19) res = 5;  // flagged by the backbone kernel; build it as GLY
  const float *a = ang + (size_t)i * 12;
  V3 N = ld3(out), CA = ld3(out + 3), C = ld3(out + 6);
  lds_put(pts, 0, tid, N);
  lds_put(pts, 1, tid, CA);
  lds_put(pts, 2, tid, C);
  float s, c, st, ct;
  // O = nerf(N, CA, C; c-o, 2.0944, psi - pi)   (StructureBuilder.py:170-173,188-190)
  sincosf(BA_CA_C_O, &st, &ct);
  sincosf(a[1] - PI_F, &s, &c);
  st3(out + 9, place(N, CA, C, BL_C_O, st, ct, s, c));
  V3 ext = (i == 0) ? ld3(out + 42) /* N of residue 1 */ : ld3(out - 42 + 6) /* C of residue i-1 */;
  const int nsc = c_pt_nsc[res];
  float last = 0.f;
  for (int k = 0; k < nsc; ++k) {
    const PtScAtom at = c_pt_sc[res][k];
    V3 pa, pb, pc;
    if (k == 0) {
      if (i == 0) {
        pa = ext; pb = C; pc = CA;
      } else {
        pa = ext; pb = N; pc = CA;
      }
    } else {
      pa = lds_get(pts, at.pa, tid);
      pb = lds_get(pts, at.pb, tid);
      pc = lds_get(pts, at.pc, tid);
    }
    float chi = at.kind == PT_TORS_PRED ? a[6 + (k < 6 ? k : 5)] : (at.kind == PT_TORS_INFER ? last - PI_F : at.tors_const);
    sincosf(at.angle, &st, &ct);
    sincosf(chi, &s, &c);
    V3 d = place(pa, pb, pc, at.bond, st, ct, s, c);
    lds_put(pts, 4 + k, tid, d);
    st3(out + (4 + k) * 3, d);
    last = chi;
  }
  for (int k = (4 + nsc) * 3; k < 42; ++k) out[k] = 0.f;
}

// ------------------------------------------------------------------------------------------------
// O + side chain, adjoint.  Writes dang[b,i,:] (chi columns, psi from O, zeros elsewhere) and
// gbb[b,i,0..11] = adjoints flowing into (N, CA, C, ext) where ext = C_{i-1} (i>=1) or N_1 (i==0).
__global__ __launch_bounds__(SC_BLOCK) void nerf_sidechain_bwd_kernel(const float *__restrict__ ang,
                                                                      const int64_t *__restrict__ seq,
                                                                      const float *__restrict__ crd,
                                                                      const float *__restrict__ dcrd, int L,
                                                                      float *__restrict__ dang,
                                                                      float *__restrict__ gbb) {
  __shared__ float pts[14 * 3 * SC_BLOCK];
  __shared__ float grd[14 * 3 * SC_BLOCK];
  __shared__ int s_len;
  const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * SC_BLOCK + tid;
  ang += (size_t)b * L * 12;
  seq += (size_t)b * L;
  crd += (size_t)b * L * 42;
  dcrd += (size_t)b * L * 42;
  dang += (size_t)b * L * 12;
  gbb += (size_t)b * L * 12;
  {
    int32_t dummy = 0;
    int len = protein_len(seq, L, tid, &dummy);
    if (tid == 0) s_len = len;
  }
  __syncthreads();
  const int len = s_len;
  if (i >= L) return;
  float *da = dang + (size_t)i * 12;
  float *gb = gbb + (size_t)i * 12;
  if (i >= len || len < 2) {
    for (int k = 0; k < 12; ++k) {
      da[k] = 0.f;
      gb[k] = 0.f;
    }
    return;
  }
  int res = (int)seq[i];
  if (res < 0 || res > 19) res = 5;
  const float *a = ang + (size_t)i * 12;
  const float *p = crd + (size_t)i * 42;
  const float *g = dcrd + (size_t)i * 42;
  const int nsc = c_pt_nsc[res];
  for (int s = 0; s < 4 + nsc; ++s) {
    lds_put(pts, s, tid, ld3(p + s * 3));
    lds_put(grd, s, tid, ld3(g + s * 3));
  }
  V3 ext = (i == 0) ? ld3(p + 42) : ld3(p - 42 + 6);
  V3 gext = {0.f, 0.f, 0.f};
  float dchi[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // chi of every atom is needed before walking backwards ('i' atoms depend on the previous torsion)
  for (int k = nsc - 1; k >= 0; --k) {
    const PtScAtom at = c_pt_sc[res][k];
    float chi;
    int src;  // angle column that receives d/dchi, -1 for constants
    if (at.kind == PT_TORS_PRED) {
      chi = a[6 + (k < 6 ? k : 5)];
      src = k;
    } else if (at.kind == PT_TORS_INFER) {
      const PtScAtom pv = c_pt_sc[res][k - 1];  // planar partners always follow a predicted torsion
      chi = (pv.kind == PT_TORS_PRED ? a[6 + (k - 1 < 6 ? k - 1 : 5)] : pv.tors_const) - PI_F;
      src = pv.kind == PT_TORS_PRED ? k - 1 : -1;
    } else {
      chi = at.tors_const;
      src = -1;
    }
    float st, ct, s, c;
    sincosf(at.angle, &st, &ct);
    sincosf(chi, &s, &c);
    V3 gd = lds_get(grd, 4 + k, tid);
    V3 ga = {0, 0, 0}, gbv = {0, 0, 0}, gc = {0, 0, 0};
    float gth = 0.f, gchi = 0.f;
    if (k == 0) {
      V3 pb = (i == 0) ? lds_get(pts, 2, tid) : lds_get(pts, 0, tid);
      V3 pc = lds_get(pts, 1, tid);
      place_bwd(ext, pb, pc, at.bond, st, ct, s, c, gd, ga, gbv, gc, gth, gchi);
      gext = gext + ga;
      int sb = (i == 0) ? 2 : 0;
      lds_put(grd, sb, tid, lds_get(grd, sb, tid) + gbv);
      lds_put(grd, 1, tid, lds_get(grd, 1, tid) + gc);
    } else {
      place_bwd(lds_get(pts, at.pa, tid), lds_get(pts, at.pb, tid), lds_get(pts, at.pc, tid), at.bond, st, ct, s, c,
                gd, ga, gbv, gc, gth, gchi);
      lds_put(grd, at.pa, tid, lds_get(grd, at.pa, tid) + ga);
      lds_put(grd, at.pb, tid, lds_get(grd, at.pb, tid) + gbv);
      lds_put(grd, at.pc, tid, lds_get(grd, at.pc, tid) + gc);
    }
    if (src >= 0 && src < 6) dchi[src] += gchi;
  }
  // O
  float dpsi = 0.f;
  {
    float st, ct, s, c, gth = 0.f;
    sincosf(BA_CA_C_O, &st, &ct);
    sincosf(a[1] - PI_F, &s, &c);
    V3 ga = {0, 0, 0}, gbv = {0, 0, 0}, gc = {0, 0, 0};
    place_bwd(lds_get(pts, 0, tid), lds_get(pts, 1, tid), lds_get(pts, 2, tid), BL_C_O, st, ct, s, c,
              lds_get(grd, 3, tid), ga, gbv, gc, gth, dpsi);
    lds_put(grd, 0, tid, lds_get(grd, 0, tid) + ga);
    lds_put(grd, 1, tid, lds_get(grd, 1, tid) + gbv);
    lds_put(grd, 2, tid, lds_get(grd, 2, tid) + gc);
  }
  da[0] = 0.f;
  da[1] = dpsi;
  da[2] = da[3] = da[4] = da[5] = 0.f;
  for (int k = 0; k < 6; ++k) da[6 + k] = dchi[k];
  st3(gb + 0, lds_get(grd, 0, tid));
  st3(gb + 3, lds_get(grd, 1, tid));
  st3(gb + 6, lds_get(grd, 2, tid));
  st3(gb + 9, gext);
}

// ------------------------------------------------------------------------------------------------
// Backbone chain, adjoint, as SUFFIX SUMS of force and torque.
//
// With the side chains and O already folded onto the backbone atoms (gbb), let g_j = dL/dP_j for the 3*len chain
// atoms.  Changing chi_k (theta_k) rotates every atom placed at or after k rigidly about the axis x_k (a_k)
// through c_k = P_{k-1}, where x_k is the b->c bond direction and a_k = sin(chi) y_k - cos(chi) z_k is the
// normal of the plane (b, c, d).  Hence, with F_k = sum_{j>=k} g_j and T_k = sum_{j>=k} P_j x g_j,
//     dL/dchi_k = x_k . (T_k - c_k x F_k)        dL/dtheta_k = a_k . (T_k - c_k x F_k).
// F and T are plain running sums: each lane reduces a contiguous chunk (fp64), one wave-wide suffix scan joins
// the chunks, each lane walks its chunk backwards.  This is the exact derivative of the same chain function the
// reference differentiates with autograd; the graph quirks come for free: P_0..P_2 are constants (first C is
// detached, StructureBuilder.py:185-187), so only placements k >= 3 receive gradients, and the last residue's
// omega / CA-C-N / C-N-CA have nothing downstream.
// BB (backbone-only adjoint): crd and gbb are the compact [3 L, 3] coordinates and their gradient - chain atom j at 3 j, nothing
// hangs off the backbone
template <bool BB>
__device__ __forceinline__ void chain_atom(const float *__restrict__ crd, const float *__restrict__ gbb, int len, int j,
                                           V3 &P, V3 &g) {
  if (BB) {
    P = ld3(crd + (size_t)j * 3);
    g = ld3(gbb + (size_t)j * 3);
    return;
  }
  const int i = j / 3, a = j - 3 * i;
  P = ld3(crd + (size_t)i * 42 + a * 3);
  g = ld3(gbb + (size_t)i * 12 + a * 3);
  if (a == 2 && i + 1 < len) g = g + ld3(gbb + (size_t)(i + 1) * 12 + 9);  // CB of residue i+1 hangs off C_i
  if (j == 3) g = g + ld3(gbb + 9);                                        // CB of residue 0 hangs off N_1
}

// (NW wavefronts per protein, as in the forward kernel: the suffix sums of the later wavefronts come through LDS)
// BB: gbb = dL/d(compact coordinates) itself; every channel of dang is written here (zeros where nothing flows: the side-chain
// torsions, the channels the reference's graph leaves out), no kernel runs in front
template <int NW, bool BB>
__global__ __launch_bounds__(PT_WAVE * NW) void nerf_backbone_bwd_kernel(const float *__restrict__ ang,
                                                                         const int64_t *__restrict__ seq,
                                                                         const float *__restrict__ crd,
                                                                         const float *__restrict__ gbb, int L,
                                                                         float *__restrict__ dang) {
  constexpr int NT = PT_WAVE * NW;
  __shared__ double wave_total[NW][6];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (PT_WAVE - 1), wave = tid / PT_WAVE;
  ang += (size_t)b * L * 12;
  seq += (size_t)b * L;
  crd += (size_t)b * L * (BB ? 9 : 42);
  gbb += (size_t)b * L * (BB ? 9 : 12);
  dang += (size_t)b * L * 12;
  int32_t dummy = 0;
  const int len = protein_len(seq, L, lane, &dummy);
  if (BB) {   // the zeros first, behind a barrier: an angle that receives a gradient is stored once more below, by another thread
    for (int k = tid; k < L * 12; k += NT) dang[k] = 0.f;
    __syncthreads();
  }
  if (len < 2) return;
  const int n = 3 * len, chunk = (n + NT - 1) / NT;
  const int j0 = min(n, tid * chunk), j1 = min(n, j0 + chunk);

  double F[3] = {0, 0, 0}, T[3] = {0, 0, 0};
  for (int j = j0; j < j1; ++j) {
    V3 P, g;
    chain_atom<BB>(crd, gbb, len, j, P, g);
    F[0] += g.x; F[1] += g.y; F[2] += g.z;
    T[0] += (double)P.y * g.z - (double)P.z * g.y;
    T[1] += (double)P.z * g.x - (double)P.x * g.z;
    T[2] += (double)P.x * g.y - (double)P.y * g.x;
  }
  // inclusive suffix scan over lanes, then shift: (F, T) = contribution of all LATER lanes
#pragma unroll
  for (int d = 1; d < PT_WAVE; d <<= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double of = __shfl_down(F[c], d, 64), ot = __shfl_down(T[c], d, 64);
      if (lane + d < PT_WAVE) {
        F[c] += of;
        T[c] += ot;
      }
    }
  }
  if (NW > 1 && lane == 0) {   // my wavefront's total, for the wavefronts in front of it
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wave_total[wave][c] = F[c];
      wave_total[wave][3 + c] = T[c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double of = __shfl_down(F[c], 1, 64), ot = __shfl_down(T[c], 1, 64);
    F[c] = lane + 1 < PT_WAVE ? of : 0.0;
    T[c] = lane + 1 < PT_WAVE ? ot : 0.0;
  }
  if (NW > 1) {
    __syncthreads();
    for (int v = wave + 1; v < NW; ++v) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        F[c] += wave_total[v][c];
        T[c] += wave_total[v][3 + c];
      }
    }
  }
  for (int j = j1 - 1; j >= j0; --j) {
    V3 P, g;
    chain_atom<BB>(crd, gbb, len, j, P, g);
    F[0] += g.x; F[1] += g.y; F[2] += g.z;
    T[0] += (double)P.y * g.z - (double)P.z * g.y;
    T[1] += (double)P.z * g.x - (double)P.x * g.z;
    T[2] += (double)P.x * g.y - (double)P.y * g.x;
    if (j < 3) continue;
    int res, cth, cchi, slot;
    float l;
    placement_params(j - 3, res, cth, cchi, l, slot);
    const int ia = (j - 3) / 3, ib = (j - 2) / 3, ic = (j - 1) / 3;
    const V3 pa = ld3(BB ? crd + (size_t)(j - 3) * 3 : crd + (size_t)ia * 42 + ((j - 3) - 3 * ia) * 3);
    const V3 pb = ld3(BB ? crd + (size_t)(j - 2) * 3 : crd + (size_t)ib * 42 + ((j - 2) - 3 * ib) * 3);
    const V3 pc = ld3(BB ? crd + (size_t)(j - 1) * 3 : crd + (size_t)ic * 42 + ((j - 1) - 3 * ic) * 3);
    float n0, n1, n2;
    const V3 W = unit(pb - pa, n0), x = unit(pc - pb, n1);
    const V3 z = unit(cross(W, x), n2), y = cross(z, x);
    float sx, cx;
    sincosf(ang[res * 12 + cchi], &sx, &cx);
    const V3 ax = {sx * y.x - cx * z.x, sx * y.y - cx * z.y, sx * y.z - cx * z.z};
    const double tq0 = T[0] - ((double)pc.y * F[2] - (double)pc.z * F[1]);
    const double tq1 = T[1] - ((double)pc.z * F[0] - (double)pc.x * F[2]);
    const double tq2 = T[2] - ((double)pc.x * F[1] - (double)pc.y * F[0]);
    const float dchi = (float)(x.x * tq0 + x.y * tq1 + x.z * tq2);
    const float dth = (float)(ax.x * tq0 + ax.y * tq1 + ax.z * tq2);
    dang[res * 12 + cth] = dth;
    if (!BB && cchi == 1) dang[res * 12 + 1] += dchi;  // psi also placed O (the side-chain kernel wrote that part)
    else dang[res * 12 + cchi] = dchi;
  }
}

// ------------------------------------------------------------------------------------------------
// stand-alone helpers of the public API: batched single placements and an explicit distance matrix
__global__ void nerf_place_kernel(const float *__restrict__ a, const float *__restrict__ b, const float *__restrict__ c,
                                  const float *__restrict__ l, const float *__restrict__ theta,
                                  const float *__restrict__ chi, int64_t n, float *__restrict__ d,
                                  int32_t *__restrict__ status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float th = theta[i];
  if (!(fabsf(th) <= PI_F)) atomicOr(status, PTAMD_ST_BAD_THETA);
  float st, ct, sx, cx;
  sincosf(th, &st, &ct);
  sincosf(chi[i], &sx, &cx);
  st3(d + i * 3, place(ld3(a + i * 3), ld3(b + i * 3), ld3(c + i * 3), l[i], st, ct, sx, cx));
}

// losses.py:233-253 by direct differences: out[i][j] = sqrt(max(|x_i - x_j|^2, 1e-30))
__global__ void pairwise_dist_kernel(const float *__restrict__ x, int n, int dim, float *__restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (j >= n) return;
  float s = 0.f;
  for (int k = 0; k < dim; ++k) {
    const float d = x[(size_t)i * dim + k] - x[(size_t)j * dim + k];
    s += d * d;
  }
  out[(size_t)i * n + j] = sqrtf(fmaxf(s, 1e-30f));
}

}  // namespace

// ================================================================================================
// Wavefronts per protein of the two backbone-chain kernels.  The ADJOINT runs on four (its fp64 sums do not care how they are
// cut).  The FORWARD chain stays on one: four re-round the backbone in another order - by 1e-6 ... 1e-5 A, inside every
// tolerance - but the side-chain builder behind it follows the reference's cross products, which amplify such a difference by
// up to 1 / |sin| of a backbone bond angle on arbitrary (random-init) angles: one L = 200 protein of the parity record's config-5
// draws moved from 0.75 to 16 units of 1.6e-3 A (the reference's own fp32 chain: 2.4), past that record's bar - not worth 12 us.
constexpr int FWD_CHAIN_WAVES = 1, BWD_CHAIN_WAVES = 4;

namespace {
// the backbone scan, into the 14-slot layout (BB = false) or the compact backbone array (BB = true)
template <bool BB>
int launch_backbone_fwd(const float *ang, const int64_t *seq, int B, int L, float *crd, int32_t *status, void *stream) {
  constexpr int nt = PT_WAVE * FWD_CHAIN_WAVES;
  const size_t lds = (size_t)((3 * L + nt - 1) / nt) * nt * sizeof(float4);  // trig cache of the scan
  auto kern = nerf_backbone_fwd_kernel<FWD_CHAIN_WAVES, BB>;
  if (lds > 48 * 1024) {
    PT_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipLaunchKernelGGL(kern, dim3(B), dim3(nt), lds, (hipStream_t)stream, ang, seq, L, crd, status);
  return pt_check_launch();
}
}  // namespace

extern "C" {

int ptamd_sidechain_atoms(int residue) { return (residue < 0 || residue > 19) ? -1 : h_pt_nsc[residue]; }

int ptamd_angles_fwd(const float *sincos, float *ang, int64_t n, void *stream) {
  if (n < 0) return PTAMD_ERR_BAD_SHAPE;
  if (n == 0) return PTAMD_OK;
  hipLaunchKernelGGL(angles_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2 *>(sincos), ang, n);
  return pt_check_launch();
}

int ptamd_angles_bwd(const float *sincos, const float *dang, float *dsincos, int64_t n, void *stream) {
  if (n < 0) return PTAMD_ERR_BAD_SHAPE;
  if (n == 0) return PTAMD_OK;
  hipLaunchKernelGGL(angles_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const float2 *>(sincos), dang, reinterpret_cast<float2 *>(dsincos), n);
  return pt_check_launch();
}

int ptamd_nerf_place(const float *a, const float *b, const float *c, const float *l, const float *theta,
                     const float *chi, int64_t n, float *d, int32_t *status, void *stream) {
  if (n <= 0) return PTAMD_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(nerf_place_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, c, l,
                     theta, chi, n, d, status);
  return pt_check_launch();
}

int ptamd_pairwise_dist(const float *x, int n, int dim, float *out, void *stream) {
  if (n <= 0 || dim <= 0 || n > 65535) return PTAMD_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(pairwise_dist_kernel, dim3((n + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, x, n, dim, out);
  return pt_check_launch();
}

size_t ptamd_nerf_workspace_bytes(int B, int L) { return (size_t)(B > 0 ? B : 0) * (L > 0 ? L : 0) * 12 * sizeof(float); }

int ptamd_nerf_fwd(const float *ang, const int64_t *seq, int B, int L, float *crd, int32_t *status, void *stream) {
  if (B <= 0 || L <= 0) return PTAMD_ERR_BAD_SHAPE;
  if (L > MAX_L_CHAIN) return PTAMD_ERR_TOO_LONG;
  int rc = launch_backbone_fwd<false>(ang, seq, B, L, crd, status, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(nerf_sidechain_fwd_kernel, dim3((L + SC_BLOCK - 1) / SC_BLOCK, B), dim3(SC_BLOCK), 0,
                     (hipStream_t)stream, ang, seq, L, crd);
  return pt_check_launch();
}

int ptamd_nerf_bb_fwd(const float *ang, const int64_t *seq, int B, int L, float *crd_bb, int32_t *status, void *stream) {
  if (B <= 0 || L <= 0) return PTAMD_ERR_BAD_SHAPE;
  if (L > MAX_L_CHAIN) return PTAMD_ERR_TOO_LONG;
  return launch_backbone_fwd<true>(ang, seq, B, L, crd_bb, status, stream);
}

int ptamd_nerf_bb_bwd(const float *ang, const int64_t *seq, const float *crd_bb, const float *dcrd_bb, int B, int L,
                      float *dang, void *stream) {
  if (B <= 0 || L <= 0) return PTAMD_ERR_BAD_SHAPE;
  if (L > MAX_L_CHAIN) return PTAMD_ERR_TOO_LONG;
  auto kern = nerf_backbone_bwd_kernel<BWD_CHAIN_WAVES, true>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(PT_WAVE * BWD_CHAIN_WAVES), 0, (hipStream_t)stream, ang, seq, crd_bb, dcrd_bb, L, dang);
  return pt_check_launch();
}

int ptamd_nerf_bwd(const float *ang, const int64_t *seq, const float *crd, const float *dcrd, int B, int L,
                   float *dang, void *workspace, size_t workspace_bytes, void *stream) {
  if (B <= 0 || L <= 0) return PTAMD_ERR_BAD_SHAPE;
  if (L > MAX_L_CHAIN) return PTAMD_ERR_TOO_LONG;
  if (!workspace || workspace_bytes < ptamd_nerf_workspace_bytes(B, L)) return PTAMD_ERR_WORKSPACE;
  float *gbb = static_cast<float *>(workspace);
  hipLaunchKernelGGL(nerf_sidechain_bwd_kernel, dim3((L + SC_BLOCK - 1) / SC_BLOCK, B), dim3(SC_BLOCK), 0,
                     (hipStream_t)stream, ang, seq, crd, dcrd, L, dang, gbb);
  int rc = pt_check_launch();
  if (rc) return rc;
  auto kern = nerf_backbone_bwd_kernel<BWD_CHAIN_WAVES, false>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(PT_WAVE * BWD_CHAIN_WAVES), 0, (hipStream_t)stream, ang, seq, crd, gbb, L, dang);
  return pt_check_launch();
}

}  // extern "C"
