// Frame-aligned error matrix of K structures around a reference, for gfx950: entry (i, j) is how far the C-alpha of residue j
// lies from where the reference has it once both structures are seen from the backbone frame of residue i - AlphaFold's aligned
// error (Jumper et al., Nature 596:583-589 (2021), supplementary 1.9.7), taken here over a dropout ensemble
// (`ensemble.predict_ensemble(..., aligned_error=True)`, `predict --pae`) or against a native structure (K = 1, the truth as the
// reference: `eval_metrics.aligned_error_batch`, `score --aligned_error`).
//
// The reference (protein_transformer) has no counterpart.  csrc/ensemble.hip fits every sample ONCE, globally; a changed phi / psi
// at one residue, which swings everything behind it, is smeared over the whole chain by that fit.  Here every residue's own frame
// is the fit, so a hinge shows as two blocks.  The definition - frames, points, usable samples, the NaN cases, the two stats - is
// in include/ptamd.h; this file restates only what the kernels do with it.
//
// Three launches per batch:
//   records   ONE WAVEFRONT PER (protein, structure), structure 0 being the reference, 64 residues per step.  Lane = residue
//             reads N, CA, C where they lie (36 bytes of a 168-byte row, as csrc/ensemble.hip reads its C-alphas), builds the frame
//             (csrc/backbone_frame.h) and writes a 64-byte record {CA, validity bits, e1, e2, e3} into the workspace.  The
//             reference's wavefront ballots its frames and points into counts[b]; a sample's wavefront tests the reference's
//             residues again - the same device function on the same floats, so the same verdict - and settles whether the sample
//             is usable.  No wavefront waits for another.
//   tiles     ONE WORKGROUP OF FOUR WAVEFRONTS PER TILE of 64 frames x 64 points of a protein.  Lane = point (column), a
//             wavefront owns 16 frames (rows): a row of the tile leaves as 256 contiguous bytes.  The records of the tile's frames
//             and points are staged in LDS with one coalesced 16-byte read per thread; a frame is read from LDS by all lanes at one
//             address (a broadcast, no bank conflict).  The reference's local coordinates stay in registers (48), one fp32
//             accumulator per row (16) takes the usable samples in the order k = 0 .. K - 1.  Each row's defined entries are then
//             summed over the 64 lanes in fp64 by a butterfly - the mean's and the TM term's partial sum per (row, column tile).
//   finalize  ONE WAVEFRONT PER PROTEIN adds the partial sums in a fixed order (column tiles, then rows by lane, then the
//             butterfly), takes the best row, and writes stats[b] and usable[b].
// x_ij is `backbone_frame::local_coords` for the reference and for a sample alike; the norm is fp32 without an epsilon.  No
// atomics, no order-dependent reduction: two runs give the same bits.
#include <limits.h>
#include <math.h>

#include "backbone_frame.h"
#include "common.h"

namespace {

using backbone_frame::Frame;

constexpr int N_SLOT = 0;                         // N, CA, C of a residue are slots 0, 1, 2: nine consecutive floats
constexpr int TS = 64;                            // frames and points per tile = lanes of a wavefront
constexpr int WAVES = 4;                          // wavefronts per tile
constexpr int RPW = TS / WAVES;                   // rows (frames) per wavefront
constexpr int ROW = PTAMD_NUM_SLOTS * 3;          // floats of a residue in memory
constexpr int NRES = 20;
constexpr float CRD_MAX = 1.0e18f;                // beyond this a coordinate is unusable (csrc/atom_tiles.h)
constexpr int IS_FRAME = 1, IS_POINT = 2;

struct __attribute__((aligned(16))) Rec {   // 64 bytes per (protein, structure, residue): four float4
  float ca[3];                              // the point, and the frame's origin
  int flags;                                // IS_FRAME | IS_POINT (the reference's records; 0 in a sample's)
  float e[9];                               // e1, e2, e3
  float pad[3];
};
static_assert(sizeof(Rec) == 64, "a record is four float4");

struct Counts {   // per protein, from the reference
  int nframes, npoints;
};

inline int tiles_of(int L) { return (L + TS - 1) / TS; }
inline bool ae_shape_ok(int B, int K, int L) {
  if (!(B > 0 && K > 0 && L > 0 && L <= INT_MAX / 28)) return false;
  const int64_t t = tiles_of(L);
  // (a launch addresses fewer than 2^32 threads: 256 per tile)
  return (int64_t)B * ((int64_t)K + 1) <= INT_MAX && (int64_t)B * t * t <= INT_MAX / (TS * WAVES);
}
inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
// workspace: records [B, K + 1, L] | sample-usable flags [B, K] | counts [B] | partial sums [B, tiles, L] of double2
struct Layout {
  size_t rec, flag, counts, part, total;
};
inline Layout layout_of(int B, int K, int L) {
  Layout y;
  y.rec = 0;
  y.flag = y.rec + align256((size_t)B * ((size_t)K + 1) * L * sizeof(Rec));
  y.counts = y.flag + align256((size_t)B * K * sizeof(int));
  y.part = y.counts + align256((size_t)B * sizeof(Counts));
  y.total = y.part + align256((size_t)B * tiles_of(L) * L * sizeof(double2));
  return y;
}

__device__ __forceinline__ bool usable3(const float *p) {   // (NaN fails every test)
  return fabsf(p[0]) <= CRD_MAX && fabsf(p[1]) <= CRD_MAX && fabsf(p[2]) <= CRD_MAX;
}

// ---- launch 1
// N, CA, C of residue r (zeros for r >= L), the frame they span, and what the residue is: a frame, a point
__device__ __forceinline__ int classify(const float *__restrict__ crd, int r, int L, bool present, float (&p)[9], Frame &f) {
#pragma unroll
  for (int u = 0; u < 9; ++u) p[u] = 0.f;
  if (r < L) {
    const float *src = crd + ((size_t)r * PTAMD_NUM_SLOTS + N_SLOT) * 3;
#pragma unroll
    for (int u = 0; u < 9; ++u) p[u] = src[u];
  }
  const bool spans = backbone_frame::build_frame(p, f);
  const bool point = present && usable3(p + 3);
  const bool frame = point && usable3(p) && usable3(p + 6) && spans;
  return (frame ? IS_FRAME : 0) | (point ? IS_POINT : 0);
}

__global__ __launch_bounds__(64) void ae_records_kernel(const float *__restrict__ ref, const float *__restrict__ samples,
                                                        const int64_t *__restrict__ seq, int K, int L, Rec *__restrict__ rec,
                                                        int *__restrict__ sample_ok, Counts *__restrict__ counts) {
  const int b = blockIdx.x / (K + 1), s = blockIdx.x - b * (K + 1), lane = threadIdx.x;   // s = 0: the reference
  const size_t nfl = (size_t)L * ROW;
  ref += (size_t)b * nfl;
  if (s > 0) samples += ((size_t)b * K + (s - 1)) * nfl;
  seq += (size_t)b * L;
  rec += (size_t)blockIdx.x * L;
  int nframes = 0, npoints = 0;   // (wavefront-uniform)
  bool bad = false;
  for (int r0 = 0; r0 < L; r0 += 64) {
    const int r = r0 + lane;
    bool present = false;
    if (r < L) {
      const int64_t type = seq[r];
      present = type >= 0 && type < NRES;
    }
    float p[9];
    Frame f;
    int flags = classify(ref, r, L, present, p, f);
    if (s == 0) {
      nframes += __popcll(__ballot((flags & IS_FRAME) != 0));
      npoints += __popcll(__ballot((flags & IS_POINT) != 0));
    } else {
      const int mine = classify(samples, r, L, present, p, f);
      bad = bad || (flags & ~mine) != 0;   // a frame or a point of the reference that the sample does not have
      flags = 0;
    }
    if (r < L) {
      float4 *out = reinterpret_cast<float4 *>(rec + r);
      out[0] = make_float4(p[3], p[4], p[5], __int_as_float(flags));
      out[1] = make_float4(f.e[0], f.e[1], f.e[2], f.e[3]);
      out[2] = make_float4(f.e[4], f.e[5], f.e[6], f.e[7]);
      out[3] = make_float4(f.e[8], 0.f, 0.f, 0.f);
    }
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
    if (s == 0) {
      Counts c;
      c.nframes = nframes;
      c.npoints = npoints;
      counts[b] = c;
    } else {
      sample_ok[(size_t)b * K + (s - 1)] = any_bad ? 0 : 1;
    }
  }
}

// ---- launch 2
// the records of `rows` residues, one float4 per thread, into LDS; zeros behind the last residue
__device__ __forceinline__ void stage(float4 *__restrict__ dst, const Rec *__restrict__ src, int rows, int tid) {
  dst[tid] = tid < rows * 4 ? reinterpret_cast<const float4 *>(src)[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
}
// {CA, flags} of `cols` residues, one per lane of the first wavefront
__device__ __forceinline__ void stage_points(float4 *__restrict__ dst, const Rec *__restrict__ src, int cols, int tid) {
  if (tid < TS) dst[tid] = tid < cols ? *reinterpret_cast<const float4 *>(src + tid) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ Frame frame_of(const float4 *__restrict__ r) {
  const float4 a = r[0], e0 = r[1], e1 = r[2], e2 = r[3];
  Frame f;
  f.e[0] = e0.x; f.e[1] = e0.y; f.e[2] = e0.z; f.e[3] = e0.w;
  f.e[4] = e1.x; f.e[5] = e1.y; f.e[6] = e1.z; f.e[7] = e1.w;
  f.e[8] = e2.x;
  f.t[0] = a.x; f.t[1] = a.y; f.t[2] = a.z;
  return f;
}

__global__ __launch_bounds__(TS * WAVES) void ae_tile_kernel(const Rec *__restrict__ rec, const int *__restrict__ sample_ok,
                                                             const Counts *__restrict__ counts, int K, int L, int tiles,
                                                             float *__restrict__ ae, double2 *__restrict__ part) {
  __shared__ float4 s_frames[TS * 4], s_points[TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / (tiles * tiles), rest = blockIdx.x - b * (tiles * tiles), rt = rest / tiles, ct = rest - rt * tiles;
  const int i0 = rt * TS, j0 = ct * TS, nrows = min(TS, L - i0), ncols = min(TS, L - j0);
  const int row0 = wave * RPW, j = j0 + lane;
  const Rec *mine = rec + (size_t)b * (K + 1) * L;
  stage(s_frames, mine + i0, nrows, tid);
  stage_points(s_points, mine + j0, ncols, tid);
  __syncthreads();
  float xr[RPW][3], acc[RPW];
  unsigned row_is_frame = 0u;   // (wavefront-uniform)
  const bool col_is_point = (__float_as_int(s_points[lane].w) & IS_POINT) != 0;
  {
    const float4 pt = s_points[lane];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const float4 *fr = s_frames + (row0 + r) * 4;
      if (__float_as_int(fr[0].w) & IS_FRAME) row_is_frame |= 1u << r;
      const Frame f = frame_of(fr);
      float dx, dy, dz;
      backbone_frame::local_coords(f, pt.x, pt.y, pt.z, dx, dy, dz, xr[r][0], xr[r][1], xr[r][2]);
      acc[r] = 0.f;
    }
  }
  int kused = 0;   // (uniform over the workgroup: a flag is per (protein, sample))
  for (int k = 0; k < K; ++k) {
    if (sample_ok[(size_t)b * K + k] == 0) continue;
    ++kused;
    __syncthreads();   // the previous structure's records have been read
    stage(s_frames, mine + (size_t)(1 + k) * L + i0, nrows, tid);
    stage_points(s_points, mine + (size_t)(1 + k) * L + j0, ncols, tid);
    __syncthreads();
    const float4 pt = s_points[lane];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const Frame f = frame_of(s_frames + (row0 + r) * 4);
      float dx, dy, dz, lx, ly, lz;
      backbone_frame::local_coords(f, pt.x, pt.y, pt.z, dx, dy, dz, lx, ly, lz);
      const float ex = lx - xr[r][0], ey = ly - xr[r][1], ez = lz - xr[r][2];
      acc[r] += sqrtf(fmaf(ez, ez, fmaf(ey, ey, __fmul_rn(ex, ex))));
    }
  }
  const int npoints = counts[b].npoints;
  const double d0 = 1.24 * cbrt((double)(max(npoints, 19) - 15)) - 1.8;
  const float nan = __builtin_nanf("");
  double keep_sum = 0.0, keep_tm = 0.0;
#pragma unroll
  for (int r = 0; r < RPW; ++r) {
    const int i = i0 + row0 + r;
    const bool defined = kused > 0 && col_is_point && (row_is_frame >> r & 1u) != 0u;
    const float v = defined ? acc[r] / (float)kused : nan;
    if (i < L && j < L) ae[((size_t)b * L + i) * L + j] = v;
    const double q = (double)v / d0;
    const double sum = wave_sum_d(defined ? (double)v : 0.0), tm = wave_sum_d(defined ? 1.0 / (1.0 + q * q) : 0.0);
    if (lane == r) {
      keep_sum = sum;
      keep_tm = tm;
    }
  }
  if (lane < RPW && i0 + row0 + lane < L) part[((size_t)b * tiles + ct) * L + i0 + row0 + lane] = make_double2(keep_sum, keep_tm);
}

// ---- launch 3
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(64) void ae_finalize_kernel(const double2 *__restrict__ part, const int *__restrict__ sample_ok,
                                                         const Counts *__restrict__ counts, int K, int L, int tiles,
                                                         float *__restrict__ stats, int32_t *__restrict__ usable) {
  const int b = blockIdx.x, lane = threadIdx.x;
  double sum = 0.0, best = 0.0;   // a row that is no frame has a TM sum of 0, and a frame's is positive
  for (int i = lane; i < L; i += 64) {
    double row_sum = 0.0, row_tm = 0.0;
    for (int ct = 0; ct < tiles; ++ct) {
      const double2 p = part[((size_t)b * tiles + ct) * L + i];
      row_sum += p.x;
      row_tm += p.y;
    }
    sum += row_sum;
    best = fmax(best, row_tm);
  }
  sum = wave_sum_d(sum);
  best = wave_max_d(best);
  if (lane == 0) {
    int kused = 0;
    for (int k = 0; k < K; ++k) kused += sample_ok[(size_t)b * K + k] != 0 ? 1 : 0;
    const Counts c = counts[b];
    const bool defined = kused > 0 && c.nframes > 0 && c.npoints > 0;
    stats[2 * b] = defined ? (float)(sum / ((double)c.nframes * (double)c.npoints)) : __builtin_nanf("");
    stats[2 * b + 1] = defined ? (float)(best / (double)c.npoints) : __builtin_nanf("");
    usable[b] = kused;
  }
}

}  // namespace

extern "C" {

size_t ptamd_aligned_error_workspace_bytes(int B, int K, int L) {
  if (!ae_shape_ok(B, K, L)) return 0;
  return layout_of(B, K, L).total;
}

int ptamd_aligned_error(const float *ref_crd, const float *sample_crd, const int64_t *seq, int B, int K, int L, float *ae,
                        float *stats, int32_t *usable, void *workspace, size_t workspace_bytes, void *stream) {
  if (!ae_shape_ok(B, K, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!ref_crd || !sample_crd || !seq || !ae || !stats || !usable) return PTAMD_ERR_BAD_SHAPE;
  const Layout y = layout_of(B, K, L);
  if (!workspace || workspace_bytes < y.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  char *ws = static_cast<char *>(workspace);
  Rec *rec = reinterpret_cast<Rec *>(ws + y.rec);
  int *sample_ok = reinterpret_cast<int *>(ws + y.flag);
  Counts *counts = reinterpret_cast<Counts *>(ws + y.counts);
  double2 *part = reinterpret_cast<double2 *>(ws + y.part);
  const int tiles = tiles_of(L);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ae_records_kernel, dim3((unsigned)(B * (K + 1))), dim3(64), 0, st, ref_crd, sample_crd, seq, K, L, rec,
                     sample_ok, counts);
  int rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ae_tile_kernel, dim3((unsigned)(B * tiles * tiles)), dim3(TS * WAVES), 0, st, rec, sample_ok, counts, K, L,
                     tiles, ae, part);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ae_finalize_kernel, dim3((unsigned)B), dim3(64), 0, st, part, sample_ok, counts, K, L, tiles, stats, usable);
  return pt_check_launch();
}

}  // extern "C"
