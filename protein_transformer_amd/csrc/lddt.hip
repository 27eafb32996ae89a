// Batched lDDT (local Distance Difference Test), all-atom and C-alpha, for gfx950: the evaluation metrics `lddt-full` / `lddt-ca`.
//
// The reference (protein_transformer) has no counterpart: its evaluation stops at dRMSD and the superposed RMSD.  This is the
// score of Mariani, Biasini, Barbato & Schwede, "lDDT: a local superposition-free score for comparing protein structures and
// models using distance difference tests", Bioinformatics 29(21):2722-2728 (2013), without the stereochemistry checks of the
// full tool.  Definition (include/ptamd.h repeats it): the atoms of a protein are the slots s of non-pad residues whose true
// coordinate has no NaN (the set of kabsch_rmsd_kernel), an atom's residue is s / 14.  An ordered pair (i, j) of atoms in
// DIFFERENT residues is included if its true distance dt < cutoff and preserved at t in {0.5, 1, 2, 4} if |dp - dt| < t (dp the
// predicted distance; both comparisons strict, both distances sqrt(dx^2 + dy^2 + dz^2) of coordinate DIFFERENCES in fp32).
// counts[r] = {total, p0.5, p1, p2, p4} over the pairs whose i lies in residue r, for set 0 (every atom) and set 1 (C-alpha,
// slot 1, paired with C-alphas only); score = (p0.5 + p1 + p2 + p4) / (4 total), NaN without an included pair.
//
// Three launches per batch behind the zero fill of `counts`:
//   compact   the present atoms of each protein, in slot order, into the caller's workspace, and the bounding box of the true
//             coordinates of every tile of 64 of them: csrc/atom_tiles.h, shared with csrc/slddt.hip.  This file's record
//             marks the C-alphas.  (csrc/drmsd.hip packs differently: the backbone first, for its backbone-only loss.)
//   sweep     all ORDERED pairs (the counts belong to the row atom's residue: nothing flows to the column side, so no column
//             partials and no triangle).  A wavefront owns a row tile of 64 atoms, one per lane, in registers; it walks a chunk
//             of column tiles, skips those whose true bounding box lies farther than the cutoff from its own (no pair of such
//             tiles can be included: counts unchanged), stages a column tile in its own LDS slice and reads the column atoms as
//             broadcasts.  Per pair: 6 subtractions, 6 multiply-adds, 2 v_sqrt_f32, and ONE packed add for the five counters -
//             the thresholds are powers of two, so "|dp - dt| < 2^e" is a test of the difference's exponent field and the
//             number of thresholds passed is a clamp of that field (lddt_sweep_kernel).  Integer counters, a segmented
//             wavefront reduction over the lanes of one residue, one integer atomicAdd per (wavefront, residue, counter):
//             the result does not depend on scheduling.  No fp64, no float atomics.
//   finalize  counts -> per-residue and per-protein scores (64-bit sums over the residues).
#include <math.h>

#include "atom_tiles.h"

namespace {

using namespace atom_tiles;

constexpr int STRIP_TILES = 4;    // row tiles (wavefronts) per workgroup of the sweep
constexpr int CHUNK_TILES = 32;   // column tiles per work item (<= 64: a wavefront keeps its live tiles as one ballot mask)
constexpr int FIN_THREADS = 256;
constexpr int NSET = 2, NCNT = 5;
constexpr int CA_SLOT = 1;
// a row or column lane behind the protein's last atom sits here in the TRUE structure (rows at +FAR, columns at -FAR): every
// distance to it is ~1e19, finite, and fails `dt < cutoff` - no test per pair
constexpr float FAR = 3.0e18f;

// stage 1, atom_tiles::compact_kernel: the sweep reads a compacted atom from LDS as two ds_read_b128 broadcasts;
// code = residue << 1 | (slot == C-alpha), the prediction as it came
struct CaRecord {
  static __device__ __forceinline__ Atom8 make(float px, float py, float pz, float tx, float ty, float tz, int res, int slot) {
    return Atom8{px, py, pz, tx, ty, tz, (res << 1) | (slot - res * PTAMD_NUM_SLOTS == CA_SLOT), 0};
  }
};

// ---- stage 2: the pair sweep.  Workgroup = 4 wavefronts = 4 consecutive row tiles against one chunk of column tiles; the
// wavefronts do not talk to each other (each stages its column tiles in its own LDS slice: no workgroup barrier anywhere).
//
// The five counters of a pair in one add.  With d = |dp - dt| as an fp32 number and E its biased exponent field,
//   d < 2^e  <=>  E < 127 + e     (exact for every non-negative float, zero and denormals included; NaN and inf have E = 255
//                                  and pass nothing - a non-finite predicted coordinate simply fails the comparisons)
// so h = clamp(E, 125, 129) - 125 in 0..4 says which thresholds the pair passes: h = 0 all four (d < 0.5), h = 1 three (d < 1),
// h = 2 two, h = 3 one (d < 4), h = 4 none.  A lane keeps the HISTOGRAM of h over its included pairs in one 32-bit word, five
// fields of 6 bits: the pair adds 1 << 6 h, an excluded pair adds 1 << 30 (h = 5: bits 30, 31 wrap and are never read).  A
// field holds 63; the word is emptied into five full counters every 32 columns.  At the end
//   total = H0 + H1 + H2 + H3 + H4,  p0.5 = H0,  p1 = H0 + H1,  p2 = H0 + H1 + H2,  p4 = H0 + H1 + H2 + H3.
constexpr int FIELD_BITS = 6, FLUSH_COLS = 32, NHIST = 5;

__device__ __forceinline__ void flush_hist(unsigned &packed, int (&hist)[NHIST]) {
#pragma unroll
  for (int k = 0; k < NHIST; ++k) hist[k] += (int)((packed >> (FIELD_BITS * k)) & ((1u << FIELD_BITS) - 1u));
  packed = 0u;
}

__global__ __launch_bounds__(TS * STRIP_TILES) void lddt_sweep_kernel(const Atom8 *__restrict__ atoms,
                                                                      const Box8 *__restrict__ boxes,
                                                                      const int *__restrict__ natoms, int L, int nstride,
                                                                      int tiles, int chunks, float cutoff,
                                                                      int32_t *__restrict__ counts) {
  __shared__ Atom8 s_col[STRIP_TILES][TS];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int strip = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  const int I = strip * STRIP_TILES + w;
  const int J0 = chunk * CHUNK_TILES, J1 = min(nT, J0 + CHUNK_TILES);
  if (I >= nT || J0 >= J1) return;   // wavefront-uniform; no barrier below
  atoms += (size_t)b * nstride;
  boxes += (size_t)b * tiles;

  // which column tiles of the chunk can hold an included pair: lane l tests tile J0 + l against this row tile's box
  unsigned long long todo;
  {
    const Box8 me = boxes[I];
    bool near = false;
    if (J0 + lane < J1) near = boxes_near(me, boxes[J0 + lane], cutoff);
    todo = __ballot(near);
  }
  if (todo == 0ull) return;

  const int i = I * TS + lane;
  Atom8 me = Atom8{0.f, 0.f, 0.f, FAR, FAR, FAR, -2, 0};
  if (i < n) me = atoms[i];
  const bool me_ca = (me.code & 1) != 0;
  Atom8 *const col = s_col[w];
  auto load_tile = [&](int J) __attribute__((always_inline)) {
    const int j = J * TS + lane;
    Atom8 a = Atom8{0.f, 0.f, 0.f, -FAR, -FAR, -FAR, -4, 0};
    if (j < n) a = atoms[j];
    return a;
  };
  auto next_tile = [&]() __attribute__((always_inline)) {   // pops the lowest live tile of the chunk
    const int k = __builtin_ctzll(todo);
    todo &= todo - 1ull;
    return J0 + k;
  };

  int hist[NSET][NHIST];
#pragma unroll
  for (int s = 0; s < NSET; ++s)
#pragma unroll
    for (int k = 0; k < NHIST; ++k) hist[s][k] = 0;
  unsigned packed0 = 0u, packed1 = 0u;

  Atom8 nxt = load_tile(next_tile());
  for (;;) {
    col[lane] = nxt;   // (LDS operations of one wavefront complete in order: the reads of the previous tile are behind us)
    const bool more = todo != 0ull;
    if (more) nxt = load_tile(next_tile());   // in flight while this tile is swept
    for (int j0 = 0; j0 < TS; j0 += FLUSH_COLS) {
#pragma unroll 4
      for (int j = j0; j < j0 + FLUSH_COLS; ++j) {
        const Atom8 c = col[j];   // broadcast
        const float dxt = me.tx - c.tx, dyt = me.ty - c.ty, dzt = me.tz - c.tz;
        const float dxp = me.px - c.px, dyp = me.py - c.py, dzp = me.pz - c.pz;
        const float dt = true_dist(dxt, dyt, dzt), dp = true_dist(dxp, dyp, dzp);
        const bool incl = dt < cutoff && (unsigned)(me.code ^ c.code) > 1u;   // strict; different residues
        const unsigned E = (__float_as_uint(dp - dt) >> 23) & 0xffu;
        const unsigned h = min(max(E, 125u), 129u) - 125u;
        const unsigned inc = 1u << (FIELD_BITS * (incl ? h : (unsigned)NHIST));
        packed0 += inc;
        if (__builtin_amdgcn_readfirstlane(c.code) & 1) packed1 += me_ca ? inc : (1u << (FIELD_BITS * NHIST));   // C-alpha column
      }
      flush_hist(packed0, hist[0]);
      flush_hist(packed1, hist[1]);
    }
    if (!more) break;
  }

  // histogram -> {total, p0.5, p1, p2, p4}
  int v[NSET * NCNT];
#pragma unroll
  for (int s = 0; s < NSET; ++s) {
    const int h0 = hist[s][0], h1 = hist[s][1], h2 = hist[s][2], h3 = hist[s][3], h4 = hist[s][4];
    v[s * NCNT + 0] = h0 + h1 + h2 + h3 + h4;
    v[s * NCNT + 1] = h0;
    v[s * NCNT + 2] = h0 + h1;
    v[s * NCNT + 3] = h0 + h1 + h2;
    v[s * NCNT + 4] = h0 + h1 + h2 + h3;
  }
  // the lanes of one residue are neighbours: segmented inclusive scan over the wavefront, the last lane of a residue holds its
  // sums and adds them to `counts` - one integer atomic per (wavefront, residue, non-zero counter)
  const int res = me.code >> 1;   // (-1 behind the last atom: a segment of zeros)
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int r_up = __shfl_up(res, o, 64);
    const bool same = lane >= o && r_up == res;
#pragma unroll
    for (int k = 0; k < NSET * NCNT; ++k) {
      const int up = __shfl_up(v[k], o, 64);
      v[k] += same ? up : 0;
    }
  }
  const int r_dn = __shfl_down(res, 1, 64);
  if (res >= 0 && (lane == 63 || r_dn != res)) {
    int32_t *out = counts + ((size_t)b * L + res) * (NSET * NCNT);
#pragma unroll
    for (int k = 0; k < NSET * NCNT; ++k)
      if (v[k] != 0) atomicAdd(out + k, v[k]);
  }
}

// ---- stage 3: scores.  One workgroup per protein: per residue and set (p0.5 + p1 + p2 + p4) / (4 total), NaN without an
// included pair; the protein's score is the same ratio of the 64-bit sums over its residues.
__global__ __launch_bounds__(FIN_THREADS) void lddt_finalize_kernel(const int32_t *__restrict__ counts, int L,
                                                                    float *__restrict__ per_res, float *__restrict__ score) {
  __shared__ long long s_sum[FIN_THREADS / 64][2 * NSET];
  const int b = blockIdx.x, tid = threadIdx.x;
  long long sum[2 * NSET] = {0, 0, 0, 0};   // per set: total, preserved
  for (int r = tid; r < L; r += FIN_THREADS) {
    const int32_t *c = counts + ((size_t)b * L + r) * (NSET * NCNT);
#pragma unroll
    for (int s = 0; s < NSET; ++s) {
      const long long total = c[s * NCNT];
      const long long kept = (long long)c[s * NCNT + 1] + c[s * NCNT + 2] + c[s * NCNT + 3] + c[s * NCNT + 4];
      per_res[((size_t)b * L + r) * NSET + s] = total > 0 ? (float)((double)kept / (double)(4 * total)) : __builtin_nanf("");
      sum[2 * s] += total;
      sum[2 * s + 1] += kept;
    }
  }
#pragma unroll
  for (int k = 0; k < 2 * NSET; ++k) {
    long long x = sum[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((tid & 63) == 0) s_sum[tid >> 6][k] = x;
  }
  __syncthreads();
  if (tid < NSET) {
    long long total = 0, kept = 0;
    for (int w = 0; w < FIN_THREADS / 64; ++w) {
      total += s_sum[w][2 * tid];
      kept += s_sum[w][2 * tid + 1];
    }
    score[(size_t)b * NSET + tid] = total > 0 ? (float)((double)kept / (double)(4 * total)) : __builtin_nanf("");
  }
}

}  // namespace

extern "C" {

size_t ptamd_lddt_workspace_bytes(int B, int L) {
  if (!tile_shape_ok(B, L)) return 0;
  return TileLayout(B, L).end;   // the tiles are all of it
}

int ptamd_lddt(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float cutoff, int32_t *counts,
               float *per_res, float *score, void *workspace, size_t workspace_bytes, void *stream) {
  if (!tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !counts || !per_res || !score) return PTAMD_ERR_BAD_SHAPE;
  if (!(cutoff > 0.f) || !isfinite(cutoff)) return PTAMD_ERR_BAD_SHAPE;
  const TileLayout l(B, L);
  if (!workspace || workspace_bytes < l.end) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  char *ws = static_cast<char *>(workspace);
  Atom8 *atoms = reinterpret_cast<Atom8 *>(ws + l.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.natoms);
  hipStream_t st = (hipStream_t)stream;
  PT_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)B * L * NSET * NCNT * sizeof(int32_t), st));   // the sweep only adds
  hipLaunchKernelGGL(compact_kernel<CaRecord>, dim3(B), dim3(COMPACT_THREADS), 0, st, pred_crd, true_crd, seq, L, l.nstride, l.tiles,
                     atoms, boxes, natoms);
  int rc = pt_check_launch();
  if (rc) return rc;
  const int strips = (l.tiles + STRIP_TILES - 1) / STRIP_TILES, chunks = (l.tiles + CHUNK_TILES - 1) / CHUNK_TILES;
  hipLaunchKernelGGL(lddt_sweep_kernel, dim3((unsigned)strips * chunks, B), dim3(TS * STRIP_TILES), 0, st, atoms, boxes, natoms, L,
                     l.nstride, l.tiles, chunks, cutoff, counts);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(lddt_finalize_kernel, dim3(B), dim3(FIN_THREADS), 0, st, counts, L, per_res, score);
  return pt_check_launch();
}

}  // extern "C"
