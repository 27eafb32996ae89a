// Symmetric side-chain renaming of the ground truth, for a whole batch on gfx950: `train.py --rename_symmetric`.
//
// ASP, GLU, PHE and TYR carry pairs of chemically identical atoms (OD1/OD2, OE1/OE2, CD1/CD2 + CE1/CE2) whose names in a
// deposited structure are arbitrary; chi and chi + pi build the same molecule with the names exchanged.  Jumper et al., "Highly
// accurate protein structure prediction with AlphaFold", Nature 596:583-589 (2021), supplementary 1.8.5, algorithm 26: per
// residue, keep the naming of the truth under which the distances from its ambiguous atoms to all non-ambiguous atoms agree
// better with the prediction.  The losses and metrics behind it see the renamed truth and need no change.  Definition:
// include/ptamd.h.
//
// Five launches per batch:
//   compact    the present atoms of each protein, in slot order: csrc/atom_tiles.h with its SlotRecord, as csrc/fape.hip
//              (which atoms exist is decided there and nowhere else; the bounding boxes it also leaves are not used).
//   residues   one workgroup per protein.  Zero flags and costs for every residue; from the compacted atoms, where each
//              ambiguous atom of a residue sits in the compaction (amb_pos, -1 = absent) - the atom's `aux` is rewritten to
//              "ambiguous" for the sweep; then one wavefront compacts the candidate residues in residue order into their swap
//              pairs (ballot prefix sums, as fape_frames_kernel): a row of the sweep is ONE SWAP PAIR (a, a').
//   sweep      a work item is one wavefront: a tile of 64 swap pairs (lane = pair, both atoms in registers) against a chunk of 4
//              atom tiles, each staged in LDS and read as broadcasts.  Per partner q the four distances dp(a,q), dp(a',q),
//              dt(a,q), dt(a',q) give both atoms' terms of both costs (four roots for four terms, where a lane per atom would
//              take three roots for two).  Lane-private sums, fp32 inside an atom tile and fp64 across tiles; no cross-lane
//              traffic at all, so no wavefront reduction is needed.
//   finalize   one lane per candidate residue: the sums of its pairs over the chunks in chunk order, in fp64, rounded once;
//              swapped = alt < orig on the rounded values that are reported.
//   apply      elementwise over all residues: the coordinate copy with the slot pairs of swapped residues exchanged, the angle
//              copy with the sign bit of the chi column flipped; 32-bit words are moved, so NaN payloads survive.
// No atomics, wavefronts share nothing; two runs give the same bits.  Pair order, row tiles and chunk bounds depend on the
// protein's own atoms alone, so its bits depend neither on the batch around it nor on its padding.
#include <limits.h>
#include <math.h>

#include "atom_tiles.h"

namespace {

using namespace atom_tiles;

constexpr int CHUNK_TILES = 4;        // atom tiles of a work item of the sweep
constexpr int RES_THREADS = 256;      // the residues kernel
constexpr int APPLY_THREADS = 256;

// ---- the swap table (include/ptamd.h).  Four slots as nibbles: a0 | b0 << 4 | a1 << 8 | b1 << 12, pairs (a0, b0), (a1, b1);
// 0 = the residue type has none.  Index i of an ambiguous atom = its nibble; its partner is nibble i ^ 1.
__host__ __device__ __forceinline__ unsigned swap_slots(int64_t type) {
  return type == 2 ? 0x0076u : type == 3 ? 0x0087u : type == 4 ? 0x97A6u : type == 19 ? 0xA7B6u : 0u;
}
__host__ __device__ __forceinline__ int swap_pairs(unsigned packed) { return packed == 0u ? 0 : (packed >> 8) ? 2 : 1; }
__host__ __device__ __forceinline__ int amb_index(unsigned packed, int slot) {   // -1: not a member of a swap pair
  int idx = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (slot >= 4 && (int)((packed >> (4 * i)) & 15u) == slot) idx = i;
  return idx;
}
// the angle column (of 12) whose torsion places the first ambiguous atom: 6 + (slot - 4), csrc/geometry.hip
__host__ __device__ __forceinline__ int chi_column(unsigned packed) { return 6 + (int)(packed & 15u) - 4; }

struct Layout {
  TileLayout t;
  size_t amb_pos, pairs, cand, npairs, ncand, unusable, part, total;
  int rtiles, chunks;
  Layout(int B, int L) : t(B, L) {
    rtiles = (2 * L + TS - 1) / TS;   // at most two swap pairs per residue
    chunks = (t.tiles + CHUNK_TILES - 1) / CHUNK_TILES;
    total = t.end;
    amb_pos = take(total, (size_t)B * L * 4 * sizeof(int));                     // [b][residue][4]
    pairs = take(total, (size_t)B * L * 2 * sizeof(int2));                      // [b][pair]: compacted indices of (a, a')
    cand = take(total, (size_t)B * L * sizeof(int2));                           // [b][candidate]: residue, its first pair
    npairs = take(total, (size_t)B * sizeof(int));
    ncand = take(total, (size_t)B * sizeof(int));
    unusable = take(total, (size_t)B * sizeof(int));
    part = take(total, (size_t)B * rtiles * chunks * TS * sizeof(double2));     // [b][row tile][chunk][lane]: {orig, alt}
  }
};

// ---- stage 2: grid B (behind the compaction)
__global__ __launch_bounds__(RES_THREADS) void rename_residues_kernel(const int64_t *__restrict__ seq, Atom8 *atoms,
                                                                      const int *__restrict__ natoms, int L, int nstride,
                                                                      int *amb_pos, int2 *__restrict__ pairs,
                                                                      int2 *__restrict__ cand, int *__restrict__ npairs,
                                                                      int *__restrict__ ncand, int *__restrict__ unusable,
                                                                      int32_t *__restrict__ swapped, float *__restrict__ cost) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  seq += (size_t)b * L;
  atoms += (size_t)b * nstride;
  amb_pos += (size_t)b * L * 4;
  pairs += (size_t)b * L * 2;
  cand += (size_t)b * L;
  swapped += (size_t)b * L;
  cost += (size_t)b * L * 2;
  __shared__ int s_bad[RES_THREADS / 64];
  const int n = natoms[b];
  for (int r = tid; r < L; r += RES_THREADS) {
    reinterpret_cast<int4 *>(amb_pos)[r] = make_int4(-1, -1, -1, -1);
    swapped[r] = 0;
    cost[2 * r] = cost[2 * r + 1] = 0.f;
  }
  __threadfence_block();   // amb_pos and cost are GLOBAL memory that other lanes of the workgroup write next: fence, then meet
  __syncthreads();
  int bad = 0;
  for (int j = tid; j < n; j += RES_THREADS) {
    const Atom8 a = atoms[j];
    const int res = a.code >> 1, slot = a.aux - res * PTAMD_NUM_SLOTS;
    const int i = amb_index(swap_slots(seq[res]), slot);
    bad |= a.code & 1;
    if (i >= 0) amb_pos[res * 4 + i] = j;
    atoms[j].aux = i >= 0;   // what the sweep asks of a partner: is it ambiguous
  }
  const bool wave_bad = __ballot(bad != 0) != 0ull;
  if (lane == 0) s_bad[tid >> 6] = wave_bad;
  __threadfence_block();   // amb_pos and the atoms' aux, written above, are read below by the first wavefront
  __syncthreads();
  if (tid >= 64) return;
  int any_bad = 0;
#pragma unroll
  for (int w = 0; w < RES_THREADS / 64; ++w) any_bad |= s_bad[w];
  const float nan = __builtin_nanf("");
  int p0 = 0, c0 = 0;
  for (int r0 = 0; r0 < L; r0 += TS) {
    const int r = r0 + lane;
    const unsigned packed = r < L ? swap_slots(seq[r]) : 0u;
    const int np = swap_pairs(packed);
    int4 pos = make_int4(-1, -1, -1, -1);
    if (np > 0) pos = reinterpret_cast<const int4 *>(amb_pos)[r];
    const bool ok = np > 0 && pos.x >= 0 && pos.y >= 0 && (np == 1 || (pos.z >= 0 && pos.w >= 0));
    const unsigned long long m1 = __ballot(ok), m2 = __ballot(ok && np == 2);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (ok) {
      const int p = p0 + __popcll(m1 & below) + __popcll(m2 & below);
      pairs[p] = make_int2(pos.x, pos.y);
      if (np == 2) pairs[p + 1] = make_int2(pos.z, pos.w);
      cand[c0 + __popcll(m1 & below)] = make_int2(r, p);
      if (any_bad) cost[2 * r] = cost[2 * r + 1] = nan;
    }
    p0 += __popcll(m1) + __popcll(m2);
    c0 += __popcll(m1);
  }
  if (lane == 0) {
    npairs[b] = p0;
    ncand[b] = c0;
    unusable[b] = any_bad;
  }
}

// ---- stage 3: grid (rtiles * chunks, B), one wavefront per workgroup = one work item
__global__ __launch_bounds__(TS) void rename_sweep_kernel(const Atom8 *__restrict__ atoms, const int *__restrict__ natoms,
                                                          const int2 *__restrict__ pairs, const int *__restrict__ npairs,
                                                          const int *__restrict__ unusable, int nstride, int L, int rtiles,
                                                          int chunks, double2 *__restrict__ part) {
  __shared__ Atom8 s_atom[TS];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int rt = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const int n = natoms[b], np = npairs[b], nT = (n + TS - 1) / TS;
  const int J0 = ch * CHUNK_TILES, J1 = min(nT, J0 + CHUNK_TILES);
  if (unusable[b] || rt * TS >= np || J0 >= J1) return;   // the finalize kernel reads none of these items
  atoms += (size_t)b * nstride;
  const int i = rt * TS + lane;
  Atom8 a = Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0}, c = a;
  if (i < np) {
    const int2 p = pairs[(size_t)b * L * 2 + i];
    a = atoms[p.x];
    c = atoms[p.y];
  }
  double orig = 0.0, alt = 0.0;
  for (int J = J0; J < J1; ++J) {
    const int cnt = min(TS, n - J * TS);   // live atoms of the tile
    {
      const int j = J * TS + lane;
      s_atom[lane] = j < n ? atoms[j] : Atom8{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 1};
    }
    __builtin_amdgcn_wave_barrier();
    float o = 0.f, s = 0.f;
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
      const Atom8 q = s_atom[j];   // broadcast
      // prediction and truth through the same expression: a prediction equal to a naming of the truth has an exactly zero cost
      const float dpa = true_dist(a.px - q.px, a.py - q.py, a.pz - q.pz), dpc = true_dist(c.px - q.px, c.py - q.py, c.pz - q.pz);
      const float dta = true_dist(a.tx - q.tx, a.ty - q.ty, a.tz - q.tz), dtc = true_dist(c.tx - q.tx, c.ty - q.ty, c.tz - q.tz);
      const float to = fabsf(dpa - dta) + fabsf(dpc - dtc), ta = fabsf(dpa - dtc) + fabsf(dpc - dta);
      o += q.aux ? 0.f : to;   // an ambiguous partner is left out
      s += q.aux ? 0.f : ta;
    }
    orig += (double)o;
    alt += (double)s;
    __builtin_amdgcn_wave_barrier();   // s_atom is rewritten for the next tile
  }
  part[(((size_t)b * rtiles + rt) * chunks + ch) * TS + lane] = make_double2(orig, alt);   // (lanes behind the last pair: nobody reads)
}

// ---- stage 4: grid (ceil(L / 64), B), one lane per candidate residue
__global__ __launch_bounds__(TS) void rename_finalize_kernel(const int64_t *__restrict__ seq, const int *__restrict__ natoms,
                                                             const int2 *__restrict__ cand, const int *__restrict__ ncand,
                                                             const int *__restrict__ unusable, const double2 *__restrict__ part,
                                                             int L, int rtiles, int chunks, int32_t *__restrict__ swapped,
                                                             float *__restrict__ cost) {
  const int b = blockIdx.y, k = blockIdx.x * TS + threadIdx.x;
  if (unusable[b] || k >= ncand[b]) return;
  const int nCH = ((natoms[b] + TS - 1) / TS + CHUNK_TILES - 1) / CHUNK_TILES;
  const int2 c = cand[(size_t)b * L + k];
  const int np = swap_pairs(swap_slots(seq[(size_t)b * L + c.x]));
  double orig = 0.0, alt = 0.0;
  for (int p = c.y; p < c.y + np; ++p)   // pair order, then chunk order
    for (int ch = 0; ch < nCH; ++ch) {
      const double2 v = part[(((size_t)b * rtiles + p / TS) * chunks + ch) * TS + p % TS];
      orig += v.x;
      alt += v.y;
    }
  const float o = (float)orig, s = (float)alt;
  const size_t r = (size_t)b * L + c.x;
  cost[r * 2] = o;
  cost[r * 2 + 1] = s;
  swapped[r] = s < o;   // strict: a tie keeps the names
}

// ---- stage 5: one thread per 32-bit word of the coordinates, then of the angles
__global__ __launch_bounds__(APPLY_THREADS) void rename_apply_kernel(const uint32_t *__restrict__ true_crd,
                                                                     const uint32_t *__restrict__ true_ang,
                                                                     const int64_t *__restrict__ seq,
                                                                     const int32_t *__restrict__ swapped, size_t nres,
                                                                     uint32_t *__restrict__ crd_out, uint32_t *__restrict__ ang_out) {
  constexpr int CW = PTAMD_NUM_SLOTS * 3, AW = PTAMD_NUM_ANGLES * 2;
  const size_t ncrd = nres * CW, nang = true_ang ? nres * AW : 0;
  for (size_t e = (size_t)blockIdx.x * APPLY_THREADS + threadIdx.x; e < ncrd + nang; e += (size_t)gridDim.x * APPLY_THREADS) {
    if (e < ncrd) {
      const size_t r = e / CW;
      const int w = (int)(e - r * CW), slot = w / 3;
      int from = slot;
      if (swapped[r]) {
        const unsigned packed = swap_slots(seq[r]);
        const int i = amb_index(packed, slot);
        if (i >= 0) from = (int)((packed >> (4 * (i ^ 1))) & 15u);
      }
      crd_out[e] = true_crd[r * CW + from * 3 + (w - slot * 3)];
    } else {
      const size_t f = e - ncrd, r = f / AW;
      const int col = (int)(f - r * AW) >> 1;
      const bool turn = swapped[r] && col == chi_column(swap_slots(seq[r]));
      ang_out[f] = true_ang[f] ^ (turn ? 0x80000000u : 0u);   // chi + pi: (cos, sin) -> (-cos, -sin)
    }
  }
}

bool overlap(const void *p, size_t pn, const void *q, size_t qn) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), c = reinterpret_cast<uintptr_t>(q);
  return p && q && a < c + qn && c < a + pn;
}

}  // namespace

extern "C" {

size_t ptamd_rename_symmetric_workspace_bytes(int B, int L) {
  if (!tile_shape_ok(B, L)) return 0;
  return Layout(B, L).total;
}

int ptamd_rename_symmetric(const float *pred_crd, const float *true_crd, const float *true_ang, const int64_t *seq, int B, int L,
                           float *true_crd_out, float *true_ang_out, int32_t *swapped, float *cost, void *workspace,
                           size_t workspace_bytes, void *stream) {
  if (!tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !true_crd_out || !swapped || !cost) return PTAMD_ERR_BAD_SHAPE;
  if ((true_ang == nullptr) != (true_ang_out == nullptr)) return PTAMD_ERR_BAD_SHAPE;
  const size_t nres = (size_t)B * L, crd_bytes = nres * PTAMD_NUM_SLOTS * 3 * sizeof(float);
  const size_t ang_bytes = nres * PTAMD_NUM_ANGLES * 2 * sizeof(float);
  // an output on top of an input: the copy would read what it has already exchanged
  if (overlap(true_crd_out, crd_bytes, true_crd, crd_bytes) || overlap(true_crd_out, crd_bytes, pred_crd, crd_bytes) ||
      overlap(true_ang_out, ang_bytes, true_ang, ang_bytes))
    return PTAMD_ERR_BAD_SHAPE;
  const Layout l(B, L);
  if (!workspace || workspace_bytes < l.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  if ((size_t)l.rtiles * l.chunks > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;   // (a grid dimension; its workspace is beyond any device)
  char *ws = static_cast<char *>(workspace);
  Atom8 *atoms = reinterpret_cast<Atom8 *>(ws + l.t.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.t.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.t.natoms);
  int *amb_pos = reinterpret_cast<int *>(ws + l.amb_pos);
  int2 *pairs = reinterpret_cast<int2 *>(ws + l.pairs), *cand = reinterpret_cast<int2 *>(ws + l.cand);
  int *npairs = reinterpret_cast<int *>(ws + l.npairs), *ncand = reinterpret_cast<int *>(ws + l.ncand);
  int *unusable = reinterpret_cast<int *>(ws + l.unusable);
  double2 *part = reinterpret_cast<double2 *>(ws + l.part);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(compact_kernel<SlotRecord>, dim3(B), dim3(COMPACT_THREADS), 0, st, pred_crd, true_crd, seq, L, l.t.nstride, l.t.tiles,
                     atoms, boxes, natoms);
  int rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(rename_residues_kernel, dim3(B), dim3(RES_THREADS), 0, st, seq, atoms, natoms, L, l.t.nstride, amb_pos, pairs, cand,
                     npairs, ncand, unusable, swapped, cost);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(rename_sweep_kernel, dim3((unsigned)(l.rtiles * l.chunks), B), dim3(TS), 0, st, atoms, natoms, pairs, npairs, unusable,
                     l.t.nstride, L, l.rtiles, l.chunks, part);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(rename_finalize_kernel, dim3((unsigned)((L + TS - 1) / TS), B), dim3(TS), 0, st, seq, natoms, cand, ncand, unusable,
                     part, L, l.rtiles, l.chunks, swapped, cost);
  rc = pt_check_launch();
  if (rc) return rc;
  const size_t words = nres * (PTAMD_NUM_SLOTS * 3 + (true_ang ? PTAMD_NUM_ANGLES * 2 : 0));
  const size_t want = (words + APPLY_THREADS - 1) / APPLY_THREADS;
  const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);   // grid-stride beyond
  hipLaunchKernelGGL(rename_apply_kernel, dim3(blocks), dim3(APPLY_THREADS), 0, st, reinterpret_cast<const uint32_t *>(true_crd),
                     reinterpret_cast<const uint32_t *>(true_ang), seq, swapped, nres, reinterpret_cast<uint32_t *>(true_crd_out),
                     reinterpret_cast<uint32_t *>(true_ang_out));
  return pt_check_launch();
}

}  // extern "C"
