// The compacted atom tiles that the lDDT family sweeps: csrc/lddt.hip (the metric) and csrc/slddt.hip (the training loss) read
// the same records, so which atoms exist - the pad test, the NaN test and slot order - is decided here and nowhere else.
// csrc/fape.hip (the FAPE training loss) sweeps the same atoms against backbone frames.  csrc/pair_sweep.h builds the sweep that
// csrc/slddt.hip and csrc/clash.hip share on these tiles; csrc/clash.hip fills them with a compaction of its own (presence by
// residue type, boxes of the prediction) from the pieces below.
// csrc/drmsd.hip packs differently on purpose (backbone first, an interleaved record) and is not a user of this header.
#pragma once
#include <limits.h>

#include "common.h"

namespace atom_tiles {

constexpr int TS = 64;   // atoms per tile = lanes of a wavefront
constexpr int COMPACT_THREADS = 1024;

// a compacted atom: 32 bytes, so two 16-byte loads per lane on the way to a register or to LDS, where seven separate planes
// would be seven 4-byte ones.  code = residue << 1 | flag; the flag and aux belong to the consumer (its record policy below)
struct __attribute__((aligned(32))) Atom8 {
  float px, py, pz, tx, ty, tz;
  int code, aux;
};
struct __attribute__((aligned(32))) Box8 {   // bounding box of the true coordinates of a tile of compacted atoms
  float lox, loy, loz, hix, hiy, hiz, r0, r1;
};

// slot indices and residue codes are ints
inline bool tile_shape_ok(int B, int L) { return B > 0 && L > 0 && L <= INT_MAX / (2 * PTAMD_NUM_SLOTS); }

// the next 256-byte aligned piece of a workspace
inline size_t take(size_t &off, size_t bytes) {
  const size_t o = off;
  off += (bytes + 255) & ~(size_t)255;
  return o;
}
// what the compaction leaves at the head of a consumer's workspace; the consumer's own pieces follow at `end`
struct TileLayout {
  size_t atoms, boxes, natoms, end;
  int nstride, tiles;   // compacted atoms per protein (a whole number of tiles), tiles per protein
  TileLayout(int B, int L) {
    tiles = (L * PTAMD_NUM_SLOTS + TS - 1) / TS;
    nstride = tiles * TS;
    end = 0;
    atoms = take(end, (size_t)B * nstride * sizeof(Atom8));
    boxes = take(end, (size_t)B * tiles * sizeof(Box8));
    natoms = take(end, (size_t)B * sizeof(int));
  }
};

// the record of the two training losses (csrc/slddt.hip, csrc/fape.hip): code = residue << 1 | (predicted coordinate unusable),
// aux = slot.  Unusable = not finite, or beyond 1e18 (squared differences would not be finite): replaced by 0 and marked, so
// nothing non-finite enters a sweep.
constexpr float PRED_MAX = 1.0e18f;
__device__ __forceinline__ bool pred_unusable(float px, float py, float pz) {
  return !(fabsf(px) <= PRED_MAX && fabsf(py) <= PRED_MAX && fabsf(pz) <= PRED_MAX);   // (NaN fails every test)
}
struct SlotRecord {
  static __device__ __forceinline__ Atom8 make(float px, float py, float pz, float tx, float ty, float tz, int res, int slot) {
    const bool bad = pred_unusable(px, py, pz);
    if (bad) px = py = pz = 0.f;
    return Atom8{px, py, pz, tx, ty, tz, (res << 1) | (int)bad, slot};
  }
};

// the bounding boxes of the tiles of a protein's n compacted atoms, by the wavefronts of the workgroup that wrote the atoms, behind
// its barrier.  get(j, x, y, z) reads the boxed coordinate of atom j
template <class Get>
__device__ __forceinline__ void tile_boxes(int n, Box8 *boxes, Get get) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inf = __builtin_inff();
  for (int t = w; t * TS < n; t += COMPACT_THREADS / 64) {
    const int j = t * TS + lane;
    const bool live = j < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) get(j, x, y, z);
    const float lox = wave_min(live ? x : inf), loy = wave_min(live ? y : inf), loz = wave_min(live ? z : inf);
    const float hix = wave_max(live ? x : -inf), hiy = wave_max(live ? y : -inf), hiz = wave_max(live ? z : -inf);
    if (lane == 0) boxes[t] = Box8{lox, loy, loz, hix, hiy, hiz, 0.f, 0.f};
  }
}

// ---- compaction.  One workgroup per protein; each of its 16 wavefronts owns a contiguous share of the atom slots and walks it
// 64 slots at a time (position of a present atom = atoms in the shares before + running count + rank among the lanes before
// it), first counting, then writing: slot order is kept, so the atoms of a residue are neighbours.  Then, behind a barrier, the
// bounding boxes of the tiles just written.  Record::make(px, py, pz, tx, ty, tz, residue, slot) builds the atom's record.
template <class Record>
__global__ __launch_bounds__(COMPACT_THREADS) void compact_kernel(const float *__restrict__ pred, const float *__restrict__ truth,
                                                                  const int64_t *__restrict__ seq, int L, int nstride, int tiles,
                                                                  Atom8 *atoms, Box8 *boxes, int *__restrict__ natoms) {
  constexpr int NWAVE = COMPACT_THREADS / 64;
  __shared__ int s_cnt[NWAVE];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nslot = L * PTAMD_NUM_SLOTS;
  pred += (size_t)b * nslot * 3;
  truth += (size_t)b * nslot * 3;
  seq += (size_t)b * L;
  atoms += (size_t)b * nstride;
  boxes += (size_t)b * tiles;
  const int per = ((nslot + NWAVE - 1) / NWAVE + 63) / 64 * 64;   // slots of a wavefront: whole rows of 64
  const int s0 = min(w * per, nslot), s1 = min(s0 + per, nslot);
  auto present = [&](int s, float &tx, float &ty, float &tz) __attribute__((always_inline)) {
    tx = ty = tz = 0.f;
    if (s >= s1 || seq[s / PTAMD_NUM_SLOTS] == PTAMD_PAD_ID) return false;   // batch padding carries zeros, not NaN
    tx = truth[(size_t)s * 3]; ty = truth[(size_t)s * 3 + 1]; tz = truth[(size_t)s * 3 + 2];
    return !(isnan(tx) || isnan(ty) || isnan(tz));
  };
  int cnt = 0;   // (wavefront-uniform)
  for (int r = s0; r < s1; r += 64) {
    float tx, ty, tz;
    cnt += __popcll(__ballot(present(r + lane, tx, ty, tz)));
  }
  if (lane == 0) s_cnt[w] = cnt;
  __syncthreads();
  int pos0 = 0, n = 0;
#pragma unroll
  for (int t = 0; t < NWAVE; ++t) {
    if (t < w) pos0 += s_cnt[t];
    n += s_cnt[t];
  }
  for (int r = s0; r < s1; r += 64) {
    float tx, ty, tz;
    const int s = r + lane;
    const bool ok = present(s, tx, ty, tz);
    const unsigned long long m = __ballot(ok);
    if (ok) {
      const int pos = pos0 + __popcll(m & ((1ull << lane) - 1ull));
      atoms[pos] = Record::make(pred[(size_t)s * 3], pred[(size_t)s * 3 + 1], pred[(size_t)s * 3 + 2], tx, ty, tz,
                                s / PTAMD_NUM_SLOTS, s);
    }
    pos0 += __popcll(m);
  }
  if (tid == 0) natoms[b] = n;
  __syncthreads();   // the atoms this workgroup wrote are visible to all of it
  tile_boxes(n, boxes, [&](int j, float &x, float &y, float &z) __attribute__((always_inline)) {
    const Atom8 a = atoms[j];
    x = a.tx; y = a.ty; z = a.tz;
  });
}

// can a pair of atoms of two tiles be included?  Its true distance is at least the gap between the boxes; 0.1 % on the squares
// covers the rounding of both sides (a NaN gap keeps the tile)
__device__ __forceinline__ bool boxes_near(const Box8 &a, const Box8 &c, float cutoff) {
  const float gx = fmaxf(0.f, fmaxf(a.lox - c.hix, c.lox - a.hix));
  const float gy = fmaxf(0.f, fmaxf(a.loy - c.hiy, c.loy - a.hiy));
  const float gz = fmaxf(0.f, fmaxf(a.loz - c.hiz, c.loz - a.hiz));
  return !(gx * gx + gy * gy + gz * gz > cutoff * cutoff * 1.001f);
}

// the distance of both sweeps, from the coordinate differences: which pairs the metric and the loss include rests on this one
// expression (dt < cutoff, strict)
__device__ __forceinline__ float true_dist(float dx, float dy, float dz) {
  return __builtin_amdgcn_sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
}

}  // namespace atom_tiles
