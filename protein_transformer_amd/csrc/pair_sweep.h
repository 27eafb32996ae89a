// The strip-by-chunk sweep over the UPPER TRIANGLE of atom-tile pairs, every unordered pair of atoms once, and what its finalize
// kernels share.  Two users: csrc/slddt.hip (the smooth lDDT loss) and csrc/clash.hip (the steric clash term).  This header owns
// the tuning constants, the workspace pieces behind the head of csrc/atom_tiles.h with their index formulas, the skeleton of the
// sweep kernel, and the two gathers of the finalize kernels; a user owns its atom record, its pair term (a policy, below), its
// statistics and its gradient scale.  csrc/rename.hip and csrc/fape.hip sweep rectangles with other partials and are not users.
//
//   sweep     A work item is one wavefront: a STRIP of 4 row tiles (one atom per lane and tile, in registers) against a CHUNK of
//             8 column tiles.  Per column tile J the wavefront stages the tile in LDS and visits the row tiles I <= J of its
//             strip whose bounding box lies within the policy's reach of J's (no pair of two farther tiles can contribute).
//             16 columns at a time:
//               phase 1  lane = row atom, column atom broadcast from LDS: the pair term, its share of the row atom's gradient,
//                        and its coefficient cf_ij left in LDS (row-major, 17-word rows);
//               phase 2  that 64 x 16 tile re-read TRANSPOSED (lane = column, a quarter of the rows): S_j = sum_i cf_ij and
//                        V_j = sum_i cf_ij x_i, the quarters folded by two lane exchanges - the column atom's share is
//                        x_j S_j - V_j (the scheme of csrc/drmsd.hip, without its DPP operands).
//             The (S, V) of a column tile are summed over the strip's row tiles in tile order and written once per (strip,
//             column tile) with a flag "this strip touched the tile"; row gradients once per (row tile, chunk); the sum of the
//             pair values (fp32 inside a tile pair, fp64 across them) and the pair count once per work item.  Wavefronts share
//             nothing: LDS is reused across wave barriers only, no workgroup barrier, no atomics.
//   finalize  per protein the work items' sums in an order that depends on the protein's atom count alone (not on B, not on
//             L), and per atom row partials (chunk order) + column partials (strip order).
// Every sum has a fixed order: two runs give the same bits, and a protein's bits do not depend on the batch around it or on its
// padding - for both users, because both run this code.
#pragma once
#include "atom_tiles.h"

namespace pair_sweep {

using namespace atom_tiles;

constexpr int STRIP_TILES = 4;    // row tiles of a work item
constexpr int CHUNK_TILES = 8;    // column tiles of a work item
constexpr int SUB = 16, CF_LD = SUB + 1;   // the coefficient tile is kept for 16 columns at a time: 4.3 KB
constexpr int FIN_THREADS = 256;
static_assert(CHUNK_TILES <= 64, "a lane tests one column tile's box");
static_assert(TS == 4 * SUB, "phase 2 folds the rows in four quarters");

struct __attribute__((aligned(16))) Item {   // what one work item of the sweep leaves for the finalize kernel
  double sum;        // of the pair values
  long long count;   // of the counted pairs
};

// tiles, strips and chunks per protein of the launch (of L, not of a protein's own atom count), and where a piece keeps what
struct Dims {
  int tiles, strips, chunks;
  __device__ size_t rowpart_at(int b, int I, int chunk, int lane) const { return (((size_t)b * tiles + I) * chunks + chunk) * TS + lane; }
  __device__ size_t kept_at(int b, int strip, int J) const { return ((size_t)b * strips + strip) * tiles + J; }
  __device__ size_t colpart_at(int b, int strip, int J, int lane) const { return kept_at(b, strip, J) * TS + lane; }
  __device__ size_t items_at(int b, int strip, int chunk) const { return ((size_t)b * strips + strip) * chunks + chunk; }
};

// the sweep's pieces of a workspace, from `off` on (behind atom_tiles::TileLayout and whatever the user placed first); `off`
// is left behind the last of them
struct SweepLayout {
  Dims d;
  size_t rowpart, colpart, kept, items;
  SweepLayout(int B, int tiles, size_t &off) {
    d.tiles = tiles;
    d.strips = (tiles + STRIP_TILES - 1) / STRIP_TILES;
    d.chunks = (tiles + CHUNK_TILES - 1) / CHUNK_TILES;
    rowpart = take(off, (size_t)B * tiles * d.chunks * TS * sizeof(float4));   // [b][row tile][chunk][lane]
    colpart = take(off, (size_t)B * d.strips * tiles * TS * sizeof(float4));   // [b][strip][column tile][lane]
    kept = take(off, (size_t)B * d.strips * tiles * sizeof(int));              // [b][strip][column tile]
    items = take(off, (size_t)B * d.strips * d.chunks * sizeof(Item));         // [b][strip][chunk]
  }
};

// what a policy's pair term returns: the value to add to the work item's sum, whether the pair is counted, and for the gradient
// the coefficient cf and the coordinate differences row - column: d(value) / d(row atom) = cf * (dx, dy, dz)
struct Term {
  float value;
  bool counted;
  float cf, dx, dy, dz;
};

// ---- the pair sweep: the body of a kernel on grid (strips * chunks, B), one wavefront per workgroup = one work item.
// `Pair` is the user's policy, an object that carries the constants of the launch:
//   Atom                      the compacted record: 32 bytes with an int `code` = residue << 1 | flag, -1 behind the last atom
//   SPARSE                    phase 2 is skipped for 16 columns without a counted pair
//   dead()                    the record behind the last atom
//   position(a)               (x, y, z, 0) of the coordinate the gradient is taken in
//   reach()                   no pair of two tiles whose boxes are farther apart contributes
//   row(a)                    whatever the term wants computed once per row tile, handed back to it
//   term(a, row, c, apart)    the pair of row atom a and column atom c: `apart` = different residues, both live, and on the
//                             diagonal tile row before column.  Returns a Term
template <bool WITH_GRAD, class Pair>
__device__ __forceinline__ void sweep(const Pair &pair, const typename Pair::Atom *__restrict__ atoms, const Box8 *__restrict__ boxes,
                                      const int *__restrict__ natoms, int nstride, Dims d, float4 *__restrict__ rowpart,
                                      float4 *__restrict__ colpart, int *__restrict__ kept, Item *__restrict__ items) {
  using Atom = typename Pair::Atom;
  static_assert(sizeof(Atom) == sizeof(Atom8) && sizeof(Atom8) == 32, "the tiles and the workspace head of csrc/atom_tiles.h");
  __shared__ Atom s_col[TS];
  __shared__ float s_cf[TS * CF_LD];
  __shared__ float4 s_row[TS];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int strip = blockIdx.x / d.chunks, chunk = blockIdx.x % d.chunks;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  const int I0 = strip * STRIP_TILES;
  const int J0 = max(I0, chunk * CHUNK_TILES), J1 = min(nT, (chunk + 1) * CHUNK_TILES);
  if (I0 >= nT || J0 >= J1) return;   // below the diagonal or behind the protein: item_sums skips these items too
  atoms += (size_t)b * nstride;
  boxes += (size_t)b * d.tiles;

  // near[r]: bit l = column tile J0 + l can hold a contributing pair with row tile I0 + r
  unsigned long long near[STRIP_TILES];
  {
    Box8 c = Box8{0, 0, 0, 0, 0, 0, 0, 0};
    const bool have = J0 + lane < J1;
    if (have) c = boxes[J0 + lane];
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) {
      near[r] = 0ull;
      if (I0 + r < nT) near[r] = __ballot(have && I0 + r <= J0 + lane && boxes_near(boxes[I0 + r], c, pair.reach()));
    }
  }

  Atom me[STRIP_TILES];
  float gx[STRIP_TILES], gy[STRIP_TILES], gz[STRIP_TILES];
#pragma unroll
  for (int r = 0; r < STRIP_TILES; ++r) {
    me[r] = Pair::dead();
    const int i = (I0 + r) * TS + lane;
    if (i < n) me[r] = atoms[i];
    gx[r] = gy[r] = gz[r] = 0.f;
  }
  double sum = 0.0;
  int count = 0;

  for (int J = J0; J < J1; ++J) {
    const int jb = J - J0;
    unsigned long long near_any = 0ull;
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) near_any |= near[r];
    const bool any = (near_any >> jb) & 1ull;
    if (lane == 0) kept[d.kept_at(b, strip, J)] = any;
    if (!any) continue;   // wavefront-uniform
    const int cnt = min(TS, n - J * TS);   // live columns of the tile
    {
      const int j = J * TS + lane;
      s_col[lane] = j < n ? atoms[j] : Pair::dead();
    }
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);   // (S, Vx, Vy, Vz) of column `lane` of the tile
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) {
      if (!((near[r] >> jb) & 1ull)) continue;   // wavefront-uniform
      const Atom a = me[r];
      const bool a_live = a.code >= 0;
      const bool diag = I0 + r == J;   // the diagonal tile: pairs i < j only
      const auto row = pair.row(a);
      if (WITH_GRAD) s_row[lane] = Pair::position(a);
      float sum_t = 0.f;
      for (int j0 = 0; j0 < cnt; j0 += SUB) {
        __builtin_amdgcn_wave_barrier();
        bool sub_hit = false;
#pragma unroll 4
        for (int jj = 0; jj < SUB; ++jj) {
          const int j = j0 + jj;
          const Atom c = s_col[j];   // broadcast
          // different residues; a column behind the last atom has code -1 (and a dead row is excluded by a_live)
          const bool apart = (unsigned)(a.code ^ c.code) > 1u && c.code >= 0 && a_live && (!diag || lane < j);
          const auto t = pair.term(a, row, c, apart);
          sum_t += t.value;
          count += t.counted ? 1 : 0;
          if (WITH_GRAD) {
            gx[r] = fmaf(t.cf, t.dx, gx[r]);
            gy[r] = fmaf(t.cf, t.dy, gy[r]);
            gz[r] = fmaf(t.cf, t.dz, gz[r]);
            s_cf[lane * CF_LD + jj] = t.cf;
            sub_hit |= t.counted;
          }
        }
        if (WITH_GRAD && (!Pair::SPARSE || __ballot(sub_hit) != 0ull)) {   // (wavefront-uniform)
          // phase 2 for these 16 columns: lane = (column j0 + (lane & 15), quarter lane >> 4 of the rows)
          __builtin_amdgcn_wave_barrier();
          const int col = lane & (SUB - 1), r0 = (lane >> 4) * SUB;
          float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int rr = 0; rr < SUB; ++rr) {
            const float c = s_cf[(r0 + rr) * CF_LD + col];
            const float4 x = s_row[r0 + rr];
            q.x += c;
            q.y = fmaf(c, x.x, q.y);
            q.z = fmaf(c, x.y, q.z);
            q.w = fmaf(c, x.z, q.w);
          }
          // fold the four row quarters (lanes l, l ^ 16, l ^ 32, l ^ 48) in a fixed order: every lane ends with the sum
          q.x += __shfl_xor(q.x, 16, 64); q.y += __shfl_xor(q.y, 16, 64); q.z += __shfl_xor(q.z, 16, 64); q.w += __shfl_xor(q.w, 16, 64);
          q.x += __shfl_xor(q.x, 32, 64); q.y += __shfl_xor(q.y, 32, 64); q.z += __shfl_xor(q.z, 32, 64); q.w += __shfl_xor(q.w, 32, 64);
          if ((lane >> 4) == (j0 >> 4)) {   // lane l keeps column l of the tile
            cs.x += q.x; cs.y += q.y; cs.z += q.z; cs.w += q.w;
          }
        }
      }
      sum += (double)sum_t;
      __builtin_amdgcn_wave_barrier();   // s_row is rewritten for the next row tile
    }
    if (WITH_GRAD) colpart[d.colpart_at(b, strip, J, lane)] = cs;
    __builtin_amdgcn_wave_barrier();     // s_col is rewritten for the next column tile
  }
  if (WITH_GRAD) {
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r)
      if (I0 + r < nT) rowpart[d.rowpart_at(b, I0 + r, chunk, lane)] = make_float4(gx[r], gy[r], gz[r], 0.f);
  }
  sum = wave_sum_d(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);   // (<= 4 * 8 * 64 * 64: an int)
  if (lane == 0) items[d.items_at(b, strip, chunk)] = Item{sum, (long long)count};
}

// ---- the finalize kernels' shares: workgroups of FIN_THREADS threads on grid (ceil(nstride / FIN_THREADS), B).
// The sums of protein b's work items, for every thread of a workgroup that calls this as a whole: thread t takes the items t,
// t + 256, ... of the protein's OWN triangle (strips and chunks of its nT tiles, whatever L is), then a fixed tree.
__device__ __forceinline__ Item item_sums(const Item *__restrict__ items, Dims d, int b, int nT) {
  __shared__ double s_sum[FIN_THREADS];
  __shared__ long long s_cnt[FIN_THREADS];
  const int tid = threadIdx.x;
  const int sN = (nT + STRIP_TILES - 1) / STRIP_TILES, cN = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
  double e = 0.0;
  long long c = 0;
  for (int r = tid; r < sN * cN; r += FIN_THREADS) {
    const int s = r / cN, ch = r % cN;
    if ((ch + 1) * CHUNK_TILES <= s * STRIP_TILES) continue;   // below the diagonal: never written
    const Item it = items[d.items_at(b, s, ch)];
    e += it.sum;
    c += it.count;
  }
  s_sum[tid] = e;
  s_cnt[tid] = c;
  __syncthreads();
  for (int o = FIN_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_cnt[tid] += s_cnt[tid + o];
    }
    __syncthreads();
  }
  return Item{s_sum[0], s_cnt[0]};
}

// The unscaled gradient of compacted atom j (< n, of nT tiles) of protein b at pos = Pair::position of its record: its row
// partials in chunk order plus its column partials x S - V in strip order
__device__ __forceinline__ float3 atom_gradient(const float4 *__restrict__ rowpart, const float4 *__restrict__ colpart,
                                                const int *__restrict__ kept, Dims d, int b, int j, int nT, float4 pos) {
  const int J = j / TS, lane = j & (TS - 1), sJ = J / STRIP_TILES;
  float rx = 0.f, ry = 0.f, rz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  {  // row side: the chunks of the atom's strip that had work, in chunk order
    const int c0 = (STRIP_TILES * sJ) / CHUNK_TILES, c1 = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
    for (int c = c0; c < c1; ++c) {
      const float4 r = rowpart[d.rowpart_at(b, J, c, lane)];
      rx += r.x; ry += r.y; rz += r.z;
    }
  }
  for (int s = 0; s <= sJ; ++s) {  // column side: the strips at or above the atom's tile that touched it, in strip order
    if (!kept[d.kept_at(b, s, J)]) continue;
    const float4 cp = colpart[d.colpart_at(b, s, J, lane)];
    cx += fmaf(pos.x, cp.x, -cp.y);
    cy += fmaf(pos.y, cp.x, -cp.z);
    cz += fmaf(pos.z, cp.x, -cp.w);
  }
  return make_float3(rx + cx, ry + cy, rz + cz);
}

}  // namespace pair_sweep
