// Steric clash term, forward + analytic backward, for a whole batch on gfx950: the auxiliary training term
// `train.py --clash_weight` and the metric `--eval_clash`.
//
// The reference (protein_transformer) has no counterpart: every loss and metric it has compares the prediction with the truth,
// and none says whether the predicted all-atom structure is physically possible.  This is the between-residue part of the
// structural violation loss of Jumper et al., "Highly accurate protein structure prediction with AlphaFold", Nature 596:583-589
// (2021), supplementary 1.9.11 - the only violation an angle-to-NeRF model can commit, since the NeRF build fixes every bond
// length and bond angle.  The truth is not an argument.  Definition: include/ptamd.h.
//
// Three launches per batch (behind the zero fill of `dcrd`, unless the call accumulates):
//   compact   the atoms of each protein - the slots its residue types have, whatever they hold - in slot order into the
//             workspace, with their van der Waals radius and what the two exclusions need, and the bounding box of the PREDICTED
//             coordinates of every tile of 64 of them.  The records and the workspace head are those of csrc/atom_tiles.h; its
//             compact_kernel is not used, because it decides presence by the truth and boxes the truth.  An unusable predicted
//             coordinate (not finite, or beyond atom_tiles::PRED_MAX) is replaced by 0 and counted: the protein's loss is NaN.
//   sweep     the UPPER TRIANGLE of tile pairs, every unordered pair of atoms once: the sweep of csrc/slddt.hip (a strip of 4 row
//             tiles in registers against a chunk of 8 column tiles staged in LDS, 16 columns at a time, the coefficient tile
//             re-read transposed for the column atoms' shares) with the pair term max(0, r_a + r_b - tau - d) in place of the
//             logistics.  A tile pair is skipped when the gap between its boxes exceeds 2 * 1.8 - tau: atoms in slot order are
//             neighbours in space, so almost every tile pair goes; and the transposed pass is skipped for 16 columns without a
//             violating pair, which is nearly all of the rest.
//   finalize  per protein the work items' sums in an order that depends on the protein's atom count alone, the loss, and per
//             atom row partials (chunk order) + column partials (strip order), scaled by 1 / n, and weight times that written or added to
//             the slot layout.
// No atomics; two runs give the same bits; a protein's bits do not depend on the batch around it or on its padding.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "atom_tiles.h"

namespace {

using namespace atom_tiles;

constexpr int STRIP_TILES = 4;    // row tiles of a work item
constexpr int CHUNK_TILES = 8;    // column tiles of a work item (<= 64: a lane tests one column tile's box)
constexpr int SUB = 16, CF_LD = SUB + 1;   // the coefficient tile is kept for 16 columns at a time
constexpr int FIN_THREADS = 256;
constexpr int NRES = 20;
constexpr float R_MAX = 1.8f;     // the largest radius (S): no pair beyond 2 R_MAX - tau violates

// van der Waals radii by element (Bondi, J. Phys. Chem. 68:441, 1964), in the order of the element codes below
constexpr int EL_C = 0, EL_N = 1, EL_O = 2, EL_S = 3;
const float h_radius[4] = {1.7f, 1.55f, 1.52f, 1.8f};
// element of every slot of every residue type (ids follow ACDEFGHIKLMNPQRSTVWY; slots 0 N, 1 CA, 2 C, 3 O, then the side chain
// in build order): the first letters of protein/PDB_Creator.py's ATOM_MAP_14 (tests/test_clash_cli.py compares the two through
// ptamd_clash_radius).  How many slots a type has is NOT taken from here but from csrc/nerf_tables.h (ptamd_sidechain_atoms).
const char *const h_elements[NRES] = {
    /* A */ "NCCOC",          /* C */ "NCCOCS",         /* D */ "NCCOCCOO",    /* E */ "NCCOCCCOO",  /* F */ "NCCOCCCCCCC",
    /* G */ "NCCO",           /* H */ "NCCOCCNCNC",     /* I */ "NCCOCCCC",    /* K */ "NCCOCCCCN",  /* L */ "NCCOCCCC",
    /* M */ "NCCOCCSC",       /* N */ "NCCOCCON",       /* P */ "NCCOCCC",     /* Q */ "NCCOCCCON",  /* R */ "NCCOCCCNCNN",
    /* S */ "NCCOCO",         /* T */ "NCCOCOC",        /* V */ "NCCOCCC",     /* W */ "NCCOCCCNCCCCCC",
    /* Y */ "NCCOCCCCCOCC"};
constexpr int CYS_ID = 1, SG_SLOT = 5;

// per residue type one word for the compaction: bits 2 s, 2 s + 1 = element code of slot s; bits 28..31 = side-chain atoms
struct ResidueTable {
  unsigned info[NRES];
};
int element_code(char c) { return c == 'C' ? EL_C : c == 'N' ? EL_N : c == 'O' ? EL_O : c == 'S' ? EL_S : -1; }
// false if the element strings and csrc/nerf_tables.h disagree about the atoms of a residue type (a build error, not an input)
bool make_table(ResidueTable &t) {
  for (int r = 0; r < NRES; ++r) {
    const int nsc = ptamd_sidechain_atoms(r);
    if (nsc < 0 || (int)strlen(h_elements[r]) != 4 + nsc) return false;
    unsigned w = (unsigned)nsc << 28;
    for (int s = 0; s < 4 + nsc; ++s) {
      const int e = element_code(h_elements[r][s]);
      if (e < 0) return false;
      w |= (unsigned)e << (2 * s);
    }
    t.info[r] = w;
  }
  return true;
}

// a compacted atom: the 32 bytes of atom_tiles::Atom8, so its tiles and its workspace head are atom_tiles'.  code = residue << 1
// | (predicted coordinate unusable), -1 behind the last atom; kind: what the two exclusions ask about
constexpr int KIND_N = 1, KIND_C = 2, KIND_SG = 4;
struct __attribute__((aligned(32))) ClashAtom {
  float x, y, z, r;
  int code, slot, kind, unused;
};
static_assert(sizeof(ClashAtom) == sizeof(Atom8), "the tiles of csrc/atom_tiles.h");
__device__ __forceinline__ ClashAtom dead_atom() { return ClashAtom{0.f, 0.f, 0.f, 0.f, -1, 0, 0, 0}; }

struct __attribute__((aligned(16))) Item {   // what one work item of the sweep leaves for the finalize kernel
  double sum;          // sum of v over its violating pairs
  long long nclash;    // its violating pairs
};

struct Layout {
  TileLayout t;
  size_t nbad, rowpart, colpart, kept, items, total;
  int strips, chunks;
  Layout(int B, int L) : t(B, L) {
    strips = (t.tiles + STRIP_TILES - 1) / STRIP_TILES;
    chunks = (t.tiles + CHUNK_TILES - 1) / CHUNK_TILES;
    total = t.end;
    nbad = take(total, (size_t)B * sizeof(int));                                  // [b] atoms with an unusable prediction
    rowpart = take(total, (size_t)B * t.tiles * chunks * TS * sizeof(float4));   // [b][row tile][chunk][lane]
    colpart = take(total, (size_t)B * strips * t.tiles * TS * sizeof(float4));   // [b][strip][column tile][lane]
    kept = take(total, (size_t)B * strips * t.tiles * sizeof(int));              // [b][strip][column tile]
    items = take(total, (size_t)B * strips * chunks * sizeof(Item));             // [b][strip][chunk]
  }
};

// ---- stage 1: compaction, the scheme of atom_tiles::compact_kernel (one workgroup per protein, 16 wavefronts with contiguous
// shares of the slots, count then write, slot order kept) with this file's presence test and the boxes of the prediction.
__global__ __launch_bounds__(COMPACT_THREADS) void clash_compact_kernel(const float *__restrict__ pred, const int64_t *__restrict__ seq,
                                                                        int L, int nstride, int tiles, ResidueTable tab,
                                                                        ClashAtom *atoms, Box8 *boxes, int *__restrict__ natoms,
                                                                        int *__restrict__ nbad) {
  constexpr int NWAVE = COMPACT_THREADS / 64;
  __shared__ int s_cnt[NWAVE], s_bad[NWAVE];
  __shared__ unsigned s_info[NRES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nslot = L * PTAMD_NUM_SLOTS;
  pred += (size_t)b * nslot * 3;
  seq += (size_t)b * L;
  atoms += (size_t)b * nstride;
  boxes += (size_t)b * tiles;
  if (tid < NRES) s_info[tid] = tab.info[tid];
  __syncthreads();
  const int per = ((nslot + NWAVE - 1) / NWAVE + 63) / 64 * 64;   // slots of a wavefront: whole rows of 64
  const int s0 = min(w * per, nslot), s1 = min(s0 + per, nslot);
  // the slot exists for its residue type: neither pad nor an unknown id, and within the type's atoms.  What the slot holds is
  // not looked at
  auto present = [&](int s, int &res, int &ls, unsigned &info) __attribute__((always_inline)) {
    if (s >= s1) return false;
    res = s / PTAMD_NUM_SLOTS;
    ls = s - res * PTAMD_NUM_SLOTS;
    const int64_t id = seq[res];
    if (id < 0 || id >= NRES) return false;
    info = s_info[(int)id];
    return ls < 4 + (int)(info >> 28);
  };
  int cnt = 0;   // (wavefront-uniform)
  for (int r = s0; r < s1; r += 64) {
    int res, ls;
    unsigned info;
    cnt += __popcll(__ballot(present(r + lane, res, ls, info)));
  }
  if (lane == 0) s_cnt[w] = cnt;
  __syncthreads();
  int pos0 = 0, n = 0;
#pragma unroll
  for (int t = 0; t < NWAVE; ++t) {
    if (t < w) pos0 += s_cnt[t];
    n += s_cnt[t];
  }
  int bad_cnt = 0;   // (wavefront-uniform)
  for (int r = s0; r < s1; r += 64) {
    int res = 0, ls = 0;
    unsigned info = 0u;
    const int s = r + lane;
    const bool ok = present(s, res, ls, info);
    const unsigned long long m = __ballot(ok);
    bool bad = false;
    if (ok) {
      const int pos = pos0 + __popcll(m & ((1ull << lane) - 1ull));
      float x = pred[(size_t)s * 3], y = pred[(size_t)s * 3 + 1], z = pred[(size_t)s * 3 + 2];
      bad = !(fabsf(x) <= PRED_MAX && fabsf(y) <= PRED_MAX && fabsf(z) <= PRED_MAX);   // (NaN fails every test)
      if (bad) x = y = z = 0.f;
      const int el = (int)(info >> (2 * ls)) & 3;
      const float rad = el == EL_C ? 1.7f : el == EL_N ? 1.55f : el == EL_O ? 1.52f : 1.8f;
      const int kind = ls == 0 ? KIND_N : ls == 2 ? KIND_C : (ls == SG_SLOT && seq[res] == CYS_ID) ? KIND_SG : 0;
      atoms[pos] = ClashAtom{x, y, z, rad, (res << 1) | (int)bad, s, kind, 0};
    }
    bad_cnt += __popcll(__ballot(bad));
    pos0 += __popcll(m);
  }
  if (lane == 0) s_bad[w] = bad_cnt;
  if (tid == 0) natoms[b] = n;
  __syncthreads();   // the atoms this workgroup wrote are visible to all of it
  if (tid == 0) {
    int nb = 0;
    for (int t = 0; t < NWAVE; ++t) nb += s_bad[t];
    nbad[b] = nb;
  }
  const float inf = __builtin_inff();
  for (int t = w; t * TS < n; t += NWAVE) {
    const int j = t * TS + lane;
    const bool live = j < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
      const ClashAtom a = atoms[j];
      x = a.x; y = a.y; z = a.z;
    }
    const float lox = wave_min(live ? x : inf), loy = wave_min(live ? y : inf), loz = wave_min(live ? z : inf);
    const float hix = wave_max(live ? x : -inf), hiy = wave_max(live ? y : -inf), hiz = wave_max(live ? z : -inf);
    if (lane == 0) boxes[t] = Box8{lox, loy, loz, hix, hiy, hiz, 0.f, 0.f};
  }
}

// ---- stage 2: the pair sweep.  grid (strips * chunks, B), one wavefront per workgroup = one work item (csrc/slddt.hip).
// Per pair: 3 subtractions, 3 multiply-adds, v_sqrt_f32, and for the gradient v_rsq_f32.  The clamp under the root is the 1e-30
// of csrc/drmsd.hip and csrc/slddt.hip, added to the rounded sum of the squares.  A row atom always precedes its column atom in
// slot order (upper triangle of tiles in slot order, lane < column on the diagonal), so the peptide bond is (row C, column N).
template <bool WITH_GRAD>
__global__ __launch_bounds__(TS) void clash_sweep_kernel(const ClashAtom *__restrict__ atoms, const Box8 *__restrict__ boxes,
                                                         const int *__restrict__ natoms, int nstride, int tiles, int strips,
                                                         int chunks, float tau, float reach, float4 *__restrict__ rowpart,
                                                         float4 *__restrict__ colpart, int *__restrict__ kept,
                                                         Item *__restrict__ items) {
  __shared__ ClashAtom s_col[TS];
  __shared__ float s_cf[TS * CF_LD];
  __shared__ float4 s_row[TS];
  const int b = blockIdx.y, lane = threadIdx.x;
  const int strip = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  const int I0 = strip * STRIP_TILES;
  const int J0 = max(I0, chunk * CHUNK_TILES), J1 = min(nT, (chunk + 1) * CHUNK_TILES);
  if (I0 >= nT || J0 >= J1) return;   // below the diagonal or behind the protein: the finalize kernel skips these items too
  atoms += (size_t)b * nstride;
  boxes += (size_t)b * tiles;

  // near[r]: bit l = column tile J0 + l can hold a violating pair with row tile I0 + r
  unsigned long long near[STRIP_TILES];
  {
    Box8 c = Box8{0, 0, 0, 0, 0, 0, 0, 0};
    const bool have = J0 + lane < J1;
    if (have) c = boxes[J0 + lane];
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) {
      near[r] = 0ull;
      if (I0 + r < nT) near[r] = __ballot(have && I0 + r <= J0 + lane && boxes_near(boxes[I0 + r], c, reach));
    }
  }

  ClashAtom me[STRIP_TILES];
  float gx[STRIP_TILES], gy[STRIP_TILES], gz[STRIP_TILES];
#pragma unroll
  for (int r = 0; r < STRIP_TILES; ++r) {
    me[r] = dead_atom();
    const int i = (I0 + r) * TS + lane;
    if (i < n) me[r] = atoms[i];
    gx[r] = gy[r] = gz[r] = 0.f;
  }
  double v_sum = 0.0;
  int hits = 0;

  for (int J = J0; J < J1; ++J) {
    const int jb = J - J0;
    const bool any = ((near[0] | near[1] | near[2] | near[3]) >> jb) & 1ull;
    if (lane == 0) kept[((size_t)b * strips + strip) * tiles + J] = any;
    if (!any) continue;   // wavefront-uniform
    const int cnt = min(TS, n - J * TS);   // live columns of the tile
    {
      const int j = J * TS + lane;
      s_col[lane] = j < n ? atoms[j] : dead_atom();
    }
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);   // (S, Vx, Vy, Vz) of column `lane` of the tile
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r) {
      if (!((near[r] >> jb) & 1ull)) continue;   // wavefront-uniform
      const ClashAtom a = me[r];
      const bool a_live = a.code >= 0;
      const bool diag = I0 + r == J;   // the diagonal tile: pairs i < j only
      const float ra = a.r - tau;
      const int a_next = (a.code >> 1) + 1;   // the residue whose N is bonded to this atom, if this atom is a C
      if (WITH_GRAD) s_row[lane] = make_float4(a.x, a.y, a.z, 0.f);
      float v_t = 0.f;
      for (int j0 = 0; j0 < cnt; j0 += SUB) {
        __builtin_amdgcn_wave_barrier();
        bool sub_hit = false;
#pragma unroll 4
        for (int jj = 0; jj < SUB; ++jj) {
          const int j = j0 + jj;
          const ClashAtom c = s_col[j];   // broadcast
          const float dx = a.x - c.x, dy = a.y - c.y, dz = a.z - c.z;
          const float q = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) + 1e-30f;
          const float d = __builtin_amdgcn_sqrtf(q);
          const float v = (ra + c.r) - d;
          // different residues; a column behind the last atom has code -1 (and a dead row is excluded by a_live)
          const bool pair = (unsigned)(a.code ^ c.code) > 1u && c.code >= 0 && a_live && (!diag || lane < j);
          const bool peptide = a.kind == KIND_C && c.kind == KIND_N && (c.code >> 1) == a_next;
          const bool disulfide = (a.kind & c.kind & KIND_SG) != 0;
          const bool hit = pair && !peptide && !disulfide && v > 0.f;
          v_t += hit ? v : 0.f;
          hits += hit ? 1 : 0;
          if (WITH_GRAD) {
            // d(v)/d(x_a) = -(x_a - x_c) / d; atoms that coincide exactly (q is the clamp alone) have a zero gradient
            const float cf = hit && q > 1e-30f ? -__builtin_amdgcn_rsqf(q) : 0.f;
            gx[r] = fmaf(cf, dx, gx[r]);
            gy[r] = fmaf(cf, dy, gy[r]);
            gz[r] = fmaf(cf, dz, gz[r]);
            s_cf[lane * CF_LD + jj] = cf;
            sub_hit |= hit;
          }
        }
        if (WITH_GRAD && __ballot(sub_hit) != 0ull) {   // (wavefront-uniform) violations are rare: most 16 columns have none
          // phase 2 for these 16 columns: lane = (column j0 + (lane & 15), quarter lane >> 4 of the rows)
          __builtin_amdgcn_wave_barrier();
          const int col = lane & (SUB - 1), r0 = (lane >> 4) * SUB;
          float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int rr = 0; rr < SUB; ++rr) {
            const float c = s_cf[(r0 + rr) * CF_LD + col];
            const float4 x = s_row[r0 + rr];
            p.x += c;
            p.y = fmaf(c, x.x, p.y);
            p.z = fmaf(c, x.y, p.z);
            p.w = fmaf(c, x.z, p.w);
          }
          // fold the four row quarters (lanes l, l ^ 16, l ^ 32, l ^ 48) in a fixed order: every lane ends with the sum
          p.x += __shfl_xor(p.x, 16, 64); p.y += __shfl_xor(p.y, 16, 64); p.z += __shfl_xor(p.z, 16, 64); p.w += __shfl_xor(p.w, 16, 64);
          p.x += __shfl_xor(p.x, 32, 64); p.y += __shfl_xor(p.y, 32, 64); p.z += __shfl_xor(p.z, 32, 64); p.w += __shfl_xor(p.w, 32, 64);
          if ((lane >> 4) == (j0 >> 4)) {   // lane l keeps column l of the tile
            cs.x += p.x; cs.y += p.y; cs.z += p.z; cs.w += p.w;
          }
        }
      }
      v_sum += (double)v_t;
      __builtin_amdgcn_wave_barrier();   // s_row is rewritten for the next row tile
    }
    if (WITH_GRAD) colpart[(((size_t)b * strips + strip) * tiles + J) * TS + lane] = cs;
    __builtin_amdgcn_wave_barrier();     // s_col is rewritten for the next column tile
  }
  if (WITH_GRAD) {
#pragma unroll
    for (int r = 0; r < STRIP_TILES; ++r)
      if (I0 + r < nT) rowpart[(((size_t)b * tiles + I0 + r) * chunks + chunk) * TS + lane] = make_float4(gx[r], gy[r], gz[r], 0.f);
  }
  v_sum = wave_sum_d(v_sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) hits += __shfl_xor(hits, o, 64);   // (<= 4 * 8 * 64 * 64: an int)
  if (lane == 0) items[((size_t)b * strips + strip) * chunks + chunk] = Item{v_sum, (long long)hits};
}

// ---- stage 3: grid (ceil(nstride / 256), B).  Every workgroup of a protein sums the protein's work items: thread t takes the
// items t, t + 256, ... of the protein's OWN triangle (strips and chunks of its atom count, whatever L is), then a fixed tree.
// `dcrd` was zeroed before unless the call accumulates; only the slots of atoms are touched here.
__global__ __launch_bounds__(FIN_THREADS) void clash_finalize_kernel(const ClashAtom *__restrict__ atoms, const int *__restrict__ natoms,
                                                                     const int *__restrict__ nbad, const float4 *__restrict__ rowpart,
                                                                     const float4 *__restrict__ colpart,
                                                                     const int *__restrict__ kept, const Item *__restrict__ items,
                                                                     int nstride, int tiles, int strips, int chunks, float weight,
                                                                     int accumulate, float *__restrict__ stats,
                                                                     long long *__restrict__ nclash, float *dcrd, int nslot) {
  __shared__ double s_sum[FIN_THREADS];
  __shared__ long long s_cnt[FIN_THREADS];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  if ((int)blockIdx.x * FIN_THREADS >= max(n, 1)) return;
  const bool unusable = nbad[b] > 0;
  if (blockIdx.x == 0) {
    const int sN = (nT + STRIP_TILES - 1) / STRIP_TILES, cN = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
    double e = 0.0;
    long long c = 0;
    for (int r = tid; r < sN * cN; r += FIN_THREADS) {
      const int s = r / cN, ch = r % cN;
      if ((ch + 1) * CHUNK_TILES <= s * STRIP_TILES) continue;   // below the diagonal: never written
      const Item it = items[((size_t)b * strips + s) * chunks + ch];
      e += it.sum;
      c += it.nclash;
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
    if (tid == 0) {
      const bool valued = n > 0 && !unusable;
      stats[(size_t)b * 2] = valued ? (float)(s_sum[0] / (double)n) : __builtin_nanf("");
      stats[(size_t)b * 2 + 1] = (float)n;
      nclash[b] = valued ? s_cnt[0] : 0ll;   // (no pair of an unusable protein counts)
    }
  }
  if (dcrd == nullptr || unusable) return;   // an unusable protein: zeros (filled before), or nothing added
  const int j = blockIdx.x * FIN_THREADS + tid;
  if (j >= n) return;
  const float inv_n = (float)(1.0 / (double)n);
  const ClashAtom a = atoms[(size_t)b * nstride + j];
  const int J = j / TS, lane = j & (TS - 1), sJ = J / STRIP_TILES;
  float rx = 0.f, ry = 0.f, rz = 0.f, cx = 0.f, cy = 0.f, cz = 0.f;
  {  // row side: the chunks of the atom's strip that had work, in chunk order
    const int c0 = (STRIP_TILES * sJ) / CHUNK_TILES, c1 = (nT + CHUNK_TILES - 1) / CHUNK_TILES;
    const float4 *rp = rowpart + ((size_t)b * tiles + J) * chunks * TS + lane;
    for (int c = c0; c < c1; ++c) {
      const float4 r = rp[(size_t)c * TS];
      rx += r.x; ry += r.y; rz += r.z;
    }
  }
  for (int s = 0; s <= sJ; ++s) {  // column side: the strips at or above the atom's tile that touched it, in strip order
    const size_t at = ((size_t)b * strips + s) * tiles + J;
    if (!kept[at]) continue;
    const float4 cp = colpart[at * TS + lane];
    cx += fmaf(a.x, cp.x, -cp.y);
    cy += fmaf(a.y, cp.x, -cp.z);
    cz += fmaf(a.z, cp.x, -cp.w);
  }
  float *out = dcrd + ((size_t)b * nslot + a.slot) * 3;
  // g is rounded as the unweighted call rounds it; weight * g, or dcrd + weight * g in one multiply-add, is rounded once more
  const float g0 = inv_n * (rx + cx), g1 = inv_n * (ry + cy), g2 = inv_n * (rz + cz);
  out[0] = accumulate ? fmaf(weight, g0, out[0]) : weight * g0;
  out[1] = accumulate ? fmaf(weight, g1, out[1]) : weight * g1;
  out[2] = accumulate ? fmaf(weight, g2, out[2]) : weight * g2;
}

}  // namespace

extern "C" {

float ptamd_clash_radius(int residue, int slot) {
  if (residue < 0 || residue >= NRES || slot < 0) return -1.f;
  const int nsc = ptamd_sidechain_atoms(residue);
  if (slot >= 4 + nsc || slot >= (int)strlen(h_elements[residue])) return -1.f;
  const int e = element_code(h_elements[residue][slot]);
  return e < 0 ? -1.f : h_radius[e];
}

size_t ptamd_clash_workspace_bytes(int B, int L) {
  if (!tile_shape_ok(B, L)) return 0;
  return Layout(B, L).total;
}

int ptamd_clash_fwd_bwd(const float *pred_crd, const int64_t *seq, int B, int L, float tolerance, float weight, int accumulate,
                        float *stats, int64_t *nclash, float *dcrd, void *workspace, size_t workspace_bytes, void *stream) {
  if (!tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !seq || !stats || !nclash) return PTAMD_ERR_BAD_SHAPE;
  if (!(tolerance >= 0.f) || !isfinite(tolerance) || !isfinite(weight)) return PTAMD_ERR_BAD_SHAPE;
  const Layout l(B, L);
  if (!workspace || workspace_bytes < l.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  if ((size_t)l.strips * l.chunks > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;   // (a grid dimension; its workspace is beyond any device)
  ResidueTable tab;
  if (!make_table(tab)) return PTAMD_ERR_BAD_SHAPE;
  char *ws = static_cast<char *>(workspace);
  ClashAtom *atoms = reinterpret_cast<ClashAtom *>(ws + l.t.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.t.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.t.natoms), *nbad = reinterpret_cast<int *>(ws + l.nbad);
  float4 *rowpart = reinterpret_cast<float4 *>(ws + l.rowpart), *colpart = reinterpret_cast<float4 *>(ws + l.colpart);
  int *kept = reinterpret_cast<int *>(ws + l.kept);
  Item *items = reinterpret_cast<Item *>(ws + l.items);
  const float reach = fmaxf(0.f, 2.f * R_MAX - tolerance);
  hipStream_t st = (hipStream_t)stream;
  const int nslot = L * PTAMD_NUM_SLOTS;
  if (dcrd && !accumulate) PT_HIP_TRY(hipMemsetAsync(dcrd, 0, (size_t)B * nslot * 3 * sizeof(float), st));   // slots without an atom stay 0
  hipLaunchKernelGGL(clash_compact_kernel, dim3(B), dim3(COMPACT_THREADS), 0, st, pred_crd, seq, L, l.t.nstride, l.t.tiles, tab, atoms,
                     boxes, natoms, nbad);
  int rc = pt_check_launch();
  if (rc) return rc;
  auto sweep = dcrd ? clash_sweep_kernel<true> : clash_sweep_kernel<false>;
  hipLaunchKernelGGL(sweep, dim3((unsigned)(l.strips * l.chunks), B), dim3(TS), 0, st, atoms, boxes, natoms, l.t.nstride, l.t.tiles,
                     l.strips, l.chunks, tolerance, reach, rowpart, colpart, kept, items);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(clash_finalize_kernel, dim3(dcrd ? (unsigned)((l.t.nstride + FIN_THREADS - 1) / FIN_THREADS) : 1u, B),
                     dim3(FIN_THREADS), 0, st, atoms, natoms, nbad, rowpart, colpart, kept, items, l.t.nstride, l.t.tiles, l.strips,
                     l.chunks, weight, accumulate ? 1 : 0, stats, reinterpret_cast<long long *>(nclash), dcrd, nslot);
  return pt_check_launch();
}

}  // extern "C"
