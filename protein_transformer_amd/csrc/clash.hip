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
//   sweep     the strip-by-chunk sweep of csrc/pair_sweep.h over the upper triangle of tile pairs, shared with csrc/slddt.hip;
//             this file owns the pair term (ClashPair below: max(0, r_a + r_b - tau - d) and the two exclusions).  A tile pair
//             is skipped when the gap between its boxes exceeds 2 * 1.8 - tau: atoms in slot order are neighbours in space, so
//             almost every tile pair goes; and the transposed pass is skipped for 16 columns without a violating pair, which
//             is nearly all of the rest.
//   finalize  per protein the work items' sums (pair_sweep::item_sums), the loss, and per atom the gathered gradient
//             (pair_sweep::atom_gradient) scaled by 1 / n, and weight times that written or added to the slot layout.
// No atomics; two runs give the same bits; a protein's bits do not depend on the batch around it or on its padding.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "pair_sweep.h"

namespace {

using namespace pair_sweep;

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

struct Layout {
  TileLayout t;
  size_t total, nbad;   // nbad: [b] atoms with an unusable prediction, ahead of the sweep's pieces
  SweepLayout s;
  Layout(int B, int L) : t(B, L), total(t.end), nbad(take(total, (size_t)B * sizeof(int))), s(B, t.tiles, total) {}
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
      bad = pred_unusable(x, y, z);
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
  tile_boxes(n, boxes, [&](int j, float &x, float &y, float &z) __attribute__((always_inline)) {
    const ClashAtom a = atoms[j];
    x = a.x; y = a.y; z = a.z;
  });
}

// ---- stage 2: the pair term of the sweep.  An Item is the sum of v over the violating pairs, and their number.
// Per pair: 3 subtractions, 3 multiply-adds, v_sqrt_f32, and for the gradient v_rsq_f32.  The clamp under the root is the 1e-30
// of csrc/drmsd.hip and csrc/slddt.hip, added to the rounded sum of the squares.  A row atom always precedes its column atom in
// slot order (upper triangle of tiles in slot order, lane < column on the diagonal), so the peptide bond is (row C, column N).
struct ClashPair {
  using Atom = ClashAtom;
  static constexpr bool SPARSE = true;   // violations are rare: most 16 columns have none
  struct Row {
    float ra;     // r_a - tau
    int a_next;   // the residue whose N is bonded to this atom, if this atom is a C
  };
  float tau, reach_;
  static __device__ __forceinline__ Atom dead() { return ClashAtom{0.f, 0.f, 0.f, 0.f, -1, 0, 0, 0}; }
  static __device__ __forceinline__ float4 position(const Atom &a) { return make_float4(a.x, a.y, a.z, 0.f); }
  __device__ __forceinline__ float reach() const { return reach_; }
  __device__ __forceinline__ Row row(const Atom &a) const { return Row{a.r - tau, (a.code >> 1) + 1}; }
  __device__ __forceinline__ Term term(const Atom &a, Row row, const Atom &c, bool apart) const {
    const float dx = a.x - c.x, dy = a.y - c.y, dz = a.z - c.z;
    const float q = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) + 1e-30f;
    const float d = __builtin_amdgcn_sqrtf(q);
    const float v = (row.ra + c.r) - d;
    const bool peptide = a.kind == KIND_C && c.kind == KIND_N && (c.code >> 1) == row.a_next;
    const bool disulfide = (a.kind & c.kind & KIND_SG) != 0;
    const bool hit = apart && !peptide && !disulfide && v > 0.f;
    // d(v)/d(x_a) = -(x_a - x_c) / d; atoms that coincide exactly (q is the clamp alone) have a zero gradient
    const float cf = hit && q > 1e-30f ? -__builtin_amdgcn_rsqf(q) : 0.f;
    return Term{hit ? v : 0.f, hit, cf, dx, dy, dz};
  }
};

template <bool WITH_GRAD>
__global__ __launch_bounds__(TS) void clash_sweep_kernel(const ClashAtom *__restrict__ atoms, const Box8 *__restrict__ boxes,
                                                         const int *__restrict__ natoms, int nstride, Dims d, float tau, float reach,
                                                         float4 *__restrict__ rowpart, float4 *__restrict__ colpart,
                                                         int *__restrict__ kept, Item *__restrict__ items) {
  sweep<WITH_GRAD>(ClashPair{tau, reach}, atoms, boxes, natoms, nstride, d, rowpart, colpart, kept, items);
}

// ---- stage 3: grid (ceil(nstride / 256), B).  The first workgroup of a protein sums the protein's work items.
// `dcrd` was zeroed before unless the call accumulates; only the slots of atoms are touched here.
__global__ __launch_bounds__(FIN_THREADS) void clash_finalize_kernel(const ClashAtom *__restrict__ atoms, const int *__restrict__ natoms,
                                                                     const int *__restrict__ nbad, const float4 *__restrict__ rowpart,
                                                                     const float4 *__restrict__ colpart,
                                                                     const int *__restrict__ kept, const Item *__restrict__ items,
                                                                     int nstride, Dims d, float weight, int accumulate,
                                                                     float *__restrict__ stats, long long *__restrict__ nclash,
                                                                     float *dcrd, int nslot) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = natoms[b], nT = (n + TS - 1) / TS;
  if ((int)blockIdx.x * FIN_THREADS >= max(n, 1)) return;
  const bool unusable = nbad[b] > 0;
  if (blockIdx.x == 0) {
    const Item all = item_sums(items, d, b, nT);
    if (tid == 0) {
      const bool valued = n > 0 && !unusable;
      stats[(size_t)b * 2] = valued ? (float)(all.sum / (double)n) : __builtin_nanf("");
      stats[(size_t)b * 2 + 1] = (float)n;
      nclash[b] = valued ? all.count : 0ll;   // (no pair of an unusable protein counts)
    }
  }
  if (dcrd == nullptr || unusable) return;   // an unusable protein: zeros (filled before), or nothing added
  const int j = blockIdx.x * FIN_THREADS + tid;
  if (j >= n) return;
  const float inv_n = (float)(1.0 / (double)n);
  const ClashAtom a = atoms[(size_t)b * nstride + j];
  const float3 g = atom_gradient(rowpart, colpart, kept, d, b, j, nT, ClashPair::position(a));
  float *out = dcrd + ((size_t)b * nslot + a.slot) * 3;
  // g is rounded as the unweighted call rounds it; weight * g, or dcrd + weight * g in one multiply-add, is rounded once more
  const float g0 = inv_n * g.x, g1 = inv_n * g.y, g2 = inv_n * g.z;
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
  const Dims d = l.s.d;
  if (!workspace || workspace_bytes < l.total) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  if ((size_t)d.strips * d.chunks > (size_t)INT_MAX) return PTAMD_ERR_BAD_SHAPE;   // (a grid dimension; its workspace is beyond any device)
  ResidueTable tab;
  if (!make_table(tab)) return PTAMD_ERR_BAD_SHAPE;
  char *ws = static_cast<char *>(workspace);
  ClashAtom *atoms = reinterpret_cast<ClashAtom *>(ws + l.t.atoms);
  Box8 *boxes = reinterpret_cast<Box8 *>(ws + l.t.boxes);
  int *natoms = reinterpret_cast<int *>(ws + l.t.natoms), *nbad = reinterpret_cast<int *>(ws + l.nbad);
  float4 *rowpart = reinterpret_cast<float4 *>(ws + l.s.rowpart), *colpart = reinterpret_cast<float4 *>(ws + l.s.colpart);
  int *kept = reinterpret_cast<int *>(ws + l.s.kept);
  Item *items = reinterpret_cast<Item *>(ws + l.s.items);
  const float reach = fmaxf(0.f, 2.f * R_MAX - tolerance);
  hipStream_t st = (hipStream_t)stream;
  const int nslot = L * PTAMD_NUM_SLOTS;
  if (dcrd && !accumulate) PT_HIP_TRY(hipMemsetAsync(dcrd, 0, (size_t)B * nslot * 3 * sizeof(float), st));   // slots without an atom stay 0
  hipLaunchKernelGGL(clash_compact_kernel, dim3(B), dim3(COMPACT_THREADS), 0, st, pred_crd, seq, L, l.t.nstride, l.t.tiles, tab, atoms,
                     boxes, natoms, nbad);
  int rc = pt_check_launch();
  if (rc) return rc;
  auto sweep = dcrd ? clash_sweep_kernel<true> : clash_sweep_kernel<false>;
  hipLaunchKernelGGL(sweep, dim3((unsigned)(d.strips * d.chunks), B), dim3(TS), 0, st, atoms, boxes, natoms, l.t.nstride, d,
                     tolerance, reach, rowpart, colpart, kept, items);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(clash_finalize_kernel, dim3(dcrd ? (unsigned)((l.t.nstride + FIN_THREADS - 1) / FIN_THREADS) : 1u, B),
                     dim3(FIN_THREADS), 0, st, atoms, natoms, nbad, rowpart, colpart, kept, items, l.t.nstride, d,
                     weight, accumulate ? 1 : 0, stats, reinterpret_cast<long long *>(nclash), dcrd, nslot);
  return pt_check_launch();
}

}  // extern "C"
