// Batched TM-score and GDT_TS / GDT_HA over the C-alphas, for gfx950: the evaluation metrics `tm-ca`, `gdt-ts`, `gdt-ha` of
// `train.py --eval_tm`.
//
// The reference (protein_transformer) has no counterpart: its evaluation stops at dRMSD and the superposed RMSD.  These are the
// scores CASP ranks predictions by - Zhang & Skolnick, "Scoring function for automated assessment of protein structure template
// quality", Proteins 57:702-710 (2004), with the seed-and-refine superposition search of the public TMscore program.  Both are
// MAXIMA over superpositions, not values at the least-squares one (csrc/kabsch.hip): the search needs the rotation itself and
// runs thousands of small superpositions per protein.  The definition - residues, d0, seeds, refinement, what the maxima are
// taken over - is in include/ptamd.h; this file restates only what the kernels do with it.
//
// Three launches per batch:
//   compact   one wavefront per protein writes the (pred, true) C-alpha pairs of its present residues, in sequence order, into the
//             caller's workspace: 24 B per residue, N of them, and whether a present C-alpha has a non-finite prediction.
//             (csrc/atom_tiles.h compacts ATOMS - all 14 slots of a residue, 32-byte records, a bounding box per tile of 64 - for
//             the pair sweeps; a residue-level list of one slot in 14 is neither a subset of its records nor cheaper to derive
//             from them than from the inputs, so this file has its own 20 lines.)
//   search    ONE WAVEFRONT OWNS ONE SEED AT A TIME and walks its <= 21 superpositions.  Lane l owns residues l, l + 64, ...;
//             its share of the current selection is one bit per owned residue in a 64-bit register (hence L <= 4096).  Per
//             superposition: the lanes sum the 15 moments of the selected pairs in fp64, a butterfly (wave_sum_d) leaves the
//             same bits in every lane, every lane solves for the rotation (csrc/tm_rotation.h: Horn's quaternion matrix,
//             cyclic Jacobi), then the same lanes score all N residues - TM sum, five GDT counts (ballots) - and reselect.
//             "Selection unchanged" is one wave-wide vote.  Moments, rotation, distances and every threshold decision are fp64
//             on the fp32 inputs; thresholds are tested on SQUARED distances (d^2 < c^2: the same decision as d < c unless d is
//             within rounding, 1e-16 relative, of c).  The compacted coordinates are re-read from the workspace in every pass:
//             12 KB per protein at L = 512, resident in L2 / the vector L1 - one code path for every N.  A wavefront merges its
//             SEEDS_PER_WAVE consecutive seeds in seed order and writes one record: TM sum, counts, transform.
//   finalize  one wavefront per protein takes the maxima over the records in seed order (the first record that reaches the
//             largest TM sum gives the transform) and writes score, counts, xform.
// No atomics, no order-dependent reduction: two runs give the same bits.
#include <math.h>

#include "atom_tiles.h"
#include "tm_rotation.h"

namespace {

using atom_tiles::take;
using tm_rotation::NMOM;

constexpr int CA_SLOT = 1;          // the C-alpha of a residue (csrc/lddt.hip)
constexpr int TM_MAX_L = 4096;      // 64 lanes x 64 selection bits
constexpr int SEEDS_PER_WAVE = 4;   // consecutive seeds a wavefront of the search merges into one record
constexpr int SEARCH_WAVES = 4;     // wavefronts per workgroup of the search; they never talk to each other
constexpr int MAX_REFINE = 20;
constexpr int NLEN = 6;             // fragment lengths N, N>>1, N>>2, N>>3, N>>4, 4
constexpr int NCUT = 5;             // GDT cutoffs 0.5, 1, 2, 4, 8 A

struct __attribute__((aligned(8))) CaPair {
  float px, py, pz, tx, ty, tz;
};
struct __attribute__((aligned(16))) SeedBest {   // 128 bytes
  double tm_sum;
  int c[NCUT];
  int pad;
  double x[12];
};

inline bool tm_shape_ok(int B, int L) { return B > 0 && L > 0 && L <= TM_MAX_L; }

struct TmLayout {
  size_t hdr, ca, best, end;
  int chunks;   // records per protein: every seed of a protein of L residues has one (at most NLEN * L seeds)
  TmLayout(int B, int L) {
    chunks = (NLEN * L + SEEDS_PER_WAVE - 1) / SEEDS_PER_WAVE;
    end = 0;
    hdr = take(end, (size_t)B * sizeof(int2));
    ca = take(end, (size_t)B * L * sizeof(CaPair));
    best = take(end, (size_t)B * chunks * sizeof(SeedBest));
  }
};

// The seed list of a protein of N >= 3 residues, without a table: returns the number of seeds and, for 0 <= seed < that number,
// its fragment length and start.  Lengths max(N >> k, 4) for k = 0..4, then 4, lowered to N when N = 3; the list never
// increases, so duplicates are neighbours.
__device__ __forceinline__ int seed_locate(int N, int seed, int &len, int &start) {
  int prev = -1, base = 0;
#pragma unroll
  for (int k = 0; k < NLEN; ++k) {
    int l = k < NLEN - 1 ? N >> k : 4;
    l = min(max(l, 4), N);
    if (l != prev) {
      const int cnt = N - l + 1;
      if (seed >= base && seed < base + cnt) {
        len = l;
        start = seed - base;
      }
      base += cnt;
      prev = l;
    }
  }
  return base;
}

__device__ __forceinline__ double tm_d0(int N) { return N > 21 ? fmax(1.24 * cbrt((double)(N - 15)) - 1.8, 0.5) : 0.5; }

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- stage 1
__global__ __launch_bounds__(64) void tm_compact_kernel(const float *__restrict__ pred, const float *__restrict__ truth,
                                                        const int64_t *__restrict__ seq, int L, CaPair *__restrict__ ca,
                                                        int2 *__restrict__ hdr) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const size_t nslot = (size_t)L * PTAMD_NUM_SLOTS;
  pred += (size_t)b * nslot * 3;
  truth += (size_t)b * nslot * 3;
  seq += (size_t)b * L;
  ca += (size_t)b * L;
  int n = 0;   // (wavefront-uniform)
  bool bad = false;
  for (int r0 = 0; r0 < L; r0 += 64) {
    const int r = r0 + lane;
    const size_t at = ((size_t)r * PTAMD_NUM_SLOTS + CA_SLOT) * 3;
    float tx = 0.f, ty = 0.f, tz = 0.f;
    bool ok = false;
    if (r < L && seq[r] != PTAMD_PAD_ID) {   // batch padding carries zeros, not NaN
      tx = truth[at]; ty = truth[at + 1]; tz = truth[at + 2];
      ok = !(isnan(tx) || isnan(ty) || isnan(tz));
    }
    const unsigned long long m = __ballot(ok);
    if (ok) {   // what the prediction holds never decides presence
      const float px = pred[at], py = pred[at + 1], pz = pred[at + 2];
      bad = bad || !(isfinite(px) && isfinite(py) && isfinite(pz));
      ca[n + __popcll(m & ((1ull << lane) - 1ull))] = CaPair{px, py, pz, tx, ty, tz};
    }
    n += __popcll(m);
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) hdr[b] = make_int2(n, any_bad ? 1 : 0);
}

// ---- stage 2
struct Pair64 {
  double p[3], q[3];
};
// pair i relative to the protein's origin `org` (its first pair): moments of coordinates of the size of the protein, not of its
// distance from the origin of the file, so a structure 1e3 A away loses nothing to cancellation
__device__ __forceinline__ Pair64 load_pair(const CaPair *__restrict__ ca, int i, const Pair64 &org) {
  const float2 *g = reinterpret_cast<const float2 *>(ca + i);
  const float2 a = g[0], b = g[1], c = g[2];
  return Pair64{{(double)a.x - org.p[0], (double)a.y - org.p[1], (double)b.x - org.p[2]},
                {(double)b.y - org.q[0], (double)c.x - org.q[1], (double)c.y - org.q[2]}};
}

// least-squares superposition of the selected pairs: x = (R row-major, t), the same bits in every lane
__device__ __forceinline__ void superpose(const CaPair *__restrict__ ca, const Pair64 &org, int N, int lane,
                                          unsigned long long bits, int nsel, double (&x)[12]) {
  double m[NMOM];
#pragma unroll
  for (int k = 0; k < NMOM; ++k) m[k] = 0.0;
  for (int r = 0, i = lane; r * 64 < N; ++r, i += 64) {
    if ((bits >> r) & 1ull) {
      const Pair64 a = load_pair(ca, i, org);
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        m[u] += a.p[u];
        m[3 + u] += a.q[u];
#pragma unroll
        for (int v = 0; v < 3; ++v) m[6 + 3 * u + v] = fma(a.p[u], a.q[v], m[6 + 3 * u + v]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NMOM; ++k) m[k] = wave_sum_d(m[k]);
  tm_rotation::solve(m, nsel, x);
}

// all N residues under x: this lane's bits of {i : d_i^2 < cut2} and their number over the wavefront, the smallest d^2 this lane
// left out, and with SCORE the TM sum and the five counts
template <bool SCORE>
__device__ __forceinline__ void sweep(const CaPair *__restrict__ ca, const Pair64 &org, int N, int lane, const double (&x)[12],
                                      double cut2, double d0sq, unsigned long long &bits, int &nsel, double &out_min, double &tm_sum,
                                      int (&cnt)[NCUT]) {
  constexpr double K2[NCUT] = {0.25, 1.0, 4.0, 16.0, 64.0};
  bits = 0ull;
  nsel = 0;
  out_min = __builtin_inf();
  double tm = 0.0;
  if (SCORE) {
#pragma unroll
    for (int k = 0; k < NCUT; ++k) cnt[k] = 0;
  }
  for (int r = 0, i = lane; r * 64 < N; ++r, i += 64) {
    const bool live = i < N;
    double d2 = __builtin_inf();
    if (live) {
      const Pair64 a = load_pair(ca, i, org);
      const double ex = fma(x[0], a.p[0], fma(x[1], a.p[1], fma(x[2], a.p[2], x[9]))) - a.q[0];
      const double ey = fma(x[3], a.p[0], fma(x[4], a.p[1], fma(x[5], a.p[2], x[10]))) - a.q[1];
      const double ez = fma(x[6], a.p[0], fma(x[7], a.p[1], fma(x[8], a.p[2], x[11]))) - a.q[2];
      d2 = fma(ex, ex, fma(ey, ey, ez * ez));
      if (SCORE) tm += d0sq / (d0sq + d2);   // 1 / (1 + (d / d0)^2)
    }
    const bool in = live && d2 < cut2;
    if (live && !in) out_min = fmin(out_min, d2);
    bits |= (unsigned long long)in << r;
    nsel += __popcll(__ballot(in));
    if (SCORE) {
#pragma unroll
      for (int k = 0; k < NCUT; ++k) cnt[k] += __popcll(__ballot(live && d2 <= K2[k]));
    }
  }
  if (SCORE) tm_sum = wave_sum_d(tm);
}

__global__ __launch_bounds__(64 * SEARCH_WAVES) void tm_search_kernel(const CaPair *__restrict__ ca, const int2 *__restrict__ hdr,
                                                                      int L, int chunks, SeedBest *__restrict__ best) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int chunk = blockIdx.x * SEARCH_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int2 h = hdr[b];
  const int N = h.x;
  if (N < 3 || h.y != 0) return;   // everything below is wavefront-uniform control flow; no barrier anywhere
  int len = 0, start = 0;
  const int nseeds = seed_locate(N, -1, len, start);
  const int seed0 = chunk * SEEDS_PER_WAVE, seed1 = min(seed0 + SEEDS_PER_WAVE, nseeds);
  if (seed0 >= nseeds) return;
  ca += (size_t)b * L;
  const Pair64 zero = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  const Pair64 org = load_pair(ca, 0, zero);
  const double d0 = tm_d0(N), d0sq = d0 * d0;
  const double d_search = fmin(8.0, fmax(4.5, d0));

  double best_tm = -1.0, best_x[12];
  int best_c[NCUT];
#pragma unroll
  for (int k = 0; k < 12; ++k) best_x[k] = 0.0;
#pragma unroll
  for (int k = 0; k < NCUT; ++k) best_c[k] = 0;

  for (int seed = seed0; seed < seed1; ++seed) {
    seed_locate(N, seed, len, start);
    // the fragment as a selection: lane l owns residue l + 64 r as bit r
    unsigned long long bits = 0ull;
    for (int r = 0, i = lane; r * 64 < N; ++r, i += 64) bits |= (unsigned long long)(i >= start && i < start + len) << r;
    int nsel = len;
    for (int it = 0; it <= MAX_REFINE; ++it) {
      double x[12], tm_sum = 0.0, out_min, dummy_tm;
      int cnt[NCUT], dummy_cnt[NCUT];
      superpose(ca, org, N, lane, bits, nsel, x);
      // score, and select with d_search - 1 behind the fragment, d_search + 1 in the refinement; while fewer than 3 are
      // selected the cutoff rises in steps of 0.5 - here in one jump to the first step that admits the nearest residue left
      // out, which is where the stepwise loop arrives (a jump per admitted residue: at most 3; the 9th round, reachable only
      // with distances beyond 1e15 A where 0.5 is below the spacing of doubles, selects everything)
      const double c0 = it == 0 ? d_search - 1.0 : d_search + 1.0;
      unsigned long long nbits;
      int nn;
      sweep<true>(ca, org, N, lane, x, c0 * c0, d0sq, nbits, nn, out_min, tm_sum, cnt);
      double steps = 0.0;
      for (int round = 0; nn < 3; ++round) {
        const double nearest = sqrt(wave_min_d(out_min));
        steps = fmax(floor((nearest - c0) * 2.0) + 1.0, steps + 1.0);
        const double c = round < 8 ? c0 + 0.5 * steps : __builtin_inf();
        sweep<false>(ca, org, N, lane, x, c * c, d0sq, nbits, nn, out_min, dummy_tm, dummy_cnt);
      }
      if (tm_sum > best_tm) {   // strict: the earliest visited superposition that reaches the maximum keeps the transform
        best_tm = tm_sum;
#pragma unroll
        for (int k = 0; k < 12; ++k) best_x[k] = x[k];
      }
#pragma unroll
      for (int k = 0; k < NCUT; ++k) best_c[k] = max(best_c[k], cnt[k]);
      const bool same = __ballot(nbits != bits) == 0ull;
      bits = nbits;
      nsel = nn;
      if (it > 0 && same) break;
    }
  }
  if (lane == 0) {
    SeedBest out;
    out.tm_sum = best_tm;
#pragma unroll
    for (int k = 0; k < NCUT; ++k) out.c[k] = best_c[k];
    out.pad = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) out.x[k] = best_x[k];
#pragma unroll
    for (int u = 0; u < 3; ++u)   // the translation, back in the coordinates of the inputs
      out.x[9 + u] = best_x[9 + u] + org.q[u] - (best_x[3 * u] * org.p[0] + best_x[3 * u + 1] * org.p[1] + best_x[3 * u + 2] * org.p[2]);
    best[(size_t)b * chunks + chunk] = out;
  }
}

// ---- stage 3
__global__ __launch_bounds__(64) void tm_finalize_kernel(const int2 *__restrict__ hdr, const SeedBest *__restrict__ best, int chunks,
                                                         float *__restrict__ score, int32_t *__restrict__ counts,
                                                         float *__restrict__ xform) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int2 h = hdr[b];
  const int N = h.x;
  score += (size_t)b * 3;
  counts += (size_t)b * (1 + NCUT);
  if (xform) xform += (size_t)b * 12;
  if (N < 3 || h.y != 0) {
    const float nan = __builtin_nanf("");
    if (lane < 3) score[lane] = nan;
    if (lane < 1 + NCUT) counts[lane] = lane == 0 ? N : 0;
    if (xform && lane < 12) xform[lane] = nan;
    return;
  }
  int len, start;
  const int nrec = (seed_locate(N, -1, len, start) + SEEDS_PER_WAVE - 1) / SEEDS_PER_WAVE;
  best += (size_t)b * chunks;
  double tm = -2.0;
  int at = INT_MAX, c[NCUT];
#pragma unroll
  for (int k = 0; k < NCUT; ++k) c[k] = 0;
  for (int j = lane; j < nrec; j += 64) {   // ascending: a lane keeps the first of its records that reaches its maximum
    const double v = best[j].tm_sum;
    if (v > tm) {
      tm = v;
      at = j;
    }
#pragma unroll
    for (int k = 0; k < NCUT; ++k) c[k] = max(c[k], best[j].c[k]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {   // (larger TM sum, then lower record) is a total order: the butterfly's order is immaterial
    const double v = __shfl_xor(tm, o, 64);
    const int j = __shfl_xor(at, o, 64);
    if (v > tm || (v == tm && j < at)) {
      tm = v;
      at = j;
    }
#pragma unroll
    for (int k = 0; k < NCUT; ++k) c[k] = max(c[k], __shfl_xor(c[k], o, 64));
  }
  const double n4 = 4.0 * (double)N;
  const bool found = at < nrec;   // (always, for finite inputs: a TM sum is >= 0; a NaN sum would never be taken)
  if (lane == 0) {
    score[0] = found ? (float)(tm / (double)N) : __builtin_nanf("");
    score[1] = (float)((double)(c[1] + c[2] + c[3] + c[4]) / n4);   // GDT_TS: 1, 2, 4, 8 A
    score[2] = (float)((double)(c[0] + c[1] + c[2] + c[3]) / n4);   // GDT_HA: 0.5, 1, 2, 4 A
    counts[0] = N;
#pragma unroll
    for (int k = 0; k < NCUT; ++k) counts[1 + k] = c[k];
  }
  if (xform && lane < 12) xform[lane] = found ? (float)best[at].x[lane] : __builtin_nanf("");
}

}  // namespace

extern "C" {

size_t ptamd_tm_workspace_bytes(int B, int L) {
  if (!tm_shape_ok(B, L)) return 0;
  return TmLayout(B, L).end;
}

int ptamd_tm_score(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float *score, int32_t *counts,
                   float *xform, void *workspace, size_t workspace_bytes, void *stream) {
  if (!tm_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !score || !counts) return PTAMD_ERR_BAD_SHAPE;
  const TmLayout l(B, L);
  if (!workspace || workspace_bytes < l.end) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  char *ws = static_cast<char *>(workspace);
  int2 *hdr = reinterpret_cast<int2 *>(ws + l.hdr);
  CaPair *ca = reinterpret_cast<CaPair *>(ws + l.ca);
  SeedBest *best = reinterpret_cast<SeedBest *>(ws + l.best);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tm_compact_kernel, dim3(B), dim3(64), 0, st, pred_crd, true_crd, seq, L, ca, hdr);
  int rc = pt_check_launch();
  if (rc) return rc;
  const unsigned groups = (unsigned)((l.chunks + SEARCH_WAVES - 1) / SEARCH_WAVES);
  hipLaunchKernelGGL(tm_search_kernel, dim3(groups, B), dim3(64 * SEARCH_WAVES), 0, st, ca, hdr, L, l.chunks, best);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(tm_finalize_kernel, dim3(B), dim3(64), 0, st, hdr, best, l.chunks, score, counts, xform);
  return pt_check_launch();
}

}  // extern "C"
