// Batched secondary-structure agreement for gfx950: the evaluation metrics `ss-q3`, `ss-h`, `ss-e` of `train.py --eval_ss`.
//
// The reference (protein_transformer) has no counterpart.  Both structures get a three-state string (H / E / C) by the method of
// Kabsch & Sander, Biopolymers 22:2577-2637 (1983) - backbone hydrogen bonds from an electrostatic energy, then turns, helices
// and bridges from the pattern of the bonds - and the agreement of the two strings is Q3.  The definition, with what is
// simplified against the DSSP program, is in include/ptamd.h; this file restates only what the kernels do with it.
//
// Four launches per batch:
//   records   one workgroup per protein: presence of every residue (decided by the TRUTH alone, one mask for both structures),
//             the amide hydrogens, and the backbone records of both structures - O, C, N, H and two flags in 64 bytes, indexed by
//             residue, absent residues zeroed so that nothing a caller left in an absent slot reaches the sweep; the presence
//             mask as one ballot word per 64 residues; per protein the number of present residues and whether a present residue
//             has a non-finite prediction.
//   bonds     the O(L^2) sweep, one wavefront per 64 x 64 (acceptor x donor) tile.  A lane OWNS A DONOR (N and H in registers);
//             the 64 acceptors (O and C) are staged in the wavefront's own LDS slice and read as broadcasts; per pair 4 squared
//             distances, 4 v_rsq_f32, one comparison, and the 64 answers of an acceptor are ONE `__ballot` word - the tile's piece
//             of row i of the bit matrix - that lane i keeps and stores with a plain vector store after the loop.
//   patterns  one wavefront per 64 residues, both structures in turn: the turn tests read single bits of rows i-n .. i, the
//             bridge tests whole words of rows i-1 and i and, for hb(j, i) and hb(j, i+1), the TRANSPOSE of the 64 x 64 bit block
//             (rows j, columns of this wavefront's residues), which is 64 ballots - and none at all for a block without a bond.
//             No energy is computed again.  States of both structures, and the wavefront's share of the 3 x 3 confusion counts
//             as popcounts of ballots.
//   finalize  one wavefront per protein adds the shares and writes counts and scores.
// Integers throughout, no atomics: two runs give the same bits, and a protein's result depends on nothing but its own residues.
#include <math.h>

#include "atom_tiles.h"

namespace {

using atom_tiles::take;

constexpr int TS = 64;               // residues per tile = lanes of a wavefront = bits of a word
constexpr int SLOT_N = 0, SLOT_C = 2, SLOT_O = 3;   // (slot 1 is the C-alpha; N, CA, C, O decide presence)
constexpr int REC_THREADS = 256, SWEEP_WAVES = 4;
constexpr int ST_H = 0, ST_E = 1, ST_C = 2;
constexpr float Q_KCAL = 27.888f;    // 332 * 0.42 * 0.20 kcal/mol A
constexpr float E_BOND = -0.5f;
constexpr float R2_MIN = 0.25f;      // a distance below 0.5 A is taken as 0.5 A

constexpr int F_PRESENT = 1, F_HAS_H = 2;
struct __attribute__((aligned(16))) BbRecord {   // 64 bytes: four 16-byte loads
  float ox, oy, oz;
  int flags;
  float cx, cy, cz, pad0;
  float nx, ny, nz, pad1;
  float hx, hy, hz, pad2;
};

struct SsLayout {
  size_t rec, pres, hdr, part, bits, end;
  int words;      // 64-bit words per row of bits = tiles per protein
  size_t lp;      // record slots per (protein, structure): whole tiles
  SsLayout(int B, int L) {
    words = (L + TS - 1) / TS;
    lp = (size_t)words * TS;
    end = 0;
    rec = take(end, (size_t)B * 2 * lp * sizeof(BbRecord));
    pres = take(end, (size_t)B * words * sizeof(unsigned long long));
    hdr = take(end, (size_t)B * sizeof(int2));
    part = take(end, (size_t)B * words * 9 * sizeof(int));
    bits = take(end, (size_t)B * 2 * L * words * sizeof(unsigned long long));
  }
};

// ---- stage (a)
__global__ __launch_bounds__(REC_THREADS) void ss_records_kernel(const float *__restrict__ pred, const float *__restrict__ truth,
                                                                 const int64_t *__restrict__ seq, int L, int words, size_t lp,
                                                                 BbRecord *__restrict__ rec, unsigned long long *__restrict__ pres,
                                                                 int2 *__restrict__ hdr) {
  constexpr int NWAVE = REC_THREADS / 64;
  __shared__ int s_n[NWAVE], s_bad[NWAVE];
  const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const size_t nslot = (size_t)L * PTAMD_NUM_SLOTS;
  pred += (size_t)b * nslot * 3;
  truth += (size_t)b * nslot * 3;
  seq += (size_t)b * L;
  BbRecord *rec_p = rec + (size_t)b * 2 * lp, *rec_t = rec_p + lp;
  pres += (size_t)b * words;
  // four backbone atoms of residue r, 12 consecutive floats; true: the residue is present
  auto present = [&](int r) __attribute__((always_inline)) {
    if (r < 0 || r >= L || seq[r] == PTAMD_PAD_ID) return false;   // batch padding carries zeros, not NaN
    const float *t = truth + (size_t)r * PTAMD_NUM_SLOTS * 3;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 12; ++k) nan = nan || isnan(t[k]);
    return !nan;
  };
  int n = 0;   // (wavefront-uniform)
  bool bad = false;
  for (int t = w; t < words; t += NWAVE) {
    const int r = t * TS + lane;
    const bool ok = present(r);
    const unsigned long long m = __ballot(ok);
    // the residue in front: a neighbour lane, or, for lane 0, the last residue of the tile in front
    const bool prev = lane > 0 ? ((m >> (lane - 1)) & 1ull) != 0ull : present(r - 1);
    BbRecord rp = {0.f, 0.f, 0.f, 0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rt = rp;
    if (ok) {
      const bool has_h = prev;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float *x = (s == 0 ? pred : truth) + (size_t)r * PTAMD_NUM_SLOTS * 3;
        BbRecord &o = s == 0 ? rp : rt;
        o.flags = F_PRESENT | (has_h ? F_HAS_H : 0);
        o.nx = x[SLOT_N * 3]; o.ny = x[SLOT_N * 3 + 1]; o.nz = x[SLOT_N * 3 + 2];
        o.cx = x[SLOT_C * 3]; o.cy = x[SLOT_C * 3 + 1]; o.cz = x[SLOT_C * 3 + 2];
        o.ox = x[SLOT_O * 3]; o.oy = x[SLOT_O * 3 + 1]; o.oz = x[SLOT_O * 3 + 2];
        if (s == 0) {   // what the prediction holds never decides presence; it decides whether the protein has scores
#pragma unroll
          for (int k = 0; k < 12; ++k) bad = bad || !isfinite(x[k]);
        }
        if (has_h) {   // H = N + unit(C' - O') of the residue in front
          const float *y = x - PTAMD_NUM_SLOTS * 3;
          const float ux = y[SLOT_C * 3] - y[SLOT_O * 3], uy = y[SLOT_C * 3 + 1] - y[SLOT_O * 3 + 1],
                      uz = y[SLOT_C * 3 + 2] - y[SLOT_O * 3 + 2];
          const float inv = 1.0f / sqrtf(fmaf(uz, uz, fmaf(uy, uy, ux * ux)));
          o.hx = fmaf(ux, inv, o.nx); o.hy = fmaf(uy, inv, o.ny); o.hz = fmaf(uz, inv, o.nz);
        }
      }
    }
    rec_p[r] = rp;   // (r < lp: every slot of the tile is written, the absent ones with zeros)
    rec_t[r] = rt;
    if (lane == 0) pres[t] = m;
    n += __popcll(m);
  }
  const bool any_bad = __ballot(bad) != 0ull;
  if (lane == 0) {
    s_n[w] = n;
    s_bad[w] = any_bad ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tn = 0, tb = 0;
#pragma unroll
    for (int k = 0; k < NWAVE; ++k) {
      tn += s_n[k];
      tb |= s_bad[k];
    }
    hdr[b] = make_int2(tn, tb);
  }
}

// ---- stage (b)
__device__ __forceinline__ float inv_dist(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return __builtin_amdgcn_rsqf(fmaxf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)), R2_MIN));
}

__global__ __launch_bounds__(64 * SWEEP_WAVES) void ss_bonds_kernel(const BbRecord *__restrict__ rec, int L, int words, size_t lp,
                                                                    unsigned long long ntiles,
                                                                    unsigned long long *__restrict__ bits) {
  __shared__ float4 s_acc[SWEEP_WAVES][2][TS];   // per wavefront: (O, flags) and (C, -) of the 64 acceptors
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned long long nwave = (unsigned long long)gridDim.x * SWEEP_WAVES;
  // tile t = ((protein * 2 + structure) * words + acceptor tile) * words + donor tile; wavefront-uniform control flow, no barrier
  for (unsigned long long t = (unsigned long long)blockIdx.x * SWEEP_WAVES + w; t < ntiles; t += nwave) {
    const int tj = (int)(t % words), ti = (int)((t / words) % words);
    const size_t bs = (size_t)(t / words / words);
    const BbRecord *r = rec + bs * lp;
    const float4 *ra = reinterpret_cast<const float4 *>(r + (size_t)ti * TS + lane);
    s_acc[w][0][lane] = ra[0];
    s_acc[w][1][lane] = ra[1];
    const int j = tj * TS + lane;
    const float4 *rd = reinterpret_cast<const float4 *>(r + j);
    const float4 dn = rd[2], dh = rd[3];
    const bool donor = (__float_as_int(rd[0].w) & F_HAS_H) != 0;   // present, and so is the residue in front
    __builtin_amdgcn_wave_barrier();   // (the wavefront's own slice: its LDS operations execute in order)
    unsigned long long mine = 0ull;
#pragma unroll 4
    for (int ii = 0; ii < TS; ++ii) {
      const float4 o = s_acc[w][0][ii], c = s_acc[w][1][ii];   // broadcasts
      const int i = ti * TS + ii;
      const bool pair = donor && (__float_as_int(o.w) & F_PRESENT) != 0 && (j - i >= 2 || i - j >= 2);
      const float e = Q_KCAL * (inv_dist(o.x, o.y, o.z, dn.x, dn.y, dn.z) + inv_dist(c.x, c.y, c.z, dh.x, dh.y, dh.z) -
                                inv_dist(o.x, o.y, o.z, dh.x, dh.y, dh.z) - inv_dist(c.x, c.y, c.z, dn.x, dn.y, dn.z));
      const unsigned long long row = __ballot(pair && e < E_BOND);   // (a NaN energy is no bond)
      if (lane == ii) mine = row;
    }
    const int i = ti * TS + lane;
    if (i < L) bits[(bs * L + i) * words + tj] = mine;
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- stage (c)
// bits lo .. hi (0 <= hi - lo < 64) of the presence mask all set?  Residues outside 0 .. L-1 are absent.
__device__ __forceinline__ bool all_present(const unsigned long long *__restrict__ pres, int L, int lo, int hi) {
  if (lo < 0 || hi >= L) return false;
  const int w0 = lo >> 6, s = lo & 63, n = hi - lo + 1;
  unsigned long long x = pres[w0] >> s;
  if (s != 0 && (hi >> 6) != w0) x |= pres[w0 + 1] << (64 - s);
  const unsigned long long need = n == 64 ? ~0ull : (1ull << n) - 1ull;
  return (x & need) == need;
}
__device__ __forceinline__ bool bond(const unsigned long long *__restrict__ rows, int words, int i, int j) {
  return ((rows[(size_t)i * words + (j >> 6)] >> (j & 63)) & 1ull) != 0ull;
}
// bit j of the result = bit j + 1 (shr1) / bit j - 1 (shl1) of a row of which `cur` is a word and next / prev its neighbours
__device__ __forceinline__ unsigned long long shr1(unsigned long long cur, unsigned long long next) { return (cur >> 1) | (next << 63); }
__device__ __forceinline__ unsigned long long shl1(unsigned long long cur, unsigned long long prev) { return (cur << 1) | (prev >> 63); }

__global__ __launch_bounds__(64) void ss_patterns_kernel(const unsigned long long *__restrict__ bits,
                                                         const unsigned long long *__restrict__ pres_all,
                                                         const int2 *__restrict__ hdr, int L, int words, unsigned long long ntiles,
                                                         int8_t *__restrict__ states, int *__restrict__ part) {
  const int lane = threadIdx.x;
  for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int ti = (int)(t % words);
    const size_t b = (size_t)(t / words);
    const unsigned long long *pres = pres_all + b * words;
    const bool bad = hdr[b].y != 0;
    const int i = ti * TS + lane;
    const bool here = ((pres[ti] >> lane) & 1ull) != 0ull;
    const bool ok3 = all_present(pres, L, i - 1, i + 1);   // i can be a bridge partner
    int state[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned long long *rows = bits + (b * 2 + s) * (size_t)L * words;
      // helices: n-turns at k = i-n .. i; two consecutive ones at k-1, k cover k .. k+n-1
      bool helix[3];
#pragma unroll
      for (int n = 3; n <= 5; ++n) {
        bool in = false, before = false;
        for (int k = i - n; k <= i; ++k) {
          const bool turn = here && all_present(pres, L, k, k + n) && bond(rows, words, k, k + n);
          in = in || (before && turn && k > i - n);
          before = turn;
        }
        helix[n - 3] = in;
      }
      // bridges: every partner j of word wj at once
      unsigned long long found = 0ull;
      unsigned long long ri = 0ull, rm = 0ull, ti_prev = 0ull, tp_prev = 0ull;   // rows i and i-1; columns i and i+1
      if (ok3) {
        ri = rows[(size_t)i * words];
        rm = rows[(size_t)(i - 1) * words];
      }
      for (int wj = 0; wj < words; ++wj) {
        unsigned long long ri_next = 0ull, rm_next = 0ull;
        if (ok3 && wj + 1 < words) {
          ri_next = rows[(size_t)i * words + wj + 1];
          rm_next = rows[(size_t)(i - 1) * words + wj + 1];
        }
        // the transpose: lane l reads row j = 64 wj + l at the word of this tile's columns, lane k takes bit k of all of them
        const int j = wj * TS + lane;
        const unsigned long long x = j < L ? rows[(size_t)j * words + ti] : 0ull;
        const bool y = j < L && ti + 1 < words && (rows[(size_t)j * words + ti + 1] & 1ull) != 0ull;   // column 64 (ti + 1)
        unsigned long long t_i = 0ull;
        if (__ballot(x != 0ull) != 0ull) {
          for (int k = 0; k < TS; ++k) {
            const unsigned long long col = __ballot(((x >> k) & 1ull) != 0ull);
            if (lane == k) t_i = col;
          }
        }
        const unsigned long long last = __ballot(y);
        const unsigned long long down = __shfl_down(t_i, 1, 64);
        const unsigned long long t_p = lane == TS - 1 ? last : down;
        // partners that can be one: j-1 .. j+1 present, |i - j| >= 3
        const unsigned long long pw = pres[wj], pw_prev = wj > 0 ? pres[wj - 1] : 0ull, pw_next = wj + 1 < words ? pres[wj + 1] : 0ull;
        unsigned long long can = pw & shl1(pw, pw_prev) & shr1(pw, pw_next);
        const long long lo = (long long)i - 2 - (long long)wj * TS, hi = lo + 4;
        if (hi >= 0 && lo <= 63) {
          const int l0 = (int)(lo < 0 ? 0 : lo), h0 = (int)(hi > 63 ? 63 : hi);
          can &= ~(((1ull << (h0 - l0 + 1)) - 1ull) << l0);   // (at most 5 bits)
        }
        const unsigned long long par = (rm & t_p) | (shl1(t_i, ti_prev) & shr1(ri, ri_next));
        const unsigned long long anti = (ri & t_i) | (shr1(rm, rm_next) & shl1(t_p, tp_prev));
        found |= (par | anti) & can;
        ri = ri_next; rm = rm_next; ti_prev = t_i; tp_prev = t_p;
      }
      const bool strand = ok3 && found != 0ull;
      state[s] = !here ? -1 : helix[1] ? ST_H : strand ? ST_E : (helix[0] || helix[2]) ? ST_H : ST_C;
    }
    if (bad) state[0] = -1;   // a present residue of this protein has a non-finite prediction: no predicted string
    if (states && i < L) {
      int8_t *out = states + (b * L + i) * 2;
      out[0] = (int8_t)state[0];
      out[1] = (int8_t)state[1];
    }
    int cnt = 0;   // lane k < 9 keeps count [k / 3][k % 3]: true state x predicted state
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int c = __popcll(__ballot(here && !bad && state[1] == k / 3 && state[0] == k % 3));
      if (lane == k) cnt = c;
    }
    if (lane < 9) part[t * 9 + lane] = cnt;
  }
}

// ---- stage (d)
__global__ __launch_bounds__(64) void ss_finalize_kernel(const int2 *__restrict__ hdr, const int *__restrict__ part, int words,
                                                         float *__restrict__ score, int32_t *__restrict__ confusion) {
  const int b = blockIdx.x, lane = threadIdx.x;
  part += (size_t)b * words * 9;
  int c[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) c[k] = 0;
  for (int t = lane; t < words; t += 64) {
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] += part[(size_t)t * 9 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
  }
  if (lane == 0) {
    const float nan = __builtin_nanf("");
    const bool bad = hdr[b].y != 0;
    const int n = hdr[b].x;   // present residues = the sum of the nine counts, unless bad
    const int same = c[0] + c[4] + c[8], th = c[0] + c[1] + c[2], te = c[3] + c[4] + c[5];
    score[(size_t)b * 3] = bad || n == 0 ? nan : (float)((double)same / (double)n);
    score[(size_t)b * 3 + 1] = bad || th == 0 ? nan : (float)((double)c[0] / (double)th);
    score[(size_t)b * 3 + 2] = bad || te == 0 ? nan : (float)((double)c[4] / (double)te);
#pragma unroll
    for (int k = 0; k < 9; ++k) confusion[(size_t)b * 9 + k] = c[k];
  }
}

inline unsigned grid_for(unsigned long long items) {
  return (unsigned)(items < 0x7fffffffull ? items : 0x7fffffffull);   // the kernels stride over what a grid cannot hold
}

}  // namespace

extern "C" {

size_t ptamd_ss_workspace_bytes(int B, int L) {
  if (!atom_tiles::tile_shape_ok(B, L)) return 0;
  return SsLayout(B, L).end;
}

int ptamd_ss(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float *score, int32_t *confusion,
             int8_t *states, uint64_t *hbonds, void *workspace, size_t workspace_bytes, void *stream) {
  if (!atom_tiles::tile_shape_ok(B, L)) return PTAMD_ERR_BAD_SHAPE;
  if (!pred_crd || !true_crd || !seq || !score || !confusion) return PTAMD_ERR_BAD_SHAPE;
  const SsLayout l(B, L);
  if (!workspace || workspace_bytes < l.end) return PTAMD_ERR_WORKSPACE;
  if (!pt_aligned16(workspace)) return PTAMD_ERR_ALIGN;
  char *ws = static_cast<char *>(workspace);
  BbRecord *rec = reinterpret_cast<BbRecord *>(ws + l.rec);
  unsigned long long *pres = reinterpret_cast<unsigned long long *>(ws + l.pres);
  int2 *hdr = reinterpret_cast<int2 *>(ws + l.hdr);
  int *part = reinterpret_cast<int *>(ws + l.part);
  unsigned long long *bits = hbonds ? reinterpret_cast<unsigned long long *>(hbonds) : reinterpret_cast<unsigned long long *>(ws + l.bits);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ss_records_kernel, dim3(B), dim3(REC_THREADS), 0, st, pred_crd, true_crd, seq, L, l.words, l.lp, rec, pres, hdr);
  int rc = pt_check_launch();
  if (rc) return rc;
  const unsigned long long ntiles = (unsigned long long)B * 2 * l.words * l.words;
  hipLaunchKernelGGL(ss_bonds_kernel, dim3(grid_for((ntiles + SWEEP_WAVES - 1) / SWEEP_WAVES)), dim3(64 * SWEEP_WAVES), 0, st, rec, L,
                     l.words, l.lp, ntiles, bits);
  rc = pt_check_launch();
  if (rc) return rc;
  const unsigned long long nres_tiles = (unsigned long long)B * l.words;
  hipLaunchKernelGGL(ss_patterns_kernel, dim3(grid_for(nres_tiles)), dim3(64), 0, st, bits, pres, hdr, L, l.words, nres_tiles, states,
                     part);
  rc = pt_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ss_finalize_kernel, dim3(B), dim3(64), 0, st, hdr, part, l.words, score, confusion);
  return pt_check_launch();
}

}  // extern "C"
