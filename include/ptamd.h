/*
 * ptamd.h - C ABI of libptamd.so: the MI355X (gfx950) implementation of the
 * protein-transformer training hot path.
 *
 * The upstream reference has no FFI/plugin layer: its hot path sits behind plain
 * Python call signatures.  Each entry point below names the
 * reference function(s) whose arithmetic it replaces (paths relative to
 * /root/reference/protein_transformer/), and `protein_transformer_amd/` keeps
 * those Python signatures on top of this ABI via ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host;
 *   - row-major, innermost dimension contiguous, fp32 unless stated otherwise;
 *   - no allocation inside the library: the caller owns outputs and workspaces
 *     (query sizes with the *_workspace_bytes functions);
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing
 *     synchronises;
 *   - return value: PTAMD_OK or a negative PTAMD_ERR_* code for host-detectable
 *     problems; device-detected anomalies are OR-ed into a caller-provided
 *     int32 status word (PTAMD_ST_* bits) and never trap.
 *
 * Shapes: B proteins, L padded residues, 12 angles / 14 atom slots per residue,
 * T = B*L tokens, D model width, F feed-forward width, H heads, dk = D/H.
 */
#ifndef PTAMD_H
#define PTAMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTAMD_OK 0
#define PTAMD_ERR_BAD_SHAPE (-1)  /* non-positive or unsupported size                      */
#define PTAMD_ERR_TOO_LONG (-2)   /* L exceeds what the kernel's LDS staging supports      */
#define PTAMD_ERR_WORKSPACE (-3)  /* workspace pointer NULL or too small                   */
#define PTAMD_ERR_HIP (-4)        /* a HIP runtime call failed (see ptamd_last_hip_error)  */
#define PTAMD_ERR_ALIGN (-5)      /* pointer / leading dimension not 16-byte aligned       */

/* device status bits (int32 word, OR-ed by kernels) */
#define PTAMD_ST_BAD_RESIDUE 1 /* id outside 0..19 before the padding (Sequence.py:50-51 KeyError)   */
#define PTAMD_ST_TOO_SHORT 2   /* fewer than 2 residues (StructureBuilder.py:58-59 StopIteration)    */
#define PTAMD_ST_BAD_THETA 4   /* bond angle outside [-pi, pi] (Structure.py:42 AssertionError)      */
#define PTAMD_ST_NONFINITE 8   /* NaN/inf loss (log.py:182-185 exits the process)                    */

#define PTAMD_PAD_ID 20
#define PTAMD_NUM_ANGLES 12
#define PTAMD_NUM_SLOTS 14

const char *ptamd_version(void);
const char *ptamd_last_hip_error(void);
/* number of side-chain atoms of residue type r (0..19); -1 if r is out of range */
int ptamd_sidechain_atoms(int residue);

/* ------------------------------------------------------------------ angles
 * inverse_trig_transform (losses.py:26-36): sincos[n,2] = (cos, sin) -> ang[n] = atan2(sin, cos). */
int ptamd_angles_fwd(const float *sincos, float *ang, int64_t n, void *stream);
/* d(ang)/d(cos, sin): dsincos[n,2] = dang[n] * (-sin, cos) / (cos^2 + sin^2)   */
int ptamd_angles_bwd(const float *sincos, const float *dang, float *dsincos, int64_t n, void *stream);

/* ------------------------------------------------------------------ NeRF
 * generate_coords / StructureBuilder.build / ResidueBuilder.build_bb,build_sc / nerf
 * (protein/Structure.py:12-65, protein/StructureBuilder.py:55-92,147-236).
 *   ang [B,L,12] radians; seq [B,L] int64 residue ids with trailing PTAMD_PAD_ID;
 *   crd [B,L*14,3] out (unused slots and padded residues = 0); status: int32[1], OR-ed. */
size_t ptamd_nerf_workspace_bytes(int B, int L);
/* nerf (protein/Structure.py:23-65), n independent placements: a, b, c, d [n,3]; l, theta, chi [n] */
int ptamd_nerf_place(const float *a, const float *b, const float *c, const float *l, const float *theta,
                     const float *chi, int64_t n, float *d, int32_t *status, void *stream);
/* pairwise_internal_dist (losses.py:233-253): x [n,dim] -> out [n,n] = sqrt(max(|x_i - x_j|^2, 1e-30)); the
 * training path never materialises this matrix (ptamd_drmsd_fwd_bwd), it exists for API parity */
int ptamd_pairwise_dist(const float *x, int n, int dim, float *out, void *stream);
int ptamd_nerf_fwd(const float *ang, const int64_t *seq, int B, int L, float *crd, int32_t *status,
                   void *stream);
/* adjoint of the build: dcrd [B,L*14,3] -> dang [B,L,12] (overwritten). Reproduces the
 * reference's graph: first residue's C is detached (StructureBuilder.py:185-187). */
int ptamd_nerf_bwd(const float *ang, const int64_t *seq, const float *crd, const float *dcrd, int B, int L,
                   float *dang, void *workspace, size_t workspace_bytes, void *stream);
/* The backbone alone, for the backbone-only loss (losses.py:83-92 with backbone_only = True, i.e. train.py --backbone_loss;
 * get_backbone_from_full_coords, structure_utils.py:19-32): the chain of ResidueBuilder.build_bb (StructureBuilder.py:147-191)
 * WITHOUT the O and side-chain placements of build_sc.
 *   crd_bb [B,L*3,3] out: N, CA, C of every residue, COMPACT (3 atoms per residue, not the 14-slot layout; padded residues and
 *   proteins of fewer than two residues = 0) - bit for bit slots 0..2 of what ptamd_nerf_fwd writes (same one-wavefront scan,
 *   same composition order); status as for ptamd_nerf_fwd.  One launch. */
int ptamd_nerf_bb_fwd(const float *ang, const int64_t *seq, int B, int L, float *crd_bb, int32_t *status, void *stream);
/* its adjoint: dcrd_bb [B,L*3,3] -> dang [B,L,12], ALL 12 channels written (exact zeros where nothing flows: the six side-chain
 * torsions, padded residues, and what the reference's graph leaves out - first residue's C detached, StructureBuilder.py:185-187,
 * the last residue's psi / omega / CA-C-N / C-N-CA); no workspace, no fill in front.  One launch. */
int ptamd_nerf_bb_bwd(const float *ang, const int64_t *seq, const float *crd_bb, const float *dcrd_bb, int B, int L,
                      float *dang, void *stream);

/* ------------------------------------------------------------------ dRMSD
 * drmsd_work's loss part for a whole batch (losses.py:63-92,233-278; structure_utils.py:19-32).
 *   pred_crd, true_crd [B,L*14,3]; NaN in true_crd = atom absent.
 *   stats [B,8] out: {drmsd, drmsd/n, bb_drmsd, bb_drmsd/n_bb, n, n_bb, 0, 0}
 *   dcrd [B,L*14,3] out or NULL: d(drmsd/n)/d(pred_crd)  (the reference always
 *   differentiates the length-normalised loss, losses.py:80,91-92).  A protein with fewer than two present atoms has no pair:
 *   its dcrd is all zeros and its drmsd, drmsd/n are NaN (the mean over an empty set, as in the reference); likewise the two
 *   backbone statistics with fewer than two present backbone atoms.  The other proteins of the batch are not affected.
 * Workspace: 52 B per atom slot (compacted copies: predicted coordinates, (predicted, true) interleaved per axis, index) plus
 * the fixed-order partial sums of the upper-triangle sweep - one 1 KB column partial per (4-row-tile strip, 64-atom column
 * tile) and one 4 KB row partial per (strip, chunk of 8 column tiles): O(n^2 / 256) per protein (n = 14 L atom slots) -
 * CAPPED at 200 MB: beyond that the strips are swept in passes over groups of strips with the same buffers (+ 32 B per atom slot
 * of running sums), same bits as one launch.  B = 32: 159 MB at L = 512, 242 MB at L = 1500 (1.39 GB in round 4).  The size is
 * a function of (B, L) only - nothing is read from the process environment.  The *_budget forms take the cap on the partial
 * sums as an argument (bytes; 0 = the built-in 200 MB): for callers short of memory and for the test that forces passes on a
 * small batch; the same budget must be given to both calls. */
size_t ptamd_drmsd_workspace_bytes(int B, int L);
int ptamd_drmsd_fwd_bwd(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L,
                        float *stats, float *dcrd, void *workspace, size_t workspace_bytes, void *stream);
size_t ptamd_drmsd_workspace_bytes_budget(int B, int L, size_t partial_budget_bytes);
int ptamd_drmsd_fwd_bwd_budget(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L,
                               float *stats, float *dcrd, void *workspace, size_t workspace_bytes,
                               size_t partial_budget_bytes, void *stream);
/* The backbone-only loss (losses.py:83-92: drmsd over get_backbone_from_full_coords of both structures, structure_utils.py:19-32,
 * and the gradient of its length-normalised form): the same compaction, upper-triangle sweep and finalisation over the present
 * N, CA, C alone.
 *   pred_bb [B,L*3,3]: the COMPACT backbone of ptamd_nerf_bb_fwd (predicted coordinates travel between the two kernels in this
 *   layout: there are no side-chain slots to leave unwritten); true_crd [B,L*14,3] as above - only its slots s % 14 < 3 are read,
 *   NaN = atom absent.
 *   stats [B,8] out, same layout: entries 2, 3, 5 = {bb_drmsd, bb_drmsd/n_bb, n_bb} - what ptamd_drmsd_fwd_bwd reports there -
 *   and entries 0, 1, 4 MIRROR them.
 *   dbb [B,L*3,3] out or NULL: d(bb_drmsd/n_bb)/d(pred_bb); a protein with fewer than two present backbone atoms gets zeros
 *   (its statistics are NaN, the mean over an empty pair set, as in the reference).
 * Workspace, tiles, strips, work items, partial sums and passes are those of the full sweep cut for n = 3 L atoms per protein
 * instead of 14 L (B = 32, L = 512: 11.5 MiB against 158.6 MiB = 12.0e6 against 166.3e6 bytes); fixed-order partials, no atomics, passes give the bits of one launch. */
size_t ptamd_drmsd_bb_workspace_bytes(int B, int L);
int ptamd_drmsd_bb_fwd_bwd(const float *pred_bb, const float *true_crd, const int64_t *seq, int B, int L,
                           float *stats, float *dbb, void *workspace, size_t workspace_bytes, void *stream);
size_t ptamd_drmsd_bb_workspace_bytes_budget(int B, int L, size_t partial_budget_bytes);
int ptamd_drmsd_bb_fwd_bwd_budget(const float *pred_bb, const float *true_crd, const int64_t *seq, int B, int L,
                                  float *stats, float *dbb, void *workspace, size_t workspace_bytes,
                                  size_t partial_budget_bytes, void *stream);

/* rmsd (losses.py:281-286, ProDy calcTransformation + calcRMSD) for a whole batch: RMSD of the predicted atoms after optimal
 * rigid superposition (Kabsch) onto the true ones, over the atoms whose truth is present (NaN = absent), residues with
 * PTAMD_PAD_ID skipped.  rmsd [B] out (NaN for a protein without atoms).  One workgroup per protein, fp64 moments.
 * A NaN or infinite coordinate on a present atom gives that protein NaN (never 0); finite ones of any size (1e30) are used as
 * they are; what absent slots and padded residues hold is never read into the result. */
int ptamd_kabsch_rmsd(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float *rmsd,
                      void *stream);

/* The superposed RMSD as a training loss, forward + analytic backward, for a whole batch (csrc/kabsch_loss.hip): `-l kabsch`.
 * It stands beside rmsd (losses.py:281-286), which the reference - and ptamd_kabsch_rmsd above - only evaluate: the metric models
 * are selected by, made trainable.  Like ptamd_fape_fwd_bwd and unlike every distance-based loss here it tells a structure from
 * its mirror image: the superposition is over PROPER rotations, so a mirrored prediction has dRMSD 0 and a large loss here.
 *   Atoms.  The present atoms of protein i are the slots of non-pad residues whose true coordinate has no NaN, as in
 *   ptamd_kabsch_rmsd; what the prediction holds never decides presence.  Let their predicted coordinates be a_1..a_n, their true
 *   ones b_1..b_n, abar and bbar the means, and R the proper rotation (det = +1) that minimises sum |R (a_k - abar) - (b_k - bbar)|^2.
 *   Loss.  With the residual r_k = R (a_k - abar) - (b_k - bbar):  loss_i = sqrt(sum |r_k|^2 / n).
 *   Gradient.  d(loss_i)/d(a_k) = R^T r_k / (n loss_i).  R is optimal, so it contributes no term; sum r_k = 0, so the centring
 *   contributes none.  Every other slot - absent atoms, pad residues, slots beyond the sequence - gets exactly zero.
 *   Edges.  loss_i = 0: every residual is 0, the gradient is exactly zero and nothing is divided; a prediction whose present atoms
 *   equal the truth bit for bit gets R = 1 exactly, loss_i = 0 and an all-zero gradient.  n < 3: loss_i = NaN and a zero gradient
 *   (the rotation is not determined).  A NaN or infinite predicted coordinate on a present atom: loss_i = NaN and a zero gradient
 *   for that whole protein (the rule of ptamd_fape_fwd_bwd, found by ptamd_kabsch_rmsd's test on the sums of squares); finite
 *   coordinates of any size are used as they are; the other proteins of the batch are untouched.  Where the two largest
 *   eigenvalues of Horn's 4x4 matrix coincide (for instance n collinear atoms) R is not unique and the loss is not differentiable:
 *   a set of measure zero, on which the call returns the loss - it is the same for every minimiser - and R^T r_k / (n loss_i) under
 *   ONE of the minimisers: finite, zero outside the present atoms, summing to zero over the atoms and of squared norm 1 / n, as
 *   under any rotation.  Which minimiser: eigenvalues within Jacobi's rounding of each other (64 eps of the diagonal) count as
 *   equal and the first column of them is taken (csrc/tm_rotation.h), so the bits are reproducible, and a collinear prediction
 *   that equals its truth gets R = 1 like any other, not the half turn about the line that ties with it.
 *   Batch.  The reported batch value is the mean over the proteins with a finite loss; the back-propagated quantity is the SUM
 *   over proteins of loss_i, as for every structural loss here.
 *   stats [B,2] out = {loss_i, n_i}; dcrd [B,L*14,3] out, or NULL for the forward-only form (no gradient work; the same bits in
 *   stats).
 * One workgroup per protein, one launch, no workspace: moments in fp64 relative to the protein's first present atom pair (a
 * structure 1e3 A from the origin loses nothing to cancellation), Horn's closed-form rotation (csrc/tm_rotation.h), the loss from
 * the residuals themselves under that R (not from a trace formula), results rounded to fp32 once.  No atomics and fixed-order
 * sums: two runs give the same bits, and a protein's result does not depend on the batch around it.  B or L <= 0, L beyond
 * INT_MAX / 28 (the bound of ptamd_lddt), or a NULL crd, true_crd, seq or stats: PTAMD_ERR_BAD_SHAPE, nothing is launched or
 * written.  No getenv, no state between calls. */
int ptamd_kabsch_loss_fwd_bwd(const float *crd, const float *true_crd, const int64_t *seq, int B, int L,
                              float *stats /* [B,2] = {loss_i, n_i} */, float *dcrd /* [B,L*14,3] or NULL */, void *stream);

/* lDDT, all-atom and C-alpha, for a whole batch (csrc/lddt.hip).  The reference has no counterpart - its evaluation stops at
 * dRMSD and the superposed RMSD; this is the score of Mariani, Biasini, Barbato & Schwede, "lDDT: a local superposition-free
 * score for comparing protein structures and models using distance difference tests", Bioinformatics 29(21):2722-2728 (2013),
 * without the stereochemistry checks of the full tool.
 *   pred_crd, true_crd [B,L*14,3], seq [B,L]: as for ptamd_kabsch_rmsd - the atoms of a protein are the slots s of residues
 *   other than PTAMD_PAD_ID whose true coordinate has no NaN; an atom's residue is s / 14.
 *   An ordered pair (i, j) of atoms in DIFFERENT residues is included if its true distance dt < cutoff (the usual cutoff is
 *   15 A) and preserved at t in {0.5, 1, 2, 4} A if |dp - dt| < t, dp the predicted distance; both comparisons are strict, both
 *   distances are sqrt(dx^2 + dy^2 + dz^2) of coordinate differences in fp32.  A non-finite predicted coordinate fails the
 *   comparisons, nothing traps.
 *   counts [B,L,2,5] out: per residue r and atom set (0: every atom; 1: C-alpha = slot 1, paired with C-alphas only)
 *   {total, p0.5, p1, p2, p4} over the included pairs whose i lies in r; zero-filled by the call itself, zeros for padded
 *   residues and residues without a present atom.
 *   per_res [B,L,2] out: (p0.5 + p1 + p2 + p4) / (4 total), NaN where total == 0.
 *   score [B,2] out: the same ratio of the 64-bit sums over the protein's residues, NaN without an included pair.
 * Integer counters and integer atomics only: the same bits whatever the scheduling, and a protein's counts do not depend on
 * the batch around it.  Workspace: 32 B per atom slot (the present atoms compacted in slot order) + 32 B per tile of 64 of them
 * (bounding boxes) - a function of (B, L) only.  cutoff not finite and positive, a NULL array, B or L <= 0 (or L beyond
 * INT_MAX / 28): PTAMD_ERR_BAD_SHAPE; workspace NULL or too small: PTAMD_ERR_WORKSPACE; nothing is launched or written then.
 * No length limit otherwise, no state between calls, nothing read from the environment. */
size_t ptamd_lddt_workspace_bytes(int B, int L);
int ptamd_lddt(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float cutoff,
               int32_t *counts, float *per_res, float *score, void *workspace, size_t workspace_bytes, void *stream);

/* TM-score and GDT_TS / GDT_HA over the C-alphas, for a whole batch (csrc/tmscore.hip): the metrics of `train.py --eval_tm`.
 * The reference has no counterpart.  These are the scores CASP predictions are ranked by: Zhang & Skolnick, "Scoring function
 * for automated assessment of protein structure template quality", Proteins 57:702-710 (2004), and the GDT counts of the same
 * superposition search, as in the public TMscore program (zhanggroup.org/TM-score).  PARITY UNPINNED, like ptamd_kabsch_rmsd:
 * no TM-score binary is at hand, so what is pinned is this definition, restated in numpy fp64 by tests/tm_ref.py.
 *   Residues.  Per protein, the residues other than PTAMD_PAD_ID whose true C-alpha (slot 1 of the residue) has no NaN
 *   coordinate - the presence rule of ptamd_kabsch_rmsd - taken in sequence order and compacted to indices 0..N-1; all fragment
 *   arithmetic below is on compacted indices.  What the prediction holds never decides presence.  N < 3, or a non-finite
 *   predicted coordinate on a present C-alpha: the three scores are NaN, counts = {N,0,0,0,0,0}, the transform is NaN.
 *   Scales.  d0 = 1.24 (N - 15)^(1/3) - 1.8 for N > 21, floored at 0.5, and 0.5 for N <= 21; d_search = min(8, max(4.5, d0)).
 *   Scoring a superposition (R, t).  d_i = |R p_i + t - q_i|, p the prediction, q the truth; TM(R,t) = (1/N) sum_i
 *   1 / (1 + (d_i / d0)^2); c_k(R,t) = #{i : d_i <= k} for k in {0.5, 1, 2, 4, 8} A.
 *   Seeds.  Fragment lengths l in {N, N>>1, N>>2, N>>3, N>>4, 4}, each raised to at least 4 (lowered to N when N = 3),
 *   duplicates dropped; for each l every start s = 0..N-l is a seed; seeds are numbered in (l descending, s ascending) order.
 *   Per seed.  (1) Superpose the fragment by least squares (proper rotation, det = +1) and score all N residues.  (2) Select
 *   S = {i : d_i < d_search - 1}; while |S| < 3 raise that cutoff by 0.5 and reselect.  (3) Up to 20 times: superpose S and score
 *   all N residues; reselect with cutoff d_search + 1 under the same widening rule; stop when S is unchanged.  Every (R,t) scored
 *   in (1) and (3) is a VISITED superposition.
 *   Results.  tm = max of TM over the visited superpositions; each count c_k is maximised separately over them, as the TMscore
 *   program does; gdt_ts = (c1 + c2 + c4 + c8) / (4N), gdt_ha = (c0.5 + c1 + c2 + c4) / (4N); xform = the (R,t) of the
 *   lowest-numbered seed, and within it the earliest iteration, that reaches tm.
 *   score [B,3] out = {tm, gdt_ts, gdt_ha}; counts [B,6] out = {N, c0.5, c1, c2, c4, c8}; xform [B,12] out or NULL: R row-major,
 *   then t, so that R p + t lies on q.
 * Moments, rotations (Horn's quaternion matrix, cyclic Jacobi), distances and every threshold decision are fp64 on the fp32
 * inputs, thresholds being tested on squared distances; scores are rounded to fp32 once.  No atomics, no order-dependent
 * reduction: two runs give the same bits, and a protein's result does not depend on the batch around it.  A selection is kept as
 * one bit per residue in the registers of a wavefront, which bounds L at 4096.  Workspace: 24 B per residue + 32 B per possible
 * seed - a function of (B, L) only; B = 32, L = 512: 3.5e6 bytes.  A NULL array other than xform, B or L <= 0, or L > 4096:
 * PTAMD_ERR_BAD_SHAPE; workspace NULL or too small: PTAMD_ERR_WORKSPACE; nothing is launched or written then.  No state
 * between calls, nothing read from the environment. */
size_t ptamd_tm_workspace_bytes(int B, int L);
int ptamd_tm_score(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float *score, int32_t *counts,
                   float *xform, void *workspace, size_t workspace_bytes, void *stream);

/* Secondary-structure agreement, for a whole batch (csrc/dssp.hip): the metrics `ss-q3`, `ss-h`, `ss-e` of `train.py --eval_ss`.
 * The reference has no counterpart.  Both structures get a three-state string by the method of Kabsch & Sander, "Dictionary of
 * protein secondary structure: pattern recognition of hydrogen-bonded and geometrical features", Biopolymers 22:2577-2637 (1983)
 * - backbone hydrogen bonds from an electrostatic energy, turns, helices and bridges from the bond pattern - and the agreement
 * of the strings is Q3.  This is DSSP SIMPLIFIED: every bond under the energy threshold counts, where the DSSP program keeps
 * only the two strongest bonds per group; bends and turns are not states; isolated bridges (B) and ladders (E) are not told
 * apart; three states, not eight.  PARITY UNPINNED: what is pinned is this definition, restated in numpy fp64 by tests/ss_ref.py.
 * Inputs as for ptamd_lddt; the backbone slots of a residue are 0 N, 1 CA, 2 C, 3 O.
 *   Presence.  Residue r is PRESENT when seq[r] is not PTAMD_PAD_ID and none of its four TRUE backbone atoms has a NaN
 *   coordinate.  The same mask is applied to the prediction: a residue absent from the truth is absent from both structures, so
 *   both see the same chain breaks.  What the prediction holds never decides presence.  A non-finite predicted coordinate on a
 *   backbone atom of a present residue - the rule of ptamd_kabsch_rmsd - makes the three scores of that protein NaN, its
 *   confusion counts 0, its predicted states -1 and the bond bits of its prediction unspecified; its true states and bits, and
 *   every other protein, are what they would be.
 *   Amide hydrogen.  Residue j has an H when j-1 and j are present: H_j = N_j + (C_{j-1} - O_{j-1}) / |C_{j-1} - O_{j-1}|.
 *   H-bond hb(i,j), the C=O of i accepting from the N-H of j: i and j present, j has an H, |i - j| >= 2, and
 *   E = 27.888 (1/r(O_i,N_j) + 1/r(C_i,H_j) - 1/r(O_i,H_j) - 1/r(C_i,N_j)) kcal/mol < -0.5, strictly; a distance below 0.5 A is
 *   taken as 0.5 A.  EVERY bond under the threshold counts (the simplification above).
 *   Turns and helices.  n-turn at i, n = 3, 4, 5: hb(i, i+n) with i .. i+n all present.  Two consecutive n-turns at i-1 and i
 *   put the residues i .. i+n-1 in an n-helix.
 *   Bridges.  Partners i, j need |i - j| >= 3 with i-1 .. i+1 and j-1 .. j+1 all present.  Parallel: [hb(i-1,j) and hb(j,i+1)]
 *   or [hb(j-1,i) and hb(i,j+1)].  Antiparallel: [hb(i,j) and hb(j,i)] or [hb(i-1,j+1) and hb(j-1,i+1)].  A residue with any
 *   bridge partner is a strand residue.
 *   State of a present residue: H (0) in a 4-helix; else E (1) if a strand residue; else H in a 3-helix or a 5-helix; else
 *   C (2).  Absent and pad residues: -1.
 *   Scores per protein over its n present residues: q3 = the share with pred state == true state; h = the share of the true-H
 *   residues predicted H; e = the share of the true-E residues predicted E; each NaN when its denominator is 0.
 *   score [B,3] out = {q3, h, e}; confusion [B,3,3] out: confusion[t][p] = present residues of true state t and predicted
 *   state p (states in the order H, E, C); states [B,L,2] out or NULL = {pred, true} per residue; hbonds [B,2,L,ceil(L/64)] out
 *   or NULL: structure 0 the prediction, 1 the truth; bit (j & 63) of word j >> 6 of row i = hb(i,j).
 * Energies are fp32 on the fp32 inputs (H is rounded to fp32 once; v_rsq_f32 on the squared distances): a pair whose fp64 energy
 * lies within 2e-3 kcal/mol of -0.5 may be decided either way for coordinates within +-64 A (tests/ss_ref.py derives the
 * figure); outside that band the bits, and everything derived from them, are exact.  All results are integers or ratios of
 * integers rounded once; no atomics; two runs give the same bits, and a protein's result does not depend on the batch around
 * it or on how far its row is padded.  Workspace: 128 B per residue slot for the backbone records of both structures and
 * L^2 / 4 bytes per protein for the bond bits of both, used when hbonds is NULL - a function of (B, L) only; B = 32, L = 512:
 * 4.2e6 bytes.  A NULL pred_crd, true_crd, seq, score or confusion, B or L <= 0, or L beyond INT_MAX / 28 (the bound of
 * ptamd_lddt): PTAMD_ERR_BAD_SHAPE; workspace NULL or too small: PTAMD_ERR_WORKSPACE; nothing is launched or written then.  No
 * state between calls, nothing read from the environment. */
size_t ptamd_ss_workspace_bytes(int B, int L);
int ptamd_ss(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float *score, int32_t *confusion,
             int8_t *states, uint64_t *hbonds, void *workspace, size_t workspace_bytes, void *stream);

/* Side-chain accuracy, for a whole batch (csrc/sidechain.hip): the share of correct rotamers, the mean chi error and the
 * side-chain RMSD in the residue's own backbone frame - `eval_metrics.sidechain_batch`, `python -m protein_transformer_amd.score`.
 * The reference has no counterpart.  The chi angles are those of the IUPAC-IUB Commission on Biochemical Nomenclature,
 * "Abbreviations and symbols for the description of the conformation of polypeptide chains", Biochemistry 9:3471-3479 (1970).
 * PARITY UNPINNED: what is pinned is this definition, restated in numpy fp64 by tests/sidechain_ref.py.
 * Inputs as for ptamd_lddt; slots of a residue: 0 N, 1 CA, 2 C, 3 O, 4 + k side-chain atom k in the order of csrc/nerf_tables.h.
 * Residues whose id is outside 0..19 (PTAMD_PAD_ID, unknown ids) take no part, the rule of ptamd_clash_fwd_bwd.
 *   Chi angles.  Residue types in the order ACDEFGHIKLMNPQRSTVWY have {0,1,2,3,2,0,2,2,4,2,3,2,2,3,4,1,1,1,2,2} of them.  In
 *   this atom layout the IUPAC chi_k, k = 1..4, is the dihedral of slots (0,1,4,5), (1,4,5,6), (4,5,6,7), (5,6,7,8) for EVERY
 *   type: side-chain atom k >= 1 of every type that has a chi_k is built on the parents (N,CA,CB), (CA,CB,atom 1), ... of
 *   csrc/nerf_tables.h, and the atom names of those slots are the IUPAC ones (ILE: CB, CG1, CD1; THR: OG1; VAL: CG1).  So chi_k
 *   is also the build torsion of angle column 6 + k.  Dihedral of p0..p3: b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2, n1 = b1 x b2,
 *   n2 = b2 x b3, chi = atan2(|b2| b1 . n2, n1 . n2).
 *   chi_k of a residue is SCORED when its four TRUE atoms are present (no NaN) and the true |n1|^2 and |n2|^2 both exceed
 *   1e-8 A^4, a test made in fp64 on the fp32 coordinates, as the frame test of ptamd_fape_fwd_bwd is.  What the prediction
 *   holds never decides what is scored; its dihedral is taken as it comes.  Delta_k = |chi_pred - chi_true| wrapped into
 *   [0, 180] degrees; for ASP chi2, GLU chi3, PHE chi2 and TYR chi2, whose far atoms are interchangeable (the pairs of
 *   ptamd_rename_symmetric), Delta_k = min(Delta_k, 180 - Delta_k).  A hit is Delta_k <= threshold_deg; the usual value is 40.
 *   The flips of ASN, GLN and HIS (N and O, or the ring, exchanged in the crystallographer's assignment) are NOT resolved.
 *   Local-frame side-chain RMSD.  A residue is COUNTED when its type has at least one side-chain atom, its true N, CA, C and
 *   all its true side-chain atoms are present, and its TRUE N, CA, C span a frame: algorithm 21 of Jumper et al. with the 1e-8
 *   tests of ptamd_fape_fwd_bwd.  In each structure the side-chain atoms are expressed in that structure's own frame,
 *   x = R^T (p - CA); d2(r) = sum over the atoms of |x_pred - x_true|^2; for ASP, GLU, PHE and TYR the smaller of that sum and
 *   the same sum with the predicted slots of the pairs of ptamd_rename_symmetric exchanged.
 *   Unusable prediction.  A non-finite predicted coordinate on any atom of a scored chi or on N, CA, C or a side-chain atom of
 *   a counted residue, or predicted N, CA, C of a counted residue that span no frame, makes all four scores of that protein NaN
 *   and its hit counts 0 - the rule of ptamd_ss; its other counts, and every other protein, are what they would be.
 *   score [B,4] out = {chi1, chi12, chi_mae, sc_rmsd}: chi1 = hits_1 / scored_1; chi12 = among the residues whose chi1 and chi2
 *   are both scored, the share where both hit; chi_mae = the mean Delta in degrees over every scored chi1..chi4; sc_rmsd =
 *   sqrt(sum d2(r) / sum atoms) over the counted residues; each NaN when its denominator is 0.
 *   counts [B,12] out = {scored_1, hit_1, scored_2, hit_2, scored_3, hit_3, scored_4, hit_4, n12, hit12, residues counted,
 *   atoms counted}.
 *   per_res [B,L,5] out or NULL = {Delta_1 .. Delta_4 in degrees, sqrt(d2(r) / n_sc)}, NaN where not scored / not counted, and
 *   on the columns of a residue that its own prediction makes unusable.
 * Per-residue arithmetic is fp32 on the fp32 inputs (frames: fp64, rounded once), except the two degeneracy tests; prediction
 * and truth go through the same device functions, so a prediction equal to the truth has Delta == 0 and d2 == 0 exactly.  For
 * coordinates within +-64 A, bonds of 1-2 A and bond angles of 60-150 degrees a Delta is within 5.5e-4 degrees of its fp64 value
 * (tests/sidechain_ref.py derives the figure): a Delta that close to the threshold may be decided either way; outside that band
 * the counts are exact.  Per-protein sums are fp64 in a fixed order, no atomics: two runs give the same bits, and a protein's
 * result depends neither on the batch around it nor on how far its row is padded.  Workspace: 80 B per 64 residue slots - a
 * function of (B, L) only.  A NULL pred_crd, true_crd, seq, score or counts, B or L <= 0, L beyond INT_MAX / 28 (the bound of
 * ptamd_lddt), or a threshold that is negative or not finite: PTAMD_ERR_BAD_SHAPE; workspace NULL or too small:
 * PTAMD_ERR_WORKSPACE; a workspace that is not 16-byte aligned, or a pred_crd or true_crd that is not 8-byte aligned (the kernel
 * reads the coordinates as pairs of floats): PTAMD_ERR_ALIGN; nothing is launched or written then.  No state between calls,
 * nothing read from the environment. */
size_t ptamd_sidechain_workspace_bytes(int B, int L);
int ptamd_sidechain(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float threshold_deg,
                    float *score, int32_t *counts, float *per_res, void *workspace, size_t workspace_bytes, void *stream);

/* Superposed per-residue spread of K structures around a reference, for a whole batch (csrc/ensemble.hip): what
 * `ensemble.predict_ensemble` and `python -m protein_transformer_amd.predict` make of K dropout passes of a model around its
 * deterministic prediction.  The reference has no counterpart; ptamd_kabsch_rmsd returns one number per pair and ptamd_tm_score
 * fits by TM-score - this returns what each residue does after a least-squares fit.  There is no truth: every array is a
 * prediction.  PARITY UNPINNED: what is pinned is this definition, restated in numpy fp64 by tests/ensemble_ref.py.
 *   ref_crd [B,L*14,3] the reference; sample_crd [B,K,L*14,3] the K samples of every protein; seq [B,L]; slots of a residue:
 *   0 N, 1 CA, 2 C, 3 O, 4 + k side-chain atom k in the order of csrc/nerf_tables.h.
 *   Presence.  Residue i is PRESENT when seq[i] is in 0..19 (neither PTAMD_PAD_ID nor an unknown id), the rule of
 *   ptamd_clash_fwd_bwd; n_b is the number of present residues of protein b.  The ATOMS of a present residue are the slots its
 *   type has, s < 4 + ptamd_sidechain_atoms(seq[i]); what any other slot holds is never read into a result.
 *   Usable samples.  Sample (b,k) is USABLE when n_b >= 3 and the C-alpha (slot 1) of every present residue is finite in the
 *   sample and in the reference.  usable[b] = K', the number of usable samples of protein b.
 *   Fit.  For a usable sample, (R_k, t_k) is the PROPER rotation (det = +1) and the translation that minimise
 *   sum_i |R s_ki + t - r_i|^2 over the present C-alphas, s the sample and r the reference: a mirror image is not fitted by a
 *   reflection.  The moments are fp64 on the fp32 inputs and the solve is that of ptamd_tm_score (csrc/tm_rotation.h: Horn's
 *   quaternion matrix, cyclic Jacobi); (R_k, t_k) is then rounded to fp32 once.
 *   rmsd [B,K] out: sqrt((1 / n_b) sum_i |R_k s_ki + t_k - r_i|^2) over the present C-alphas; NaN where the sample is unusable.
 *   rmsf [B,L,2] out, over the usable samples of the protein:
 *     [b,i,0] = sqrt((1 / K') sum_k |R_k s_ki + t_k - r_i|^2) on the C-alpha of residue i;
 *     [b,i,1] = sqrt((1 / K') sum_k (1 / |A_ki|) sum_{a in A_ki} |R_k s_ka + t_k - r_a|^2), A_ki being the atoms of residue i
 *     that are finite in the reference and in sample k;
 *     both NaN for an absent residue and where K' = 0.
 *   A non-finite side-chain (or N, C, O) atom does not make a sample unusable: that atom is LEFT OUT OF ITS OWN TERM, in the sum
 *   and in |A_ki|; were a residue left with no atom in a usable sample, its all-atom value would be NaN (0 / 0) - which cannot
 *   happen to a present residue, since its C-alpha is one of its atoms and is finite in every usable sample.
 * A deviation |R s + t - r|^2 is fp32 on the fp32 inputs under the fp32 (R, t) - the same arithmetic for rmsd and rmsf -, the
 * sum over the atoms of a residue is fp32 in slot order, the sums over residues and over samples are fp64 in a fixed order, and
 * every result is rounded to fp32 once.  For coordinates within +-X A every result is within 32 x 2^-23 x X A of its fp64 value
 * (tests/ensemble_ref.py derives the figure).  No atomics, no order-dependent reduction: two runs give the same bits, and a
 * protein's result depends neither on the batch around it nor on how far its row is padded.  Every element of rmsd, rmsf and
 * usable is written, whatever the workspace held on arrival.  Workspace: 64 B per (protein, sample) - the fitted transforms
 * between the two launches; ptamd_ensemble_workspace_bytes is a function of (B, K, L) only.  A NULL array, B, K or L <= 0,
 * L beyond INT_MAX / 28 (the bound of ptamd_lddt), or B * K or B * ceil(L / 64) beyond INT_MAX: PTAMD_ERR_BAD_SHAPE (a size of
 * 0); workspace NULL or too small: PTAMD_ERR_WORKSPACE; a workspace that is not 16-byte aligned: PTAMD_ERR_ALIGN; nothing is
 * launched or written then.  No state between calls, nothing read from the environment. */
size_t ptamd_ensemble_workspace_bytes(int B, int K, int L);
int ptamd_ensemble_spread(const float *ref_crd, const float *sample_crd, const int64_t *seq, int B, int K, int L, float *rmsd,
                          float *rmsf, int32_t *usable, void *workspace, size_t workspace_bytes, void *stream);

/* Frame-aligned error matrix of K structures around a reference, for a whole batch (csrc/aligned_error.hip): entry (i, j) is the
 * error of residue j's C-alpha when the two structures are aligned on the backbone frame of residue i - the aligned error of
 * Jumper et al., Nature 596:583-589 (2021), supplementary 1.9.7.  ptamd_ensemble_spread fits every sample once, globally, and
 * smears a hinge over the whole chain; here domains and hinges show as blocks.  With the K dropout samples of
 * `ensemble.predict_ensemble` it is a self-consistency matrix (`predict --pae`); with K = 1, the native structure as the
 * reference and the prediction as the sample it is the true aligned error (`score --aligned_error`).  The reference
 * (protein_transformer) has no counterpart.  PARITY UNPINNED: what is pinned is this definition, restated in numpy fp64 by
 * tests/aligned_error_ref.py.
 *   ref_crd [B,L*14,3], sample_crd [B,K,L*14,3], seq [B,L]: the layout of ptamd_ensemble_spread; only slots 0 N, 1 CA, 2 C are
 *   read.  Residue i is PRESENT when seq[i] is in 0..19, the rule of ptamd_ensemble_spread.
 *   Frames and points.  Residue i is a FRAME of protein b when it is present, its N, CA and C are finite and within 1e18 in
 *   ref_crd, and they span a frame (algorithm 21, csrc/backbone_frame.h: |C - CA|^2 and the squared rejection of N - CA from it
 *   above 1e-8 A^2, tested in fp64 on the fp32 coordinates).  Residue j is a POINT when it is present and its CA is finite and
 *   within 1e18 in ref_crd.  Frames and points depend on the reference only (the rule of ptamd_fape_fwd_bwd for the truth); n_b
 *   is the number of points.
 *   Usable samples.  Sample (b,k) is USABLE when every frame of the reference is a frame in the sample too (finite N, CA, C
 *   within 1e18 that span a frame) and every point's CA is finite and within 1e18 in the sample.  usable[b] = K', the number of
 *   usable samples.  What any other slot of a sample holds is never read: a non-finite atom there changes not one bit.
 *   ae [B,L,L] out: x_ij(S) being the CA of j in the coordinates of frame i of structure S,
 *     ae[b,i,j] = (1 / K') sum over the usable k of |x_ij(sample k) - x_ij(ref)|,
 *   the plain Euclidean norm, no epsilon under the root; i = j gives exactly 0.  NaN where i is no frame, where j is no point,
 *   in padded rows and columns, and everywhere when K' = 0.  Row = frame, column = point: the matrix is not symmetric.
 *   stats [B,2] out: {mean, tm}.  mean is the mean of the defined entries of protein b.  tm = max over the frames i of
 *   (1 / n_b) sum_j 1 / (1 + (ae_ij / d0)^2), d0 = 1.24 cbrt(max(n_b, 19) - 15) - 1.8: the pTM formula of the same supplement -
 *   APPLIED TO THE MEAN ERROR, not to a predicted distribution of errors, so with dropout samples it is a self-consistency
 *   number and not a calibrated pTM.  Both NaN when no entry is defined.
 * The frame is fp64 arithmetic on the fp32 coordinates, rounded to fp32 once; x_ij is the one device function for reference and
 * sample (backbone_frame::local_coords), the difference and the norm are fp32, the sum over k is fp32 in the order k = 0..K-1
 * followed by one fp32 division; the sums of the stats are fp64 in a fixed order and each stat is rounded to fp32 once.  For
 * coordinates within +-X A and K <= 8 every entry and the mean are within 72 x 2^-23 x X A of their fp64 values, tm within
 * 0.65 / d0 times that (tests/aligned_error_ref.py derives the figures).  No atomics, no order-dependent reduction: two runs
 * give the same bits, and a protein's result depends neither on the batch around it nor on how far its row is padded.  Every
 * element of ae, stats and usable is written, whatever they and the workspace held on arrival.  Workspace: a 64-byte record per
 * (protein, structure, residue), the samples' verdicts, and a pair of fp64 partial sums per (row, column tile of 64);
 * ptamd_aligned_error_workspace_bytes is a function of (B, K, L) only.  A NULL array, B, K or L <= 0, L beyond INT_MAX / 28 (the
 * bound of ptamd_lddt), or B * (K + 1) beyond INT_MAX or B * ceil(L / 64)^2 beyond INT_MAX / 256 (what one launch addresses):
 * PTAMD_ERR_BAD_SHAPE (a size of 0); workspace NULL or too small: PTAMD_ERR_WORKSPACE; a workspace that is not 16-byte aligned:
 * PTAMD_ERR_ALIGN; nothing is launched or written then.  No state between calls, nothing read from the environment. */
size_t ptamd_aligned_error_workspace_bytes(int B, int K, int L);
int ptamd_aligned_error(const float *ref_crd, const float *sample_crd, const int64_t *seq, int B, int K, int L, float *ae,
                        float *stats, int32_t *usable, void *workspace, size_t workspace_bytes, void *stream);

/* Smooth lDDT loss, forward + analytic backward, for a whole batch (csrc/slddt.hip): the training loss `-l slddt`.  The
 * reference has no counterpart; this is the differentiable lDDT of Abramson et al., "Accurate structure prediction of
 * biomolecular interactions with AlphaFold 3", Nature 630:493-500 (2024), supplementary algorithm 27 - sigmoids in place of the
 * four threshold tests of lDDT.  It departs from that algorithm in a temperature tau that divides the argument of the sigmoids
 * (tau = 1 is AlphaFold 3's loss, tau -> 0 approaches 1 - the hard all-atom lDDT of ptamd_lddt).
 *   Atoms and pairs.  Per protein, the atoms are exactly those of ptamd_lddt: slots of non-pad residues whose true coordinate
 *   has no NaN; an atom's residue is slot / 14.  An unordered pair {a, b} of atoms in different residues is included if its true
 *   distance dt < cutoff.  The comparison is strict; dt = sqrt(dx^2 + dy^2 + dz^2) of fp32 coordinate differences, as in
 *   ptamd_lddt.  Inclusion depends on the truth only.
 *   Pair score.  delta = |dp - dt|, with dp the predicted distance under the same clamp under the root that the dRMSD kernel
 *   applies (1e-30 added to the squares).  eps(delta) = 1/4 sum over t in {0.5, 1, 2, 4} of sigma((t - delta) / tau), with sigma
 *   the logistic function and tau > 0 the temperature.  AlphaFold 3 uses tau = 1.
 *   Per-protein outputs.  score_i is the mean of eps over the included pairs; loss_i = 1 - score_i; npairs_i is the number of
 *   included unordered pairs, as an exact 64-bit integer.  A protein without an included pair has loss_i = score_i = NaN,
 *   npairs_i = 0 and an all-zero gradient.  It is left out of every mean, as the metric does.
 *   Gradient.  dcrd = d(loss_i)/d(pred_crd).  For atom a: -(1 / npairs_i) sum_b eps'(delta) sign(dp - dt) (x_a - x_b) / dp, with
 *   sign(0) = 0.  A prediction equal to the truth therefore gets an exactly zero gradient.  Empty slots and padded residues get
 *   zeros.  A non-finite predicted coordinate does not trap: the pairs of that atom are counted, contribute eps = 0 and no
 *   gradient - neither to the atom itself (its row of dcrd is zero) nor to its partners.  A finite coordinate beyond 1e18 in
 *   magnitude is treated the same way (its squared differences would overflow fp32).
 *   Batch.  The reported batch value is the mean over proteins with a score; the back-propagated quantity is the SUM over
 *   proteins of loss_i - the convention of every other structural loss here (SURVEY A-7), which keeps data parallelism a plain
 *   SUM all-reduce with no global count.
 *   stats [B,2] out = {loss_i, score_i}; npairs [B] out (int64); dcrd [B,L*14,3] out, or NULL for the forward-only form (no
 *   gradient work; the same bits in stats and npairs).
 * No floating-point atomics and fixed-order partial sums: two runs give the same bits, and a protein's result depends neither on
 * the batch around it nor on how far its row is padded.  Workspace: a function of (B, L) only - 32 B per atom slot, and the
 * partial sums of the upper-triangle sweep over tiles of 64 compacted atoms: 1 KB per (row tile, chunk of 8 column tiles) and
 * per (strip of 4 row tiles, column tile); B = 32, L = 512: 162e6 bytes.  No getenv, no state between calls.
 * cutoff or temperature not finite and positive, a NULL array other than dcrd, B or L <= 0, or L beyond INT_MAX / 28 (the bound
 * of ptamd_lddt): PTAMD_ERR_BAD_SHAPE; workspace NULL or too small: PTAMD_ERR_WORKSPACE; nothing is launched or written in
 * either case.  (The arguments t / tau of the exponentials are carried as integer + fraction: any tau down to 1e-8 keeps the
 * definition; below that the four sigmoids saturate towards a step at their thresholds.) */
size_t ptamd_slddt_workspace_bytes(int B, int L);
int ptamd_slddt_fwd_bwd(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float cutoff,
                        float temperature, float *stats, int64_t *npairs, float *dcrd, void *workspace, size_t workspace_bytes,
                        void *stream);

/* Frame aligned point error (FAPE), forward + analytic backward, for a whole batch (csrc/fape.hip): the training loss
 * `-l fape`.  The reference has no counterpart, and every other structural loss here is a function of internal distances, blind
 * to a mirror image; this is the loss of Jumper et al., "Highly accurate protein structure prediction with AlphaFold", Nature
 * 596:583-589 (2021), supplementary algorithms 21 (a frame from three points) and 28 (FAPE), over backbone frames and all atoms.
 *   Atoms.  Per protein, exactly those of ptamd_lddt and ptamd_slddt_fwd_bwd: slots of non-pad residues whose true coordinate
 *   has no NaN.
 *   Frames.  The non-pad residues whose slots 0, 1, 2 (N, CA, C) are all present in the truth and whose TRUE frame is not
 *   degenerate.  Algorithm 21 with origin t = CA: v1 = C - CA, v2 = N - CA, e1 = v1 / |v1|, u2 = v2 - e1 (e1 . v2),
 *   e2 = u2 / |u2|, e3 = e1 x e2, R = (e1 e2 e3); degenerate when |v1|^2 <= 1e-8 A^2 or |u2|^2 <= 1e-8 A^2.  Which frames exist
 *   depends on the truth only.  (Evaluated in fp64 on the fp32 coordinates and rounded once.)
 *   Pair.  For every ordered (frame i, atom j), atoms of residue i included: x_ij = R_i^T (x_j - t_i) for the prediction and
 *   likewise for the truth, Delta_ij their difference, d_ij = sqrt(|Delta_ij|^2 + 1e-4 A^2), pair value = min(d_ij, clamp) / Z
 *   with Z = 10 A.  The clamp test is strict: a pair with d < clamp is unclamped; a clamped pair carries no gradient.  clamp
 *   must be positive and not NaN; +inf means unclamped.
 *   Per-protein outputs.  loss_i is the mean of the pair values; npairs_i = frames x atoms and nclamped_i the number of clamped
 *   pairs, exact 64-bit integers.  A protein with no frame or no atom has loss_i = NaN, both counts 0 and an all-zero gradient.
 *   It is left out of every mean.
 *   Gradient.  dcrd = d(loss_i)/d(pred_crd), analytic: each unclamped pair gives R_i Delta_ij / (d_ij Z npairs_i) to atom j,
 *   and to the predicted N, CA, C of frame i what follows through t_i and through the backward of algorithm 21.  The true frame
 *   is a constant.  Empty slots and padded residues get zeros.  Prediction and truth go through the same device functions, so a
 *   prediction whose present atoms equal the truth bit for bit has Delta = 0 exactly: dcrd all zeros, loss_i = 1e-3.
 *   Unusable predictions.  A present atom whose predicted coordinate is not finite or beyond 1e18 in magnitude, or a predicted
 *   frame that is degenerate by the same 1e-8 test, makes the whole protein unusable: loss_i = NaN and an all-zero gradient;
 *   npairs_i is still reported, and nclamped_i = 0 (no pair of it is evaluated).  Nothing traps, other proteins are untouched.
 *   Batch.  The reported batch value is the mean over the proteins with a finite loss; the back-propagated quantity is the SUM
 *   over proteins of loss_i, as for every structural loss here (SURVEY A-7): data parallelism stays a plain SUM all-reduce.
 *   stats [B,2] out = {loss_i, nclamped_i / npairs_i}; npairs, nclamped [B] out (int64); dcrd [B,L*14,3] out, or NULL for the
 *   forward-only form (no gradient work; the same bits in stats and the counts).
 * No floating-point atomics and fixed-order partial sums: two runs give the same bits, and a protein's result depends neither on
 * the batch around it nor on how far its row is padded.  Workspace: a function of (B, L) only - 32 B per atom slot, 100 B per
 * residue (frame records) and 3 KB per (tile of 64 frames, chunk of 8 tiles of 64 atoms); B = 32, L = 512: 20e6 bytes.  No
 * getenv, no state between calls.  A bad clamp, a NULL array other than dcrd, B or L <= 0, or L beyond INT_MAX / 28 (the bound
 * of ptamd_lddt): PTAMD_ERR_BAD_SHAPE; workspace NULL or too small: PTAMD_ERR_WORKSPACE; nothing is launched or written in
 * either case. */
size_t ptamd_fape_workspace_bytes(int B, int L);
int ptamd_fape_fwd_bwd(const float *pred_crd, const float *true_crd, const int64_t *seq, int B, int L, float clamp,
                       float *stats, int64_t *npairs, int64_t *nclamped, float *dcrd, void *workspace, size_t workspace_bytes,
                       void *stream);

/* Steric clash term, forward + analytic backward, for a whole batch (csrc/clash.hip): the auxiliary training term
 * `--clash_weight` and the metric `--eval_clash`.  The reference has no counterpart, and every other loss and metric here
 * compares the prediction with the truth; this one asks whether the predicted all-atom structure is physically possible.  It is
 * the between-residue part of the structural violation loss of Jumper et al., "Highly accurate protein structure prediction
 * with AlphaFold", Nature 596:583-589 (2021), supplementary 1.9.11 - the NeRF build fixes every bond length and bond angle, so a
 * clash between residues is the only violation an angle model can commit.  The truth is not an argument.
 *   Atoms.  Per protein, slot s of residue i is an atom when seq[i] is in 0..19 (neither PTAMD_PAD_ID nor an unknown id) and
 *   s % 14 < 4 + ptamd_sidechain_atoms(seq[i]): the slot exists for that residue type.  This differs from ptamd_lddt and its
 *   family, whose atoms are the truth's present atoms.  What any other slot holds (the NeRF build zero-fills them, so they all
 *   coincide at the origin), NaN and 1e30 included, is never read and changes no output.
 *   Radii.  The van der Waals radius by element, r = 1.7 A (C), 1.55 A (N), 1.52 A (O), 1.8 A (S); the element is the first
 *   letter of the atom's name (ptamd_clash_radius below).
 *   Pairs.  The unordered pairs {a, b} of atoms in DIFFERENT residues, except slot 2 (C) of residue i with slot 0 (N) of residue
 *   i + 1 (the peptide bond) and slot 5 of a CYS (id 1) with slot 5 of any other CYS (a possible disulfide): AlphaFold's two
 *   exclusions.  Pairs within a residue are never looked at.
 *   Pair term.  v_ab = max(0, r_a + r_b - tau - d_ab) with the tolerance tau >= 0 (AlphaFold: 1.5 A) and d_ab = sqrt(|x_a -
 *   x_b|^2 + 1e-30), the clamp under the root of the dRMSD and smooth-lDDT kernels.
 *   Per-protein outputs.  loss_i = (1 / n_i) sum v_ab, n_i the protein's atom count: Angstrom per atom and, like lndrmsd,
 *   independent of the length.  nclash_i is the number of pairs with v_ab > 0, an exact 64-bit integer.  A protein with atoms but
 *   no violating pair has loss_i = 0; a protein without an atom has loss_i = NaN, nclash_i = 0 and a zero gradient.
 *   Gradient.  g = d(loss_i)/d(pred_crd), analytic: atom a gets -(1 / n_i) sum_b [v_ab > 0] (x_a - x_b) / d_ab; atoms that
 *   coincide exactly have a finite, zero share.  Exactly zero in every slot that is not an atom.
 *   Unusable predictions.  An atom whose predicted coordinate is not finite or beyond 1e18 in magnitude makes the whole protein
 *   unusable (the policy of ptamd_fape_fwd_bwd): loss_i = NaN, nclash_i = 0 and a zero gradient.  Nothing traps, other proteins
 *   are untouched.
 *   Batch.  The reported batch value is the mean over the proteins with a finite loss; the back-propagated quantity is the SUM
 *   over proteins of loss_i, as for every structural loss here: data parallelism stays a plain SUM all-reduce.
 *   stats [B,2] out = {loss_i, n_i}; nclash [B] out (int64).  dcrd [B,L*14,3], or NULL for the forward-only form (no gradient
 *   work; the same bits in stats and nclash): with accumulate == 0 the call writes dcrd = weight * g (zeros where there is no
 *   atom); with accumulate != 0 it computes dcrd += weight * g in place and touches the slots of atoms only - how the term joins
 *   another loss's gradient in front of the one NeRF adjoint.
 * No atomics and fixed-order partial sums: two runs give the same bits, and a protein's result depends neither on the batch
 * around it nor on how far its row is padded.  Tile pairs whose bounding boxes of PREDICTED coordinates are farther apart than
 * 2 * 1.8 - tau are skipped.  Workspace: a function of (B, L) only - that of ptamd_slddt_fwd_bwd and one int per protein;
 * B = 32, L = 512: 162e6 bytes.  No getenv, no state between calls.  tolerance not finite or negative, weight not finite, a NULL
 * array other than dcrd, B or L <= 0, or L beyond INT_MAX / 28 (the bound of ptamd_lddt): PTAMD_ERR_BAD_SHAPE; workspace NULL or
 * too small: PTAMD_ERR_WORKSPACE; nothing is launched or written in either case.
 * ptamd_clash_radius (host only): the radius of slot `slot` of residue type `residue`, -1 where the type has no such slot. */
float ptamd_clash_radius(int residue, int slot);
size_t ptamd_clash_workspace_bytes(int B, int L);
int ptamd_clash_fwd_bwd(const float *pred_crd, const int64_t *seq, int B, int L, float tolerance, float weight, int accumulate,
                        float *stats, int64_t *nclash, float *dcrd, void *workspace, size_t workspace_bytes, void *stream);

/* Symmetric side-chain renaming of the ground truth, for a whole batch (csrc/rename.hip): `train.py --rename_symmetric`.  The
 * reference has no counterpart.  ASP, GLU, PHE and TYR have side chains with a 180 degree symmetry: OD1/OD2, OE1/OE2, CD1/CD2 and
 * CE1/CE2 are chemically the same atoms, which of them carries which name in a deposited structure is arbitrary, and chi and
 * chi + pi build the same molecule with the names exchanged.  This is the renaming of Jumper et al., "Highly accurate protein
 * structure prediction with AlphaFold", Nature 596:583-589 (2021), supplementary 1.8.5, algorithm 26: the truth is renamed,
 * residue by residue, to the naming that agrees better with the prediction, and every loss and metric then runs against the
 * renamed truth unchanged.
 *   Swap pairs.  Slots are 0 N, 1 CA, 2 C, 3 O, 4 + k for side-chain atom k; residue ids follow ACDEFGHIKLMNPQRSTVWY.
 *     ASP (2):  (6,7) OD1/OD2;                    chi column 8
 *     GLU (3):  (7,8) OE1/OE2;                    chi column 9
 *     PHE (4):  (6,10) CD1/CD2, (7,9) CE1/CE2;    chi column 8
 *     TYR (19): (6,11) CD1/CD2, (7,10) CE1/CE2;   chi column 8
 *   The chi column is the angle column (of 12) whose torsion places the first atom of the first pair - side-chain atom k is
 *   placed with column 6 + k (csrc/geometry.hip; column 6 is CB's own torsion, so what the literature calls chi2 of ASP is
 *   column 8): turning it by pi builds the residue with the names exchanged.  An AMBIGUOUS atom is a member of a swap pair, in a
 *   candidate residue or not.  No other residue type is touched (ARG, LEU and VAL are not symmetric in this sense).
 *   Present atoms.  Exactly the atoms of ptamd_lddt, ptamd_slddt_fwd_bwd and ptamd_fape_fwd_bwd: slots of non-pad residues
 *   whose true coordinate has no NaN (csrc/atom_tiles.h decides).
 *   Candidate residue.  A non-pad ASP, GLU, PHE or TYR ALL of whose ambiguous atoms are present.  Every other residue is left as
 *   it is, with flag 0 and cost 0.  (Simpler than AlphaFold's partial-presence handling through alt_gt_exists: a residue with a
 *   missing swap partner keeps its names.)
 *   Cost.  Over the ambiguous atoms a of a candidate residue, a' the partner of a:
 *     cost_orig = sum_a sum_q |d_pred(a,q) - d_true(a,q)|,   cost_alt = sum_a sum_q |d_pred(a,q) - d_true(a',q)|,
 *   q over every present, non-ambiguous atom of the protein, those of the residue itself included; d = sqrt(dx^2 + dy^2 + dz^2)
 *   of fp32 coordinate differences, prediction and truth through the same expression (algorithm 26 without the 1e-10 that the
 *   published code adds under the root).  Sums: fp32 within a tile of 64 partners, fp64 beyond, rounded once.
 *   Decision.  swapped = cost_alt < cost_orig on the reported fp32 values; strict, so a tie keeps the names.  A present atom
 *   whose predicted coordinate is not finite or beyond 1e18 in magnitude (the test of the two training losses) leaves the WHOLE
 *   protein unswapped: flags 0, and cost = NaN for its candidates.  Nothing traps, other proteins are untouched.
 *   Application.  true_crd_out [B,L*14,3]: a copy of true_crd with the slot pairs of swapped residues exchanged; NaNs, padding
 *   and every other value are copied bit for bit.  true_ang_out [B,L,24] (cos and sin interleaved): a copy of true_ang with
 *   both entries of the chi column of swapped residues negated (the sign bit flipped: NaN stays NaN); true_ang and true_ang_out
 *   are optional, both NULL or neither.
 *   Gradient.  The renaming is a constant for the gradient (a stop-gradient, as in AlphaFold): there is no adjoint.
 *   swapped [B,L] out (int32: 0 or 1), cost [B,L,2] out = {cost_orig, cost_alt}; both written for every residue.
 * No atomics and fixed-order sums: two runs give the same bits, and a protein's result depends neither on the batch around it
 * nor on how far its row is padded.  Workspace: a function of (B, L) only - 32 B per atom slot, 40 B per residue and 1 KB per
 * (tile of 64 swap pairs, chunk of 4 tiles of 64 atoms); B = 32, L = 512: 23e6 bytes.  No getenv, no state between calls.
 * B or L <= 0, L beyond INT_MAX / 28 (the bound of ptamd_lddt), a NULL array other than the angle pair, only one of true_ang and
 * true_ang_out NULL, an output that overlaps its input, or true_crd_out overlapping pred_crd: PTAMD_ERR_BAD_SHAPE; workspace NULL
 * or too small: PTAMD_ERR_WORKSPACE; a workspace that is not 16-byte aligned: PTAMD_ERR_ALIGN; nothing is launched or written in
 * any of these cases.  The partial sums grow with L^2 (pair tiles x atom chunks: 175 MB per protein at L = 10000), and the sweep's
 * grid covers the largest protein the shape allows - workgroups beyond a protein's own pairs and atoms return at once. */
size_t ptamd_rename_symmetric_workspace_bytes(int B, int L);
int ptamd_rename_symmetric(const float *pred_crd, const float *true_crd, const float *true_ang, const int64_t *seq, int B, int L,
                           float *true_crd_out, float *true_ang_out, int32_t *swapped, float *cost, void *workspace,
                           size_t workspace_bytes, void *stream);

/* mse_over_angles x3 (losses.py:175-214; train.py:64-66) in one pass.
 *   pred, truth [T,24]; out[6] = {sum_full, cnt_full, sum_bb, cnt_bb, sum_sc, cnt_sc} (fp32); the workspace holds
 *   the fp64 partial sums of the first pass.  A row enters a slice when any truth element of the slice is != 0: NaN and a
 *   denormal (1e-40: nothing flushes to zero) select it, -0.0 does not; its NaN truth elements are left out of sum and count.
 *   T <= 0: PTAMD_ERR_BAD_SHAPE; pred or truth not 16-byte aligned: PTAMD_ERR_ALIGN; workspace NULL or short:
 *   PTAMD_ERR_WORKSPACE; nothing is launched or written then. */
size_t ptamd_mse_angles_workspace_bytes(void);
int ptamd_mse_angles_fwd(const float *pred, const float *truth, int64_t T, float *out, void *workspace,
                         size_t workspace_bytes, void *stream);
/* dpred[T,24] (+)= coef * 2*(pred-truth)/cnt_full on the selected elements; accumulate != 0 adds.  Every other element is
 * exactly 0 (accumulating: unchanged), also when cnt_full = sums[1] is 0.  No alignment requirement; T <= 0: PTAMD_ERR_BAD_SHAPE. */
int ptamd_mse_angles_bwd(const float *pred, const float *truth, int64_t T, const float *sums, float coef,
                         int accumulate, float *dpred, void *stream);

/* Binned-lDDT loss of the confidence head (csrc/plddt.hip; protein_transformer_amd/confidence.py): the pLDDT head of AlphaFold 2
 * (Jumper et al., Nature 596:583-589 (2021), supplementary 1.9.6) - a softmax over nbins equal bins of [0, 1], trained by
 * cross-entropy against the bin of the per-residue lDDT-C-alpha of the model's own prediction (ptamd_lddt, per_res[..., 1]).  Not
 * in the reference.
 *   logits [T, ld] in, 2 <= nbins <= 64, ld >= nbins a row stride in floats: row t reads logits[t * ld + k] for k < nbins and
 *     nothing else of the row (the spare columns may hold anything).
 *   target in, or NULL.  Row t reads target[t * target_stride] (target_stride >= 1: per_res[..., 1] is read in place with 2).
 *     A row COUNTS when its target is finite; its bin is min(nbins - 1, max(0, (int)floorf(target * nbins))), the product one fp32
 *     multiply.  NULL is inference: only plddt is written; ce, sums and the workspace may be NULL.
 *   plddt [T] out, every row: 100 * sum_k p_k (k + 0.5) / nbins, p the max-subtracted softmax of the row's nbins logits.
 *   ce [T] out: -log p_bin of a counted row, NaN of any other.
 *   sums [2] out: {mean of ce over the counted rows (NaN when there is none), number of counted rows}.
 *   ptamd_plddt_bwd: dlogits[t * ldd + k] = coef / sums[1] * (p_k - [k == bin_t]) for k < nbins of a counted row, and exactly 0
 *     in every other row, in the columns nbins .. ldd - 1 of every row, and everywhere when sums[1] is 0; all T * ldd floats are
 *     written.  ldd >= nbins; sums is what ptamd_plddt_fwd left, read on the device (no host synchronisation).
 * fp32 throughout, the sum of ce over the rows in fp64: ptamd_plddt_rows_per_block() rows in index order per workgroup, a record
 * of 16 bytes each in the workspace (ptamd_plddt_workspace_bytes, a function of T only), then the records in index order in one
 * further launch.  No atomics: two calls give the same bits.  T <= 0, nbins outside 2 .. 64, ld or ldd below nbins,
 * target_stride < 1, a NULL array that the call would read or write: PTAMD_ERR_BAD_SHAPE; with a target, a workspace NULL or too
 * small: PTAMD_ERR_WORKSPACE, not 16-byte aligned: PTAMD_ERR_ALIGN; nothing is launched or written then.  Nothing is allocated,
 * no state between calls, nothing read from the environment. */
int ptamd_plddt_rows_per_block(void);
size_t ptamd_plddt_workspace_bytes(int64_t T);
int ptamd_plddt_fwd(const float *logits, int ld, const float *target, int target_stride, int64_t T, int nbins, float *plddt,
                    float *ce, float *sums, void *workspace, size_t workspace_bytes, void *stream);
int ptamd_plddt_bwd(const float *logits, int ld, const float *target, int target_stride, int64_t T, int nbins, const float *sums,
                    float coef, float *dlogits, int ldd, void *stream);

/* Pair sweep of the trained PAE head (csrc/pae_head.hip; protein_transformer_amd/confidence.py, class PaeHead): the aligned-error
 * head of AlphaFold 2 (Jumper et al., Nature 596:583-589 (2021), supplementary 1.9.7) without its relative-position features - a
 * softmax over nbins bins of 1 / bins_per_angstrom A each, the last one open, for every (frame i, point j) of a protein, trained
 * by cross-entropy against the bin of the true aligned error of the model's own prediction (ptamd_aligned_error with K = 1, the
 * truth as the reference).  Not in the reference.
 *   uv [B*L, lduv] in: row b * L + i holds u_i (the frame side) in the columns 0 .. H-1 and v_i (the point side) in H .. 2H-1;
 *     lduv >= 2H is a row stride in floats and the spare columns are never read.  H a multiple of 4 in 4 .. 64.
 *   w2 [nbins, H], b2 [nbins] in, 2 <= nbins <= 64.  z_ij = relu(u_i + v_j), logits_ij = w2 z_ij + b2, p the max-subtracted
 *     softmax of the pair's nbins logits, c_k = (k + 0.5) / bins_per_angstrom the centre of bin k.
 *   seq [B,L]: residue i is PRESENT when seq[i] is in 0..19, the rule of ptamd_ensemble_spread; n_b is the number of present
 *     residues and pair (i, j) is DEFINED when both are present, the diagonal included.
 *   pae [B,L,L] out: sum_k p_k c_k on every defined pair, NaN on every other and in padded rows and columns; every one of the
 *     B * L * L elements is written.
 *   stats [B,2] out: {mean, ptm}.  mean is the mean of the defined entries of pae; ptm = max over the present i of
 *     (1 / n_b) sum over the present j of sum_k p_k / (1 + (c_k / d0)^2), d0 = 1.24 cbrt(max(n_b, 19) - 15) - 1.8: the d0 of
 *     ptamd_aligned_error, but the formula APPLIED TO THE PREDICTED DISTRIBUTION and not to a mean error.  Both NaN when n_b = 0.
 *   target [B,L,L] in, or NULL.  A pair COUNTS when it is defined and its target is finite; its bin is min(nbins - 1, max(0,
 *     (int)floorf(target * bins_per_angstrom))), the product one fp32 multiply (the rule of ptamd_plddt_fwd).
 *     sums [2] out: {mean of -log p_bin over the counted pairs of the whole batch (NaN when there is none), their number}.
 *     NULL is inference: sums and the workspace may be NULL and nothing but pae and stats is written.
 *   ptamd_pae_head_bwd: with g_ijk = coef / sums[1] * (p_k - [k == bin_ij]) on the counted pairs and 0 elsewhere,
 *     db2 = sum g, dw2[k,h] = sum_ij g_ijk z_ijh, dz_ij = w2^T g_ij masked by z_ijh > 0 (the derivative at exactly 0 is 0),
 *     du_i = sum_j dz_ij into duv[:, :H], dv_j = sum_i dz_ij into duv[:, H:2H].  All B * L * ldd floats of duv (ldd >= 2H) are
 *     written: the spare columns, absent residues and padding are exactly +0 (whatever the sign of coef), and so is everything
 *     when sums[1] is 0.  sums is
 *     what ptamd_pae_head_fwd left, read on the device (no host synchronisation).  dw2 and db2 are overwritten.
 * Logits are formed pair by pair and formed again in the backward pass: nothing of size L * L * nbins or L * L * H is stored.
 * The workspace (ptamd_pae_head_workspace_bytes, a function of (B, L, H, nbins) only, the larger of the two passes' needs) holds
 * a 32-byte record per residue in the forward pass and, in the backward pass, partial sums of dv, dw2 and db2 per (protein, one
 * of a fixed number of frame slabs): it grows with B * L * H, not with L^2.  fp32 products and softmax; the sums along j of a
 * row of pae, of the pTM term and of the cross-entropy are fp64 in the order j = 0 .. L-1, the rows and then the proteins are
 * added in fp64 in index order and every result is rounded to fp32 once; the gradient partials are fp32 and are added in fp64 in
 * index order.  No atomics, no order-dependent reduction: two calls give the same bits, and pae and stats of a protein depend
 * neither on the batch around it nor on how far its row is padded.  B or L <= 0, B beyond 65535 or B * L beyond INT_MAX (what one
 * launch addresses), H outside 4 .. 64 or no multiple of 4, nbins outside 2 .. 64, lduv or ldd below 2H, bins_per_angstrom not
 * finite and positive, a NULL array that the call would read or write: PTAMD_ERR_BAD_SHAPE (a size of 0); where the call uses a
 * workspace (the backward pass, the forward pass with a target), one that is NULL or too small: PTAMD_ERR_WORKSPACE, not 16-byte
 * aligned: PTAMD_ERR_ALIGN; nothing is launched or written then.  Nothing is allocated, no state between calls, nothing read
 * from the environment. */
size_t ptamd_pae_head_workspace_bytes(int B, int L, int H, int nbins);
int ptamd_pae_head_fwd(const float *uv, int lduv, const float *w2, const float *b2, const int64_t *seq, const float *target, int B,
                       int L, int H, int nbins, float bins_per_angstrom, float *pae, float *stats, float *sums, void *workspace,
                       size_t workspace_bytes, void *stream);
int ptamd_pae_head_bwd(const float *uv, int lduv, const float *w2, const float *b2, const int64_t *seq, const float *target, int B,
                       int L, int H, int nbins, float bins_per_angstrom, const float *sums, float coef, float *duv, int ldd,
                       float *dw2, float *db2, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ encoder building blocks
 * Row-major fp32 GEMM on the matrix cores (the `arith` field selects the arithmetic, see PTAMD_GEMM_* below):
 *     C[M,N] = epilogue( A (*) B )          with reduction length K
 *   a_kmajor = 0: A is [M,K] (K contiguous, lda);  1: A is stored [K,M] (M contiguous, lda)
 *   b_kmajor = 0: B is [N,K] (K contiguous, ldb) - the torch.nn.Linear weight layout;
 *              1: B is stored [K,N] (N contiguous, ldb)
 * epilogue, in order: + bias[N] (may be NULL); ReLU if (flags & PTAMD_EPI_RELU);
 *   dropout(p, seed, stream_id) if p > 0;  + residual[M,N] (ldr; may be NULL), or the ReLU/dropout gate of
 *   PTAMD_EPI_GATE;  tanh if (flags & PTAMD_EPI_TANH).
 * A leading dimension may exceed the extent of its rows (what lies between is neither read into the result nor written) but not
 * fall short of it: lda, ldb, ldc or (with a residual) ldr - and `ld` of ptamd_hp_split / a split job - smaller than the row it
 * strides is PTAMD_ERR_BAD_SHAPE in ptamd_gemm, ptamd_gemm_group, ptamd_gemm_hp and the hp split entry points; nothing is launched.
 * Replaces torch.nn.Linear (Attention.py:49,69; Sublayers.py:34; encoder_only.py:39)
 * and their autograd backward GEMMs. */
#define PTAMD_EPI_RELU 1
#define PTAMD_EPI_TANH 2
#define PTAMD_EPI_ACCUM 4 /* C += result (used for split reductions) */
#define PTAMD_EPI_SLABS 16 /* split_k > 1 only, plain epilogue only (no bias / residual / activation / dropout / colsum): the K
                            * slices' partial products stay in `workspace` as [splits][M][N] fp32 and NO reduction is launched -
                            * the caller sums them in slab order in the kernel that reads the product next
                            * (ptamd_layernorm_bwd_dropout: dy_slabs; ptamd_layernorm_fwd_sum).  C is not written; with an
                            * effective split of 1 (K of one or two 32-blocks) the flag is ignored and C is. */
#define PTAMD_EPI_GATE 8  /* result = residual[m,n] > 0 ? result * gate_scale : 0 - the backward of ReLU + dropout through
                            the saved activation (Sublayers.py:34), instead of adding `residual` */
typedef struct {
  int M, N, K;
  const float *A; int lda; int a_kmajor;
  const float *B; int ldb; int b_kmajor;
  float *C; int ldc;
  const float *bias;
  const float *residual; int ldr;
  int flags;
  float dropout_p; uint64_t seed; uint32_t stream_id;
  int split_k;            /* >1: partials go to workspace and are reduced deterministically */
  void *workspace; size_t workspace_bytes;
  float *colsum;          /* optional, a_kmajor only: colsum[m] += sum_k A[k][m] (the bias gradient of a dW product) */
  float gate_scale;       /* PTAMD_EPI_GATE: 1 / (1 - p) of the dropout that followed the ReLU */
  int arith;              /* PTAMD_GEMM_* below: the arithmetic of THIS call (the library keeps no mode of its own) */
  int reserved_cus;       /* the persistent kernels leave this many CUs free, e.g. for an RCCL all-reduce of the layer above
                             that runs beside the backward GEMMs under data parallelism; 0 = take every CU */
  /* F16X2 arithmetic only, optional: the row scales of the operands (uint32 bits of a power of two s with
   * max |x_row| * s < 2^15, see PTAMD_GEMM_F16X2) when the caller already has them - written by the kernel that
   * produced the operand (ptamd_layernorm_fwd, ptamd_layernorm_bwd_dropout) or derived from a bound of the row maxima
   * (ptamd_weight_scales, ptamd_bound_scales).  NULL: ptamd_gemm finds them with a pass over the operand (needs the workspace).
   * a_scale_stride / b_scale_stride: 1 = one scale per operand row (A: per m, B: per n); 0 = ONE scale for every row of
   * the operand - the array then holds FOUR copies of it (row-contiguous operands load the scales of four rows at once).
   * With uniform scales on both sides the weight-gradient products (k-major A and B) can run in F16X2 without any pass:
   * the error is then relative to the largest row of the operand (norm-wise over the whole product). */
  const uint32_t *a_scale; int a_scale_stride;
  const uint32_t *b_scale; int b_scale_stride;
  /* PTAMD_EPI_GATE from ONE BIT per element instead of the [M, N] fp32 activation (exactly one of `residual` and
   * `gate_mask` with that flag): what ptamd_gemm_hp wrote through `gate_mask_out` when it produced the activation
   * (ptamd_gate_mask_bytes(M, N) bytes).  F16X2 arithmetic (AUTO resolves to it for K-contiguous A), float4 epilogue (N, ldc % 4 == 0, C 16-byte
   * aligned), split_k <= 1 and dropout_p == 0 only - PTAMD_ERR_BAD_SHAPE otherwise.  Same result, bit for bit, as gating by the activation. */
  const uint64_t *gate_mask;
} ptamd_gemm_args;
/* Layout of the 1-bit gate of an [M, N] activation: entry ((cb * ceil(M / 32) + rb) * 16 + r), one uint64 = the 64 lane
 * decisions of accumulator register r of the 32 x 32 block (rb, cb) of v_mfma_f32_32x32x*: bit l set <=> element
 * (row 32 rb + (r & 3) + 8 (r >> 2) + 4 (l >> 5), column 32 cb + (l & 31)) is > 0.  The producing epilogue stores the
 * ballots of its compares, the gated epilogue reads them as scalar loads and selects with them: 4 MB instead of 134 MB per
 * layer for the hidden layer of the feed-forward block at 32 x 512 tokens (Sublayers.py:28-34, ReLU + dropout). */
size_t ptamd_gate_mask_bytes(int M, int N);
size_t ptamd_gemm_workspace_bytes(int M, int N, int split_k);
int ptamd_gemm(const ptamd_gemm_args *args, void *stream);

/* Arithmetic of a ptamd_gemm call (`arith` field of its arguments; the library holds no process-wide mode - two
 * models, or two streams, may use different arithmetics side by side).  The reference computes its Linear layers in fp32 (torch.nn.Linear on fp32 tensors); all modes take and
 * return fp32 and accumulate in fp32:
 *   PTAMD_GEMM_F32          v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf chain over k (157 TF/s peak).
 *   PTAMD_GEMM_BF16X3       every f32 operand is split EXACTLY into three bf16 terms x = x1 + x2 + x3 (round to nearest
 *                           at each level: 3 x 8 significand bits = the 24 of an f32) while it is staged into LDS, and
 *                           x*y is evaluated on the bf16 matrix pipe (v_mfma_f32_32x32x16_bf16, f32 accumulate) as the
 *                           six products x1y1 + x1y2 + x2y1 + x1y3 + x2y2 + x3y1.  The three dropped terms are below
 *                           2^-23 |x y| and unbiased, so the result is at least as close to the exact dot product as the
 *                           fp32 fma chain is (asserted against fp64 in tests/test_gpu_kernels.py), at 6/16 of the
 *                           matrix-pipe cost.
 *   PTAMD_GEMM_BF16X3_FULL  all nine products.
 *   PTAMD_GEMM_F16X2        every operand row (A: per m, B: per n) is scaled by the power of two that takes its largest
 *                           |x| into [2^14, 2^15) - found by a pass over the operands in front of the product, kept in
 *                           the workspace - and split into TWO f16 terms (2 x 11 significand bits); x*y is the three
 *                           products x1y1 + x1y2 + x2y1 on v_mfma_f32_32x32x16_f16 and the scales are taken out of the
 *                           f32 accumulators before the epilogue.  Half the matrix-pipe work of BF16X3.  The error is
 *                           fp32-grade in the NORM-WISE sense: an element keeps 22 bits down to 2^-18 of its row's
 *                           maximum and an absolute 2^-39 of that maximum below, so
 *                               |error| <= 2^-20 sum|x||y| + 2^-36 K max|x_row| max|y_col|     (worst case)
 *                           - on the tensors of the training step (rows spanning a few binades) it measures slightly
 *                           BELOW the fp32 fma chain (4e-7 vs 6e-7 max, 4e-8 vs 7e-8 rms in units of sum|x||y|), for
 *                           rows spanning 40 binades it does not (tests/test_gpu_kernels.py shows both).  A row of
 *                           subnormals only is flushed to zero.  Needs the workspace also when split_k <= 1.
 *   PTAMD_GEMM_AUTO         per call: F16X2 when A is K-contiguous (activations / per-token gradients x weights: the
 *                           pass over the operands is cheap next to the product), BF16X3 when A is k-major (the
 *                           weight-gradient reductions over all tokens, where that pass would read both big operands
 *                           once more).  Measured on the benchmark step: 15.0 ms against 15.8 (all BF16X3) and 15.25
 *                           (all F16X2); gradients of a whole step against fp64: same level in every mode
 *                           (tests/test_gpu_model.py).
 * Whatever the mode, products with K < 16 or an operand of 4 GiB or more run in PTAMD_GEMM_F32. */
#define PTAMD_GEMM_F32 0
#define PTAMD_GEMM_BF16X3 1
#define PTAMD_GEMM_BF16X3_FULL 2
#define PTAMD_GEMM_F16X2 3
#define PTAMD_GEMM_AUTO 4
/* matrix-pipe products per fp32 product that ptamd_gemm would use for these arguments (shapes, layouts, `arith`):
 * 1 (F32), 3 (F16X2), 6 (BF16X3), 9 (BF16X3_FULL); host only, nothing is launched */
int ptamd_gemm_products(const ptamd_gemm_args *args);
/* Up to four INDEPENDENT weight-gradient products in ONE launch (+ one launch for all their split-K reductions): the four
 * dW = dy^T x of an encoder layer (autograd of the nn.Linear layers of Attention.py:49,69 and Sublayers.py:28-34), whose
 * output matrices are too few tiles to fill the chip one by one.  The work items (256 x 128 tile, K split) of the members
 * are concatenated and dealt out in contiguous ranges, so the launch is balanced when the members' K per split agree (four
 * members with 96 tiles and split_k = 8: three items per CU).  Same results, bit for bit, as ptamd_gemm called on each member
 * with the same split_k.  Every member must be: a_kmajor and b_kmajor, PTAMD_GEMM_F16X2 with a_scale and b_scale given,
 * split_k >= 2 with its own workspace (ptamd_gemm_workspace_bytes), flags == PTAMD_EPI_ACCUM and no other epilogue, N and ldc
 * multiples of 4, C 16-byte aligned, colsum in all members or in none - PTAMD_ERR_BAD_SHAPE otherwise (nothing is launched). */
int ptamd_gemm_group(const ptamd_gemm_args *args, int n, void *stream);

/* ------------------------------------------------------------------ pre-split ("half-pair", hp) operands
 * An fp32 matrix [rows, K] stored as TWO f16 planes + one power-of-two scale per row, x * scale = hi + lo to 22 bits (the
 * PTAMD_GEMM_F16X2 arithmetic with the splitting done once by the WRITER of the operand instead of by every GEMM that
 * reads it).  4 bytes per element; 32 x 16 blocks that are byte-for-byte the LDS image of an MFMA operand, so that the
 * GEMM fills its stages by LDS-DMA without touching the vector ALU (layout: csrc/hp_format.h).  rows / K are zero padded
 * to multiples of 32.
 *   ptamd_hp_bytes        size of the planes buffer;  ptamd_hp_padded_rows  length of the scale array
 *   ptamd_hp_split        x [rows, K] (ld; transposed != 0: x is stored [K, rows] and the operand is its transpose)
 *                         -> planes, scale.  Row maximum pass + write pass.
 *   ptamd_gemm_hp         C[M,N] = epilogue(A B^T), A = hp [M,K], B = hp [N,K]; same epilogue, flags, dropout masks and
 *                         split-K convention as ptamd_gemm.  Replaces the same torch.nn.Linear forward / dX products
 *                         (Attention.py:49,69; Sublayers.py:34; encoder_only.py:39). */
size_t ptamd_hp_bytes(int rows, int K);
int ptamd_hp_padded_rows(int rows);
int ptamd_hp_split(const float *x, int ld, int rows, int K, int transposed, void *planes, float *scale, void *stream);
/* ptamd_hp_split_rows: up to 16 K-contiguous matrices [rows, K] (K % 4 == 0, K <= 2048) -> planes + scales in ONE launch
 * (one wavefront per row: maximum, scale, split): the weight matrices of a model once per step. */
typedef struct {
  const float *x; int ld, rows, K;
  void *planes; float *scale;
} ptamd_hp_split_job;
int ptamd_hp_split_rows(const ptamd_hp_split_job *jobs_host, int njobs, void *stream);
/* ptamd_hp_split_cols: up to 16 ROW-contiguous matrices x [K, rows] (row stride ld) -> the planes of their TRANSPOSES (operand
 * rows = the columns of x: the weights as B operands of the dX products dy W, Sublayers.py:28-34 backward) in ONE launch,
 * with the operand rows' scales GIVEN in `scale` (an INPUT here: floats that are powers of two, e.g. the column scales
 * ptamd_weight_scales wrote, reinterpreted). */
int ptamd_hp_split_cols(const ptamd_hp_split_job *jobs_host, int njobs, void *stream);
typedef struct {
  int M, N, K;
  const void *A; const float *A_scale;
  const void *B; const float *B_scale;
  float *C; int ldc;
  const float *bias;
  const float *residual; int ldr;
  int flags;
  float dropout_p; uint64_t seed; uint32_t stream_id;
  int split_k;
  void *workspace; size_t workspace_bytes;
  float gate_scale;
  int reserved_cus;
  const uint64_t *gate_mask;   /* PTAMD_EPI_GATE from the 1-bit gate (see ptamd_gemm_args.gate_mask) */
  uint64_t *gate_mask_out;     /* optional: the 1-bit gate "result > 0" of THIS product's output (after bias / ReLU /
                                  dropout), ptamd_gate_mask_bytes(M, N) bytes; float4 epilogue and split_k <= 1 only */
  /* optional, the QKV product (Attention.py:49): columns kv_col0 .. N - 1 = K then V, kv_heads heads of 64 columns each
   * (N == kv_col0 + 128 kv_heads), leave the epilogue as the pre-split planes the f16x2 attention kernels read
   * (ptamd_attention_kv_bytes / _kv_inv_floats; csrc/kv_format.h) INSTEAD of fp32 - C[:, kv_col0:] is not written; columns in
   * front (Q) are stored as usual.  M a multiple of 32, bias only (flags 0, no dropout / residual / gate), split_k <= 1. */
  void *kv_planes; float *kv_inv; int kv_col0, kv_heads;
} ptamd_gemm_hp_args;
size_t ptamd_gemm_hp_workspace_bytes(int M, int N, int split_k);
int ptamd_gemm_hp(const ptamd_gemm_hp_args *args, void *stream);

/* ------------------------------------------------------------------ f16x2 bookkeeping without passes over activations
 * (csrc/scales.hip).  Scales are uint32 bit patterns of powers of two, as ptamd_gemm_args.a_scale / b_scale take them.
 * ptamd_weight_scales: for each job (a weight matrix or a sub-matrix / vector of the flat parameter buffer,
 *   w [rows, cols], row stride ld): row_scale[rows] (B operand of x W^T), col_scale[cols] (B operand of dy W),
 *   stats[4] = {largest row L2 norm, largest column L2 norm, largest |w|, 0}; any output may be NULL.  Two launches for
 *   the whole list (at most 40 jobs per call).
 * ptamd_bound_scales: out = ((max|gamma| sqrt_d + |beta|_2) if a LayerNorm feeds the product else 1) * w_stats[w_stat_index]
 *   [+ max|bias|], times post_scale - an upper bound of |x W^T + b|_inf for every row x = LN(.) (Cauchy-Schwarz), or of
 *   |dy W|_inf / |dy|_2 when no LayerNorm is given; out_scale[0..3] receive the f16x2 scale of a row with that maximum (four
 *   copies, to be used with a_scale_stride / b_scale_stride = 0), out_value the bound itself (the `bound_factor` of
 *   ptamd_layernorm_bwd_dropout).
 *   ln_*_stats / w_stats / bias_stats point at stats[4] records written by ptamd_weight_scales earlier on the stream. */
typedef struct {
  const float *w; int rows, cols, ld;
  uint32_t *row_scale; uint32_t *col_scale; float *stats;
  int rows_only;          /* != 0: no column pass (stats[1] stays 0): for a big activation whose row scales / largest |x| are wanted */
} ptamd_wscale_job;
int ptamd_weight_scales(const ptamd_wscale_job *jobs_host, int njobs, void *stream);
typedef struct {
  const float *ln_gamma_stats; const float *ln_beta_stats;
  const float *w_stats; int w_stat_index;
  const float *bias_stats;
  float sqrt_d, post_scale;
  uint32_t *out_scale; float *out_value;
} ptamd_bound_job;
int ptamd_bound_scales(const ptamd_bound_job *jobs_host, int njobs, void *stream);
/* Presets of up to 8 small device buffers in ONE launch (dst[0..n) = value): the atomicMin targets of a backward pass (the
 * uniform scales of dy2 / dz1 / dyo / dqkv and the row scales of dqkv start at 0x7F000000, the largest finite power of two). */
typedef struct { uint32_t *dst; int64_t n; uint32_t value; } ptamd_fill_job;
int ptamd_fill_u32(const ptamd_fill_job *jobs_host, int njobs, void *stream);

/* ------------------------------------------------------------------ the weights of a step in ONE pass (csrc/wprep.hip)
 * ptamd_weights_prep: what ptamd_weight_scales + ptamd_bound_scales + ptamd_hp_split_rows + ptamd_hp_split_cols compute for
 *   the weight matrices of a model (row / column f16x2 scales, statistics, weight-derived bounds, W as hp planes, W^T as hp
 *   planes) in two launches and one read of the weights; same bits.
 * ptamd_sgd_step_prep / ptamd_adam_step_prep: ptamd_sgd_step / ptamd_adam_step (clip + optimizer.step(), train.py:41-46,
 *   371-381) that leave all of that behind for the NEXT forward pass, in the pass that writes the weights anyway.
 * The description of the model is a PLAN whose tables live in DEVICE memory (built once by the caller):
 *   segs        the listed matrices (or vectors, rows = 1) of the flat parameter buffer, K-contiguous, row stride = cols,
 *               cols % 4 == 0 and cols <= 512 (wider ones as column panels, see rowmax_index); pairwise disjoint;
 *               statistics entry [0] (largest row norm) of a panelled matrix is NOT computed (it stays 0): no bound job reads it;
 *   blocks_a    [nblocks_a][2] int32: (segment, block of 32 rows inside it) for the first nblocks_a_matrices entries, then
 *               (-(range + 1), block of ptamd_wprep_plain_floats_per_block() floats inside plain range `range`): the plain
 *               ranges [nplain][2] int64 (first element, elements) cover everything that is not a segment - segments + plain
 *               ranges partition [0, numel);
 *   blocks_b    [nblocks_b][4] int32: (0, segment, block of 2048 columns, 0) column scales; (1, segment, block of 256 16-byte
 *               chunks of its col_planes, 0); (2, bounds group, 0, 0); (3, panelled matrix, block of 256 rows, 0) row scales;
 *   bounds / groups [ngroups][4] int32 (first bound job, jobs, first entry of colnorm_segs, entries): a group = an encoder layer;
 *               a bound job is ptamd_bound_job with indices instead of pointers (statistics record, entry of `scales`, entry of
 *               `values`; -1 = none);
 *   scales      uint32 row / column / bound scales; values: floats (bound values); colmax [2][ncolmax], stats [2][nstats][4]:
 *               zeroed ONCE by the caller, `parity` (0 / 1) must alternate from call to call on a plan; colsq: column
 *               sum-of-squares partials in fp64, [(rows + 31) / 32][cols] doubles per segment that asks for them (16-byte
 *               aligned; colsq_index counts doubles). */
typedef struct {
  int64_t offset;              /* first element in the flat parameter buffer */
  int32_t rows, cols;
  int32_t stats_row0;          /* rows >= stats_row0 enter the statistics (a sub-matrix: W_v inside W_qkv) */
  int32_t stats_index;         /* record of `stats` {largest row L2 norm, largest column L2 norm, largest |w|, -}, or -1 */
  int32_t row_scale_index;     /* first entry of `scales` for the rows' scales, or -1 */
  int32_t col_scale_index;     /* ... for the columns' scales, or -1 (then no column work at all) */
  int32_t colmax_index;        /* first entry of this matrix's columns in a copy of `colmax` */
  int32_t colsq_index;         /* first double of its partials in `colsq` (the column NORM is wanted: statistics [1]), or -1 */
  uint64_t row_planes;         /* device pointer: W as hp planes (ptamd_hp_bytes(rows, cols)) split with the row scales; rows and
                                  cols multiples of 32; 0 = none */
  uint64_t col_planes;         /* device pointer: W^T as hp planes (ptamd_hp_bytes(cols, rows)) split with the column scales; 0 = none */
  int32_t ld;                  /* row stride in floats (= cols for a whole matrix) */
  int32_t rowmax_index;        /* >= 0: this segment is a COLUMN PANEL (<= 512 columns) of a wider matrix - kernel A keeps whole rows
                                  in registers, 512 columns at most: its row maxima go by atomicMax to colmax[rowmax_index + r] (the
                                  pool of maxima is shared), the row scales come from a block (3, full matrix, .) of kernel B, where
                                  the full matrix is a segment of its own that blocks_a does not list (row_scale_index, rowmax_index,
                                  rows; col_planes with colmax_index = its first panel's); a panel has stats_row0 = -1: its
                                  statistics are the maximum only.  -1: not a panel */
} ptamd_wprep_seg;
typedef struct {
  int32_t ln_gamma_stats, ln_beta_stats, w_stats, w_stat_index, bias_stats;   /* w_stats = -1: factor 1 (the bound of the input row) */
  float sqrt_d, post_scale;
  int32_t out_scale, out_value;
} ptamd_wprep_bound;
typedef struct {
  const ptamd_wprep_seg *segs; int32_t nsegs;
  const int32_t *blocks_a; int32_t nblocks_a, nblocks_a_matrices;
  const int64_t *plain; int32_t nplain;
  const int32_t *blocks_b; int32_t nblocks_b;
  const ptamd_wprep_bound *bounds; int32_t nbounds;
  const int32_t *groups; int32_t ngroups;
  const int32_t *colnorm_segs;
  uint32_t *scales; float *values;
  uint32_t *colmax; int32_t ncolmax;
  void *colsq;
  float *stats; int32_t nstats;
  int64_t numel;               /* floats in the flat parameter buffer */
  int32_t with_planes;         /* this call writes the row_planes / col_planes of the segments (0: scales and bounds only -
                                  what a pass needs whose products do not run on ptamd_gemm_hp) */
} ptamd_wprep_plan;
int ptamd_wprep_rows_per_block(void);
int ptamd_wprep_plain_floats_per_block(void);
int ptamd_weights_prep(const ptamd_wprep_plan *plan_host, const float *w, int parity, void *stream);
/* zero_grad != 0 (here and in ptamd_sgd_step / ptamd_adam_step): g is zeroed behind its last read - the `optimizer.zero_grad()`
 * of the NEXT step (train.py:37) in the pass that streams g anyway instead of a 76 MB fill of its own. */
int ptamd_sgd_step_prep(const ptamd_wprep_plan *plan_host, int parity, float *w, float *g, int64_t n, const float *sqnorm,
                        float max_norm, float lr, float weight_decay, int zero_grad, void *stream);
int ptamd_adam_step_prep(const ptamd_wprep_plan *plan_host, int parity, float *w, float *g, float *m, float *v, int64_t n,
                         const float *sqnorm, float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay,
                         int step, int zero_grad, void *stream);

/* torch.nn.LayerNorm(D, eps=1e-5) (Sublayers.py:13,17): y = (x-mean)*rstd*gamma+beta; saves mean,rstd [T];
 * row_scale [T] (may be NULL): the f16x2 scale of every row of y, for the GEMM that reads y as its A operand;
 * planes (may be NULL; needs row_scale and D % 32 == 0): y once more in the pre-split hp format (ptamd_hp_bytes(T, D)
 * bytes), scaled by row_scale - the A operand of ptamd_gemm_hp for the product behind the LayerNorm (QKV, FFN layer 1) */
int ptamd_layernorm_fwd(const float *x, const float *gamma, const float *beta, int64_t T, int D, float *y,
                        float *mean, float *rstd, uint32_t *row_scale, void *planes, void *stream);
/* Round 6: the same LayerNorm behind a split product whose K slices were left unreduced (PTAMD_EPI_SLABS; FFN layer 2 at few
 * tokens): the rows are first made here - x_out = residual + dropout(sum of the n_slabs (2 ... 4) [T, D] slabs, slab_stride
 * floats apart, in slab order + bias) with the decisions of the product's own epilogue (dropout_p, seed, stream_id as
 * ptamd_gemm_args; Sublayers.py:16-17) - and normalised from registers: the bits of the reduction launch + ptamd_layernorm_fwd,
 * one launch fewer.  residual / x_out [T, D] dense, D <= 512. */
int ptamd_layernorm_fwd_sum(const float *slabs, int n_slabs, int64_t slab_stride, const float *bias, const float *residual,
                            float dropout_p, uint64_t seed, uint32_t stream_id, float *x_out, const float *gamma,
                            const float *beta, int64_t T, int D, float *y, float *mean, float *rstd, uint32_t *row_scale,
                            void *planes, void *stream);
/* dx [T,D] = LN'(dy) + dres (dres: gradient of the residual branch, may be NULL; dx may alias dres);
 * dgamma, dbeta [D] accumulated (+=) through fixed-order partials in workspace */
size_t ptamd_layernorm_bwd_workspace_bytes(int D);
/* dgamma == dbeta == NULL in the two calls below: the kernel leaves its fixed-order partial sums in `workspace` and the caller
 * finishes up to 16 such sites with ONE launch of ptamd_layernorm_bwd_reduce (dgamma / dbeta += their column sums) - e.g.
 * both LayerNorms of an encoder layer, or all of a backward pass; every pending site needs a workspace of its own. */
typedef struct { const void *partials; int D; float *dgamma; float *dbeta; } ptamd_ln_reduce_job;
int ptamd_layernorm_bwd_reduce(const ptamd_ln_reduce_job *jobs_host, int njobs, void *stream);
int ptamd_layernorm_bwd(const float *dy, const float *x, const float *gamma, const float *mean, const float *rstd,
                        const float *dres, int64_t T, int D, float *dx, float *dgamma, float *dbeta, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ptamd_layernorm_bwd fused with the dropout backward that follows it in the encoder (SublayerConnection: x + drop(f(LN(x))),
 * Sublayers.py:17): dx as above, and `dropped` [T,D] = dx * mask / (1 - p) with the mask the GEMM epilogue drew for
 * (seed, stream_id) - what ptamd_dropout_bwd would make of dx (dropout_p = 0: dropped is not written, it equals dx).
 * Also, for the GEMMs that read `dropped` as their A operand: row_scale [T] = its f16x2 row scales, and bound_scale [T] =
 * the scale of a row bounded by |dropped[t]|_2 * *bound_factor (device scalar, e.g. from ptamd_bound_scales): the scale of
 * row t of dropped W.  row_scale_min[0..3] / bound_scale_min[0..3] (may be NULL): the smallest of those scales over all
 * rows, i.e. the scale of the largest row - atomicMin into four copies that the caller preset to 0x7F000000; the uniform
 * scale of `dropped` / `dropped W` as an operand of a weight-gradient product.  dropped_planes (may be NULL; needs row_scale,
 * D % 32 == 0): `dropped` a second time in the pre-split hp format (ptamd_hp_bytes(T, D) bytes) with the scales of
 * row_scale - the A operand of ptamd_gemm_hp for the dX product behind it.  Any of the outputs may be NULL.  D <= 1024.
 * dy_slabs (1 ... 4; round 6): dy is the SUM of that many [T, D] slabs, dy_slab_stride floats apart - the K slices of a split
 * product left unreduced (PTAMD_EPI_SLABS) - added in slab order while the rows are read: the bits of the reduction launch it
 * replaces, at a fraction of that launch's cost for the few tokens at which products are split (D <= 512 for dy_slabs > 1). */
int ptamd_layernorm_bwd_dropout(const float *dy, const float *x, const float *gamma, const float *mean, const float *rstd,
                                const float *dres, int64_t T, int D, float dropout_p, uint64_t seed, uint32_t stream_id,
                                float *dx, float *dropped, uint32_t *row_scale, const float *bound_factor,
                                uint32_t *bound_scale, uint32_t *row_scale_min, uint32_t *bound_scale_min,
                                void *dropped_planes, float *dgamma,
                                float *dbeta, int dy_slabs, int64_t dy_slab_stride, void *workspace, size_t workspace_bytes,
                                void *stream);

/* Embeddings * sqrt(D) and the doubled positional add of Encoder.py:30 + Sublayers.py:59-62,72:
 *   x0 = emb[seq]*sqrt(D); out = drop2(x0 + drop1(x0 + pe[pos]))      (eval: 2*x0 + pe) */
int ptamd_embed_fwd(const int64_t *seq, const float *emb, const float *pe, int B, int L, int D, float dropout_p,
                    uint64_t seed, float *out, void *stream);
/* demb [22,D] += scatter of dout with the same dropout masks (fixed-order partial tables in workspace) */
size_t ptamd_embed_bwd_workspace_bytes(int D);
int ptamd_embed_bwd(const int64_t *seq, const float *dout, int B, int L, int D, float dropout_p, uint64_t seed,
                    float *demb, void *workspace, size_t workspace_bytes, void *stream);

/* Fused masked multi-head attention (Attention.py:14-22,55-69), scores never materialised.  `arith` (head sizes 64
 * and 32; head size 128 has f16x2 and exact-f32 kernels, its bf16x3 requests run the exact-f32 ones; head sizes 8 and 16
 * always run the exact-f32 kernels):
 *   PTAMD_GEMM_F32                 the exact-f32 MFMA kernels;
 *   PTAMD_GEMM_BF16X3 / _FULL      operands split exactly into three bf16 terms, six products on the bf16 matrix pipe;
 *   PTAMD_GEMM_F16X2 / _AUTO       operands scaled by powers of two and split into two f16 terms, three products on the
 *                                  f16 matrix pipe (the f16x2 error model of ptamd_gemm: relative to the largest element of
 *                                  a scaling group - one Q / dO / K / V row, or four staged rows - instead of to every
 *                                  element); the scales are found inside the kernels, nothing is added to the interface.
 *   qkv [T,3D]: Q | K | V column blocks, head h at columns h*dk..; key-padding mask from seq != 20;
 *   softmax(QK^T/sqrt(dk)) with dropout p on the probabilities; out [T,D] heads merged.
 *   lse [B,H,L] saves log-sum-exp per query row for the backward. dk must be 8, 16, 32, 64 or 128.
 *   ptamd_attention_bwd, row_scale [T] / row_scale_min [4] (optional, both or only the first; f16x2 arithmetic with
 *   dk 32 / 64 / 128 only, PTAMD_ERR_BAD_SHAPE otherwise): the f16x2 row scales of dqkv (ptamd_gemm a_scale) and the smallest
 *   of them (4 copies: a uniform scale, stride 0), accumulated with atomicMin - preset both to 0x7F000000.
 *   keep_bits (optional, f16x2 arithmetic with dk 32 / 64 / 128 only, PTAMD_ERR_BAD_SHAPE otherwise;
 *   ptamd_attention_keep_bits_bytes bytes): the dropout decisions of the probabilities, written by ptamd_attention_fwd and handed to ptamd_attention_bwd by
 *   the caller (the library keeps nothing between calls), so that the backward kernel reads one word per key and 32
 *   queries instead of drawing the counter hash again: word [(b, h)][q / 32][key] (keys padded to a multiple of 32),
 *   bit q % 32 = 1 where query q keeps key.  The decisions are the generator's (csrc/attn_dropout.h) either way: a
 *   backward call without them, or in another arithmetic, regenerates exactly the same mask.
 *   kv_planes / kv_inv (optional, both or none; f16x2 arithmetic and shapes for which ptamd_attention_reads_kv_planes says 1,
 *   PTAMD_ERR_BAD_SHAPE otherwise): K and V PRE-SPLIT, as the epilogue of the QKV product wrote them (ptamd_gemm_hp_args.kv_planes;
 *   ptamd_attention_kv_bytes(T, H) bytes and ptamd_attention_kv_inv_floats(T, H) floats, T = B L; layout: csrc/kv_format.h).
 *   The K | V columns of `qkv` are then NOT read (they need not have been written); Q is.  The forward result is bit for bit
 *   that of the call without planes on the fp32 K / V the planes were made from; the backward one differs by rounding (a key
 *   row is scaled with its group of four there instead of on its own). */
int ptamd_attention_fwd(const float *qkv, const int64_t *seq, int B, int L, int H, int dk, float dropout_p,
                        uint64_t seed, uint32_t stream_id, int arith, float *out, float *lse, uint32_t *keep_bits,
                        const void *kv_planes, const float *kv_inv, void *stream);
int ptamd_attention_bwd(const float *qkv, const int64_t *seq, const float *out, const float *dout, const float *lse,
                        int B, int L, int H, int dk, float dropout_p, uint64_t seed, uint32_t stream_id, int arith,
                        float *dqkv, uint32_t *row_scale, uint32_t *row_scale_min, const uint32_t *keep_bits,
                        const void *kv_planes, const float *kv_inv, void *workspace, size_t workspace_bytes, void *stream);
size_t ptamd_attention_kv_bytes(int T, int H);
size_t ptamd_attention_kv_inv_floats(int T, int H);
/* 1 when ptamd_attention_fwd / _bwd of this shape and arithmetic read pre-split K / V (head size 64, L a multiple of 32, a batch
 * large enough for the 256-query forward kernel and the one-sweep backward kernel) */
int ptamd_attention_reads_kv_planes(int B, int L, int H, int dk, int arith);
/* Workspace of ptamd_attention_bwd: delta [B, H, L] and, behind it, the slabs of the SPLIT one-sweep backward kernel where this
 * shape takes it (round 6; head size 64 and at most half as many (protein, head) pairs as CUs - the per-GPU share of a strongly
 * scaled batch): the sweep runs as one workgroup per (pair, 256-key block) and, while that leaves CUs without one, per range of
 * query tiles as well; a key block's contribution to dQ goes to slab [key block][B L][D], a query range's dK | dV to slab
 * [range][B L][2 D], one more launch sums them in a fixed order (dQ: the bits of the unsplit sweep) and finishes the row
 * scales.  32 x 512 x 8 heads: 0.5 MB (delta alone); 16 / 8 / 4 proteins: + 33.5 / 50.3 / 41.9 MB.
 * The size is a function of (B, L, H, dk), the CU count of the current device and - for head size 64 - of the measurement knob
 * PTAMD_ATTN_FUSED in the process environment (read at every call: 0 = never a one-sweep kernel, 1 = the unsplit one, 2 = the split
 * one, unset = by the number of pairs): the size query and the call must see the same value; a call that finds its workspace too
 * small for the kernel it would take returns PTAMD_ERR_WORKSPACE and launches nothing. */
size_t ptamd_attention_workspace_bytes(int B, int L, int H, int dk);
size_t ptamd_attention_keep_bits_bytes(int B, int L, int H);
/* 1 when ptamd_attention_bwd of this shape and arithmetic would read keep_bits (f16x2 arithmetic, dk 32 / 64: the one-sweep
 * kernel or the dK / dV kernel of the two-kernel path), 0 when it would draw every decision again - a caller saves the buffer then */
int ptamd_attention_bwd_reads_keep_bits(int B, int L, int H, int dk, int arith);

/* column sums: out[N] (+)= sum_t x[t,N]   (bias gradients) */
size_t ptamd_colsum_workspace_bytes(int N);
int ptamd_colsum(const float *x, int64_t T, int N, int ldx, int accumulate, float *out, void *workspace,
                 size_t workspace_bytes, void *stream);
/* elementwise backward helpers.
 *   relu_dropout_bwd: y = dropout(relu(.)) -> dx = dy * (y > 0) / (1-p)   (y > 0 iff active AND kept)
 *   tanh_bwd:         dx = dy * (1 - y*y)
 *   dropout_bwd:      dx = dy * mask / (1-p), mask regenerated from (seed, stream_id) exactly as the GEMM
 *                     epilogue drew it: 16-bit field drop_field(row) of the counter hash pt_rand4(seed, drop_call_index(row, col,
 *                     cols), stream_id) of csrc/common.h */
int ptamd_relu_dropout_bwd(const float *dy, const float *y, int64_t n, float dropout_p, float *dx, void *stream);
int ptamd_tanh_bwd(const float *dy, const float *y, int64_t n, float *dx, void *stream);
int ptamd_dropout_bwd(const float *dy, int64_t rows, int cols, float dropout_p, uint64_t seed, uint32_t stream_id,
                      float *dx, void *stream);

/* ------------------------------------------------------------------ conv-enc front end
 * torch.nn.Conv1d(C, Co, k, padding=(k-1)/2) of models/convolutional_encoder.py:92-129 as im2col + ptamd_gemm:
 *   col [T, k*Cp] = im2col(x [T, C], row stride ldx)   with Cp = C rounded up to 4 (zero padded), k odd
 *   y   [T, Co]   = col @ W2^T + bias                  W2 [Co, k*Cp] = pack(W [Co, C, k])
 *   dx = col2im(dy @ W2),  dW += unpack(dy^T @ col),  db += colsum(dy)
 * Windows never cross a protein boundary (rows are grouped in B proteins of L residues): a window slot outside its protein and
 * the channels C .. Cp-1 of col and W2 are +0.  C need not be a multiple of 4 (ldx must be, and x 16-byte aligned).
 * Spare columns are never read: C .. ldx-1 of x, the channels C .. Cp-1 of dcol and of dW2, and no row of x outside the B*L.
 * col2im writes columns 0 .. C-1 of dx only: C .. lddx-1 keep what they held.
 * PTAMD_ERR_BAD_SHAPE, with nothing launched: a count <= 0, an even k, ldx not a multiple of 4, ldx < C, lddx < C, a NULL array
 * (im2col, col2im). */
int ptamd_im2col1d(const float *x, int ldx, int B, int L, int C, int k, float *col, void *stream);
int ptamd_col2im1d(const float *dcol, int B, int L, int C, int k, float *dx, int lddx, void *stream);
int ptamd_conv_weight_pack(const float *w, int Co, int C, int k, float *w2, void *stream);
int ptamd_conv_weight_unpack_add(const float *dw2, int Co, int C, int k, float *dw, void *stream);
/* x [T, Cp] = one_hot(seq, C) (convolutional_encoder.py:110-111, use_embedding=False): x[t, c] = 1 where c == seq[t] and c < C.
 * The row of an id outside 0 .. C-1 is all zeros, and the padding columns C .. Cp-1 are zero for every id. */
int ptamd_onehot(const int64_t *seq, int64_t T, int C, float *x, void *stream);
/* y = x + dropout(x + pe[pos]), pos = t mod L, and its adjoint dx = dy (1 + keep / (1-p)) (convolutional_encoder.py:118-119 with
 * Sublayers.py:59-62).  D and n are multiples of 4; rows L .. of pe are not read.  The dropout draws from stream 0xE3 of the
 * counter hash pt_rand4 of csrc/common.h: word j of the generator call i = t*(D/4) + c/4 serves column (c & ~3) + j, and an
 * element is kept iff its word >= uint32(p * 2^32) (all 32 bits; saturating at 2^32 - 1); p <= 0 draws nothing. */
int ptamd_posenc_add_fwd(const float *x, const float *pe, int B, int L, int D, float dropout_p, uint64_t seed, float *y,
                         void *stream);
int ptamd_posenc_add_bwd(const float *dy, int64_t n, float dropout_p, uint64_t seed, float *dx, void *stream);

/* ------------------------------------------------------------------ optimizer (train.py:41-46,371-381)
 * clip_grad_norm_(params, max_norm) + SGD(lr, weight_decay) / Adam(betas, eps, weight_decay) over ONE flat
 * fp32 parameter buffer.  sqnorm: out[0] = sum g^2 (zeroed inside, deterministic two-stage reduction). */
size_t ptamd_grad_sqnorm_workspace_bytes(void);
int ptamd_grad_sqnorm(const float *g, int64_t n, float *out, void *workspace, size_t workspace_bytes, void *stream);
/* clip coefficient = min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) computed on device from sqnorm[0];
 * max_norm <= 0 disables clipping */
int ptamd_sgd_step(float *w, float *g, int64_t n, const float *sqnorm, float max_norm, float lr,
                   float weight_decay, int zero_grad, void *stream);
int ptamd_adam_step(float *w, float *g, float *m, float *v, int64_t n, const float *sqnorm, float max_norm,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step, int zero_grad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PTAMD_H */
