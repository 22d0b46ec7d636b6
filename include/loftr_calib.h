/* libloftr_calib -- C-ABI of view-graph calibration (gfx950 / CDNA4): the third shared library of this project, next to libloftr_hip
 * (include/loftr_hip.h) and libloftr_global (include/loftr_global.h), whose conventions it keeps: asynchronous on the caller's
 * stream, caller-allocated buffers, a workspace sized by *_workspace_bytes, 0 = ok and the negative loftr_status values of
 * loftr_hip.h otherwise.  It links no object of the other two libraries.
 *
 * ---- view-graph calibration: focal lengths from fundamental matrices (csrc/calib_core.h holds every step) ---------------
 * An essential matrix has two equal singular values and a zero one.  One focal-length scale per camera is chosen so that
 * K_b^T F K_a is as close to essential as possible on all edges of the view graph at once.  This is the published idea of view-graph
 * calibration (as the global pipelines GLOMAP and Theia use it) restated as an order-defined rule, NOT anybody's source.  PARITY
 * UNPINNED.  loftr_calibrate_view_graph_host (csrc/calib.hip, host memory) DEFINES the result; loftr_calibrate_view_graph
 * (csrc/calib_gpu.hip, device memory) reproduces it bit for bit.  fp64, + - * / and sqrt only, no contraction.
 *
 * Input: edge_image [E,2] i32 (a, b); edge_F [E,3,3] f64 with x_b^T F x_a = 0 in pixels; edge_weight [E] i32 (inlier counts);
 *   pp [n,2] f64, the assumed principal points; f0 [n] f64, the start focals; group [n] i32, the camera of each image, 0 .. G-1;
 *   the incidence lists of the groups in CSR form, grp_offsets [G+1] i64 over grp_inc [2E] i32: entry 2e + side (side 0 is a, 1 is b)
 *   belongs to group[edge_image[e, side]], and every list ascends (the stable grouping).  1 <= G <= n; E >= 0.
 *   Scalars: loss, max_resid, prior_weight, weight_cap (>= 1), bound_lo < 1 < bound_hi, min_edges, max_iters (trials), pcg_iters,
 *   pcg_tol, ftol.
 * Rule
 *  1. Checks.  Error bits in counts[1]; every other output is then zero and the host routine returns LOFTR_ERR_BAD_ARG:
 *       1 an edge image outside [0, n), or a == b;  2 a group outside [0, G);  4 incidence lists that are not the stable grouping
 *       (spans that do not start at 0, end at 2E and ascend; a slot whose code is outside [0, 2E), whose image's group does not own
 *       the slot, or which does not exceed the slot before it in its list);  8 an f0 that is not finite or not positive, or a pp that
 *       is not finite.
 *  2. Edges.  An edge is valid iff its weight is positive, F is finite and F' below has a positive finite norm.
 *     F' = T_b^T F T_a with T the translation by pp, written out: the third column of F T_a is (F_r0 ax + F_r1 ay) + F_r2, then the
 *     third row of T_b^T (.) is (bx M_0c + by M_1c) + M_2c; F' is divided by its Frobenius norm (the square root of the nine squares
 *     added left to right).  The data weight is w_e = min(weight, weight_cap) / weight_cap.
 *  3. Groups.  A group with at least one and at least min_edges valid incidences is free (state 2, "refined"); any other group keeps
 *     scale 1: state 1 "held" when it has a valid incidence, state 0 "no valid edge" otherwise.
 *  4. Residual.  With m_g the scale of group g and f_i = f0_i m_group(i):
 *       E = diag(f_b, f_b, 1) F' diag(f_a, f_a, 1),  t = tr(E E^T),  N = 2 E E^T E - t E,  rho = N / t^(3/2)  (nine components);
 *       |rho|^2 = ((s1^2 - s2^2) / (s1^2 + s2^2))^2 for a rank-2 E, in [0, 1], smooth in the focals.
 *     Derivative by m on side a: dE = E diag(1,1,0) / m_a; on side b: dE = diag(1,1,0) E / m_b; then with A = dE E^T
 *       dN = 2 ((A + A^T) E + E E^T dE) - 2 tr(A) E - t dE,  dt = 2 tr(A),  d rho = dN / t^(3/2) - 1.5 N dt / t^(5/2).
 *     Matrix products are (x0 y0 + x1 y1) + x2 y2 per entry; nine-term dot products add left to right.
 *  5. Cost.  sum_e w_e loss^2 q_e / (loss^2 + q_e) + prior_weight sum_free (m_g - 1)^2 with q = |rho|^2 (Geman-McClure, chosen as in
 *     DESIGN §26); the osum of DESIGN §18 over the E edge terms followed by the G group terms (0 for an invalid edge or a group that
 *     is not free).  The Gauss-Newton weight is W_e = w_e (loss^2 / (loss^2 + q_e))^2.
 *  6. Linearisation.  Five scalars per edge: h_aa = W j_a.j_a, h_ab = W j_a.j_b, h_bb = W j_b.j_b, g_a = -W j_a.rho, g_b = -W j_b.rho.
 *     A group's diagonal, right-hand side and A p are the osum64 of §18 over its incidence list in list order (accumulator k mod 64,
 *     folded 32 ... 1), which a wave reproduces lane for lane: the own term is h_ss; the cross term is h_ab p_other (0 for a group
 *     that is not free), and h_ab is added to the diagonal too when both ends lie in the group.  A free group adds prior_weight to
 *     its diagonal and -prior_weight (m_g - 1) to its right-hand side.
 *  7. Levenberg-Marquardt.  Damping is §18's: the diagonal d becomes d (1 + lambda), or lambda when d is 0.  The step solves the damped
 *     system over the free groups by Jacobi-preconditioned conjugate gradients started at 0, at most pcg_iters iterations, ended when
 *     r.z <= pcg_tol^2 (r.z)_0 or when (r.z)_0 or p.Ap is not positive; the dot products are osums over the G groups.  The trial is
 *     m + delta.  Acceptance and the lambda schedule are §18's ctrl_accept: lambda starts at 1e-4; a trial whose cost is lower is
 *     accepted, lambda / 10 (at least 1e-10), converged when the gain is at most ftol times the new cost; any other trial is rejected,
 *     lambda * 10, stalled above 1e10.  A trial that takes any free m outside (bound_lo, bound_hi) is rejected and counted, as is one
 *     that is not finite (not counted).  Nothing to do (status 3) without a valid edge or a free group.  The scalars of the solver
 *     belong to one thread.
 *  8. Output: focal_scale [G] f64; focal [n] f64 = f0 m (one multiplication); edge_resid [E] f64 = |rho| at the result, 0 for an
 *     invalid edge; edge_state [E] u8: 0 invalid, 1 ok, 2 outlier (resid > max_resid); group_state [G] u8: 0 no valid edge, 1 held,
 *     2 refined; counts [16] i64: 0 trials, 1 error bits, 2 accepted trials, 3 conjugate-gradient iterations, 4 valid edges, 5 free
 *     groups, 6 outlier edges, 7 status (0 converged, 1 max_iters, 2 stalled, 3 nothing), 8 bound rejections, 9..15 zero; info [4]
 *     f64: cost at start, cost at end, final lambda, the largest |delta| of the last accepted trial.
 * Not modelled: principal point and aspect ratio (assumed), detection of degenerate configurations beyond the prior (optical axes
 * that meet), radial distortion, per-image focal priors.  The defaults of the Python layer are a prototype's, UNVALIDATED on real
 * data. */
#ifndef LOFTR_CALIB_H_
#define LOFTR_CALIB_H_

#include "loftr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOFTR_CALIB_ABI_VERSION 1
#define LOFTR_CALIB_STAGES 4 /* check, setup, refine, write */

int loftr_calib_abi_version(void);

int loftr_calibrate_view_graph_host(const int* edge_image, const double* edge_F, const int* edge_weight, long E, const double* pp,
                                    const double* f0, const int* group, int n_images, int n_groups, const long* grp_offsets,
                                    const int* grp_inc, double loss, double max_resid, double prior_weight, int weight_cap,
                                    double bound_lo, double bound_hi, int min_edges, int max_iters, int pcg_iters, double pcg_tol,
                                    double ftol, double* focal_scale, double* focal, double* edge_resid, uint8_t* edge_state,
                                    uint8_t* group_state, long* counts, double* info);

/* The same on device memory; ws of at least loftr_calibrate_view_graph_workspace_bytes(E, n_images, n_groups) bytes (about 130 bytes
 * per edge and 90 per group).  stage_ms: null, or LOFTR_CALIB_STAGES floats on the host that receive the stage times (the call then
 * waits for the stream).  A fixed launch schedule that depends on E, n_images, n_groups, max_iters and pcg_iters only; nothing is
 * read back. */
size_t loftr_calibrate_view_graph_workspace_bytes(long E, int n_images, int n_groups);
int loftr_calibrate_view_graph(const int* edge_image, const double* edge_F, const int* edge_weight, long E, const double* pp,
                               const double* f0, const int* group, int n_images, int n_groups, const long* grp_offsets,
                               const int* grp_inc, double loss, double max_resid, double prior_weight, int weight_cap, double bound_lo,
                               double bound_hi, int min_edges, int max_iters, int pcg_iters, double pcg_tol, double ftol,
                               double* focal_scale, double* focal, double* edge_resid, uint8_t* edge_state, uint8_t* group_state,
                               long* counts, double* info, void* ws, size_t ws_bytes, float* stage_ms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LOFTR_CALIB_H_ */
