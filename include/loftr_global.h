/* libloftr_global -- C-ABI of the global reconstruction stages (gfx950 / CDNA4): the second shared library of this project, next to
 * libloftr_hip (include/loftr_hip.h), whose conventions it keeps: asynchronous on the caller's stream, caller-allocated buffers, a
 * workspace sized by *_workspace_bytes, 0 = ok and the negative loftr_status values of loftr_hip.h otherwise.  It links no object of
 * the first library.
 *
 * ---- global positioning: camera centres and points from averaged rotations (csrc/position_core.h holds every step) ------
 * With one rotation per image fixed (rotation averaging), the camera centres c_i, the points X_k and one scale d_o per
 * observation are solved together from the residual
 *     r_o = v_o - d_o (X_k - c_i),        v_o = normalise(R_i^T K_i^-1 (x, y, 1)),
 * under a Huber loss on |r_o|.  This is the published idea of global positioning (Pan et al., "Global Structure-from-Motion
 * Revisited") restated as an order-defined rule, NOT anybody's source.  PARITY UNPINNED.
 * loftr_global_positions_host (csrc/position.hip, host memory) DEFINES the result; loftr_global_positions (csrc/position_gpu.hip,
 * device memory) reproduces it bit for bit.  fp64, + - * / and sqrt only, no contraction.
 *
 * Input: the tracks in CSR form as bundle adjustment takes them: offsets [T+1] i64, obs_image [N] i32, obs_xy [N,2] f32, and the stable
 *   grouping by image cam_offsets [n+1] i64, cam_obs [N] i32; K [n,3,3] f64 (upper triangular); R [n,3,3] f64 camera-from-world;
 *   in_graph [n] u8; root; the spanning tree as tree_image [Et,2] i32 (a, b) and tree_t [Et,3] f64, the translation of the pair with
 *   x_b = R_ab x_a + t; huber (a chord, unitless; 0: the square), max_iters (trials), pcg_iters, pcg_tol, ftol, min_cam_obs.
 *   n >= 1; T == 0 needs N == 0.
 * Rule
 *  1. Checks.  Error bits in counts[1]; every other output is then zero and the host routine returns LOFTR_ERR_BAD_ARG:
 *       1 obs_image outside [0, n);  2 offsets that do not start at 0, end at N and ascend;  4 cam_offsets / cam_obs that are not the
 *       stable grouping by image;  8 root outside [0, n) or outside the graph;  16 a tree edge with an end outside [0, n) or outside
 *       the graph, or a tree that is not a tree rooted at root.  The last is decided by the levels of rule 4: every edge must join two
 *       reached images at adjacent levels, and no image may be the deeper end of two edges.
 *  2. Bearings.  K^-1 in closed form (z = 1 / k22, y' = (y - k12 z) / k11, x' = (x - k01 y' - k02 z) / k00), v = R^T (x', y', z) / |.|.
 *     An image counts as in the graph iff in_graph is set and the tree reaches it.  An observation is usable iff its image is in the
 *     graph, its pixels are finite and its bearing is finite; a point is active iff it has at least 2 usable observations; an
 *     observation is active iff it is usable and its point is active.
 *  3. Cameras.  The root is fixed at 0.  A camera of the graph with at least min_cam_obs active observations is free; any other camera
 *     of the graph is "chained only": it keeps its start value and is held fixed; its observations still count.
 *  4. Start values.  Tree edge (a, b) has gamma = -R_b^T t / |t|, the direction from a to b (0 when t is not finite or zero; these are
 *     counted).  Level by level from the root, an edge with one end set at the level before and the other not set sets it:
 *     c_b = c_a + gamma or c_a = c_b - gamma.  X_k = the mean over the point's active observations, in list order, of c_i + v_o.
 *     d_o = v.e / e.e with e = X_k - c_i, 0 when e.e = 0.
 *  5. Refinement: Levenberg-Marquardt; a trial at the state (c, X, d) with damping lambda:
 *       w_o = 1 when huber = 0 or |r_o| <= huber, else huber / |r_o|; the cost term is |r|^2, else 2 huber |r| - huber^2; the cost is
 *       the osum of the N terms (0 for an inactive observation).
 *       Damping is §18's: a diagonal entry a of J^T W J becomes a (1 + lambda), or lambda when a is 0.  Elimination order: first d_o
 *       (1 x 1: den_o = e.e (1 + lambda), or lambda when e.e is 0), which leaves W_o = w d^2 (I - e e^T / den_o) and
 *       g_o = w d (r - e (e.r) / den_o); then X_k (A_k = sum W_o + damp(sum w d^2) I, inverted through its adjugate; y_k = A_k^-1 sum g_o); then the reduced system over the free
 *       centres, (S p)_i = M_i p_i - sum_{o of i} W_o u_k with M_i = sum W_o + damp(sum w d^2) I, u_k = A_k^-1 sum_{o of k} W_o p_i, and
 *       right-hand side sum_{o of i} (W_o y_k - g_o).  It is never formed: conjugate gradients with the preconditioner M_i^-1, started
 *       at 0, at most pcg_iters iterations, ended when r.z <= pcg_tol^2 (r.z)_0, or when (r.z)_0 or p.Sp is not positive.
 *       Back-substitution: dX_k = y_k + u_k(dc); dd_o = (e.r - d e.(dX_k - dc_i)) / den_o.
 *       Acceptance and the lambda schedule are §18's: lambda starts at 1e-4; a trial whose cost is lower is accepted, lambda / 10 (at
 *       least 1e-10), and the call ends converged when the gain is at most ftol times the new cost; any other trial (a value that is
 *       not finite, a block that cannot be inverted) is rejected, lambda * 10, stalled above 1e10.  The call ends on ftol or after
 *       max_iters trials.  Nothing to do (status 3) without a free camera or an active observation.
 *  6. Sums.  A point's sums run over its observations in CSR order; a camera's sums are the osum64 of §18 over its cam_obs list (64
 *     accumulators taken in turn, folded 32, 16, ..., 1), which a wave reproduces lane for lane; the dot products over the 3n scalars
 *     and the cost use osum (osum64 per chunk of 4096, then osum of the chunk sums).  The scalars of the conjugate gradients and the
 *     flags belong to one thread.
 *  7. Output: centres [n,3] f64 (NaN outside the graph); xyz [T,3] f32 (NaN for an inactive point); depth_scale [N] f64 (0 for an
 *     observation that is not active); obs_state [N] u8 (0 unused, 1 active, 2 active but ended with d <= 0); cam_state [n] u8 (0
 *     outside, 1 chained only, 2 solved, 3 root); point_active [T] u8; counts [16] i64: 0 trials, 1 error bits, 2 accepted trials, 3
 *     conjugate-gradient iterations, 4 active observations, 5 active points, 6 free cameras, 7 observations with d <= 0, 8 tree edges
 *     without a direction, 9 status (0 converged, 1 max_iters, 2 stalled, 3 nothing), 10 the depth of the tree, 11 images in the graph,
 *     12 chained-only cameras, 13..15 zero; info [4] f64: cost before, cost after, final lambda, the largest centre step of the last
 *     accepted trial.  The scale of the result is whatever the damping left; nothing is normalised.
 * Out of scope: bounds on d, more than the root's component, camera priors, positions from pairwise translations. */
#ifndef LOFTR_GLOBAL_H_
#define LOFTR_GLOBAL_H_

#include "loftr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LOFTR_GLOBAL_ABI_VERSION 1
#define LOFTR_POSITION_STAGES 5 /* check, start, setup, refine, write */

int loftr_global_abi_version(void);

int loftr_global_positions_host(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const long* cam_offsets,
                                const int* cam_obs, const double* K, const double* R, const uint8_t* in_graph, int n_images, int root,
                                const int* tree_image, const double* tree_t, long Et, double huber, int max_iters, int pcg_iters,
                                double pcg_tol, double ftol, int min_cam_obs, double* centres, float* xyz, double* depth_scale,
                                uint8_t* obs_state, uint8_t* cam_state, uint8_t* point_active, long* counts, double* info);

/* The same on device memory; ws of at least loftr_global_positions_workspace_bytes(T, N, n_images, Et) bytes (about 130 bytes per
 * observation, 170 per point and 300 per image).  stage_ms: null, or LOFTR_POSITION_STAGES floats on the host that receive the stage
 * times (the call then waits for the stream).  A fixed launch schedule that depends on the sizes and the iteration limits only; nothing
 * is read back. */
size_t loftr_global_positions_workspace_bytes(long T, long N, int n_images, long Et);
int loftr_global_positions(const long* offsets, long T, const int* obs_image, const float* obs_xy, long N, const long* cam_offsets,
                           const int* cam_obs, const double* K, const double* R, const uint8_t* in_graph, int n_images, int root,
                           const int* tree_image, const double* tree_t, long Et, double huber, int max_iters, int pcg_iters,
                           double pcg_tol, double ftol, int min_cam_obs, double* centres, float* xyz, double* depth_scale,
                           uint8_t* obs_state, uint8_t* cam_state, uint8_t* point_active, long* counts, double* info, void* ws,
                           size_t ws_bytes, float* stage_ms, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LOFTR_GLOBAL_H_ */
