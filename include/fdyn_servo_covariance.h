/* fdyn_servo_covariance.h -- C-ABI of the LQ servo's predicted performance (csrc/servo_covariance_kernels.hip): what the designed
 * loop of every aircraft will hold on its sensors -- the steady-state variance of its state, of its estimate, of the three tracking
 * errors, of the integrators, of the controls and of their change from step to step -- without flying it.  A header of its own
 * beside fdyn_servo_margins.h ("how robust") and fdyn_servo_modes.h ("how fast"), whose conventions hold: every array is a DEVICE
 * pointer, SoA [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's,
 * and no entry point synchronises or allocates, so both can be captured into a hipGraph.
 *
 * The loop is the one fdyn_servo_lqg_step_* flies in its linear region, per block (five physical states d, n_i = 2 | 1 integrators
 * i, xi = (d, i), e = d - xhat after the update):  Acl = [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]], word for word the matrix of
 * fdyn_servo_sampled_modes and fdyn_servo_loop_margins;  Bf = [-Gamma Kx ; dt C_i];  Ae = (I - L) Phi as fdyn_servo_filter_modes
 * forms it;  V = diag sigma^2 the measurement noise the loop applies;  W = diag(s^2 dt) the process noise acting, s = w_rate.  Three
 * discrete Lyapunov / Stein equations per block (5 x 5, 7 x 5 | 6 x 5, 7 x 7 | 6 x 6: the estimate-feedback loop is block
 * triangular in (xi, e), no 12 x 12 is solved), each by Smith doubling in fp64, one lane per aircraft (csrc/fdyn_stein_n.hpp):
 *   Se = Ae Se Ae^T + (I - L) W (I - L)^T + L V L^T                                   every feedback: the estimator always runs
 *   FD_LQG_TRUTH         Sx = Acl Sx Acl^T + diag(W, 0)
 *   FD_LQG_MEASUREMENT   Sx = Acl Sx Acl^T + Bf V Bf^T + diag(W, 0)
 *   FD_LQG_ESTIMATE      Sxe = Acl Sxe Ae^T - Bf Se Ae^T + (W (I - L)^T ; 0),
 *                        Sx = Acl Sx Acl^T - Acl Sxe Bf^T - Bf Sxe^T Acl^T + Bf Se Bf^T + diag(W, 0)
 * and the variances of u = -Kb xi - Kx (f - d) and of u_k - u_{k-1} from them (the formulas: csrc/fdyn_stein_n.hpp).
 *
 * What the prediction leaves out: the loop is taken as linear at the trim; control limits, error clips and angle wraps are
 * ignored (the predicted control sigma set against the trim's distance to the limits says where that stops holding); the process
 * noise is white.                                                                                                               */
#ifndef FDYN_SERVO_COVARIANCE_H
#define FDYN_SERVO_COVARIANCE_H

#include <stdint.h>
#include "fdyn.h"
#include "fdyn_servo_lqg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of report [FD_NSCV][n]: variances.  VAR_X and VAR_EST in the estimator's word order (u, w, q, theta, z | v, p, r, phi, psi),
 * VAR_ERR and VAR_INTEG in the order (V, h, psi), VAR_U and VAR_DU in FD_U_* order */
enum { FD_SCV_VAR_X = 0, FD_SCV_VAR_EST = 10, FD_SCV_VAR_ERR = 20, FD_SCV_VAR_INTEG = 23, FD_SCV_VAR_U = 26, FD_SCV_VAR_DU = 30, FD_NSCV = 34 };
/* rows of cov [FD_NSCC][n], every matrix row-major: Se 5 x 5 of the longitudinal and the lateral block, Sxe 7 x 5 and 6 x 5
 * (zero unless FD_LQG_ESTIMATE), Sx 7 x 7 and 6 x 6 */
enum { FD_SCC_E_LON = 0, FD_SCC_E_LAT = 25, FD_SCC_XE_LON = 50, FD_SCC_XE_LAT = 85, FD_SCC_X_LON = 115, FD_SCC_X_LAT = 164, FD_NSCC = 200 };
/* status bits of both entry points; the sizes fdyn_stein_solve takes */
enum { FD_SCV_NOT_CONVERGED = 1, FD_SCV_UNSTABLE = 2, FD_SCV_BAD_INPUT = 4 };
enum { FD_SCV_MIN_N = 1, FD_SCV_MAX_N = 7 };

/* fdyn_servo_covariance: K [FD_NSVK][n] as fdyn_servo_design writes it, F [FD_NSKF][n] as fdyn_servo_kf_design writes it at this
 * dt, x0 [FD_NX][n] the trim (only its u and w words are read).
 *   sigma      [FD_NSKX] or, with sigma_per_lane != 0, [FD_NSKX][n]: the measurement noise the loop applies; it may differ from the
 *              sigma the filter was designed for
 *   w_rate     NULL (no process noise: what fdyn_servo_lqg_step_* flies), [FD_NSKX] or, with w_rate_per_lane != 0, [FD_NSKX][n]:
 *              state units per sqrt(s)
 *   feedback   FD_LQG_ESTIMATE, FD_LQG_MEASUREMENT or FD_LQG_TRUTH
 *   report     [FD_NSCV][n] (FD_SCV_VAR_*): VAR_X the variance of d; VAR_EST of xhat - d, what err_est of fdyn_servo_lqg_step_* adds
 *              per step; VAR_ERR C_i Sd C_i^T of the errors e_V, e_h, e_psi of the true state; VAR_INTEG of the integrators; VAR_U of
 *              the controls; VAR_DU of u_k - u_{k-1}, what chatter adds per step
 *   cov        or NULL; [FD_NSCC][n] (FD_SCC_*)
 *   residual   [n]: the worst relative residual max|A X B^T + Q - X| / max|X| of the equations solved, both blocks (0 for an X that
 *              is exactly 0: truth feedback without process noise); NaN where nothing was solved
 *   iters      [n] int32, or NULL; doublings of the slowest solve
 *   status     [n] int32: 0, or
 *                FD_SCV_BAD_INPUT      a word read is not finite, a sigma or a rate is not finite or < 0, dt outside (1e-6, 1],
 *                                      V0 not > 0; nothing is solved
 *                FD_SCV_UNSTABLE       Acl or Ae of a block is not certified Schur by fdyn_servo_loop_margins' squaring (the zero
 *                                      gain of a failed servo design and the pass-through filter of a failed filter design
 *                                      included); nothing is solved
 *                FD_SCV_NOT_CONVERGED  a solve reached the cap of 40 doublings, met a word that is not finite, or left a
 *                                      residual above 1e-9
 *              A lane with a non-zero status gets NaN in every word of report and cov.
 * Refusals, in this order, each with no launch and nothing written: FDYN_ERR_BAD_SIZE for n < 1, n > 2^31 - 64 or an unknown feedback,
 * FDYN_ERR_NULL for a missing required pointer (K, F, x0, sigma, report, residual, status), FDYN_ERR_BAD_DT for dt outside
 * (1e-6, 1] or not a number.                                                                                                   */
int fdyn_servo_covariance(const double* K, const double* F, const double* x0, double dt, const double* sigma, int sigma_per_lane,
                          const double* w_rate, int w_rate_per_lane, int feedback, int64_t n, double* report, double* cov,
                          double* residual, int32_t* iters, int32_t* status, void* stream);

/* fdyn_stein_solve: X = A X B^T + Q per aircraft, A [N * N][n], B [M * M][n], Q and X [N * M][n] row-major, FD_SCV_MIN_N <= N, M <=
 * FD_SCV_MAX_N: the door for matrices composed on the device.  The general loop (B is squared beside A; X is not symmetrised) and
 * no stability test first: an unstable pair overflows and answers FD_SCV_NOT_CONVERGED.
 *   residual [n], iters [n] int32   or NULL
 *   status [n] int32                0, FD_SCV_NOT_CONVERGED (the cap, a word that stopped being finite, a residual above 1e-9) or
 *                                   FD_SCV_BAD_INPUT (a word of A, B or Q is not finite; nothing is solved, residual NaN, iters 0).
 *                                   A lane with a non-zero status gets NaN in every word of X.
 * Refusals, in this order: FDYN_ERR_BAD_SIZE for n < 1, n > 2^31 - 64 or N or M outside 1 .. 7, FDYN_ERR_NULL for a missing A, B, Q, X or
 * status.                                                                                                                      */
int fdyn_stein_solve(const double* A, const double* B, const double* Q, int N, int M, int64_t n, double* X, double* residual,
                     int32_t* iters, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_COVARIANCE_H */
