/* fdyn_servo_modes.h -- C-ABI of the LQ servo's flight-mode report (csrc/servo_modes_kernels.hip): where the poles of the servo loop
 * of every aircraft are -- how fast and how well damped it is, beside fdyn_servo_design's "stable" and fdyn_servo_loop_margins' "how
 * robust".  A header of its own beside fdyn_modes.h and fdyn_servo_margins.h, whose conventions hold: every array is a DEVICE
 * pointer, SoA [word][n] row-major fp64 unless marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's, and
 * no entry point synchronises or allocates, so all can be captured into a hipGraph.
 *
 * Per aircraft real N x N matrices, 2 <= N <= 7, are solved in fp64, one lane per aircraft: Householder reduction to Hessenberg
 * form, Francis double-shift QR on an active window that shrinks from the bottom, deflation to 1 x 1 and 2 x 2 blocks (exceptional
 * shifts at sweeps 10 and 20, at most 30 sweeps per deflation), 2 x 2 blocks in closed form.  No balancing.  The only operations are
 * + - * / and sqrt, one rounding each, in a fixed order (csrc/fdyn_eig_n.hpp).
 *
 * Outputs of every entry point, with fdyn_modes.h's meanings; block 0 = longitudinal, block 1 = lateral:
 *   eig_re, eig_im          per block in canonical order: real part descending, equal real parts by |Im| descending, within a
 *                           conjugate pair the member with the positive imaginary part first; both members of a pair carry the
 *                           bit-identical real part
 *   summary                 or NULL; per block the six FD_MO_* words (fdyn_layout.h) over the block's eigenvalues
 *   iters [n] int32         or NULL; QR sweeps of the slower block
 *   status [n] int32        0, FD_MO_NOT_CONVERGED (the sweep cap or a non-finite intermediate) or FD_MO_BAD_INPUT (a word that is
 *                           read is not finite, or what the entry point names below; nothing is solved).  A lane with a non-zero
 *                           status gets NaN in every eigenvalue and summary word of BOTH blocks.
 * FDYN_ERR_BAD_SIZE for n < 1 (fdyn_square_modes: or N outside 2 .. 7) and FDYN_ERR_NULL for a missing required pointer, with no
 * launch and nothing written.                                                                                                   */
#ifndef FDYN_SERVO_MODES_H
#define FDYN_SERVO_MODES_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of eig_re / eig_im of the two servo loops: the seven longitudinal poles, then the six lateral ones; of the filter: five and
 * five; the sizes fdyn_square_modes takes */
enum { FD_SMO_LON = 0, FD_SMO_LAT = 7, FD_NSMO_EIG = 13 };
enum { FD_SMO_FILTER_LON = 0, FD_SMO_FILTER_LAT = 5, FD_NSMO_FILTER_EIG = 10 };
enum { FD_SMO_MIN_N = 2, FD_SMO_MAX_N = 7 };

/* fdyn_servo_flight_modes: the poles of the CONTINUOUS augmented closed loops a_lon - b_lon K_lon (7 x 7) and a_lat - b_lat K_lat
 * (6 x 6).  A [FD_NX * FD_NX][n], B [FD_NX * FD_NU][n] as fdyn_linearize writes them, x0 [FD_NX][n] the trim (only its u and w words
 * are read), K [FD_NSVK][n] as fdyn_servo_design writes it.  The augmented model is the one fdyn_servo_design solves: the rows and
 * columns (u, w, q, theta, z | v, p, r, phi, psi) of A, the columns (elevator, throttle | aileron, rudder) of B, and the integrator
 * rows (u0 / V0, w0 / V0, 0, 0, 0), (0, 0, 0, 0, -1) | (0, 0, 0, 0, 1), V0 = sqrt(u0^2 + w0^2).  Every element of the five physical
 * rows is a - (b_0 k_0 + b_1 k_1), a = 0.0 in the integrator columns; the integrator rows are the model's own (b is zero there).
 * Only the words inside the two blocks are read.  K is required: the open-loop augmented blocks have a defective eigenvalue 0, and
 * their non-zero poles are fdyn_flight_modes' already.  V0 not > 0: FD_MO_BAD_INPUT.
 *   eig_re, eig_im [FD_NSMO_EIG][n] (FD_SMO_*), summary [2][FD_NMO][n].  FD_MO_ABSCISSA < 0: the loop is stable.               */
int fdyn_servo_flight_modes(const double* A, const double* B, const double* x0, const double* K, int64_t n, double* eig_re,
                            double* eig_im, double* summary, int32_t* iters, int32_t* status, void* stream);

/* fdyn_servo_sampled_modes: the poles of the loop as fdyn_servo_step_* flies it in its linear region (gain through a zero-order
 * hold at dt, integrators advanced by forward Euler): per block [[Phi - Gamma Kx, -Gamma Ki], [dt C_i, I]], Kb = [Kx | Ki] from K,
 * Phi and Gamma from F [FD_NSKF][n] (FD_SKF_*; L is not read) as fdyn_servo_kf_design writes it at this dt, C_i the integrator rows
 * above.  This is word for word the matrix fdyn_servo_loop_margins certifies by squaring, its elements formed in the same order
 * (the lateral block without that report's zero integrator), so the two reports speak of the same numbers.  dt outside (1e-6, 1] or
 * V0 not > 0: FD_MO_BAD_INPUT.  Outputs as fdyn_servo_flight_modes.  FD_MO_RADIUS < 1: the loop is stable.                      */
int fdyn_servo_sampled_modes(const double* K, const double* F, const double* x0, double dt, int64_t n, double* eig_re,
                             double* eig_im, double* summary, int32_t* iters, int32_t* status, void* stream);

/* fdyn_servo_filter_modes: the poles of (I - L) Phi, both 5 x 5 blocks of F (Gamma is not read); the product is formed as
 * fdyn_servo_loop_margins forms it, every element summed k = 0 .. 4 in that order.
 *   eig_re, eig_im [FD_NSMO_FILTER_EIG][n] (FD_SMO_FILTER_*), summary [2][FD_NMO][n].
 * The estimation error e = x - xhat obeys e+ = (I - L) Phi e - L v whatever the law does with xhat, integrators fed by xhat
 * included.  In the coordinates (x, i, e) the 12- and 11-state estimate-feedback loops are block triangular, so their spectrum is
 * the sampled loop's poles together with these ten: no 12 x 12 solver is needed, and none is provided.                           */
int fdyn_servo_filter_modes(const double* F, int64_t n, double* eig_re, double* eig_im, double* summary, int32_t* iters,
                            int32_t* status, void* stream);

/* fdyn_square_modes: M [N * N][n], one row-major N x N per aircraft taken as it is, FD_SMO_MIN_N <= N <= FD_SMO_MAX_N, else
 * FDYN_ERR_BAD_SIZE: the door for matrices composed on the device.
 *   eig_re, eig_im [N][n], summary [FD_NMO][n] (one block).                                                                     */
int fdyn_square_modes(const double* M, int N, int64_t n, double* eig_re, double* eig_im, double* summary, int32_t* iters,
                      int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_SERVO_MODES_H */
