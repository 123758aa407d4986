/* fdyn_modes.h -- C-ABI of the flight-mode report of libfdyn_hip.so (csrc/modes_kernels.hip): where the poles of every aircraft
 * are.  A header of its own beside fdyn.h, whose conventions hold: every array is a DEVICE pointer, SoA [word][n] row-major fp64
 * unless marked, `stream` is a hipStream_t passed as void*, the return codes are fdyn.h's, and neither entry point synchronises
 * or allocates, so both can be captured into a hipGraph.  Layout constants (FD_MO_*, FD_NMO): fdyn_layout.h.
 *
 * Per aircraft two 4 x 4 real matrices are solved in fp64, one lane per aircraft, block 0 = longitudinal (u, w, q, theta), block
 * 1 = lateral (v, p, r, phi): Householder reduction to Hessenberg form, Francis double-shift QR sweeps with deflation to 1 x 1
 * and 2 x 2 blocks (exceptional shifts at sweeps 10 and 20, at most 30 sweeps per deflation), 2 x 2 blocks in closed form.  No
 * balancing.  The only operations are + - * / and sqrt, one rounding each, in a fixed order (csrc/fdyn_eig.hpp).
 *
 * Outputs of both entry points:
 *   eig_re, eig_im [8][n]   block 0 in rows 0-3, block 1 in rows 4-7; per block in canonical order: real part descending (the
 *                           least stable first), equal real parts by |Im| descending, within a conjugate pair the member with the
 *                           positive imaginary part first; both members of a pair carry the bit-identical real part, and the
 *                           tie rule keeps them adjacent when another pole shares it
 *   summary [2][FD_NMO][n]  or NULL; per block max Re, max |.|, min |.|, min of -Re / |.| (0 for an eigenvalue at 0), the number
 *                           with Re > 0 and the number with Im != 0 (FD_MO_*)
 *   iters [n] int32         or NULL; QR sweeps of the slower block
 *   status [n] int32        0 = every eigenvalue of both blocks converged; FD_MO_NOT_CONVERGED = the sweep cap or a non-finite
 *                           intermediate; FD_MO_BAD_INPUT = a word that is read is not finite, nothing was solved.  A lane with a
 *                           non-zero status gets NaN in every eigenvalue and summary word of BOTH blocks.
 * FDYN_ERR_BAD_SIZE for n < 1 and FDYN_ERR_NULL for a missing required pointer, with no launch.                              */
#ifndef FDYN_MODES_H
#define FDYN_MODES_H

#include <stdint.h>
#include "fdyn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fdyn_flight_modes: A [FD_NX * FD_NX][n], B [FD_NX * FD_NU][n] as fdyn_linearize writes them, K [FD_NLQK][n] as fdyn_lqr_design
 * writes it.  Per block, on the rows and columns fdyn_lqr_design reads, m = a - b Kb, every element a - (b_0 k_0 + b_1 k_1); only
 * the words inside the two blocks are read.  K = NULL: the open-loop poles of a (B is then not read and may be NULL), to the bit
 * what K = 0 gives.                                                                                                          */
int fdyn_flight_modes(const double* A, const double* B, const double* K, int64_t n, double* eig_re, double* eig_im, double* summary,
                      int32_t* iters, int32_t* status, void* stream);
/* fdyn_block_modes: M [2][16][n], two row-major 4 x 4 per aircraft taken as they are -- matrices composed on the device, such as
 * the filter's Phi (I - L), the sampled closed loop Phi - Gamma Kb or the estimator loop's F_c: their spectral radius is
 * summary word FD_MO_RADIUS.                                                                                                 */
int fdyn_block_modes(const double* M, int64_t n, double* eig_re, double* eig_im, double* summary, int32_t* iters, int32_t* status,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FDYN_MODES_H */
