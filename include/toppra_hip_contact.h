/* toppra_hip_contact.h -- contact-energy limits: the effective (reflected) mass of a robot at control points, for a batch.
 * An entry of libtoppra_hip.so beside those of toppra_hip.h, whose tpr_chain, tpr_chain_points, flags and error codes it uses.
 *
 * What ISO/TS 15066 power-and-force limiting caps per body region: the energy a contact at a point of the arm can transfer,
 *   E = 1/2 mu v^2,   mu = (1 / m_body + 1 / m_R)^-1,   1 / m_R = u' J M(q)^-1 J' u,
 * with v the point's speed along the unit direction u, J the point's Jacobian, m_R the robot's effective (reflected) mass there
 * and m_body the mass of the body part it meets (kg and J; no table of body regions is shipped: the caller supplies the numbers).
 * It is first order in the path velocity -- with qd = q' sd, v^2 = s2 sd^2 -- so the cap is an upper bound on x = sd^2 per
 * gridpoint.  The kinetic energy of the whole structure (tpr_tree_momentum_batch) is its upper envelope: by Cauchy-Schwarz
 * s2^2 <= g (q'' M q') for the g below, with equality at 1 dof.
 *
 * Per gridpoint and per unit of path velocity (qd = qs), in link axes; gravity and velocity products play no part (M^-1 depends on
 * q alone).  For point p of `points`, fixed at offset o_p on link k (v_k, w_k: the velocity of that link's origin and its angular
 * velocity, the recursion of tpr_chain_tool_velocity_batch over the parent table):
 *   n_p = v_k + w_k x o_p                                            the point's velocity per unit sd
 *   velocity mode  (direction NULL):  f = n_p,          s2_p = n_p . n_p
 *   direction mode (direction[p] = u_p, link axes; the caller normalises it):  f = u_p,   s2_p = (n_p . u_p)^2
 *   g_p  = tau' M(q)^-1 tau,  tau = J_p' f                           the mobility along the applied force
 * In velocity mode 1 / m_R = g_p / s2_p; in direction mode 1 / m_R = g_p.  M^-1 is never formed.  One walk from the tips to the
 * roots (the articulated-body factorisation M^-1 = (1 - H psi K)' D^-1 (1 - H psi K)) gives every g_p in O(d):
 *   IA_i = I_i + sum over children c of X*(IA_c - U_c U_c' / D_c),   U_i = IA_i S_i,   D_i = S_i' U_i,
 *   S_i = (z; 0) for a revolute joint, (0; z) for a prismatic one; a point's bias wrench starts on its own link as
 *   b_p = -(o_p x f; f), and at every link i on its path to the root:  u = -S_i' b_p,  g_p += u^2 / D_i,  b_p += U_i u / D_i, then
 *   b_p moves into the parent's frame.
 * The order of every sum is fixed and stated at the head of csrc/tpr_effmass.hip.inc: dot products left to right; at a fork the
 * link's own inertia plus what the next link handed down, then the other children's sum, formed in descending link number; one
 * IEEE reciprocal 1 / D_i per link.  A point's bits depend neither on the other points of the set nor on its place in it; a chain
 * gives the bits of the tree -1, 0, 1, ...; every output passes through "+ 0.0" (a standstill gives speed2 = +0).
 *   speed2   [B][N+1][count] = s2_p;      mobility [B][N+1][count] = g_p;
 *   limit    [B][count][2]   = (2 E_max, 1 / m_body) of trajectory b and point p: 2 E_max > 0, 1 / m_body >= 0 (0 = a clamped body
 *            part) -- the caller's responsibility, as for tpr_chain_points_speed_batch;
 *   xbound   [B][N+1][2] = (0, min_p x_p),   x_p = (limit_0 (limit_1 + winv)) / s2_p,   winv = g_p / s2_p | g_p (direction mode),
 *            x_p = +inf where s2_p == 0 (a select, not 0 / 0); the minimum starts from +inf and takes x_p < best ? x_p : best in
 *            the set's order -- the array a TPR_BOUND_X source of tpr_stage_boxes_batch takes, where the box then keeps its 1e8.
 * A robot whose mass matrix is singular (a weightless leaf link gives D = 0) yields non-finite results by IEEE rules: nothing is
 * refused on that ground, it is the caller's responsibility.
 *
 * Any of speed2, mobility, xbound may be NULL, not all; each output is the same whichever others are asked for.  qs may be NULL
 * only in direction mode with speed2 and xbound both NULL (the mobility does not depend on it).  links, parent, points and
 * direction are host arrays, also with TPR_DEVICE_PTRS (direction: count x 3 doubles, read on the host once per call).  A further
 * root none of whose links is an ancestor of a point is skipped.
 * One wave of 64 gridpoints per block.  Dynamic LDS, in slots of 512 bytes: 2 per link (sine, cosine), 4 + 4 per point (the force
 * and s2; the wrench's moment and g, which lie over the staged q, qs rows, 2 (d | 1) slots, once the way up has read them) and 21
 * per fork: (2 d + 4 count + max(4 count, 2 (d | 1)) + 21 forks) 512 bytes, at most (64 + 64 + 66 + 84) 512 = 142 336 at 32 dof
 * with 16 points and 4 forks -- every robot and point set the structs admit fits, none is refused for its size.
 * Refused before any launch, in this order: B, N; what tpr_tree_momentum_batch refuses of links and parent; the points (NULL, a
 * count outside 1 .. TPR_CHAIN_MAX_POINTS, a link outside 0 .. d-1, an offset that is not finite: TPR_E_BADARG); a direction that
 * is not finite; a NULL q; a NULL qs where it is needed; all three outputs NULL; xbound without limit.                          */
#ifndef TOPPRA_HIP_CONTACT_H
#define TOPPRA_HIP_CONTACT_H

#include "toppra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int tpr_tree_effective_mass_batch(const tpr_chain *links, const int32_t *parent, const tpr_chain_points *points,
                                  const double *direction /* [count][3] link axes, NULL = along the velocity */,
                                  int B, int N, const double *q, const double *qs,
                                  const double *limit /* [B][count][2] = (2 E_max, 1/m_body) */,
                                  double *speed2 /* [B][N+1][count] */, double *mobility /* [B][N+1][count] = g */,
                                  double *xbound /* [B][N+1][2] */, int flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
