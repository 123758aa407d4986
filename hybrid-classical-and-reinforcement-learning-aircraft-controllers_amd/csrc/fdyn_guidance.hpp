// fdyn_guidance.hpp -- the waypoint guidance on its own: the heading, speed and altitude command that waypoint_agent
// (fdyn_core.hpp) forms before it hands them to hsa_agent, for a control law that is not the PID cascade (servo_kernels.hip).
//
// The lines below exist TWICE: here and as the head of waypoint_agent.  fdyn_core.hpp is what the benchmarked kernels of
// fdyn_kernels.hip are built from; rewriting waypoint_agent to call this function would have to leave every one of those
// kernels' instruction streams byte-identical, and that file stays untouched instead.  A change to the guidance laws goes to both
// places; tests/test_servo_mission_oracle.py pins this copy's restatement to the same oracle the cascade is tested against.
#pragma once
#include "fdyn_core.hpp"

namespace fdyn {

template <typename G> struct GuidanceCmd { G heading, speed, altitude; };

// The cascade constants -> LDS in the glue type, with the two derived 1 / (g tan bank) words the fp32 glue multiplies by
// (stage_cascade_consts of fdyn_kernels.hip).  The caller's barrier follows.
template <typename G>
FD_DEV void stage_guidance_consts(G* s_consts, const double* __restrict__ consts)
{
    for (int k = threadIdx.x; k < FD_NC; k += blockDim.x) s_consts[k] = G(consts[k]);
    if (threadIdx.x < 2) {
        const double bank = consts[threadIdx.x == 0 ? FD_C_WP_MAX_BANK_RAD : FD_C_LOS_MAX_BANK_RAD];
        s_consts[FD_CD_WP_INV_G_TAN_BANK + threadIdx.x] = G(1.0 / (9.81 * ::tan(bank)));
    }
}

// controllers/waypoint_agent.py:107-228 ; wp = {north, east, altitude, speed}.  Of C the words FD_C_GUIDANCE_TYPE ..
// FD_C_MIN_SPEED are read (and the two FD_CD_* words in the fp32 glue).
template <typename G>
FD_DEV GuidanceCmd<G> waypoint_guidance(const G* C, const G* wp, const G (&x)[FD_NX], const Derived<G>& d)
{
    const G e0 = wp[FD_WP_NORTH] - x[0], e1 = wp[FD_WP_EAST] - x[1];
    const G hd = M<G>::sqrt(e0 * e0 + e1 * e1);
    const int gtype = int(C[FD_C_GUIDANCE_TYPE]);
    const G los = M<G>::atan2(e1, e0);
    G heading_cmd = los;
    if (gtype == FD_GUIDANCE_LOS) {                                          // :118-144
        const G V = pymax(d.airspeed, G(10));
        G turn_radius;
        if constexpr (sizeof(G) == 8) turn_radius = (V * V) / (G(9.81) * M<G>::tan(C[FD_C_LOS_MAX_BANK_RAD]));
        else turn_radius = (V * V) * C[FD_CD_LOS_INV_G_TAN_BANK];
        const G heading_error = wrap_pi<G>(heading_cmd - d.heading);
        const G anticipation = turn_radius * M<G>::abs(heading_error) / deg2rad<G>(90.0);
        if (hd < anticipation && M<G>::abs(heading_error) > deg2rad<G>(20.0)) {
            const G blend = G(1) - (hd / anticipation);
            heading_cmd = wrap_pi<G>(heading_cmd + blend * C[FD_C_LOS_LEAD_ANGLE_RAD] * signv(heading_error));
        }
    } else if (gtype == FD_GUIDANCE_PP) {                                    // :146-178
        const G V = pymax(d.airspeed, G(10));
        G turn_radius;
        if constexpr (sizeof(G) == 8) turn_radius = (V * V) / (G(9.81) * M<G>::tan(C[FD_C_WP_MAX_BANK_RAD]));
        else turn_radius = (V * V) * C[FD_CD_WP_INV_G_TAN_BANK];
        G lookahead = C[FD_C_LOOKAHEAD_TIME] * V;
        const G proximity = C[FD_C_PROXIMITY_SCALE] * turn_radius;
        if (hd < proximity) lookahead *= G(0.6) + G(0.4) * (hd / proximity);
        lookahead = clipv(lookahead, C[FD_C_LOOKAHEAD_MIN], C[FD_C_LOOKAHEAD_MAX]);
        if (hd > G(1)) {
            const G eff = pymin(lookahead, hd);
            // fp64: the reference's own expression.  fp32 glue: the carrot lies on the line of sight already in heading_cmd
            if constexpr (sizeof(G) == 8) heading_cmd = M<G>::atan2((e1 / hd) * eff, (e0 / hd) * eff);
        }
    }
    heading_cmd = wrap_pi<G>(heading_cmd);                                   // :185

    G speed_cmd = (wp[FD_WP_SPEED] != wp[FD_WP_SPEED]) ? d.airspeed : wp[FD_WP_SPEED];   // None -> current airspeed
    G he = M<G>::abs(los - d.heading);                                       // :214-228
    he = M<G>::abs(wrap_pi<G>(he));
    const G td = C[FD_C_TURN_THRESHOLD_DIST];
    if (hd < td && he > C[FD_C_TURN_THRESHOLD_ANGLE_RAD]) {
        const G reduction = C[FD_C_MAX_SPEED_REDUCTION] * (G(1) - hd / td);
        speed_cmd = pymax(speed_cmd * (G(1) - reduction), C[FD_C_MIN_SPEED]);
    }
    return GuidanceCmd<G>{ heading_cmd, speed_cmd, wp[FD_WP_ALTITUDE] };
}

}  // namespace fdyn
