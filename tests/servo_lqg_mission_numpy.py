"""The waypoint missions on the servo's estimate of include/fdyn_servo_lqg_mission.h (fdyn_servo_lqg_mission_*) restated in NumPy
fp64: servo_lqg_numpy's measurement and filter, the position filter, servo_mission_numpy's mission update, guidance and
statistics, servo_numpy's law, in the header's order of operations, over ANY `step(x[12], u_clipped[4], dt) -> x[12]`.  The draws
are the twelve normals of the three Philox blocks of servo_lqg_numpy.  Shared by the CPU tests and the GPU test; nothing here
imports the product package.
"""
import math

import numpy as np

import lqr_numpy as ln
import philox_numpy as pn
import servo_lqg_numpy as lq
import servo_mission_numpy as mn
import servo_numpy as sn
from lqr_numpy import clip_controls, wrap_angle

NSKZ, NSPF, SPF_SIGMA, SPF_GAIN = 12, 2, 0, 1
ESTIMATE, MEASUREMENT, TRUTH = lq.ESTIMATE, lq.MEASUREMENT, lq.TRUTH
SIGMA_POS, RATE_POS = 1.0, 0.5                                  # the sensor layer's gps_position_stddev; s_p in m / sqrt(s)
X_N, X_E, X_U, X_V, X_W, X_ROLL, X_PITCH, X_YAW = 0, 1, 3, 4, 5, 6, 7, 8


def position_gain(sigma_pos=SIGMA_POS, rate_pos=RATE_POS, dt=0.01):
    """Steady-state Kalman gain of a random-walk position: r = sigma^2, q = s^2 dt, P- = (q + sqrt(q^2 + 4 q r)) / 2, g = P- / (P- + r)."""
    r, q = sigma_pos * sigma_pos, rate_pos * rate_pos * dt
    pm = (q + math.sqrt(q * q + 4.0 * q * r)) / 2.0
    return pm / (pm + r)


def position_words(sigma_pos=SIGMA_POS, gain=None, dt=0.01):
    return np.array([sigma_pos, position_gain(sigma_pos, RATE_POS, dt) if gain is None else gain], np.float64)


def normals(seed, rows, step):
    """[n, 12] standard normals of one step: words 0..9 in d's order, 10 and 11 the north and east position normals."""
    rows = np.atleast_1d(rows)
    c = lq.lqg_counters(rows, step)
    return pn.normals4(pn.philox(seed, c[..., 0], c[..., 1], c[..., 2], c[..., 3])).reshape(len(rows), NSKZ)


def normal_sequence(seed, rows, step0, n_steps):
    """[n_steps, n, 12]: what a launch of n_steps draws when the step word holds step0."""
    return np.stack([normals(seed, rows, step0 + s + 1) for s in range(n_steps)])


def ground_velocity(x):
    """(v_N, v_E) of R(phi, theta, psi) (u, v, w), each sum left to right as the header fixes it."""
    sphi, cphi = math.sin(x[X_ROLL]), math.cos(x[X_ROLL])
    sth, cth = math.sin(x[X_PITCH]), math.cos(x[X_PITCH])
    spsi, cpsi = math.sin(x[X_YAW]), math.cos(x[X_YAW])
    u, v, w = x[X_U], x[X_V], x[X_W]
    vn = (cth * cpsi) * u + ((sphi * sth) * cpsi - cphi * spsi) * v + ((cphi * sth) * cpsi + sphi * spsi) * w
    ve = (cth * spsi) * u + ((sphi * sth) * spsi + cphi * cpsi) * v + ((cphi * sth) * spsi - sphi * cpsi) * w
    return np.array([vn, ve])


def guidance_state(xf, phat, yp, feedback):
    """xg: the law's input with its north and east words replaced by phat (ESTIMATE) or y_p (MEASUREMENT); the stored state for TRUTH
    (xf is the stored state then)."""
    xg = np.array(xf, np.float64)
    if feedback == ESTIMATE:
        xg[X_N], xg[X_E] = phat
    elif feedback == MEASUREMENT:
        xg[X_N], xg[X_E] = yp
    return xg


def controls_from(K26, x0, u0, x, xhat, phat, integ, wps, C, idx, feedback=ESTIMATE, limits=sn.DEFAULT_LIMITS):
    """n_steps = 0: (unclipped controls, or None for a complete lane) from the stored xhat and phat (the stored state for TRUTH)."""
    xf = x if feedback == TRUTH else lq.law_input(x, x0, xhat)
    xg = guidance_state(xf, phat, phat, feedback)
    _, _, ref = mn.commands(C, wps, idx, xg)
    if ref is None:
        return None
    return sn.controls(K26, x0, u0, xf, ref, integ, limits)[0]


def fly(step, K26, F, sigma, x0, u0, x, ref, integ, wps, C, idx, dt, z, pos, phat, feedback=ESTIMATE, xhat=None, du_prev=None,
        limits=sn.DEFAULT_LIMITS, stats=None, record=None):
    """len(z) control steps of include/fdyn_servo_lqg_mission.h from state x; z [n_steps][12] standard normals, pos = (sigma_p, g).
    -> dict(x, ref, integ, xhat, phat, du_prev, idx, reached, flown, sat, u (last clipped controls or None), stats, err_est [10],
    err_meas [10], err_pos [2], chatter [4], y (last measurement), err (last errors of the true state), events).  record: optional
    list that receives (distance of the guidance's state to the active waypoint before the mission update, idx) at every step."""
    x, ref, integ = np.array(x, np.float64), np.array(ref, np.float64), np.array(integ, np.float64)
    sigma, phat = np.asarray(sigma, np.float64), np.array(phat, np.float64)
    wps, C = np.asarray(wps, np.float64), np.asarray(C, np.float64)
    xhat = np.zeros(lq.NSKX) if xhat is None else np.array(xhat, np.float64)
    du = np.zeros(4) if du_prev is None else np.array(du_prev, np.float64)
    stats = np.array(mn.STATS_START if stats is None else stats, np.float64)
    u0 = np.asarray(u0, np.float64)
    err_est, err_meas, err_pos, chatter = np.zeros(lq.NSKX), np.zeros(lq.NSKX), np.zeros(2), np.zeros(4)
    reached = flown = sat = 0
    uc, y, err, events = None, np.zeros(lq.NSKX), np.zeros(3), []
    restart = int(C[mn.C_ON_COMPLETE]) == 1
    sp, g = float(pos[SPF_SIGMA]), float(pos[SPF_GAIN])
    for s, zs in enumerate(np.asarray(z, np.float64)):
        if idx >= len(wps) and not restart:                       # complete at entry: nothing at all
            break
        # 1-2. measure, filter
        d = lq.deviation(x, x0)
        y = d + sigma * zs[:lq.NSKX]
        p = np.array([x[X_N], x[X_E]])
        yp = p + sp * zs[lq.NSKX:]
        xhat = lq.kalman_update(F, xhat, du, y)
        # 3. the law's input
        xf = x if feedback == TRUTH else lq.law_input(x, x0, xhat if feedback == ESTIMATE else y)
        # 4. position filter
        pm = phat + dt * ground_velocity(xf)
        phat = pm + g * (yp - pm)
        # 5. account
        de = xhat - d
        de[lq.PSI] = wrap_angle(de[lq.PSI])
        err_est = err_est + de ** 2
        err_meas = err_meas + (y - d) ** 2
        err_pos = err_pos + np.array([(phat[0] - p[0]) ** 2 + (phat[1] - p[1]) ** 2, (yp[0] - p[0]) ** 2 + (yp[1] - p[1]) ** 2])
        # 6. mission update, guidance, references
        xg = guidance_state(xf, phat, yp, feedback)
        if record is not None:
            record.append((mn.distance(wps[idx], xg) if idx < len(wps) else np.nan, idx))
        idx, r = mn.mission_update(C, wps, idx, xg)
        if r:
            reached += 1
            events.append(s)
        if idx >= len(wps):
            if restart:
                idx = 0
            else:
                break
        h, v, a = mn.guidance(C, wps[idx], xg, mn.derived(xg))
        ref = np.array([v, a, h, 0.0, 0.0])
        # 7. statistics of the true state
        mn.stats_update(stats, wps, idx, x, mn.derived(x))
        flown += 1
        # 8. the law on x_f, then the accounting of the true state
        u, e = sn.controls(K26, x0, u0, xf, ref, integ, limits)
        err = sn.errors(x, ref)
        uc, _ = clip_controls(u)
        lon = bool(uc[0] != u[0] or uc[3] != u[3])
        lat = bool(uc[1] != u[1] or uc[2] != u[2])
        sat += int(lon or lat)
        if not lon:
            integ[0] = integ[0] + e[0] * dt
            integ[1] = integ[1] + e[1] * dt
        if not lat:
            integ[2] = integ[2] + e[2] * dt
        chatter = chatter + (uc - (u0 + du)) ** 2
        du = uc - u0
        # 9. physics
        x = step(x, uc, dt)
    return dict(x=x, ref=ref, integ=integ, xhat=xhat, phat=phat, du_prev=du, idx=idx, reached=reached, flown=flown, sat=sat, u=uc,
                stats=stats, err_est=err_est, err_meas=err_meas, err_pos=err_pos, chatter=chatter, y=y, err=err, events=events)


# ---- what the test files fly ---------------------------------------------------------------------------------------------------
SEED = lq.SEED
STEPS = mn.SHORT_STEPS
# the issue's gates
GATE_STEPS, GATE_POS_RATIO, GATE_CHATTER, GATE_RAW = 0.02, 0.1, 1.5, 0.5
_CACHE = {}


def setup():
    """The ten aircraft of servo_numpy.compare_flights with a filter designed at dt 0.01 on the default noise, the short mission at
    the shared speed (radius 40, pure pursuit) and the replayed Philox normals z [1500][10][12] (seed SEED, row = the aircraft's
    index, step word 0).  Read-only, once per session."""
    if "setup" not in _CACHE:
        f = sn.compare_flights()
        n = len(f["type"])
        F = np.array([lq.design(f["A"][i], f["B"][i], ln.DT, lq.default_noise())["F"] for i in range(n)])
        out = dict(f=f, n=n, F=F, wps=mn.short_mission(sn.ALTITUDE, mn.SHARED_SPEED), C=mn.consts("PP", mn.RADIUS, "freeze"),
                   z=normal_sequence(SEED, np.arange(n), 0, STEPS), dt=ln.DT)
        for v in (F, out["wps"], out["z"]):
            v.setflags(write=False)
        _CACHE["setup"] = out
    return _CACHE["setup"]


def short_flights(feedback=ESTIMATE, gain=None):
    """setup()'s aircraft flown from their trims through the short mission over the CPU oracle's RK4, 1500 steps, phat started at
    the state's north and east; gain None = position_gain().  -> (list of fly()'s dicts, list of the records).  Once per session
    per (feedback, gain)."""
    key = ("short", feedback, gain)
    if key not in _CACHE:
        su = setup()
        f, pos = su["f"], position_words(gain=gain, dt=su["dt"])
        rows, records = [], []
        for i in range(su["n"]):
            rec = []
            rows.append(fly(mn.airframe_step(f["type"][i]), f["K"][i], su["F"][i], lq.DEFAULT_SIGMA, f["x0"][i], f["u0"][i], f["x0"][i],
                            f["ref0"][i], np.zeros(3), su["wps"], su["C"], 0, su["dt"], su["z"][:, i], pos, f["x0"][i][:2], feedback,
                            record=rec))
            records.append(rec)
        _CACHE[key] = (rows, records)
    return _CACHE[key]
