"""The scheduled servo on noisy sensors of include/fdyn_servo_sched_lqg.h (fdyn_servo_sched_lqg_step_*) restated in NumPy fp64: it
adds only that header's law -- the operating point (x0, u0, K, F) looked up by servo_sched_numpy's steps 0a-0b over the two tables
side by side, and the re-reference of the estimate and of du_prev -- to servo_lqg_numpy's control step and servo_numpy's law, which
are called as they are.  Shared by the CPU tests and the GPU test; nothing here imports the product package.
"""
import numpy as np

import servo_lqg_numpy as sln
import servo_numpy as sn
import servo_sched_numpy as ssn
from lqr_numpy import wrap_angle, clip_controls

NSS, NSKF = ssn.NSS, sln.NSKF
# the eight scheduled words among the ten estimated ones (u, w, q, theta, z | v, p, r, phi, psi), and the angles among them
SCHEDULED = tuple(j for j, s in enumerate(sln.EST_STATES) if s in ssn.X0_WORDS)
SCHEDULED_ANGLES = (3, 8)
NONE_YET = (np.nan, -1.0)                                       # a sched_state with no operating point


def side_by_side(table, table_f):
    """[M][FD_NSS] and [M][FD_NSKF] -> [M][FD_NSS + FD_NSKF]: the rule of step 0b applies to F as to every other word."""
    return np.concatenate([np.asarray(table, np.float64), np.asarray(table_f, np.float64)], axis=1)


def operating_point(both, sigma, origin):
    """Steps 0b and 0c at sigma -> (x0 [12] with z0, psi0 from origin, u0 [4], K [26], F [120], position)."""
    words, pos = ssn.lookup(both, sigma)
    x0, u0, K = ssn.design_of(words[:NSS])
    x0[sn.X_D], x0[sn.X_YAW] = origin
    return x0, u0, K, words[NSS:].copy(), pos


def same_bits(a, b):
    return np.float64(a).view(np.int64) == np.float64(b).view(np.int64)


def enter(both, ref, origin, sched_state):
    """Launch entry -> (sigma, x0, u0, K, F, position): rebuilt from the stored sigma, or the table entered with V_c."""
    sigma = sched_state[0] if sched_state[1] >= 0.0 else ref[0]
    return (sigma,) + operating_point(both, sigma, origin)


def rereference(xhat, du, x0, u0, x0n, u0n):
    """Step 4 -> (xhat, du_prev) relative to the new operating point."""
    xhat, du = xhat.copy(), du.copy()
    for j in SCHEDULED:
        s = sln.EST_STATES[j]
        xhat[j] = xhat[j] + (x0[s] - x0n[s])
        if j in SCHEDULED_ANGLES and not -np.pi <= xhat[j] < np.pi:       # a word inside [-pi, pi) keeps its bits
            xhat[j] = wrap_angle(xhat[j])
    for k in range(4):
        du[k] = du[k] + (u0[k] - u0n[k])
    return xhat, du


def controls_from(table, table_f, origin, x, xhat, ref, integ, feedback=sln.ESTIMATE, on=ssn.ON_AIRSPEED, sched_state=NONE_YET,
                  limits=sn.DEFAULT_LIMITS):
    """n_steps = 0 -> (u unclipped [4], sigma, position) of the operating point the law ran at; nothing is stored."""
    both = side_by_side(table, table_f)
    sigma, x0, u0, K, F, pos = enter(both, ref, origin, sched_state)
    xf = np.array(x, np.float64) if feedback == sln.TRUTH else sln.law_input(x, x0, xhat)
    s = ssn.sigma_of(xf, ref, on)
    if not same_bits(s, sigma):
        sigma = s
        x0, u0, K, F, pos = operating_point(both, sigma, origin)
    return sn.controls(K, x0, u0, xf, ref, integ, limits)[0], sigma, pos


def fly(step, table, table_f, sigma_n, origin, x, ref, integ, dt, z, feedback=sln.ESTIMATE, on=ssn.ON_AIRSPEED, xhat=None, du_prev=None,
        sched_state=NONE_YET, limits=sn.DEFAULT_LIMITS, record=None, every=1, moves=None):
    """len(z) control steps of include/fdyn_servo_sched_lqg.h from state x; z [n_steps][10] standard normals; sigma_n [10] the
    measurement noise.  -> servo_lqg_numpy.fly's dict plus sched_state = (sigma, position).  record: optional list that receives
    (x, true errors) after every `every`-th step; moves: optional list that receives, per re-reference, (x0 + xhat on the eight
    scheduled words: x0, xhat, x0', xhat'; the controls: u0, du_prev, u0', du_prev')."""
    x, ref, integ = np.array(x, np.float64), np.array(ref, np.float64), np.array(integ, np.float64)
    sigma_n = np.asarray(sigma_n, np.float64)
    xhat = np.zeros(sln.NSKX) if xhat is None else np.array(xhat, np.float64)
    du = np.zeros(4) if du_prev is None else np.array(du_prev, np.float64)
    both = side_by_side(table, table_f)
    sigma, x0, u0, K, F, pos = enter(both, ref, origin, sched_state)
    err_est, err_meas, chatter, sat = np.zeros(sln.NSKX), np.zeros(sln.NSKX), np.zeros(4), 0
    uc, y, err = None, np.zeros(sln.NSKX), np.zeros(3)
    words = [sln.EST_STATES[j] for j in SCHEDULED]
    for n, zs in enumerate(np.asarray(z, np.float64)):
        # 1. steps 1-5 of fdyn_servo_lqg.h at the current operating point
        d = sln.deviation(x, x0)
        y = d + sigma_n * zs
        xhat = sln.kalman_update(F, xhat, du, y)
        de = xhat - d
        de[sln.PSI] = wrap_angle(de[sln.PSI])
        err_est = err_est + de ** 2
        err_meas = err_meas + (y - d) ** 2
        err = sn.errors(x, ref)
        xf = x if feedback == sln.TRUTH else sln.law_input(x, x0, xhat if feedback == sln.ESTIMATE else y)
        # 2.-4. sigma, the new words, the re-reference
        s = ssn.sigma_of(xf, ref, on)
        if not same_bits(s, sigma):
            x0n, u0n, Kn, Fn, pos = operating_point(both, s, origin)
            xh2, du2 = rereference(xhat, du, x0, u0, x0n, u0n)
            if moves is not None:
                moves.append(((x0[words], xhat[list(SCHEDULED)], x0n[words], xh2[list(SCHEDULED)]), (u0, du, u0n, du2)))
            sigma, x0, u0, K, F, xhat, du = s, x0n, u0n, Kn, Fn, xh2, du2
        # 5.-7. the law, the accounting, the RK4 and the references
        u, e = sn.controls(K, x0, u0, xf, ref, integ, limits)
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
        x = step(x, uc, dt)
        ref[1] = ref[1] + ref[3] * dt
        ref[2] = wrap_angle(ref[2] + ref[4] * dt)
        if record is not None and (n + 1) % every == 0:
            record.append((x.copy(), sn.errors(x, ref)))
    return dict(x=x, ref=ref, integ=integ, xhat=xhat, du_prev=du, u=uc, sat=sat, err_est=err_est, err_meas=err_meas, chatter=chatter,
                y=y, err=err, sched_state=(sigma, pos))


# ---- what the test files fly ---------------------------------------------------------------------------------------------------
_CACHE = {}


def ladder_f(name, speeds=ssn.LADDER, dt=ssn.DT):
    """The filters of servo_sched_numpy.ladder's nodes at dt on the default noise, once per session -> read-only [M][FD_NSKF]."""
    key = ("ladder_f", name, tuple(speeds), dt)
    if key not in _CACHE:
        rows = [sln.design(d["A"], d["B"], dt, sln.default_noise()) for d in ssn.ladder(name, speeds)["designs"]]
        assert all(r["status"] == 0 for r in rows)
        out = np.array([r["F"] for r in rows])
        out.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def origin_of(x0):
    return np.array([x0[sn.X_D], x0[sn.X_YAW]])


HOWS = ("single", "command", "airspeed")
BENEFIT_SEED = sln.SEED + 7


def benefit_flight(i, how, feedback=sln.ESTIMATE):
    """Flight i of servo_sched_numpy.BENEFIT on the default sensor noise under replayed Philox normals (seed BENEFIT_SEED, row i,
    step word 0: the SAME normals for the three ways) -> dict(peak, integral of |e_h| dt, chatter [4], err_est [10], end errors).
    how: "single" (one design and one filter at the start speed: servo_lqg_numpy.fly), "command" or "airspeed"."""
    name, V_start, V_cmd = ssn.BENEFIT[i]
    lad, k = ssn.ladder(name), ssn.LADDER.index(V_start)
    start, table_f = lad["designs"][k], ladder_f(name)
    step = sn.oracle_step(start["P"])
    n1, n2 = int(round(ssn.T_COMMAND / ssn.DT)), int(round((ssn.T_END - ssn.T_COMMAND) / ssn.DT))
    z = sln.lqg_normal_sequence(BENEFIT_SEED, np.array([i]), 0, n1 + n2)[:, 0, :]
    rec = []
    ref0 = sn.reference_at(start["x0"])
    if how == "single":
        a = sln.fly(step, start["K"], table_f[k], sln.DEFAULT_SIGMA, start["x0"], start["u0"], start["x0"], ref0, np.zeros(3), ssn.DT, z[:n1],
                    feedback, record=rec)
        b = sln.fly(step, start["K"], table_f[k], sln.DEFAULT_SIGMA, start["x0"], start["u0"], a["x"], sn.command(a["ref"], speed=V_cmd),
                    a["integ"], ssn.DT, z[n1:], feedback, xhat=a["xhat"], du_prev=a["du_prev"], record=rec)
    else:
        on, org = (ssn.ON_COMMAND if how == "command" else ssn.ON_AIRSPEED), origin_of(start["x0"])
        a = fly(step, lad["table"], table_f, sln.DEFAULT_SIGMA, org, start["x0"], ref0, np.zeros(3), ssn.DT, z[:n1], feedback, on, record=rec)
        b = fly(step, lad["table"], table_f, sln.DEFAULT_SIGMA, org, a["x"], sn.command(a["ref"], speed=V_cmd), a["integ"], ssn.DT, z[n1:],
                feedback, on, xhat=a["xhat"], du_prev=a["du_prev"], sched_state=a["sched_state"], record=rec)
    eh = np.abs(np.array([e[1] for _, e in rec]))
    return dict(peak=float(eh.max()), integral=float(eh.sum() * ssn.DT), chatter=a["chatter"] + b["chatter"], err_est=a["err_est"] + b["err_est"],
                err=sn.errors(b["x"], b["ref"]), x=b["x"])


def benefit_flights():
    """The four flights three ways, once per session: {how: dict(peak [4], integral [4], chatter [4][4], err_est [4][10], err [4][3])}."""
    if "benefit" not in _CACHE:
        out = {}
        for how in HOWS:
            rows = [benefit_flight(i, how) for i in range(len(ssn.BENEFIT))]
            out[how] = {k: np.array([r[k] for r in rows]) for k in ("peak", "integral", "chatter", "err_est", "err")}
        _CACHE["benefit"] = out
    return _CACHE["benefit"]
