"""The gain schedule of include/fdyn_servo_sched.h (fdyn_servo_sched_step_*, fdyn_servo_sched_mission_*) restated in NumPy fp64:
steps 0a-0c -- sigma, the two bracketing nodes, the interpolated words -- in front of servo_numpy's control step and of
servo_mission_numpy's mission step, which are called one step at a time and are otherwise untouched.  Shared by the CPU tests and the
GPU test; nothing here imports the product package.
"""
import numpy as np

import lqr_numpy as ln
import servo_numpy as sn
import servo_mission_numpy as smn

# FD_SS_* rows, FD_NSS, FD_MAX_SCHED_NODES, FD_SCHED_ON_* (asserted against layout.py in tests/test_servo_sched_boundary.py)
SS_V, SS_X0, SS_U0, SS_K, NSS, MAX_NODES = 0, 1, 9, 13, 39, 8
ON_AIRSPEED, ON_COMMAND = 0, 1
X0_WORDS = (3, 5, 10, 7, 4, 9, 11, 6)                     # u, w, q, theta, v, p, r, phi in FD_X_* numbering


def node(V, x0, u0, K26):
    """One node's FD_NSS words from a design at the airspeed V: x0 [12], u0 [4], K [26]."""
    w = np.empty(NSS)
    w[SS_V] = V
    w[SS_X0:SS_U0] = np.asarray(x0, np.float64)[list(X0_WORDS)]
    w[SS_U0:SS_K] = u0
    w[SS_K:] = K26
    return w


def lookup(table, sigma):
    """Steps 0a-0b on one aircraft's table [M][FD_NSS] -> (words [FD_NSS], position)."""
    table = np.asarray(table, np.float64)
    last = len(table) - 1
    with np.errstate(all="ignore"):
        if not sigma > table[0][SS_V]:
            return table[0].copy(), 0.0
        if sigma >= table[last][SS_V]:
            return table[last].copy(), float(last)
        k = 0
        for j in range(1, last):
            if table[j][SS_V] <= sigma:
                k = j
        t = (sigma - table[k][SS_V]) / (table[k + 1][SS_V] - table[k][SS_V])
        return table[k] + t * (table[k + 1] - table[k]), k + t


def design_of(words):
    """Step 0c's inputs from a node's or an interpolated word list -> (x0 [12] with the eight regulated words set, u0 [4], K [26])."""
    x0 = np.zeros(12)
    x0[list(X0_WORDS)] = words[SS_X0:SS_U0]
    return x0, words[SS_U0:SS_K].copy(), words[SS_K:].copy()


def sigma_of(x, ref, on):
    """Step 0a: the airspeed as step 1 of the law forms it, or the commanded airspeed."""
    if on == ON_COMMAND:
        return ref[0]
    return np.sqrt((x[sn.X_U] * x[sn.X_U] + x[sn.X_V] * x[sn.X_V]) + x[sn.X_W] * x[sn.X_W])


def controls(table, x, ref, integ, on=ON_AIRSPEED, limits=sn.DEFAULT_LIMITS):
    """n_steps = 0 -> (u unclipped [4], sigma, position)."""
    sigma = sigma_of(x, ref, on)
    words, pos = lookup(table, sigma)
    x0, u0, K = design_of(words)
    return sn.controls(K, x0, u0, x, ref, integ, limits)[0], sigma, pos


def fly(step, table, x, ref, integ, dt, n_steps, on=ON_AIRSPEED, limits=sn.DEFAULT_LIMITS, record=None, every=1):
    """n_steps scheduled control steps -> (x, ref, integ, last clipped controls, saturated steps, sigma, position).  record: optional
    list that receives (x, errors before the clip) copies after every `every`-th step."""
    x, ref, integ = np.array(x, np.float64), np.array(ref, np.float64), np.array(integ, np.float64)
    uc, sat, sigma, pos = None, 0, np.nan, 0.0
    for s in range(n_steps):
        sigma = sigma_of(x, ref, on)
        words, pos = lookup(table, sigma)
        x0, u0, K = design_of(words)
        x, ref, integ, uc, s1 = sn.fly(step, K, x0, u0, x, ref, integ, dt, 1, limits)
        sat += s1
        if record is not None and (s + 1) % every == 0:
            record.append((x.copy(), sn.errors(x, ref)))
    return x, ref, integ, uc, sat, sigma, pos


def fly_mission(step, table, x, ref, integ, wps, C, idx, dt, n_steps, on=ON_AIRSPEED, limits=sn.DEFAULT_LIMITS):
    """n_steps scheduled mission steps -> servo_mission_numpy.fly's dict, with sigma and pos of the last control step."""
    x, ref, integ = np.array(x, np.float64), np.array(ref, np.float64), np.array(integ, np.float64)
    wps, C = np.asarray(wps, np.float64), np.asarray(C, np.float64)
    out = dict(x=x, ref=ref, integ=integ, idx=idx, reached=0, flown=0, sat=0, u=None, stats=np.array(smn.STATS_START), sigma=np.nan, pos=0.0)
    for _ in range(n_steps):
        i2, _, cmd = smn.commands(C, wps, out["idx"], out["x"])          # the V_c the guidance is about to write
        if cmd is not None:
            sigma = sigma_of(out["x"], cmd, on)
            words, pos = lookup(table, sigma)
            x0, u0, K = design_of(words)
        else:
            x0, u0, K = design_of(np.asarray(table, np.float64)[0])      # complete: the step below flies nothing
        r = smn.fly(step, K, x0, u0, out["x"], out["ref"], out["integ"], wps, C, out["idx"], dt, 1, limits, stats=out["stats"])
        for k in ("reached", "flown", "sat"):
            out[k] += r[k]
        out["idx"] = r["idx"]
        if r["flown"] == 0:
            break
        out.update(x=r["x"], ref=r["ref"], integ=r["integ"], u=r["u"], stats=r["stats"], sigma=sigma, pos=pos)
    return out


# ---- what the test files fly ---------------------------------------------------------------------------------------------------
LADDER = (15.0, 20.0, 25.0, 30.0)
AIRFRAMES = ("rc_plane", "cessna")
# the four flights of the issue: (airframe, start speed, commanded speed); default weights, dt 0.01, 40 s, the command at t = 1 s
BENEFIT = (("rc_plane", 15.0, 30.0), ("rc_plane", 30.0, 15.0), ("cessna", 15.0, 30.0), ("cessna", 30.0, 15.0))
DT, T_COMMAND, T_END, SAMPLE_EVERY = 0.01, 1.0, 40.0, 10

_CACHE = {}


def ladder(name, speeds=LADDER):
    """Level trims of one airframe at `speeds`, each designed with the default weights over the CPU oracle, once per session ->
    dict(table [M][FD_NSS], designs = servo_numpy.oracle_design's dicts)."""
    key = ("ladder", name, tuple(speeds))
    if key not in _CACHE:
        designs = [sn.oracle_design(name, V) for V in speeds]
        assert all(d["status"] == 0 for d in designs)
        table = np.array([node(V, d["x0"], d["u0"], d["K"]) for V, d in zip(speeds, designs)])
        table.setflags(write=False)
        _CACHE[key] = dict(table=table, designs=designs)
    return _CACHE[key]


def _peak(rec):
    """(largest |e_h| over the recorded samples, the last errors)."""
    return float(max(abs(e[1]) for _, e in rec))


def benefit_flight(name, V_start, V_cmd, how):
    """One flight of the issue's table -> dict(peak |e_h| sampled every SAMPLE_EVERY steps, err = the end errors, x).  how: "single"
    (one design at the start speed), "command" or "airspeed" (the ladder entered with that sigma)."""
    lad = ladder(name)
    start = lad["designs"][LADDER.index(V_start)]
    table = lad["table"][LADDER.index(V_start):LADDER.index(V_start) + 1] if how == "single" else lad["table"]
    on = ON_COMMAND if how == "command" else ON_AIRSPEED
    step = sn.oracle_step(start["P"])
    n1, n2 = int(round(T_COMMAND / DT)), int(round((T_END - T_COMMAND) / DT))
    rec = []
    x, ref, integ, _, _, _, _ = fly(step, table, start["x0"], sn.reference_at(start["x0"]), np.zeros(3), DT, n1, on, record=rec, every=SAMPLE_EVERY)
    x, ref, integ, _, _, _, _ = fly(step, table, x, sn.command(ref, speed=V_cmd), integ, DT, n2, on, record=rec, every=SAMPLE_EVERY)
    return dict(peak=_peak(rec), err=sn.errors(x, ref), x=x)


def benefit_flights():
    """The four flights three ways, once per session: dict(single, command, airspeed = peaks [4], end = end errors [3 ways][4][3])."""
    if "benefit" not in _CACHE:
        rows = {how: [benefit_flight(n, a, b, how) for n, a, b in BENEFIT] for how in ("single", "command", "airspeed")}
        out = {how: np.array([r["peak"] for r in rows[how]]) for how in rows}
        out["end"] = np.array([[r["err"] for r in rows[how]] for how in ("single", "command", "airspeed")])
        _CACHE["benefit"] = out
    return _CACHE["benefit"]


def frozen_point_modes(name, speeds=LADDER, points_per_interval=1):
    """Between the nodes of one airframe's ladder: trim and linearise there, interpolate K there, and take the eigenvalues of the two
    augmented closed loops a - b K -> list of dict(V, abscissa = the largest real part of the thirteen poles)."""
    lad = ladder(name, speeds)
    out = []
    for k in range(len(speeds) - 1):
        for j in range(points_per_interval):
            V = speeds[k] + (speeds[k + 1] - speeds[k]) * (j + 1) / (points_per_interval + 1)
            d = sn.oracle_design(name, V)
            _, _, K = design_of(lookup(lad["table"], V)[0])
            poles = np.concatenate([np.linalg.eigvals(m) for m in sn.closed_loops(d["A"], d["B"], d["x0"], K)])
            out.append(dict(V=V, abscissa=float(poles.real.max())))
    return out


CROSSING_NODES = (-1.0, 0.5, 1.5)


def crossing_flights(steps=500):
    """The ten aircraft of servo_numpy.compare_flights, each on a three-node table around its own trim speed V (CROSSING_NODES; level
    trims of its airframe, so the table's trim differs from a climbing or turning aircraft's own), flown from their trims over the
    CPU oracle with a speed command of V + 4.5 from step 100 on, which takes the airspeed across the two upper nodes.  Read-only
    arrays: type, x0, table [10][3][FD_NSS], ref0, ref_cmd, pos_100, and after `steps` steps x, u, integ, ref, sat, sigma, pos."""
    key = ("crossing", steps)
    if key not in _CACHE:
        import trim_numpy as tn
        f = sn.compare_flights()
        rows = []
        for i in range(len(f["type"])):
            name, V = tn.TYPES[int(f["type"][i])], float(f["spec"][i][0])
            table = ladder(name, tuple(V + o for o in CROSSING_NODES))["table"]
            step = smn.airframe_step(f["type"][i])
            x, ref, integ, _, sat1, _, pos_100 = fly(step, table, f["x0"][i], f["ref0"][i], np.zeros(3), ln.DT, 100)
            cmd = sn.command(ref, speed=V + 4.5)
            x, ref, integ, u, sat2, sigma, pos = fly(step, table, x, cmd, integ, ln.DT, steps - 100)
            rows.append(dict(type=f["type"][i], x0=f["x0"][i], table=table, ref0=f["ref0"][i], ref_cmd=cmd, x=x, u=u, integ=integ, ref=ref,
                             sat=sat1 + sat2, sigma=sigma, pos=pos, pos_100=pos_100))
        out = {k: np.array([r[k] for r in rows]) for k in rows[0]}
        for v in out.values():
            v.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def mission_square(V):
    """A 300 m square at 100 m whose legs carry different speeds around V: the guidance's V_c moves through the table."""
    sq = smn.square(smn.SQUARE_SIZE, smn.SQUARE_ALTITUDE, V)
    sq[:, smn.WP_SPEED] = (V, V + 4.0, V - 2.0, V + 2.0, V)
    return sq


def mission_flights(steps=300, on=ON_AIRSPEED):
    """The ten aircraft on their three-node tables through `steps` scheduled mission steps of mission_square(20) from their trims
    (acceptance radius servo_mission_numpy.RADIUS: the first waypoint, at the origin, is reached at once and the second leg's speed
    command follows): dict(f = crossing_flights()'s arrays, wps, C, rows = fly_mission's dicts)."""
    key = ("mission", steps, on)
    if key not in _CACHE:
        f = crossing_flights()
        wps, C = mission_square(smn.SHARED_SPEED), smn.consts("PP", smn.RADIUS, "freeze")
        rows = [fly_mission(smn.airframe_step(f["type"][i]), f["table"][i], f["x0"][i], f["ref0"][i], np.zeros(3), wps, C, 0, ln.DT, steps, on)
                for i in range(len(f["type"]))]
        _CACHE[key] = dict(f=f, wps=wps, C=C, rows=rows)
    return _CACHE[key]
