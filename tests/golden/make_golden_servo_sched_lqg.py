"""Writes tests/golden/servo_sched_lqg_reference.npz: the four 15 <-> 30 m/s flights of servo_sched_numpy.BENEFIT on the default
sensor noise under estimate feedback, from the restatement (tests/servo_sched_lqg_numpy.py) over the CPU oracle's RK4.  Per flight and
per way of flying it -- the single design with its single filter, the schedule entered with the command, the schedule entered with
the estimated airspeed, all on the SAME replayed normals -- the peak and the integral of |e_h|, the chatter sums and the err_est sums.

    python tests/golden/make_golden_servo_sched_lqg.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import servo_sched_lqg_numpy as sq       # noqa: E402
import servo_sched_numpy as ssn          # noqa: E402

if __name__ == "__main__":
    got = sq.benefit_flights()
    out = dict(flights=np.array([(n, str(a), str(b)) for n, a, b in ssn.BENEFIT]), seed=np.int64(sq.BENEFIT_SEED))
    for how in sq.HOWS:
        for k, v in got[how].items():
            out[f"{how}_{k}"] = v
    np.savez(os.path.join(HERE, "servo_sched_lqg_reference.npz"), **out)
    for how in sq.HOWS:
        print(how, "peak |e_h|", got[how]["peak"], "chatter", got[how]["chatter"].sum(axis=1))
