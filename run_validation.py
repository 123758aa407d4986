#!/usr/bin/env python3
"""Fleet-wide physics validation: fly one scenario on two fleets and compare every pair of aircraft on the device.

    python run_validation.py --a f64 --b mixed --type-a rc_plane --type-b rc_plane --aircraft 65536 [--spread]
    python run_validation.py --scenario trimmed --airspeed 25 --climb-deg 3 --turn-rate 0.1 --type-b cessna
--scenario level (default) flies the reference's fixed controls; trimmed solves every fleet's own equilibrium first.
Exit status 0 when every aircraft passes the scenario's thresholds (hcrl_amd/validation.py)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcrl_amd  # noqa: E402,F401
from hcrl_amd.validation import main  # noqa: E402

if __name__ == "__main__":
    sys.exit(main())
