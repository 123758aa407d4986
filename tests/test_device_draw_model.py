"""The host model of the in-kernel draws (tests/philox_numpy.py) checked on its own, without a device: the generator against the
published known-answer vectors, the counter layouts against each other (no two consumers share a counter under one seed), the
command draw's distribution on 2^20 counters, and the word -> uniform conversion over all of its 2^24 inputs -- the model's and,
through a stand-alone host program compiled from csrc/philox.hpp (tests/host/philox_check.cpp), the library's own.

Statistical bounds are 5 sigma of the binomial count they test (N p +- 5 sqrt(N p (1 - p))): they follow from N alone.
tests/test_gpu_device_draws.py then holds the kernels to this model value by value.
"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import philox_numpy as pn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RATES = np.radians([180.0, 180.0, 160.0])
SCALES = {"easy": 0.3, "medium": 0.5, "hard": 0.7}
N_STAT, STAT_SEED = 1 << 20, 2024


# ---- generator ----------------------------------------------------------------------------------------------------------------
KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, expected
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "pi-digits", "ones"])
def test_philox_known_answers(ctr, key, want):
    got = pn.philox(key[0] | (key[1] << 32), *ctr)
    assert got.dtype == np.uint32 and got.shape == (4,)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_philox_is_vectorised_and_reads_both_key_halves():
    """A batch equals its scalar calls; the high key half and every counter word change the block."""
    c = np.arange(5, dtype=np.int64)
    batch = pn.philox((7 << 32) | 9, c, 3, 2 * c, 1)
    for k in range(5):
        assert np.array_equal(batch[k], pn.philox((7 << 32) | 9, k, 3, 2 * k, 1))
    base = pn.philox(9, 1, 2, 3, 4)
    for other in (pn.philox((1 << 32) | 9, 1, 2, 3, 4), pn.philox(9, 0, 2, 3, 4), pn.philox(9, 1, 0, 3, 4),
                  pn.philox(9, 1, 2, 0, 4), pn.philox(9, 1, 2, 3, 0)):
        assert not np.array_equal(base, other)


# ---- counter layouts ----------------------------------------------------------------------------------------------------------
def _pack(ctr):
    """Counter tuples [..., 4] -> one integer each (every word of this enumeration is below 2^16)."""
    c = np.asarray(ctr, np.int64).reshape(-1, 4)
    assert c.min() >= 0 and c.max() < 1 << 16
    return ((c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]).astype(np.uint64)


def test_counter_streams_are_disjoint_under_one_seed():
    """1024 rows, episodes 0..3, steps 0..8: the counters of the reset record, the randomisation rows, the random walk, the gust
    update, the action noise and the sensor blocks never coincide, within a consumer or across two (one training run hands all
    of them the same seed, and equal counters under one key are equal numbers)."""
    rows, eps, steps = np.arange(1024), np.arange(4), np.arange(9)
    R, E = np.meshgrid(rows, eps, indexing="ij")
    R3, E3, S3 = np.meshgrid(rows, eps, steps, indexing="ij")
    sets = {
        "reset": pn.reset_counters(R, E),
        "dr_reset": pn.dr_reset_counters(R, E),
        "random_walk": pn.step_counters(R3, E3, S3, pn.W_RANDOM_WALK),
        "gust": pn.step_counters(R3, E3, S3, pn.W_GUST),
        "action": np.stack([pn.row_counters(rows, s, pn.W_ACTION, 1) for s in steps]),
        "sensor": np.stack([pn.row_counters(rows, s, pn.W_SENSOR, 5) for s in steps]),
    }
    want = {"reset": 1024 * 4 * 4, "dr_reset": 1024 * 4 * 4, "random_walk": 1024 * 4 * 9, "gust": 1024 * 4 * 9,
            "action": 1024 * 9, "sensor": 1024 * 9 * 5}
    packed = {}
    for name, ctr in sets.items():
        packed[name] = _pack(ctr)
        assert packed[name].size == want[name], name
        assert np.unique(packed[name]).size == packed[name].size, f"{name}: a counter repeats inside the consumer"
    names = list(packed)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert np.intersect1d(packed[a], packed[b]).size == 0, f"{a} and {b} share a counter"


def test_row_counters_carry_the_high_row_half_and_the_full_step_word():
    c = pn.row_counters(np.array([5, (3 << 32) + 5]), 0xFFFFFFFF, pn.W_ACTION, 1)
    assert c[0, 0].tolist() == [5, 0, 0xFFFFFFFF, 0x51] and c[1, 0].tolist() == [5, 3, 0xFFFFFFFF, 0x51]


# ---- command draw -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stat_blocks():
    b = pn.reset_blocks(STAT_SEED, np.arange(N_STAT), 0)
    b.setflags(write=False)
    return b


def _binomial_ok(count, n, p):
    return abs(count - n * p) <= 5.0 * np.sqrt(n * p * (1.0 - p))


@pytest.mark.parametrize("difficulty", ["easy", "medium", "hard"])
@pytest.mark.parametrize("cmd_name,cmd", [("step", pn.CMD_STEP), ("ramp", pn.CMD_RAMP), ("sine", pn.CMD_SINE)])
def test_command_draw_statistics(cmd_name, cmd, difficulty):
    scale = SCALES[difficulty]
    rec = pn.reset_record(STAT_SEED, np.arange(N_STAT), 0, cmd, scale, MAX_RATES, blocks=_stat_blocks())
    sine = cmd == pn.CMD_SINE
    counts = (1, 2) if sine else (1, 2, 3)
    # number of active axes: uniform on its support, nothing outside it
    assert set(np.unique(rec.count)) == set(counts)
    for k in counts:
        assert _binomial_ok(int((rec.count == k).sum()), N_STAT, 1.0 / len(counts)), ("count", k)
    # the idle axes are exactly zero, the active ones are not; `count` of them are active
    active = rec.rec[:, 8:11] != 0.0
    assert np.array_equal(active, rec.position < rec.count[:, None]) and np.array_equal(active.sum(1), rec.count)
    # which axes: each of the 3 singles, 3 pairs and the 1 triple equally likely given the count
    code = active[:, 0] * 1 + active[:, 1] * 2 + active[:, 2] * 4
    for k, subsets in ((1, (1, 2, 4)), (2, (3, 5, 6)), (3, (7,))):
        sel = rec.count == k
        nk = int(sel.sum())
        assert set(np.unique(code[sel])) <= set(subsets)
        for s in subsets:
            assert _binomial_ok(int((code[sel] == s).sum()), nk, 1.0 / len(subsets)), ("subset", k, s)
    # the permutation itself: all six orders equally likely
    order = rec.first * 2 + (rec.second == (rec.first + 2) % 3)
    for o in range(6):
        assert _binomial_ok(int((order == o).sum()), N_STAT, 1.0 / 6.0), ("order", o)
    # signs: none for sine; otherwise fair on every axis and independent between two active axes
    neg = rec.rec[:, 8:11] < 0.0
    if sine:
        assert not neg.any()
    else:
        for a in range(3):
            na = int(active[:, a].sum())
            assert _binomial_ok(int(neg[active[:, a], a].sum()), na, 0.5), ("sign", a)
            for b in range(a + 1, 3):
                both = active[:, a] & active[:, b]
                for sa in (False, True):
                    for sb in (False, True):
                        hit = int(((neg[both, a] == sa) & (neg[both, b] == sb)).sum())
                        assert _binomial_ok(hit, int(both.sum()), 0.25), ("sign pair", a, b, sa, sb)
            # and independent of where the axis sits in the permutation
            for pos in range(3):
                sel = active[:, a] & (rec.position[:, a] == pos)
                assert _binomial_ok(int(neg[sel, a].sum()), int(sel.sum()), 0.5), ("sign at place", a, pos)
    # magnitudes in [0.3, 1] scale max_rate (sine: half of it); the fp32 literals 0.3f + 0.7f exceed 1 by 2^-25, hence the slack
    half = 0.5 if sine else 1.0
    unit = np.abs(rec.rec[:, 8:11]) / (float(np.float32(scale)) * half * MAX_RATES[None, :])
    assert unit[active].min() >= 0.3 * (1 - 2.0 ** -22) and unit[active].max() <= 1.0 + 2.0 ** -22
    assert unit[active].min() < 0.3001 and unit[active].max() > 0.9999                  # and the range is used
    for q in (0.25, 0.5, 0.75):                                                        # uniform in between
        assert _binomial_ok(int((unit[active] < 0.3 + 0.7 * q).sum()), int(active.sum()), q), ("magnitude quantile", q)
    # frequency in [0.1, 2] Hz for sine, zero otherwise
    if sine:
        f = rec.rec[:, 11]
        assert f.min() >= 0.1 * (1 - 2.0 ** -22) and f.max() <= 2.0 * (1 + 2.0 ** -22) and f.min() < 0.1001 and f.max() > 1.9999
    else:
        assert not rec.rec[:, 11].any()


def test_random_walk_record_has_no_command_words():
    rec = pn.reset_record(STAT_SEED, np.arange(4096), 0, pn.CMD_RANDOM_WALK, 0.3, MAX_RATES)
    assert not rec.rec[:, 8:].any() and not rec.count.any()


# ---- the uniform conversion ---------------------------------------------------------------------------------------------------
def _all_inputs():
    return np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)


def test_model_u01_is_strictly_inside_the_unit_interval_for_every_input():
    u = pn.u01(_all_inputs())
    assert u.dtype == np.float32 and float(u.min()) > 0.0 and float(u.max()) < 1.0
    plain = pn.u01_unclamped(_all_inputs())
    # the unclamped formula fails this very check at its last input -- and only there does the clamp change a bit
    assert float(plain.max()) == 1.0 and int((plain != u).sum()) == 1 and plain[-1] != u[-1]
    assert np.all(np.diff(u.astype(np.float64)) >= 0.0)


def _hipcc():
    exe = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(exe), "hipcc not found: the library itself cannot be built without it"
    return exe


def test_library_u01_and_generator_on_the_host_under_sanitizers(tmp_path):
    """csrc/philox.hpp compiled for the host with AddressSanitizer and UBSan into a stand-alone program: it checks the three
    known-answer vectors against philox4, sweeps philox_u01 over its 2^24 inputs (exit status 0 only if min > 0 and max < 1) and
    writes the results, which must equal the model's bit for bit."""
    exe, dump = str(tmp_path / "philox_check"), str(tmp_path / "u01.f32")
    subprocess.run([_hipcc(), "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "host", "philox_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe, dump], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", (run.returncode, run.stdout, run.stderr)
    lines = run.stdout.splitlines()
    assert [ln.split()[-1] for ln in lines] == ["ok"] * 4, run.stdout
    assert "min 0x1p-25 max 0x1.fffffep-1" in lines[3], lines[3]
    got = np.fromfile(dump, dtype=np.float32)
    assert got.size == 1 << 24 and float(got.min()) > 0.0 and float(got.max()) < 1.0
    assert np.array_equal(got.view(np.uint32), pn.u01(_all_inputs()).view(np.uint32))
