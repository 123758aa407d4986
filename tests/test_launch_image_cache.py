"""CPU-side: the env's prepared launch image is a copy of the parameter table and the env constants, so it must be filled again
whenever either changes -- a tensor written in place (a curriculum switch writes env_consts), a tensor replaced, another
n_types -- and must not be filled again otherwise.  The fill itself is a device launch; here it is a counting stand-in."""
import numpy as np
import torch

from hcrl_amd import layout as L
from hcrl_amd.rate_env import LaunchImage
from hcrl_amd.params import param_table
from hcrl_amd.samplers import env_consts


def _image(precision="mixed"):
    calls = []

    def fill(params, n_types, ec, fp32_eval, image):
        calls.append((params.clone(), n_types, ec.clone(), fp32_eval))
        image[L.FD_IMG_EC:L.FD_IMG_EC + L.FD_NEC] = ec
    return LaunchImage(precision, fill), calls


def _tensors():
    return (torch.as_tensor(param_table(("rc_plane", "cessna"))), torch.as_tensor(env_consts("medium", 10.0, 0.02, "step")))


def test_layout_of_the_image():
    assert L.FD_ECD_INTS >= L.FD_NEC and L.FD_ECD_INTS + 2 <= L.FD_IMG_PARAMS          # four int32 counts in two fp64 slots
    assert L.FD_NIMG == L.FD_IMG_PARAMS + 8 * L.FD_NP_STAGED and L.FD_NP_STAGED >= L.FD_NP_USED


def test_filled_once_while_nothing_changes():
    img, calls = _image()
    P, EC = _tensors()
    first = img.ensure(P, 2, EC)
    for _ in range(5):
        assert img.ensure(P, 2, EC) is first
    assert len(calls) == 1 and img.fills == 1
    assert calls[0][3] is True and _image("f64")[0].fp32_eval is False


def test_refilled_after_in_place_write_of_env_consts():
    img, calls = _image()
    P, EC = _tensors()
    buf = img.ensure(P, 2, EC)
    EC.copy_(torch.as_tensor(env_consts("hard", 5.0, 0.02, "sine")))             # what a curriculum switch does
    assert img.ensure(P, 2, EC) is buf                                            # same buffer, new content
    assert len(calls) == 2
    assert np.array_equal(calls[1][2].numpy(), env_consts("hard", 5.0, 0.02, "sine"))
    assert np.array_equal(buf[L.FD_IMG_EC:L.FD_IMG_EC + L.FD_NEC].numpy(), env_consts("hard", 5.0, 0.02, "sine"))
    EC[L.FD_EC_MAX_STEPS] = 123.0                                                 # a single word
    img.ensure(P, 2, EC)
    assert len(calls) == 3 and calls[2][2][L.FD_EC_MAX_STEPS] == 123.0
    img.ensure(P, 2, EC)
    assert len(calls) == 3


def test_refilled_after_parameter_table_changes():
    img, calls = _image()
    P, EC = _tensors()
    img.ensure(P, 2, EC)
    P[1, L.FD_P_MASS] *= 1.25                                                     # in place
    img.ensure(P, 2, EC)
    assert len(calls) == 2 and calls[1][0][1, L.FD_P_MASS] == P[1, L.FD_P_MASS]
    P2 = P.clone()                                                                # another tensor with the same content
    img.ensure(P2, 2, EC)
    assert len(calls) == 3
    img.ensure(P2, 1, EC)                                                         # fewer types of the same table
    assert len(calls) == 4 and calls[3][1] == 1
    EC2 = EC.clone()
    img.ensure(P2, 1, EC2)
    assert len(calls) == 5
    img.ensure(P2, 1, EC2)
    assert len(calls) == 5


def test_invalidate_forces_a_fill():
    img, calls = _image()
    P, EC = _tensors()
    img.ensure(P, 2, EC)
    img.invalidate()
    img.ensure(P, 2, EC)
    assert len(calls) == 2
