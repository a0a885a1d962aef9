"""No-GPU checks of the device Adam step's host side: the per-step scalar block equals torch's own arithmetic bit for bit, and
the rule that decides which update the Adam branch runs."""
import numpy as np
import pytest
import torch

from paa_amd.training_utils.pgd import adam_scalars, adam_unsupported
from paa_amd.training_utils.train import adam_route


@pytest.mark.parametrize("lr", [1e-4, 2e-4, 5e-4 * 0.5 ** 3, 0.01, 1.0])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.99), (0.3, 0.5)])
def test_scalar_block_equals_torch_arithmetic(lr, betas):
    b1, b2 = betas
    t = np.arange(1, 10001, dtype=np.float64)
    got = np.array([adam_scalars(lr, b1, b2, float(s)) for s in t], dtype=np.float32)
    # torch/optim/adam.py _multi_tensor_adam (capturable=False): Python floats, step = state_step.item(); the foreach kernels
    # take the scalar list as float
    want = np.array([(np.float32(-lr / (1 - b1 ** s)), np.float32((1 - b2 ** s) ** 0.5)) for s in t], dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # and the pinned ring slot rounds the same way (a float32 tensor assigned Python floats)
    h = torch.zeros(4, dtype=torch.float32)
    h[2], h[3] = adam_scalars(lr, b1, b2, 7.0)
    assert h[2].item() == float(np.float32(-lr / (1 - b1 ** 7.0))) and h[3].item() == float(np.float32((1 - b2 ** 7.0) ** 0.5))


def _opt(**kw):
    return torch.optim.Adam([torch.nn.Parameter(torch.zeros(1, 16))], lr=1e-3, **kw)


def test_default_adam_runs_on_the_device():
    from paa_amd.training_utils import build
    args = type("A", (), dict(lr=1e-4, step_size=1, gamma=0.5))()
    opt, _ = build.create_optimizer(args, torch.nn.Parameter(torch.zeros(1, 8)))
    assert adam_unsupported(opt) is None
    assert adam_route(opt, 1) == "device" and adam_route(opt, 2) == "device"
    assert adam_route(_opt(betas=(0.5, 0.9), eps=1e-6), 8) == "device"


@pytest.mark.parametrize("kw,name", [(dict(weight_decay=0.01), "weight_decay"), (dict(amsgrad=True), "amsgrad"),
                                     (dict(maximize=True), "maximize")])
def test_other_adam_options_fall_back_on_one_rank_and_raise_on_two(kw, name):
    opt = _opt(**kw)
    assert adam_unsupported(opt) == name
    assert adam_route(opt, 1) == "eager"
    with pytest.raises(NotImplementedError, match=name):
        adam_route(opt, 2)


def test_other_optimizers_and_groups_are_not_the_device_step():
    p = torch.nn.Parameter(torch.zeros(4))
    assert adam_unsupported(torch.optim.SGD([p], lr=0.1)) is not None
    assert adam_unsupported(torch.optim.Adam([p, torch.nn.Parameter(torch.zeros(4))], lr=0.1)) is not None
    assert adam_unsupported(torch.optim.Adam([p], lr=0.1, foreach=False)) is not None
    with pytest.raises(NotImplementedError):
        adam_route(torch.optim.SGD([p], lr=0.1), 2)
