"""CPU: gradient-norm clipping without a device — the float64 reference against torch's clip_grad_norm_, the four new entry points in
the signature table, the driver flag, and the untouched default path of EgoAdamW.step."""
import inspect
import types

import numpy as np
import torch

from egoscaler_amd import _abi, driver, ops
from egoscaler_amd.optim import EgoAdamW
from tests import grad_clip_ref as R


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * sc for s, sc in (((37, 5), 1.0), ((1,), 3.0), ((1025,), 0.1), ((64, 64), 2.0))]


def test_reference_agrees_with_torch_clip_grad_norm():
    """torch sums in fp32: 1e-5 relative on the norm and on the clipped gradients."""
    for seed, max_norm in ((0, 1.0), (1, 1e3), (2, 0.01)):
        grads = _tensors(seed)
        ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        tn = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        norm, coef, eff = R.clip_scale(R.total_sumsq([R.seg_sumsq(g) for g in grads]), 1.0, max_norm)
        assert abs(float(norm) - tn) <= 1e-5 * tn
        assert (float(coef) < 1.0) == (tn + 1e-6 > max_norm)
        for p, g in zip(ps, grads):
            ref = g * float(eff)
            assert float((p.grad - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_reference_edge_cases():
    n, c, e = R.clip_scale(float("inf"), 0.5, 1.0)
    assert np.isinf(n) and c == 0 and e == 0
    n, c, e = R.clip_scale(float("nan"), 0.5, 1.0)
    assert np.isnan(n) and np.isnan(c) and np.isnan(e)
    n, c, e = R.clip_scale(4.0, 0.3, float("inf"))
    assert c == 1 and e.tobytes() == np.float32(0.3).tobytes()
    assert R.stats_after([(4.0, 1.0, 10.0), (400.0, 1.0, 10.0), (float("inf"), 1.0, 10.0), (float("nan"), 1.0, 10.0)]) == [4, 1, 2, 22.0, 20.0]


def test_new_symbols_are_declared():
    for name, nargs in (("egomi_grad_sumsq", 11), ("egomi_clip_scale", 6), ("egomi_adamw_ds", 15), ("egomi_adamw_g16_ds", 15)):
        assert name in _abi.PROTOS and len(_abi.PROTOS[name][1]) == nargs, name
    assert [p for p, _ in _abi.PROTOS["egomi_adamw_ds"][1]][12] == "grad_scale_dev"
    assert len(_abi.PROTOS["egomi_adamw"][1]) == 15 and [p for p, _ in _abi.PROTOS["egomi_adamw"][1]][12] == "grad_scale"


def test_driver_flag():
    assert driver.parse_args(["train", "--tiny", "--max_grad_norm", "1.0"]).max_grad_norm == 1.0
    assert driver.parse_args(["train", "--tiny", "--max_grad_norm", "inf"]).max_grad_norm == float("inf")
    assert driver.parse_args(["train", "--tiny"]).max_grad_norm == 0.0


class _StubEngine:
    """What EgoAdamW.step touches on its synchronous path, recording every use."""

    def __init__(self, grads):
        self.main_grad, self.reduced_grad, self.wT, self.trainable = grads, {}, {}, {}
        self.device, self.layer_final_hook, self.log = torch.device("cpu"), None, []

    def param_group_of(self, name):
        return "pre"

    def wait_param_updates(self):
        self.log.append("wait")

    def after_weights_update(self):
        self.log.append("after")


def test_default_step_takes_no_new_branch(monkeypatch):
    """max_grad_norm=None: step() makes exactly the ops.adamw calls of the parent commit (host grad_scale, no device scale) and never
    touches the table, the norm kernels or their state."""
    w = torch.nn.Linear(3, 2)
    eng = _StubEngine({n: torch.ones_like(p) for n, p in w.named_parameters()})
    model = types.SimpleNamespace(engine=eng, named_parameters=w.named_parameters)
    calls = []
    monkeypatch.setattr(ops, "adamw", lambda *a, **k: calls.append((a, k)))
    for name in ("grad_sumsq", "clip_scale", "GradTable"):
        monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("the default path reached the clipping code")))
    opt = EgoAdamW(model, lr=1e-3)
    assert opt.max_grad_norm is None
    opt.step(grad_scale=0.25)
    assert len(calls) == 2 and all(not k and len(a) == 12 and a[11] == 0.25 for a, k in calls)
    assert eng.log == ["wait", "after"]
    assert opt._clip_table is None and opt._clip_out is None and opt._clip_scale is None
    # clipping on, but no state entry has a gradient: the step updates nothing and builds no table, as the unclipped step does
    eng.main_grad, eng.log = {}, []
    opt2 = EgoAdamW(model, lr=1e-3, max_grad_norm=1.0)
    opt2.step()
    assert len(calls) == 2 and eng.log == ["wait", "after"] and opt2._clip_table is None
    # max_grad_norm taken back after clipped steps: the update follows it, not the device scale left behind
    eng.main_grad = {n: torch.ones_like(p) for n, p in w.named_parameters()}
    opt2._clip_scale, opt2.max_grad_norm = object(), None
    opt2.step(grad_scale=0.5)
    assert len(calls) == 4 and all(not k and a[11] == 0.5 for a, k in calls[2:])
    assert "max_grad_norm=None" in str(inspect.signature(EgoAdamW.__init__))
    assert sorted(opt.state_dict()) == ["state", "t"] and sorted(next(iter(opt.state_dict()["state"].values()))) == ["m", "master", "v"]
