"""CPU tests of the fused Adam and the densification statistics (csrc/optim.hip, sgs_hip/optim.py): the host chain the GPU tests
compare against to the bit (tests/ref_adam.py) is itself pinned, in float64, to torch.optim.Adam; every contract error of
sgs_hip.optim raises with its message before anything is launched; the host-only entry point answers.  No device work here."""
import ctypes as C
import os

import pytest
import torch

import ref_adam
from sgs_hip import _lib
from sgs_hip.optim import GaussianAdam, accumulate_densification_stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("sgs_adam_step", "sgs_adam_max_tensors", "sgs_densify_stats")


@pytest.mark.parametrize("shape", [(1003, 3), (129, 512)])
def test_ref_adam_float64_is_torch_adam(shape):
    """Chain pin: both are float64 evaluations of the same formula, so 1e-12 of the largest entry is generous (measured 3e-16),
    the bound tests/test_loss.py pins ref_loss with.  12 steps, lr changes at every step."""
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(shape, generator=g, dtype=torch.float64)
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([param], lr=0.0, eps=1e-15)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 13):
        lr = 1e-2 * 0.8 ** t
        grad = torch.randn(shape, generator=g, dtype=torch.float64) * 10.0 ** torch.empty(shape[0], 1, dtype=torch.float64).uniform_(-8, -2, generator=g)
        opt.param_groups[0]["lr"] = lr
        param.grad = grad.clone()
        opt.step()
        p, m, v = ref_adam.adam_step(p, grad, m, v, t, lr, eps=1e-15)
    st = opt.state[param]
    errs = {}
    for name, got, want in (("p", p, param.detach()), ("exp_avg", m, st["exp_avg"]), ("exp_avg_sq", v, st["exp_avg_sq"])):
        errs[name] = float((got - want).abs().max() / want.abs().max())
    print(shape, errs)
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert float(st["step"]) == 12


def test_ref_adam_mask_keeps_invisible_rows():
    g = torch.Generator().manual_seed(6)
    p, grad, m, v = (torch.randn(9, 4, generator=g) for _ in range(4))
    v = v.abs()
    mask = torch.tensor([True, False, True, True, False, False, True, False, True])
    p1, m1, v1 = ref_adam.adam_step(p, grad, m, v, 3, 1e-2, mask=mask)
    pd, md, vd = ref_adam.adam_step(p, grad, m, v, 3, 1e-2)
    for a, d, old in ((p1, pd, p), (m1, md, m), (v1, vd, v)):
        assert torch.equal(a[mask], d[mask]) and torch.equal(a[~mask], old[~mask])


def test_library_declares_and_exports_the_new_entry_points():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "sgs_raster.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(lib, s) and s + "(" in hdr, s
    assert "sgs_adam_tensor" in hdr


def test_host_only_entry_and_host_side_contract_of_the_abi():
    lib = _lib.load()
    cap = lib.sgs_adam_max_tensors()
    assert cap >= 8
    # nothing to do: 0 launches, no device work
    assert lib.sgs_adam_step(None, 0, None, None) == 0
    empty = (_lib.AdamTensor * 2)()
    assert lib.sgs_adam_step(empty, 2, None, None) == 0
    # contract errors are answered on the host, before any launch
    buf = (C.c_float * 8)()
    a = C.addressof(buf)

    def one(**kw):
        d = dict(param=a, grad=a, exp_avg=a, exp_avg_sq=a, rows=2, numel=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, step=1)
        d.update(kw)
        t = (_lib.AdamTensor * 1)()
        for k, v in d.items():
            setattr(t[0], k, v)
        return t

    for kw, msg in ((dict(step=0), "step must be >= 1"), (dict(rows=3), "multiple of rows"), (dict(grad=None), "null pointer"),
                    (dict(beta2=1.0), "hyper-parameters"), (dict(exp_avg=a + 2), "aligned to 4 bytes")):
        assert lib.sgs_adam_step(one(**kw), 1, None, None) < 0, kw
        assert msg in _lib.last_error(), (kw, _lib.last_error())
    assert lib.sgs_adam_step(None, 3, None, None) < 0
    two = (_lib.AdamTensor * 2)()
    for t, rows in zip(two, (2, 4)):
        for k, v in dict(param=a, grad=a, exp_avg=a, exp_avg_sq=a, rows=rows, numel=8, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, step=1).items():
            setattr(t, k, v)
    assert lib.sgs_adam_step(two, 2, a, None) < 0 and "same number of rows" in _lib.last_error()
    assert lib.sgs_densify_stats(-1, a, 3, a, None, a, a, a, None, None) < 0
    assert lib.sgs_densify_stats(4, a, 1, a, None, a, a, a, None, None) < 0 and "pitch" in _lib.last_error()
    assert lib.sgs_densify_stats(4, None, 3, a, None, a, a, a, None, None) < 0
    assert lib.sgs_densify_stats(0, None, 3, None, None, None, None, None, None, None) == 0


def _param(shape=(6, 3), dtype=torch.float32, grad=True):
    p = torch.nn.Parameter(torch.ones(shape, dtype=dtype))
    if grad:
        p.grad = torch.ones(shape, dtype=dtype)
    return p


def _raises_and_launches_nothing(opt, msg, **kw):
    params = [p for g in opt.param_groups for p in g["params"] if p.device.type != "meta"]
    before = [p.detach().clone() for p in params]
    with pytest.raises(RuntimeError, match=msg):
        opt.step(**kw)
    assert opt.last_launches == 0 and len(opt.state) == 0
    assert all(torch.equal(b, p.detach()) for b, p in zip(before, params))


@pytest.mark.parametrize("kw,msg", [(dict(weight_decay=0.1), "weight_decay must be 0"), (dict(amsgrad=True), "amsgrad=True is not implemented"),
                                    (dict(maximize=True), "maximize=True is not implemented"),
                                    (dict(capturable=True), "capturable=True is not implemented"),
                                    (dict(differentiable=True), "differentiable=True is not implemented")])
def test_unsupported_options_raise(kw, msg):
    with pytest.raises(RuntimeError, match=msg):
        GaussianAdam([_param()], lr=1e-3, **kw)
    # ... and when a group is edited after construction
    opt = GaussianAdam([_param()], lr=1e-3)
    opt.param_groups[0].update(kw)
    _raises_and_launches_nothing(opt, msg)


def test_tensor_contract_errors_raise_before_any_launch():
    _raises_and_launches_nothing(GaussianAdam([_param(dtype=torch.float64)], lr=1e-3), "must be float32")
    _raises_and_launches_nothing(GaussianAdam([_param(dtype=torch.float16)], lr=1e-3), "must be float32")
    # non-contiguous parameter; non-contiguous gradient
    p = torch.nn.Parameter(torch.ones(3, 6).t())
    p.grad = torch.ones(6, 3)
    _raises_and_launches_nothing(GaussianAdam([p], lr=1e-3), "must be contiguous")
    p = _param()
    p.grad = torch.ones(3, 6).t()
    _raises_and_launches_nothing(GaussianAdam([p], lr=1e-3), "must be contiguous")
    # CPU tensors: there is no CPU path
    _raises_and_launches_nothing(GaussianAdam([_param()], lr=1e-3), "no CPU path")
    # parameters on different devices
    q = torch.nn.Parameter(torch.ones(6, 3, device="meta"))
    q.grad = torch.ones(6, 3, device="meta")
    _raises_and_launches_nothing(GaussianAdam([{"params": [_param()]}, {"params": [q]}], lr=1e-3), "different devices")


def test_mask_contract_errors_raise_before_any_launch():
    def opt():
        return GaussianAdam([{"params": [_param((6, 3))]}, {"params": [_param((6, 1))]}], lr=1e-3)
    _raises_and_launches_nothing(opt(), "one entry per row", visibility=torch.ones(5, dtype=torch.bool))
    _raises_and_launches_nothing(opt(), "one entry per row", visibility=torch.ones(6, 1, dtype=torch.bool))
    _raises_and_launches_nothing(opt(), "must be bool or uint8", visibility=torch.ones(6, dtype=torch.float32))
    _raises_and_launches_nothing(opt(), "must be bool or uint8", visibility=torch.ones(6, dtype=torch.int64))
    _raises_and_launches_nothing(opt(), "another device", visibility=torch.ones(6, dtype=torch.bool, device="meta"))
    mixed = GaussianAdam([{"params": [_param((6, 3))]}, {"params": [_param((7, 3))]}], lr=1e-3)
    _raises_and_launches_nothing(mixed, "one leading size", visibility=torch.ones(6, dtype=torch.bool))
    # a parameter without a gradient does not count: the mask then fits, and what is left is the CPU error
    skipped = GaussianAdam([{"params": [_param((6, 3))]}, {"params": [_param((7, 3), grad=False)]}], lr=1e-3)
    _raises_and_launches_nothing(skipped, "no CPU path", visibility=torch.ones(6, dtype=torch.bool))


def test_group_keys_and_state_dict_layout_are_torch_adams():
    ours = GaussianAdam([{"params": [_param()], "lr": 1e-2, "name": "xyz"}], lr=0.0, eps=1e-15)
    theirs = torch.optim.Adam([{"params": [_param()], "lr": 1e-2, "name": "xyz"}], lr=0.0, eps=1e-15)
    assert list(ours.param_groups[0].keys()) == list(theirs.param_groups[0].keys())
    assert ours.state_dict()["param_groups"] == theirs.state_dict()["param_groups"]
    # no gradient anywhere: a step is a no-op, not an error
    idle = GaussianAdam([_param(grad=False)], lr=1e-3)
    idle.step()
    assert idle.last_launches == 0 and len(idle.state) == 0


def test_densification_stats_contract_errors():
    P = 5
    acc, den, mr = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
    vg, radii = torch.zeros(P, 3), torch.ones(P, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        accumulate_densification_stats(acc, den, mr, vg, radii)
    with pytest.raises(RuntimeError, match="radii must be int32"):
        accumulate_densification_stats(acc, den, mr, vg, radii.long())
    with pytest.raises(RuntimeError, match="denom must be a contiguous tensor of 5 entries"):
        accumulate_densification_stats(acc, torch.zeros(P + 1, 1), mr, vg, radii)
    with pytest.raises(RuntimeError, match="max_radii2D must be float32"):
        accumulate_densification_stats(acc, den, mr.double(), vg, radii)
    with pytest.raises(RuntimeError, match="viewspace_grad must have shape"):
        accumulate_densification_stats(acc, den, mr, torch.zeros(P, 1), radii)
    with pytest.raises(RuntimeError, match="one entry per row"):
        accumulate_densification_stats(acc, den, mr, vg, radii, visibility=torch.ones(P + 1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="another device"):
        accumulate_densification_stats(acc, den, mr, vg.to("meta"), radii)
    assert float(acc.sum()) == 0 and float(den.sum()) == 0
