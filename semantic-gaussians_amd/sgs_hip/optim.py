"""The rest of an optimisation step after loss.backward() (train.py:154-180) on the device (csrc/optim.hip):

`GaussianAdam`, torch.optim.Adam for the Gaussian parameter groups in ONE kernel launch per step, with an optional per-Gaussian
visibility mask (rows that the current view does not see are neither read nor written), and
`accumulate_densification_stats`, the three boolean-indexed statements of train.py:158-161 / add_densification_stats
(model/gaussian_model.py:608-612) as one launch that never makes the host wait.

    self.optimizer = GaussianAdam(l, lr=0.0, eps=1e-15)          # instead of: torch.optim.Adam(l, lr=0.0, eps=1e-15)

The state layout and the param_group keys are torch.optim.Adam's, so state_dict() travels both ways and the reference's state
surgery (replace_tensor_to_optimizer, _prune_optimizer, cat_tensors_to_optimizer) works unchanged.  float32 device tensors
only; no weight_decay, amsgrad, maximize, capturable or differentiable.  No CPU fallback: the HIP library is required.
"""
import ctypes as C

import torch

from . import _lib

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")


def _check_mask(visibility, rows, device, what="visibility"):
    """dtype, length, device -- in that order, and before the tensors' own device is judged (the order the CPU tests rely on)"""
    if not torch.is_tensor(visibility):
        raise RuntimeError(f"{what} must be a torch tensor")
    if visibility.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{what} must be bool or uint8 (got {visibility.dtype})")
    if visibility.dim() != 1 or visibility.shape[0] != rows:
        raise RuntimeError(f"{what} must have one entry per row: expected shape ({rows},), got {tuple(visibility.shape)}")
    if visibility.device != device:
        raise RuntimeError(f"{what} is on another device ({visibility.device}) than the tensors ({device})")
    return visibility.contiguous()


class GaussianAdam(torch.optim.Optimizer):
    """torch.optim.Adam (no amsgrad, weight_decay = 0) whose step() is one fused HIP launch over every parameter of every group.

    step(visibility=None): `visibility` is a bool / uint8 device tensor with one entry per row (leading index) of the parameters,
    which must then all have the same leading size.  Invisible rows keep param, exp_avg and exp_avg_sq bit for bit; visible rows
    get exactly the dense update.  "step" counts calls, not visits.  `last_launches` is the kernel-launch count of the last step()."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        if torch.is_tensor(lr):
            raise RuntimeError("GaussianAdam: lr must be a Python number, not a tensor")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        # the keys (and their order) of torch.optim.Adam's groups: state_dict() loads into either class
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)
        self.last_launches = 0
        for group in self.param_groups:
            self._check_group(group)

    @staticmethod
    def _check_group(group):
        if group["weight_decay"] != 0:
            raise RuntimeError(f"GaussianAdam: weight_decay must be 0 (got {group['weight_decay']}): it is not implemented")
        for key in _UNSUPPORTED:
            if group.get(key):
                raise RuntimeError(f"GaussianAdam: {key}=True is not implemented")

    def _collect(self):
        """Every (group, parameter) that has a gradient, checked; nothing is created or changed here."""
        todo, device = [], None
        for group in self.param_groups:
            self._check_group(group)   # (groups are plain dicts: a caller may have edited them since __init__)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if p.dtype != torch.float32 or g.dtype != torch.float32:
                    raise RuntimeError(f"GaussianAdam: parameters and gradients must be float32 (got {p.dtype}, {g.dtype})")
                if g.is_sparse:
                    raise RuntimeError("GaussianAdam: sparse gradients are not implemented")
                if not (p.is_contiguous() and g.is_contiguous()):
                    raise RuntimeError("GaussianAdam: parameters and gradients must be contiguous")
                if g.shape != p.shape:
                    raise RuntimeError(f"GaussianAdam: gradient shape {tuple(g.shape)} differs from the parameter's {tuple(p.shape)}")
                if device is None:
                    device = p.device
                if p.device != device or g.device != device:
                    raise RuntimeError(f"GaussianAdam: parameters on different devices ({device}, {p.device}, {g.device})")
                st = self.state.get(p)
                if st:   # (state a caller put there: the reference's surgery, load_state_dict)
                    for key in ("exp_avg", "exp_avg_sq"):
                        t = st[key]
                        if t.dtype != torch.float32 or t.device != device or not t.is_contiguous() or t.shape != p.shape:
                            raise RuntimeError(f"GaussianAdam: state '{key}' must be a contiguous float32 tensor of the parameter's shape "
                                               f"on its device (got {t.dtype}, {tuple(t.shape)}, {t.device})")
                todo.append((group, p))
        return todo, device

    @torch.no_grad()
    def step(self, closure=None, visibility=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.last_launches = 0
        todo, device = self._collect()
        if not todo:
            return loss
        rows = [p.shape[0] if p.dim() else 1 for _, p in todo]
        if visibility is not None:
            if len(set(rows)) != 1:
                raise RuntimeError(f"GaussianAdam: a visibility mask needs parameters of one leading size (got {sorted(set(rows))})")
            visibility = _check_mask(visibility, rows[0], device, "GaussianAdam: visibility")
        if device.type != "cuda":
            raise RuntimeError("GaussianAdam: parameters and gradients must be GPU tensors (there is no CPU path)")
        lib = _lib.load()
        # from here on nothing raises before the launch
        table = (_lib.AdamTensor * len(todo))()
        for d, r, (group, p) in zip(table, rows, todo):
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if not torch.is_tensor(st["step"]):
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
            st["step"] += 1   # a CPU scalar: no device work
            d.param, d.grad = p.data_ptr(), p.grad.data_ptr()
            d.exp_avg, d.exp_avg_sq = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            d.rows, d.numel = r, p.numel()
            d.lr, d.beta1, d.beta2, d.eps = float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"])
            d.step = int(st["step"].item())
        with torch.cuda.device(device):
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            rc = lib.sgs_adam_step(table, len(todo), visibility.data_ptr() if visibility is not None else None, stream)
        self.last_launches = _lib.check(rc, "adam step")
        return loss


def accumulate_densification_stats(xyz_gradient_accum, denom, max_radii2D, viewspace_grad, radii, visibility=None,
                                   return_visibility=False):
    """In place, for every Gaussian with radii > 0 (or visibility, where given):
        xyz_gradient_accum += |viewspace_grad[:, :2]|;  denom += 1;  max_radii2D = max(max_radii2D, radii)
    -- train.py:158-161 and add_densification_stats, without the host waits of boolean indexing.  Shapes as the reference keeps
    them: (P,1) or (P,), (P,1) or (P,), (P,), (P,>=2) and int32 (P,).  return_visibility=True returns the bool mask the
    statistics were taken with (radii > 0 unless `visibility` is given): the mask for GaussianAdam.step."""
    P = radii.shape[0] if torch.is_tensor(radii) and radii.dim() == 1 else -1
    named = (("xyz_gradient_accum", xyz_gradient_accum), ("denom", denom), ("max_radii2D", max_radii2D),
             ("viewspace_grad", viewspace_grad), ("radii", radii))
    for name, t in named:
        if not torch.is_tensor(t):
            raise RuntimeError(f"densification stats: {name} must be a torch tensor")
    if radii.dtype != torch.int32 or P < 0:
        raise RuntimeError(f"densification stats: radii must be int32 of shape (P,) (got {radii.dtype}, {tuple(radii.shape)})")
    for name, t in named[:4]:
        if t.dtype != torch.float32:
            raise RuntimeError(f"densification stats: {name} must be float32 (got {t.dtype})")
    for name, t in named[:3]:
        if t.numel() != P or t.shape[0] != P or not t.is_contiguous():
            raise RuntimeError(f"densification stats: {name} must be a contiguous tensor of {P} entries (got {tuple(t.shape)})")
    if viewspace_grad.dim() != 2 or viewspace_grad.shape[0] != P or viewspace_grad.shape[1] < 2:
        raise RuntimeError(f"densification stats: viewspace_grad must have shape ({P}, >= 2) (got {tuple(viewspace_grad.shape)})")
    dev = radii.device
    for name, t in named:
        if t.device != dev:
            raise RuntimeError(f"densification stats: {name} is on another device ({t.device}) than radii ({dev})")
    if visibility is not None:
        visibility = _check_mask(visibility, P, dev, "densification stats: visibility")
    if dev.type != "cuda":
        raise RuntimeError("densification stats: the tensors must be GPU tensors (there is no CPU path)")
    # read in place by its row pitch where the two entries of a row are neighbours (a column view of a wider tensor included)
    if viewspace_grad.stride(1) != 1 or (P > 1 and viewspace_grad.stride(0) < 2):
        viewspace_grad = viewspace_grad.contiguous()
    pitch = max(viewspace_grad.stride(0), 2)   # (the stride of a 1-row tensor is arbitrary and never used)
    radii = radii.contiguous()
    vis_out = torch.empty(P, dtype=torch.bool, device=dev) if return_visibility else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = lib.sgs_densify_stats(P, viewspace_grad.data_ptr(), pitch, radii.data_ptr(),
                                   visibility.data_ptr() if visibility is not None else None,
                                   xyz_gradient_accum.data_ptr(), denom.data_ptr(), max_radii2D.data_ptr(),
                                   vis_out.data_ptr() if vis_out is not None else None, stream)
    _lib.check(rc, "densification stats")
    return vis_out
