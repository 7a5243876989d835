"""The training loss of train.py:138-150 on the device: `l1_loss` and `ssim` with the signatures of the reference's
utils/loss_utils.py, and `photometric_loss`, the fused  (1 - lambda) * L1 + lambda * (1 - SSIM)  in one forward launch pair
and one backward launch (csrc/photometric_loss.hip).  All three differentiate by the FIRST image only.

    from sgs_hip.loss import l1_loss, ssim          # instead of: from utils.loss_utils import l1_loss, ssim

Images are float32 (C,H,W) or (B,C,H,W) device tensors.  A view with unit stride along the width (the `cut_edge` crop
image[:, ch:-ch, cw:-cw] of a render) is read in place by its pitches; any other layout goes through .contiguous().
No CPU fallback: the HIP library is required.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib

_LOSS, _SSIM, _L1 = 0, 1, 2


def _check(image, gt, window_size=11):
    if window_size != 11:
        raise RuntimeError(f"window_size must be 11 (got {window_size}): the HIP kernels implement the reference's default window only")
    if not (torch.is_tensor(image) and torch.is_tensor(gt)):
        raise RuntimeError("the images must be torch tensors")
    if image.dtype != torch.float32 or gt.dtype != torch.float32:
        raise RuntimeError(f"the images must be float32 (got {image.dtype}, {gt.dtype}): no other format is implemented")
    if image.shape != gt.shape:
        raise RuntimeError(f"the images must have the same shape (got {tuple(image.shape)} and {tuple(gt.shape)})")
    if image.dim() not in (3, 4) or image.numel() == 0:
        raise RuntimeError(f"the images must be non-empty (C,H,W) or (B,C,H,W) (got {tuple(image.shape)})")
    if gt.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("the second image requires grad: the loss differentiates by the first image only")
    if not (image.is_cuda and gt.is_cuda):
        raise RuntimeError("the images must be GPU tensors (there is no CPU path)")
    if image.device != gt.device:
        raise RuntimeError(f"the images are on different devices ({image.device}, {gt.device})")


def _by_pitch(t):
    """(tensor to keep alive, (row, channel, image) pitches in elements) of a 4-D tensor, without a copy where the kernels can
    read the layout."""
    W = t.shape[3]
    s = t.stride()
    if not (s[3] == 1 and s[2] >= W and s[1] >= 0 and s[0] >= 0):
        t = t.contiguous()
        s = t.stride()
    return t, (s[2], s[1], s[0])


def _need_grad(image):
    # (asked outside the Function: inside its forward grad mode is always off)
    return bool(image.requires_grad and torch.is_grad_enabled())


class _Fused(torch.autograd.Function):
    """Returns (loss, ssim, l1); `which` names the one entry that carries the gradient.  need == False (no_grad, or an image
    that does not require grad): the forward stores no derivative maps and saves nothing."""

    @staticmethod
    def forward(ctx, image, gt, lam, which, per_image, need):
        lib = _lib.load()
        x4 = image if image.dim() == 4 else image.unsqueeze(0)
        y4 = gt.detach() if gt.dim() == 4 else gt.detach().unsqueeze(0)
        B, Cn, H, W = x4.shape
        x4, xp = _by_pitch(x4.detach())
        y4, yp = _by_pitch(y4)
        dev = image.device
        with_ssim = which != _L1
        n_out = B if per_image else 1
        out = torch.empty(3, n_out, dtype=torch.float32, device=dev)
        dmaps = torch.empty(3, B, Cn, H, W, dtype=torch.float32, device=dev) if (need and with_ssim) else None
        nbytes = _lib.check(lib.sgs_photometric_loss_scratch_bytes(B, Cn, H, W), "photometric loss scratch")
        scratch = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = lib.sgs_photometric_loss_forward(
                B, Cn, H, W, x4.data_ptr(), *xp, y4.data_ptr(), *yp, float(lam), 0 if per_image else 1,
                out[0].data_ptr(), out[1].data_ptr() if with_ssim else None, out[2].data_ptr(),
                dmaps.data_ptr() if dmaps is not None else None, scratch.data_ptr(), nbytes, stream)
        _lib.check(rc, "photometric loss forward")
        ctx.meta = None
        if need:
            ctx.save_for_backward(x4, y4, dmaps)
            ctx.meta = (xp, yp, float(lam), which, per_image, tuple(image.shape))
        shape = (B,) if per_image else ()
        loss, ssim_v, l1 = (out[k].reshape(shape) for k in range(3))
        ctx.mark_non_differentiable(*[t for k, t in enumerate((loss, ssim_v, l1)) if k != which])
        return loss, ssim_v, l1

    @staticmethod
    @once_differentiable          # the gradient is a kernel's output: a double backward raises instead of treating it as constant
    def backward(ctx, *grads):
        if ctx.meta is None:
            raise RuntimeError("photometric loss backward: the forward ran without a gradient request and kept no derivative maps")
        lib = _lib.load()
        x4, y4, dmaps = ctx.saved_tensors
        xp, yp, lam, which, per_image, shape = ctx.meta
        g = grads[which]
        B, Cn, H, W = x4.shape
        dev = x4.device
        # the upstream gradient stays on the device: the step never waits for the host
        g = g.to(torch.float32).reshape(-1).contiguous()
        w_ssim, w_l1 = {_LOSS: (-lam, 1.0 - lam), _SSIM: (1.0, 0.0), _L1: (0.0, 1.0)}[which]
        out = torch.empty(B, Cn, H, W, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            rc = lib.sgs_photometric_loss_backward(
                B, Cn, H, W, x4.data_ptr(), *xp, y4.data_ptr(), *yp, w_ssim, w_l1,
                dmaps.data_ptr() if dmaps is not None else None, g.data_ptr(), 0 if per_image else 1, out.data_ptr(), stream)
        _lib.check(rc, "photometric loss backward")
        return out.reshape(shape), None, None, None, None, None


def l1_loss(network_output, gt):
    """utils/loss_utils.py:18  torch.abs(network_output - gt).mean()"""
    _check(network_output, gt)
    return _Fused.apply(network_output, gt, 0.0, _L1, False, _need_grad(network_output))[_L1]


def ssim(img1, img2, window_size=11, size_average=True):
    """utils/loss_utils.py:38.  size_average=False returns the (B,) per-image means and, like the reference, needs
    (B,C,H,W) input."""
    _check(img1, img2, window_size)
    if not size_average and img1.dim() != 4:
        raise RuntimeError("size_average=False needs (B,C,H,W) input")
    return _Fused.apply(img1, img2, 1.0, _SSIM, not size_average, _need_grad(img1))[_SSIM]


def photometric_loss(image, gt, lambda_dssim=0.2, return_terms=False):
    """train.py:149  (1.0 - lambda_dssim) * Ll1 + lambda_dssim * (1.0 - ssim(image, gt)), a scalar.
    return_terms=True returns (loss, Ll1, ssim): the two terms come out of the same launch (train.py:183 logs Ll1) and
    carry no gradient."""
    _check(image, gt)
    lam = float(lambda_dssim)
    loss, ssim_v, l1 = _Fused.apply(image, gt, lam, _LOSS, False, _need_grad(image))
    return (loss, l1, ssim_v) if return_terms else loss
