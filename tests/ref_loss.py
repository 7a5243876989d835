"""A torch restatement of the training loss  (1 - lambda) * mean|x - y| + lambda * (1 - SSIM(x, y))  with its own autograd, written
from the formula (Wang et al. 2004 with an 11-tap Gaussian window of sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2), independent of
both the reference's text and the HIP kernels.  Any dtype; float64 on the host is what the GPU tests compare against.

Two forms of the window sum:
  form="2d"         one 11x11 window whose entries are the float32-rounded products w[i] * w[j] (that is the window a float32 outer
                    product builds).  tests/test_loss.py pins this form, in float64, to the fixture of the reference's own run.
  form="separable"  rows then columns with the 11 taps: the entries are the exact products.  It differs from the other form by one
                    float32 rounding per window entry.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 0.01 ** 2, 0.03 ** 2


def taps():
    """the 11 taps as float32: exp(-(i - 5)^2 / (2 * 1.5^2)) rounded to float32, over their correctly rounded float32 sum"""
    g = np.array([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)]).astype(np.float32)
    return g / np.float32(math.fsum(float(v) for v in g))


def _window_sum(t, form):
    """t: (B,C,H,W) -> the windowed sum at every pixel, zero padding"""
    Cn = t.shape[1]
    w = torch.from_numpy(taps())
    if form == "2d":
        w2 = (w[:, None] * w[None, :]).to(t.dtype)          # float32 product, then the working type
        return F.conv2d(t, w2.expand(Cn, 1, 11, 11).contiguous(), padding=5, groups=Cn)
    assert form == "separable"
    w = w.to(t.dtype)
    rows = F.conv2d(t, w.view(1, 1, 1, 11).expand(Cn, 1, 1, 11).contiguous(), padding=(0, 5), groups=Cn)
    return F.conv2d(rows, w.view(1, 1, 11, 1).expand(Cn, 1, 11, 1).contiguous(), padding=(5, 0), groups=Cn)


def ssim_map(x, y, form="separable"):
    mu1, mu2 = _window_sum(x, form), _window_sum(y, form)
    s1 = _window_sum(x * x, form) - mu1 * mu1
    s2 = _window_sum(y * y, form) - mu2 * mu2
    s12 = _window_sum(x * y, form) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def terms(x, y, form="separable", per_image=False):
    """(ssim, l1) of (C,H,W) or (B,C,H,W) images: scalars, or (B,) with per_image"""
    if x.dim() == 3:
        x, y = x[None], y[None]
    m = ssim_map(x, y, form)
    d = (x - y).abs()
    if per_image:
        return m.mean(dim=(1, 2, 3)), d.mean(dim=(1, 2, 3))
    return m.mean(), d.mean()


def loss(x, y, lam, form="separable"):
    s, l1 = terms(x, y, form)
    return (1.0 - lam) * l1 + lam * (1.0 - s)


def loss_and_grad(x, y, lam, dtype=torch.float64, form="separable", upstream=1.0):
    """x, y: tensors of any float type (x may be a crop view).  Returns (loss, ssim, l1, grad by x) in `dtype`, grad as numpy."""
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    yy = y.detach().to(dtype)
    s, l1 = terms(xx, yy, form)
    v = (1.0 - lam) * l1 + lam * (1.0 - s)
    (upstream * v).backward()
    return v.item(), s.item(), l1.item(), xx.grad.numpy()


def load_fixture():
    """tests/golden/photometric_loss.npz (gen_loss_fixture.py) decoded: {name: dict(image, gt (float32 tensors, full size), lam, crop,
    grad32, grad64 (numpy, crop-sized for the crop case), loss32/64, ssim32/64, l132/64, e_ref[, ssim_per_image32/64])}, window"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric_loss.npz"))
    cases = {}
    for name in z["names"]:
        g = lambda k: z[f"{name}.{k}"]   # noqa: E731
        c = {"image": torch.from_numpy(g("image_u8").astype(np.float32) / np.float32(255)),
             "gt": torch.from_numpy(g("gt_u8").astype(np.float32) / np.float32(255)),
             "lam": float(g("lambda")), "crop": bool(g("crop")), "grad32": g("grad32"),
             "grad64": g("grad32").astype(np.float64) + g("grad64_q").astype(np.float64) * float(g("grad64_scale"))}
        for k in ("loss", "ssim", "l1"):
            c[k + "32"], c[k + "64"] = float(g(k + "32")), float(g(k + "64"))
        if f"{name}.ssim_per_image32" in z.files:
            c["ssim_per_image32"], c["ssim_per_image64"] = g("ssim_per_image32"), g("ssim_per_image64")
        c["e_ref"] = float(np.abs(c["grad32"] - c["grad64"]).max() / np.abs(c["grad64"]).max())
        cases[str(name)] = c
    return cases, z["window"]


def crop_of(t):
    """train.py:140-145 with cut_edge: image[:, ch:-ch, cw:-cw], ch = h // 100, cw = w // 100"""
    ch, cw = t.shape[-2] // 100, t.shape[-1] // 100
    return t[..., ch:-ch, cw:-cw]
