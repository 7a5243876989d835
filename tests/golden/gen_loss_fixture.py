"""Generates tests/golden/photometric_loss.npz by IMPORTING the reference's own loss (utils/loss_utils.py l1_loss and ssim, combined
as train.py:149 combines them) and running it on the CPU, once in float32 as it trains and once in float64, with the gradient by the
first image from autograd.  Only inputs and results are stored -- no reference source text.  Run in the build container only
(/root/reference does not exist on the GPU box):

    python tests/golden/gen_loss_fixture.py

Cases: (3,61,83); (3,7,9), smaller than the 11x11 window, where the zero padding dominates; a (2,3,40,56) batch; the `cut_edge` crop
image[:, 1:-1, 1:-1] of a (3,120,160) pair (train.py:140-145: ch = h // 100, cw = w // 100).  Inputs are smooth images plus noise
clamped to [0,1], with one block that is zero in both images (variance 0: the cancellation in sigma = E[x^2] - mu^2 shows) and one
block where image == gt (sign(0) in the L1 term).

Storage (tests/helpers-free; tests/ref_loss.py load_fixture() decodes it): the four gradients in float32 + float64 alone are past the
size limit of a committed file, so
  * inputs are stored as 8-bit codes, value = float32(code) / float32(255) (8-bit images are what the data loader reads anyway);
  * the float32 gradient is stored as it is; the float64 gradient as its difference from the float32 one in 32-bit fixed point:
    grad64 = float64(grad32) + q * scale.  The difference is at most a few 1e-5 of the largest entry, so the decoded float64
    gradient is the reference's to 2^-32 of that: ~1e-14 of the largest entry, a hundred times under what any test asks.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
sys.path.insert(0, REF)
from utils.loss_utils import gaussian, l1_loss, ssim  # noqa: E402

torch.set_num_threads(1)   # one summation order, whatever machine regenerates the file


def images(rng, shape, zero_block, equal_block):
    """smooth + noise, clamped, as 8-bit codes; shape (..., H, W)"""
    H, W = shape[-2:]
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    lead = int(np.prod(shape[:-2]))
    a = np.empty((lead, H, W))
    b = np.empty((lead, H, W))
    for i in range(lead):
        f, p = rng.uniform(1.0, 4.0, 2), rng.uniform(0, 6.28, 2)
        smooth = 0.5 + 0.3 * np.sin(6.28 * f[0] * xx + p[0]) * np.cos(6.28 * f[1] * yy + p[1]) + 0.25 * (xx - yy)
        a[i] = smooth + rng.normal(0, 0.06, (H, W))
        b[i] = smooth + 0.05 * np.sin(6.28 * 2 * yy + p[0]) + rng.normal(0, 0.04, (H, W))
    a = np.rint(np.clip(a, 0, 1) * 255).astype(np.uint8)
    b = np.rint(np.clip(b, 0, 1) * 255).astype(np.uint8)
    (y0, y1, x0, x1) = zero_block
    a[:, y0:y1, x0:x1] = 0
    b[:, y0:y1, x0:x1] = 0
    (y0, y1, x0, x1) = equal_block
    a[:, y0:y1, x0:x1] = b[:, y0:y1, x0:x1]
    return a.reshape(shape), b.reshape(shape)


def decode(code):
    return torch.from_numpy(code.astype(np.float32) / np.float32(255))


def run(img, gt, lam, dtype, crop):
    x = img.to(dtype).requires_grad_(True)
    y = gt.to(dtype)
    xi, yi = x, y
    if crop:
        ch, cw = x.shape[-2] // 100, x.shape[-1] // 100
        xi, yi = x[:, ch:-ch, cw:-cw], y[:, ch:-ch, cw:-cw]
    l1 = l1_loss(xi, yi)
    s = ssim(xi, yi)
    loss = (1.0 - lam) * l1 + lam * (1.0 - s)
    loss.backward()
    g = x.grad
    if crop:
        assert g[:, 0].abs().max() == 0 and g[:, :, 0].abs().max() == 0
        g = g[:, ch:-ch, cw:-cw]
    out = {"loss": loss.item(), "ssim": s.item(), "l1": l1.item(), "grad": g.detach().numpy().copy()}
    if x.dim() == 4:
        with torch.no_grad():
            out["ssim_per_image"] = ssim(xi, yi, size_average=False).numpy().copy()
    return out


CASES = (
    # name, shape, lambda, crop, zero block (y0, y1, x0, x1), equal block
    ("c61x83", (3, 61, 83), 0.2, False, (8, 26, 40, 70), (35, 55, 5, 30)),
    ("c7x9", (3, 7, 9), 0.2, False, (0, 2, 0, 3), (4, 7, 5, 9)),
    ("batch40x56", (2, 3, 40, 56), 0.2, False, (20, 38, 4, 24), (2, 14, 30, 50)),
    ("crop120x160", (3, 120, 160), 0.25, True, (60, 100, 20, 70), (10, 40, 90, 150)),
)

rng = np.random.RandomState(20)
out = {"names": np.array([c[0] for c in CASES]), "window": gaussian(11, 1.5).numpy()}
for name, shape, lam, crop, zb, eb in CASES:
    a, b = images(rng, shape, zb, eb)
    r32 = run(decode(a), decode(b), lam, torch.float32, crop)
    r64 = run(decode(a), decode(b), lam, torch.float64, crop)
    g32, g64 = r32["grad"], r64["grad"]
    diff = g64 - g32.astype(np.float64)
    scale = np.abs(diff).max() / (2.0 ** 31 - 1)
    assert scale > 0, "the float32 reference equals its float64 self: replace this case (its bound would be meaningless)"
    q = np.rint(diff / scale).astype(np.int32)
    e_ref = np.abs(diff).max() / np.abs(g64).max()
    assert np.abs(g32.astype(np.float64) + q * scale - g64).max() <= 2.0 ** -31 * np.abs(diff).max()
    for k in ("loss", "ssim", "l1"):
        assert r32[k] != r64[k], f"{name}: float32 {k} equals the float64 one: replace this case"
    out.update({f"{name}.image_u8": a, f"{name}.gt_u8": b, f"{name}.lambda": np.float64(lam), f"{name}.crop": np.bool_(crop),
                f"{name}.grad32": g32, f"{name}.grad64_q": q, f"{name}.grad64_scale": np.float64(scale)})
    for k in ("loss", "ssim", "l1"):
        out[f"{name}.{k}32"] = np.float32(r32[k])
        out[f"{name}.{k}64"] = np.float64(r64[k])
    if "ssim_per_image" in r32:
        out[f"{name}.ssim_per_image32"] = r32["ssim_per_image"]
        out[f"{name}.ssim_per_image64"] = r64["ssim_per_image"]
    print(f"{name}: loss64 {r64['loss']:.12f} |loss32-loss64| {abs(r32['loss'] - r64['loss']):.2e} ssim {abs(r32['ssim'] - r64['ssim']):.2e} "
          f"l1 {abs(r32['l1'] - r64['l1']):.2e}  e_ref(grad) {e_ref:.2e}")

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "photometric_loss.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
