"""The training loss alone, forward + backward, at cfg2's image size (3 x 968 x 1296): sgs_hip.loss.photometric_loss (two kernels
forward, one backward) against the same formula composed from torch ops the way utils/loss_utils.py composes it (five depthwise 11x11
conv2d, a dozen element-wise temporaries, autograd replaying them).  `composed_loss` below is written here from the formula; nothing is
imported from the reference.

    python tools/bench_photometric_loss.py [--repeats 7] [--iters 50] [--crop]

Method: both forms are warmed up, then timed alternately `repeats` times; each timing is a host clock around `iters` iterations that
ends in a device synchronise (the gradient buffer is reused, nothing is read back inside the window); the median over the repeats is
reported with the min-max spread.  Prints the value and gradient agreement of the two forms first: faster and different is not faster."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-gaussians_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def gaussian_window(channels, device):
    g = torch.tensor([-((i - 5) ** 2) / (2 * 1.5 ** 2) for i in range(11)], dtype=torch.float64).exp().float()
    w = g / g.sum()
    return (w[:, None] * w[None, :]).expand(channels, 1, 11, 11).contiguous().to(device)


def composed_loss(image, gt, lam, window):
    """(1 - lam) * L1 + lam * (1 - SSIM) from torch ops; image, gt: (C,H,W)"""
    C = image.shape[0]
    x, y = image[None], gt[None]
    mu1 = F.conv2d(x, window, padding=5, groups=C)
    mu2 = F.conv2d(y, window, padding=5, groups=C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, window, padding=5, groups=C) - mu1_sq
    s2 = F.conv2d(y * y, window, padding=5, groups=C) - mu2_sq
    s12 = F.conv2d(x * y, window, padding=5, groups=C) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))
    return (1.0 - lam) * torch.abs(image - gt).mean() + lam * (1.0 - ssim_map.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--height", type=int, default=968)
    ap.add_argument("--width", type=int, default=1296)
    ap.add_argument("--crop", action="store_true", help="time the cut_edge crop image[:, ch:-ch, cw:-cw] (a strided view) instead")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photometric_loss needs a GPU: a timing taken anywhere else says nothing")
    from sgs_hip.loss import photometric_loss
    dev, lam = "cuda:0", 0.2
    H, W = a.height, a.width
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device=dev), torch.linspace(0, 1, W, device=dev), indexing="ij")
    base = 0.5 + 0.3 * torch.sin(9.0 * xx) * torch.cos(7.0 * yy)
    leaf = (base + 0.06 * torch.randn(3, H, W, generator=g, device=dev)).clamp(0, 1).requires_grad_(True)
    target = (base + 0.04 * torch.randn(3, H, W, generator=g, device=dev)).clamp(0, 1)
    window = gaussian_window(3, dev)

    def view(t):
        return t[:, H // 100:-(H // 100), W // 100:-(W // 100)] if a.crop else t

    def fused():
        leaf.grad = None
        photometric_loss(view(leaf), view(target), lam).backward()

    def composed():
        leaf.grad = None
        composed_loss(view(leaf), view(target), lam, window).backward()

    vals = {}
    for name, fn in (("fused", fused), ("composed", composed)):
        fn()
        vals[name] = leaf.grad.clone()
    lf = float(photometric_loss(view(leaf), view(target), lam))
    lc = float(composed_loss(view(leaf), view(target), lam, window))
    gerr = float((vals["fused"] - vals["composed"]).abs().max() / vals["composed"].abs().max())
    print(f"agreement: loss fused {lf:.8f} composed {lc:.8f} (diff {abs(lf - lc):.1e}); gradient max diff {gerr:.1e} of the largest entry")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.iters * 1e6

    for fn in (fused, composed):
        for _ in range(10):
            fn()
    times = {"fused": [], "composed": []}
    for _ in range(a.repeats):
        times["fused"].append(timed(fused))
        times["composed"].append(timed(composed))
    med = {k: statistics.median(v) for k, v in times.items()}
    shape = tuple(view(leaf).shape)
    print(f"{torch.cuda.get_device_name(0)}; loss forward + backward at {shape}{' (strided crop view)' if a.crop else ''}, lambda {lam}; "
          f"{a.repeats} repeats x {a.iters} iterations, median [min .. max] in microseconds per iteration")
    for k in ("fused", "composed"):
        label = "sgs_hip.loss.photometric_loss" if k == "fused" else "composed from torch ops       "
        print(f"  {label}: {med[k]:8.1f} us  [{min(times[k]):.1f} .. {max(times[k]):.1f}]")
    print(f"  composed / fused = {med['composed'] / med['fused']:.2f}x")


if __name__ == "__main__":
    main()
