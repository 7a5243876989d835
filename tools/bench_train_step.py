"""N2 measurement: one optimisation step as train.py runs it (render -> L1 -> backward -> Adam) at cfg2
(500k Gaussians, RGB-D rasteriser, 968x1296), and the same with a 512-channel feature target at cfg3's size
(distillation-style; the reference's backward cannot run this).  A second cfg2 line runs the step with the loss train.py actually
trains with, (1 - lambda) * L1 + lambda * (1 - SSIM) (train.py:149), once through sgs_hip.loss.photometric_loss and once composed from
torch ops (tools/bench_photometric_loss.py composed_loss).  Every figure is the median of 5 timings of N iterations, each a host clock
around work that ends in a device synchronise, after 3 warm-up iterations."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-gaussians_amd"))
import torch
import rgbd_rasterization as rr
import channel_rasterization as cr
from sgs_hip.synthetic import CONFIGS, make_scene
from sgs_hip.camera import pinhole
from sgs_hip.loss import photometric_loss
from bench_photometric_loss import composed_loss, gaussian_window

dev = "cuda:0"
for name, C in (("cfg2", 3), ("cfg3", 512)):
    P, _, W, H, fx = CONFIGS[name]
    s = make_scene(P, C, W, H, fx, seed=0).to(dev)
    c = pinhole(W, H, fx).to(dev)
    mod = rr if C == 3 else cr
    kw = dict(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=s.bg, scale_modifier=1.0,
              viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0, campos=c.camera_center,
              prefiltered=False, debug=False)
    if C != 3:
        kw["num_channels"] = C
    rast = mod.GaussianRasterizer(mod.GaussianRasterizationSettings(**kw))
    xyz = s.means3D.clone().requires_grad_(True)
    colors = s.features.clone().requires_grad_(True)
    opacity = torch.logit(s.opacities.clamp(1e-3, 1 - 1e-3)).requires_grad_(True)
    scaling = torch.log(s.scales).requires_grad_(True)
    rotation = s.rotations.clone().requires_grad_(True)
    opt = torch.optim.Adam([xyz, colors, opacity, scaling, rotation], lr=1e-4, eps=1e-15)
    target = torch.rand(C, H, W, device=dev)

    losses = {"L1": lambda image: (image - target).abs().mean()}
    if name == "cfg2":
        window = gaussian_window(3, dev)
        losses["L1 + D-SSIM (sgs_hip.loss.photometric_loss)"] = lambda image: photometric_loss(image, target, 0.2)
        losses["L1 + D-SSIM (composed from torch ops)"] = lambda image: composed_loss(image, target, 0.2, window)

    def step(loss_fn):
        m2d = torch.zeros_like(xyz, requires_grad=True) + 0
        out = rast(means3D=xyz, means2D=m2d, shs=None, colors_precomp=colors, opacities=torch.sigmoid(opacity),
                   scales=torch.exp(scaling), rotations=torch.nn.functional.normalize(rotation), cov3D_precomp=None)
        loss = loss_fn(out[0])
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    N = 20 if C == 3 else 5
    for what, loss_fn in losses.items():
        for _ in range(3):
            step(loss_fn)
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(N):
                step(loss_fn)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / N)
        t = statistics.median(ts)
        print(f"{name} P={P} C={C} {W}x{H}: render + {what} + backward + Adam = {t * 1e3:.2f} ms per iteration ({1 / t:.0f} it/s)"
              f"  [min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}]")
