"""N2 measurement: one optimisation step as train.py runs it (render -> L1 -> backward -> Adam) at cfg2
(500k Gaussians, RGB-D rasteriser, 968x1296), and the same with a 512-channel feature target at cfg3's size
(distillation-style; the reference's backward cannot run this).  A second cfg2 line runs the step with the loss train.py actually
trains with, (1 - lambda) * L1 + lambda * (1 - SSIM) (train.py:149), once through sgs_hip.loss.photometric_loss and once composed from
torch ops (tools/bench_photometric_loss.py composed_loss).  Every line runs with four optimisers: torch.optim.Adam as the reference builds
it (the multi-pass foreach path), torch.optim.Adam(fused=True), sgs_hip.optim.GaussianAdam dense and GaussianAdam with the view's
visibility mask.  Between backward and the optimiser sit the densification statistics of train.py:158-161: the three boolean-indexed
statements with torch's Adam, sgs_hip.optim.accumulate_densification_stats (one launch, no host wait) with GaussianAdam.  Every figure is
the median of 5 timings of N iterations, each a host clock around work that ends in a device synchronise, after 3 warm-up iterations."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-gaussians_amd"))
import torch
import rgbd_rasterization as rr
import channel_rasterization as cr
from sgs_hip.synthetic import CONFIGS, make_scene
from sgs_hip.camera import pinhole
from sgs_hip.loss import photometric_loss
from sgs_hip.optim import GaussianAdam, accumulate_densification_stats
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
    params = [xyz, colors, opacity, scaling, rotation]
    optimisers = {"torch Adam": lambda: torch.optim.Adam(params, lr=1e-4, eps=1e-15),
                  "torch Adam fused=True": lambda: torch.optim.Adam(params, lr=1e-4, eps=1e-15, fused=True),
                  "GaussianAdam dense": lambda: GaussianAdam(params, lr=1e-4, eps=1e-15),
                  "GaussianAdam masked": lambda: GaussianAdam(params, lr=1e-4, eps=1e-15)}
    xyz_gradient_accum = torch.zeros(P, 1, device=dev)
    denom = torch.zeros(P, 1, device=dev)
    max_radii2D = torch.zeros(P, device=dev)
    target = torch.rand(C, H, W, device=dev)

    losses = {"L1": lambda image: (image - target).abs().mean()}
    if name == "cfg2":
        window = gaussian_window(3, dev)
        losses["L1 + D-SSIM (sgs_hip.loss.photometric_loss)"] = lambda image: photometric_loss(image, target, 0.2)
        losses["L1 + D-SSIM (composed from torch ops)"] = lambda image: composed_loss(image, target, 0.2, window)

    def step(loss_fn, opt, which):
        m2d = torch.zeros_like(xyz, requires_grad=True) + 0
        m2d.retain_grad()
        out = rast(means3D=xyz, means2D=m2d, shs=None, colors_precomp=colors, opacities=torch.sigmoid(opacity),
                   scales=torch.exp(scaling), rotations=torch.nn.functional.normalize(rotation), cov3D_precomp=None)
        loss = loss_fn(out[0])
        loss.backward()
        radii = out[1]
        with torch.no_grad():
            if which.startswith("torch"):
                vis = radii > 0
                max_radii2D[vis] = torch.max(max_radii2D[vis], radii[vis].float())
                xyz_gradient_accum[vis] += torch.norm(m2d.grad[vis, :2], dim=-1, keepdim=True)
                denom[vis] += 1
                opt.step()
            else:
                vis = accumulate_densification_stats(xyz_gradient_accum, denom, max_radii2D, m2d.grad, radii, return_visibility=True)
                opt.step(visibility=vis if which.endswith("masked") else None)
        opt.zero_grad(set_to_none=True)

    N = 20 if C == 3 else 5
    for what, loss_fn in losses.items():
        for which, make in optimisers.items():
            opt = make()
            for _ in range(3):
                step(loss_fn, opt, which)
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(N):
                    step(loss_fn, opt, which)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) / N)
            t = statistics.median(ts)
            print(f"{name} P={P} C={C} {W}x{H}: render + {what} + backward + stats + {which} = {t * 1e3:.2f} ms per iteration ({1 / t:.0f} it/s)"
                  f"  [min {min(ts) * 1e3:.2f}, max {max(ts) * 1e3:.2f}]", flush=True)
            del opt
