"""GPU tests of the fused L1 + D-SSIM loss, through sgs_hip.loss (hence ctypes and the C-ABI).

Every bound is built from the reference's own float32 error, never from what the kernels give:
    gradient   max|g - g64| / max|g64| <= 2 * e_ref,        e_ref = max|g32_ref - g64_ref| / max|g64_ref|
    values     |v - v64| <= 2 * |v32_ref - v64_ref| + 2^-22 * |v64|
The factor 2 allows for the kernels' different (separable) summation order -- a float32 separable evaluation on the host sits at
0.1 .. 0.45 of e_ref -- and 2^-22 for the final rounding of a value to float32.  For the fixture cases g32 / g64 / v32 / v64 are the
reference's own runs (tests/golden/photometric_loss.npz); where the fixture holds no run (ssim or l1 alone, per-image means,
full-size images) they come from tests/ref_loss.py in its 2-D-window form, float64 for the truth and float32 for e_ref; that form
is pinned to the reference at 1e-12 by tests/test_loss.py."""
import numpy as np
import pytest
import torch

import ref_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES, _ = ref_loss.load_fixture()


def _grad_err(g, g64):
    g = g.detach().double().cpu().numpy().reshape(g64.shape)
    return float(np.abs(g - g64).max() / np.abs(g64).max())


def _check_value(what, v, v32, v64):
    v = float(v.detach()) if torch.is_tensor(v) else float(v)
    bound = 2.0 * abs(v32 - v64) + 2.0 ** -22 * abs(v64)
    print(f"  {what}: |v - v64| = {abs(v - v64):.3e}  bound {bound:.3e}  (reference float32: {abs(v32 - v64):.3e})")
    assert abs(v - v64) <= bound, (what, v, v64, abs(v - v64), bound)


def _check_grad(what, g, g64, e_ref):
    e = _grad_err(g, g64)
    print(f"  {what}: gradient error {e:.3e} of the largest entry  bound {2 * e_ref:.3e}  (e_ref {e_ref:.3e})")
    assert e_ref > 0
    assert e <= 2.0 * e_ref, (what, e, e_ref)


def _leaf_and_view(c):
    """the leaf on the device and what the loss is called with: the cut_edge crop is passed as the strided view it is"""
    leaf = c["image"].to(DEV).requires_grad_(True)
    gt = c["gt"].to(DEV)
    if c["crop"]:
        return leaf, ref_loss.crop_of(leaf), ref_loss.crop_of(gt)
    return leaf, leaf, gt


def _inside(c, full):
    return ref_loss.crop_of(full) if c["crop"] else full


def _host_pair(c):
    x, y = c["image"], c["gt"]
    return (ref_loss.crop_of(x), ref_loss.crop_of(y)) if c["crop"] else (x, y)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_photometric_loss(name):
    from sgs_hip.loss import photometric_loss
    c = CASES[name]
    leaf, x, gt = _leaf_and_view(c)
    if c["crop"]:
        assert not x.is_contiguous() and x.stride(-1) == 1
    loss, l1, ssim = photometric_loss(x, gt, c["lam"], return_terms=True)
    assert loss.shape == () and loss.requires_grad and not l1.requires_grad and not ssim.requires_grad
    print(name)
    _check_value("loss", loss, c["loss32"], c["loss64"])
    _check_value("ssim", ssim, c["ssim32"], c["ssim64"])
    _check_value("l1", l1, c["l132"], c["l164"])
    loss.backward()
    assert leaf.grad.shape == leaf.shape
    _check_grad("loss", _inside(c, leaf.grad), c["grad64"], c["e_ref"])
    if c["crop"]:
        # what arrives at the full (3,120,160) leaf: the reference's gradient inside the crop, exactly 0 outside it
        outside = leaf.grad.clone()
        ref_loss.crop_of(outside).zero_()
        assert int((outside != 0).sum()) == 0
        assert float(leaf.grad[:, 0].abs().max()) == 0 and float(leaf.grad[:, :, -1].abs().max()) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_ssim_and_l1_alone(name):
    """The drop-in pair of utils/loss_utils.py.  Values against the fixture's; the fixture holds no gradient of a term alone, so
    those are ref_loss's (2-D form): float64 for the truth, float32 for e_ref."""
    from sgs_hip import loss as L
    c = CASES[name]
    hx, hy = _host_pair(c)

    def ref(fn, dtype):
        x = hx.to(dtype).clone().requires_grad_(True)
        s, l1 = ref_loss.terms(x, hy.to(dtype), form="2d")
        (s if fn == "ssim" else l1).backward()
        return x.grad.double().numpy()

    print(name)
    for fn in ("ssim", "l1"):
        leaf, x, gt = _leaf_and_view(c)
        v = L.ssim(x, gt) if fn == "ssim" else L.l1_loss(x, gt)
        assert v.shape == () and v.requires_grad
        _check_value(fn, v, c[fn + "32"], c[fn + "64"])
        v.backward()
        g64, g32 = ref(fn, torch.float64), ref(fn, torch.float32)
        _check_grad(fn, _inside(c, leaf.grad), g64, float(np.abs(g32 - g64).max() / np.abs(g64).max()))
        if fn == "l1":
            # sign(0) = 0, as torch's abs backward has it: exactly no gradient where image == gt
            eq = (hx == hy).to(DEV)
            assert int(eq.sum()) > 0 and float(_inside(c, leaf.grad)[eq].abs().max()) == 0


def test_per_image_ssim_on_the_batch_case():
    """size_average=False: the (B,) per-image means, each against the reference's, and the gradient of a weighted sum of them."""
    from sgs_hip import loss as L
    c = CASES["batch40x56"]
    leaf, x, gt = _leaf_and_view(c)
    v = L.ssim(x, gt, size_average=False)
    assert v.shape == (2,)
    for b in range(2):
        _check_value(f"ssim[{b}]", v[b], float(c["ssim_per_image32"][b]), float(c["ssim_per_image64"][b]))
    w = torch.tensor([1.0, -2.5])
    (v * w.to(DEV)).sum().backward()

    def ref(dtype):
        xx = c["image"].to(dtype).clone().requires_grad_(True)
        s, _ = ref_loss.terms(xx, c["gt"].to(dtype), form="2d", per_image=True)
        (s * w.to(dtype)).sum().backward()
        return xx.grad.double().numpy()
    g64, g32 = ref(torch.float64), ref(torch.float32)
    _check_grad("per-image ssim", leaf.grad, g64, float(np.abs(g32 - g64).max() / np.abs(g64).max()))
    with pytest.raises(RuntimeError, match="size_average=False"):
        L.ssim(x[0], gt[0], size_average=False)


@pytest.mark.parametrize("name", ["c61x83", "crop120x160"])
def test_non_unit_upstream_gradient(name):
    """(3 * loss).backward(): the upstream gradient is read on the device.  3 * x is exact in float64 and one rounding in float32,
    which the reference's float32 autograd makes too: the fixture's e_ref holds for the tripled gradient."""
    from sgs_hip.loss import photometric_loss
    c = CASES[name]
    leaf, x, gt = _leaf_and_view(c)
    (3.0 * photometric_loss(x, gt, c["lam"])).backward()
    _check_grad("3 * loss", _inside(c, leaf.grad), 3.0 * c["grad64"], c["e_ref"])


def _full_size_pair(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    base = torch.stack([0.5 + 0.3 * torch.sin(6.28 * (k + 1.5) * xx + k) * torch.cos(6.28 * (2.5 - 0.5 * k) * yy) + 0.2 * (xx - yy)
                        for k in range(3)])
    img = (base + 0.06 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gt = (base + 0.04 * torch.sin(12.56 * yy) + 0.04 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    img[:, H // 3:H // 3 + 90, W // 4:W // 4 + 130] = 0      # flat, variance 0
    gt[:, H // 3:H // 3 + 90, W // 4:W // 4 + 130] = 0
    img[:, 40:140, W - 300:W - 100] = gt[:, 40:140, W - 300:W - 100]    # sign(0)
    return img, gt


@pytest.mark.parametrize("H,W", [(968, 1296), (840, 1297)])
def test_full_size_against_float64(H, W):
    """The flagship size and a width that is a multiple of no tile, every pixel compared, against ref_loss in float64 on the host;
    e_ref and the value bounds from a float32 run of the same 2-D-window form."""
    from sgs_hip.loss import photometric_loss
    lam = 0.2
    img, gt = _full_size_pair(H, W, seed=H + W)
    v64, s64, l64, g64 = ref_loss.loss_and_grad(img, gt, lam, torch.float64, form="2d")
    v32, s32, l32, g32 = ref_loss.loss_and_grad(img, gt, lam, torch.float32, form="2d")
    e_ref = float(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max())
    leaf = img.to(DEV).requires_grad_(True)
    loss, l1, ssim = photometric_loss(leaf, gt.to(DEV), lam, return_terms=True)
    loss.backward()
    print(f"{H}x{W}")
    _check_value("loss", loss, v32, v64)
    _check_value("ssim", ssim, s32, s64)
    _check_value("l1", l1, l32, l64)
    assert torch.isfinite(leaf.grad).all()
    _check_grad("loss", leaf.grad, g64, e_ref)


def test_forward_and_backward_are_deterministic():
    """No floating-point atomics anywhere: two runs give the same bits."""
    from sgs_hip.loss import photometric_loss
    img, gt = _full_size_pair(333, 517, seed=5)
    gt = gt.to(DEV)
    runs = []
    for _ in range(2):
        leaf = img.to(DEV).requires_grad_(True)
        loss, l1, ssim = photometric_loss(leaf, gt, 0.2, return_terms=True)
        loss.backward()
        runs.append((loss.detach().clone(), l1.clone(), ssim.clone(), leaf.grad.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(runs[0][3].abs().max()) > 0


def test_no_derivative_maps_under_no_grad():
    """Without a gradient to come the forward stores no maps: same loss bits, and the call's peak allocation stays under one
    map's size where the differentiable call holds three."""
    from sgs_hip.loss import photometric_loss
    img, gt = _full_size_pair(256, 320, seed=9)
    img, gt = img.to(DEV), gt.to(DEV)
    one_map = img.numel() * 4
    leaf = img.clone().requires_grad_(True)

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return out, torch.cuda.max_memory_allocated() - base

    with torch.no_grad():
        quiet, peak_quiet = peak_of(lambda: photometric_loss(leaf, gt, 0.2))
    loud, peak_loud = peak_of(lambda: photometric_loss(leaf, gt, 0.2))
    plain, peak_plain = peak_of(lambda: photometric_loss(img, gt, 0.2))     # nothing requires grad
    print(f"peak bytes: no_grad {peak_quiet}, differentiable {peak_loud}, no leaf {peak_plain}; one map = {one_map}")
    assert not quiet.requires_grad and loud.requires_grad and not plain.requires_grad
    assert torch.equal(quiet, loud.detach()) and torch.equal(plain, quiet)
    assert peak_quiet < one_map and peak_plain < one_map
    assert peak_loud >= 3 * one_map
    assert quiet.grad_fn is None and len([t for t in loud.grad_fn.saved_tensors if t is not None]) == 3


def test_views_and_layouts():
    """Unit stride along the width goes by pitch; anything else through .contiguous(): same bits as the contiguous call."""
    from sgs_hip.loss import photometric_loss
    img, gt = _full_size_pair(70, 101, seed=2)
    img, gt = img.to(DEV), gt.to(DEV)
    want = photometric_loss(img, gt, 0.3)
    wide = torch.zeros(3, 80, 128, device=DEV)
    wide[:, 4:74, 9:110] = img
    assert torch.equal(photometric_loss(wide[:, 4:74, 9:110], gt, 0.3), want)
    hwc = img.permute(1, 2, 0).contiguous().permute(2, 0, 1)      # channel-last memory: not unit stride along the width
    assert hwc.stride(-1) != 1
    assert torch.equal(photometric_loss(hwc, gt, 0.3), want)
    assert torch.equal(photometric_loss(img, gt[:1].expand(3, 70, 101).clone(), 0.3),
                       photometric_loss(img, gt[:1].expand(3, 70, 101), 0.3))    # channel pitch 0
    assert torch.equal(photometric_loss(img[None], gt[None], 0.3), want)


def test_one_training_step_end_to_end():
    """The RGB-D rasteriser renders a small seeded scene, the step runs photometric_loss and backward(): the gradients on means3D
    and colors are finite, non-zero, and those of the same step with the loss composed from torch ops, within the rasteriser
    backward's tolerance (1e-4 of the largest entry, as tests/test_parity_gpu.py uses)."""
    import torch.nn.functional as F
    import rgbd_rasterization as rr
    from helpers import small_scene
    from sgs_hip.loss import photometric_loss
    scene, cam = small_scene(P=2000, C=3, W=160, H=112, fx=150.0, seed=3)
    s, c = scene.to(DEV), cam.to(DEV)
    settings = rr.GaussianRasterizationSettings(
        image_height=112, image_width=160, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(3, device=DEV), scale_modifier=1.0,
        viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0, campos=c.camera_center, prefiltered=False,
        debug=False)
    rast = rr.GaussianRasterizer(raster_settings=settings)
    lam = 0.2
    g = torch.Generator(device=DEV).manual_seed(1)
    target = torch.rand(3, 112, 160, generator=g, device=DEV)

    def composed(image, gt):
        w = torch.from_numpy(ref_loss.taps()).to(DEV)
        w2 = (w[:, None] * w[None, :]).expand(3, 1, 11, 11).contiguous()
        conv = lambda t: F.conv2d(t[None], w2, padding=5, groups=3)   # noqa: E731
        mu1, mu2 = conv(image), conv(gt)
        s1, s2, s12 = conv(image * image) - mu1 * mu1, conv(gt * gt) - mu2 * mu2, conv(image * gt) - mu1 * mu2
        m = ((2 * mu1 * mu2 + ref_loss.C1) * (2 * s12 + ref_loss.C2)) / ((mu1 * mu1 + mu2 * mu2 + ref_loss.C1) * (s1 + s2 + ref_loss.C2))
        return (1.0 - lam) * (image - gt).abs().mean() + lam * (1.0 - m.mean())

    grads = []
    for loss_fn in (lambda a, b: photometric_loss(a, b, lam), composed):
        xyz = s.means3D.clone().requires_grad_(True)
        colors = s.features.clone().requires_grad_(True)
        m2d = torch.zeros_like(xyz, requires_grad=True) + 0
        out = rast(means3D=xyz, means2D=m2d, shs=None, colors_precomp=colors, opacities=s.opacities, scales=s.scales,
                   rotations=s.rotations, cov3D_precomp=None)
        loss = loss_fn(out[0], target)
        loss.backward()
        grads.append((float(loss.detach()), xyz.grad.clone(), colors.grad.clone()))
    (l_a, dx_a, dc_a), (l_b, dx_b, dc_b) = grads
    assert abs(l_a - l_b) <= 1e-5 * abs(l_b)
    for what, a, b in (("means3D", dx_a, dx_b), ("colors", dc_a, dc_b)):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0, what
        err = float((a - b).abs().max() / b.abs().max())
        print(f"  d{what}: {err:.3e} of the largest entry")
        assert err <= 1e-4, (what, err)
