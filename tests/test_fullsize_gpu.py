"""BASELINE.json's headline configuration at FULL size (cfg3: 1M Gaussians, C=512, 968x1296) on the GPU.

The oracle cannot blend a whole 1M x 512 frame in seconds, so this file checks what does not need it:
size-independent properties of the domain (sortedness and consistency of the per-tile lists, agreement
of the three binning algorithms on all 16.5M instances, determinism, the partition-of-unity identity
sum_k w_k = 1 - T_final, linearity in the features), plus the oracle itself on everything integer
(preprocess + binning of the full frame) and on a sample of tile rows of the feature map."""
import numpy as np
import pytest
import torch
from helpers import has_experiments

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def cfg3():
    from sgs_hip.synthetic import CONFIGS, make_scene
    from sgs_hip.camera import pinhole
    P, C, W, H, fx = CONFIGS["cfg3"]
    scene = make_scene(P, C, W, H, fx, seed=0)
    return scene, pinhole(W, H, fx), (P, C, W, H)


def _render(scene_dev, cam_dev, C, W, H, feats=None, bg=None, fn=None, **kw):
    from sgs_hip import raster
    e = torch.Tensor([])
    s, c = scene_dev, cam_dev
    return (fn or raster.rasterize_forward)(
        s.bg[:C] if bg is None else bg, s.means3D, s.features if feats is None else feats, s.opacities, s.scales,
        s.rotations, 1.0, e, c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy, H, W, e, 0,
        c.camera_center, False, False, C, False, **kw)


def test_cfg3_lists_sorted_consistent_and_identical_across_binning_modes(cfg3, orc):
    from sgs_hip import raster
    scene, cam, (P, C, W, H) = cfg3
    s, c = scene.to(DEV), cam.to(DEV)
    feats = s.features[:, :4].contiguous()   # the lists do not depend on the channels
    gx, gy = (W + 15) // 16, (H + 15) // 16
    got = {}
    modes = (0, 1, 2) if has_experiments() else (0,)   # (1 / 2: the reference-order 45-bit sort / the 32-bit tile sort on rocPRIM, make EXPERIMENTS=1)
    for mode in modes:
        raster.set_binning_mode(mode)
        try:
            n, color, radii, geom, binn, img, _ = _render(s, c, 4, W, H, feats=feats)
        finally:
            raster.set_binning_mode(0)
        args = (geom, P, img, W, H) if mode != 1 else (None, None, None, None, None)
        b = raster.binning_views(binn, n, *args)
        iv = raster.image_views(img, W, H)
        got[mode] = dict(n=n, keys=b["keys_sorted"].clone(), plist=b["point_list"].clone(), ranges=iv["ranges"].clone(),
                         radii=radii.clone(), color=color.clone(), n_contrib=iv["n_contrib"].clone())
    a = got[0]
    for mode in modes[1:]:   # the span-partition lists == the reference-order 45-bit sort == the 32-bit tile sort
        o = got[mode]
        assert o["n"] == a["n"] and torch.equal(o["plist"], a["plist"]) and torch.equal(o["ranges"], a["ranges"])
        assert torch.equal(o["keys"], a["keys"]) and torch.equal(o["color"], a["color"])
    n, keys, plist, ranges = a["n"], a["keys"], a["plist"].long(), a["ranges"].long()
    assert n > 10_000_000
    assert bool((keys[1:] >= keys[:-1]).all())                                  # sortedness of (tile, depth)
    lens = ranges[:, 1] - ranges[:, 0]
    assert int(lens.sum()) == n and bool((lens >= 0).all())
    nz = lens > 0
    starts = torch.cumsum(lens, 0) - lens
    assert torch.equal(ranges[nz, 0], starts[nz])                               # ranges partition [0, L) in tile order
    tile_of = torch.repeat_interleave(torch.arange(gx * gy, device=DEV), lens)
    assert torch.equal(keys >> 32, tile_of)                                     # every key carries its tile
    # every listed Gaussian's rect covers its tile (reference getRect, CR/cuda_rasterizer/auxiliary.h:46-57)
    g = raster.geometry_views(geom, P)
    m2d, rad = g["means2D"][plist], a["radii"][plist].float()
    tx, ty = (tile_of % gx).float(), (tile_of // gx).float()
    x0 = torch.clamp(torch.floor((m2d[:, 0] - rad) / 16.0), 0, gx)
    x1 = torch.clamp(torch.floor((m2d[:, 0] + rad + 16.0 - 1.0) / 16.0), 0, gx)
    y0 = torch.clamp(torch.floor((m2d[:, 1] - rad) / 16.0), 0, gy)
    y1 = torch.clamp(torch.floor((m2d[:, 1] + rad + 16.0 - 1.0) / 16.0), 0, gy)
    assert bool(((tx >= x0) & (tx < x1) & (ty >= y0) & (ty < y1)).all())
    # the oracle on everything integer at full size
    pre = orc.preprocess(scene.means3D.numpy(), scene.opacities.numpy(), cam.world_view_transform.numpy(),
                         cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx, cam.tanfovy,
                         scales=scene.scales.numpy(), rotations=scene.rotations.numpy(),
                         colors_precomp=np.zeros((1, 1), np.float32))
    binn_o = orc.binning(pre, W, H)
    assert binn_o["num_rendered"] == n
    assert np.array_equal(a["radii"].cpu().numpy(), pre["radii"])
    assert np.array_equal(a["plist"].cpu().numpy().view(np.uint32), binn_o["point_list"])
    assert np.array_equal(a["ranges"].cpu().numpy().view(np.uint32), binn_o["ranges"])
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), binn_o["keys_sorted"])
    # ... and on the feature map of two tile rows (4 channels), bit for bit
    lo, hi = 30 * gx, 32 * gx
    ob = orc.blend_forward(pre, binn_o, feats.cpu().numpy(), scene.bg[:4].numpy(), W, H, tile_lo=lo, tile_hi=hi)
    rows = slice(30 * 16, 32 * 16)
    assert np.array_equal(a["color"][:, rows].cpu().numpy().view(np.uint32), ob["out"][:, rows].view(np.uint32))
    assert np.array_equal(a["n_contrib"][rows].cpu().numpy().view(np.uint32), ob["n_contrib"][rows])


def test_cfg3_feature_map_properties(cfg3, orc):
    """C = 512 at full size: determinism, partition of unity, linearity, default vs exact arithmetic, and
    the oracle on a sample of tile rows."""
    from sgs_hip import raster
    scene, cam, (P, C, W, H) = cfg3
    s, c = scene.to(DEV), cam.to(DEV)
    gx = (W + 15) // 16
    n, out, radii, geom, binn, img, _ = _render(s, c, C, W, H)
    T = raster.image_views(img, W, H)["final_T"].clone()
    n2, out2, *_ = _render(s, c, C, W, H)
    assert n2 == n and torch.equal(out, out2)                                   # deterministic
    del out2
    raster.set_blend_exact(True)
    try:
        exact = _render(s, c, C, W, H)[1]
        absc = _render(s, c, C, W, H, feats=s.features.abs(), bg=s.bg[:C].abs())[1]   # the absolute composite
        ones = _render(s, c, C, W, H, feats=torch.ones_like(s.features), bg=torch.zeros(C, device=DEV))[1]
    finally:
        raster.set_blend_exact(False)
    # default (six-product) arithmetic within 4e-6 of the absolute composite of the exact fp32 chain -- the chain's own
    # rounding; round 2's two-term split needed 5e-5 (north star: 1e-4)
    assert bool(((out - exact).abs() <= 4e-6 * absc + 1e-30).all())
    # partition of unity: with all features 1 and bg 0 every channel is sum_k w_k = 1 - T_final
    assert float((ones - (1.0 - T)[None]).abs().max()) < 2e-5
    assert torch.equal(ones[0], ones[C - 1])
    del ones, absc
    # linearity in the features (exact arithmetic, fp32 rounding only)
    f2 = torch.roll(s.features, 1, dims=1)
    lin = _render_exact(raster, s, c, C, W, H, s.features + 2.0 * f2)
    rhs = exact + 2.0 * _render_exact(raster, s, c, C, W, H, f2, bg=torch.zeros(C, device=DEV))
    assert float((lin - rhs).abs().max()) < 2e-5
    del lin, rhs, f2
    # the oracle on two tile rows, first 8 channels: bit-identical in exact mode
    pre = orc.preprocess(scene.means3D.numpy(), scene.opacities.numpy(), cam.world_view_transform.numpy(),
                         cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx, cam.tanfovy,
                         scales=scene.scales.numpy(), rotations=scene.rotations.numpy(),
                         colors_precomp=np.zeros((1, 1), np.float32))
    binn_o = orc.binning(pre, W, H)
    ob = orc.blend_forward(pre, binn_o, scene.features[:, :8].contiguous().numpy(), scene.bg[:8].numpy(), W, H,
                           tile_lo=10 * gx, tile_hi=12 * gx)
    rows = slice(10 * 16, 12 * 16)
    assert np.array_equal(exact[:8, rows].cpu().numpy().view(np.uint32), ob["out"][:, rows].view(np.uint32))
    assert np.array_equal(T[rows].cpu().numpy().view(np.uint32), ob["final_T"][rows].view(np.uint32))


def _render_exact(raster, s, c, C, W, H, feats, bg=None):
    raster.set_blend_exact(True)
    try:
        return _render(s, c, C, W, H, feats=feats, bg=bg)[1]
    finally:
        raster.set_blend_exact(False)


def test_cfg3_backward_worklist_path_matches_chunk_kernel(cfg3):
    """C = 512 at full size through autograd: the work-list MFMA backward (default) against the
    reference-shaped per-chunk kernel on every leaf gradient, plus linearity in dL/dpixel."""
    import channel_rasterization as cr
    from sgs_hip import raster
    scene, cam, (P, C, W, H) = cfg3
    s, c = scene.to(DEV), cam.to(DEV)
    settings = cr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=s.bg[:C], scale_modifier=1.0,
        viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0, campos=c.camera_center,
        prefiltered=False, debug=False, num_channels=C)
    rast = cr.GaussianRasterizer(settings)
    g = torch.Generator(device=DEV).manual_seed(3)
    dL = torch.randn(C, H, W, device=DEV, generator=g)

    def grads(mode, dl):
        leaves = [t.clone().requires_grad_(True) for t in (s.means3D, s.opacities, s.features, s.scales, s.rotations)]
        raster.set_backward_mode(mode)
        try:
            out, _ = rast(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), opacities=leaves[1],
                          colors_precomp=leaves[2], scales=leaves[3], rotations=leaves[4])
            out.backward(dl)
            torch.cuda.synchronize()
        finally:
            raster.set_backward_mode(0)
        return [l.grad for l in leaves]

    new, old, f32 = grads(0, dL), grads(1, dL), grads(3, dL)   # split-bf16 products, per-chunk VALU kernel, fp32 MFMA products
    for name, a, b, c in zip(("means3D", "opacities", "features", "scales", "rotations"), new, old, f32):
        scale = float(b.abs().max())
        err, err32 = float((a - b).abs().max()), float((c - b).abs().max())
        print(f"cfg3 backward {name}: max|split - chunk| = {err / scale:.2e}, max|fp32 - chunk| = {err32 / scale:.2e} of the largest entry")
        assert scale > 0 and err <= 1e-4 * scale and err32 <= 1e-4 * scale, name
    half = grads(0, 0.5 * dL)   # exact scaling by a power of two survives every fp32 rounding except the atomics' order
    for a, b in zip(new, half):
        assert float((a - 2.0 * b).abs().max()) <= 1e-4 * float(a.abs().max())


def test_cfg3_backward_matches_the_oracle_on_sampled_tiles(cfg3, orc):
    """cfg3's backward with the ORACLE in the loop (CR/cuda_rasterizer/backward.cu:394-552 restated in oracle/sgs_oracle.c): dL/dout is
    zero outside two sampled runs of tiles, so the full-size HIP backward (work-list products over all 4 941 tiles) equals the oracle's
    backward restricted to those tiles.  Every leaf gradient at the usual bar -- 1e-4 of the largest entry -- for the default arithmetic
    (one fused kernel, two-term bf16 products) and mode 3 (fp32 products)."""
    from sgs_hip import raster
    scene, cam, (P, C, W, H) = cfg3
    s, c = scene.to(DEV), cam.to(DEV)
    gx = (W + 15) // 16
    runs = [(10 * gx + 20, 10 * gx + 44), (41 * gx + 50, 41 * gx + 74)]   # 2 x 24 tiles, two tile rows
    g = torch.Generator().manual_seed(11)
    dL = torch.zeros(C, H, W)
    for lo, hi in runs:
        ty, x0, x1 = lo // gx, (lo % gx) * 16, (hi - 1) % gx * 16 + 16
        dL[:, ty * 16:ty * 16 + 16, x0:x1] = torch.randn(C, 16, x1 - x0, generator=g)
    # the oracle: preprocess + binning of the whole frame, the T chain and the backward on the sampled tiles only
    pre = orc.preprocess(scene.means3D.numpy(), scene.opacities.numpy(), cam.world_view_transform.numpy(),
                         cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx, cam.tanfovy,
                         scales=scene.scales.numpy(), rotations=scene.rotations.numpy(),
                         colors_precomp=np.zeros((1, 1), np.float32))
    binn_o = orc.binning(pre, W, H)
    feats = scene.features.numpy()
    bg = scene.bg[:C].numpy()
    fwd = dict(pre)
    fwd.update(binn_o)
    fwd["features"] = feats
    fwd["final_T"] = np.zeros((H, W), np.float32)
    fwd["n_contrib"] = np.zeros((H, W), np.uint32)
    want = None
    for lo, hi in runs:
        ob = orc.blend_forward(pre, binn_o, np.ascontiguousarray(feats[:, :1]), bg[:1], W, H, tile_lo=lo, tile_hi=hi)
        ty, x0, x1 = lo // gx, (lo % gx) * 16, (hi - 1) % gx * 16 + 16
        fwd["final_T"][ty * 16:ty * 16 + 16, x0:x1] = ob["final_T"][ty * 16:ty * 16 + 16, x0:x1]
        fwd["n_contrib"][ty * 16:ty * 16 + 16, x0:x1] = ob["n_contrib"][ty * 16:ty * 16 + 16, x0:x1]
    for lo, hi in runs:   # (the interval form adds into nothing: one call per run, summed here)
        gr = orc.backward(fwd, dL.numpy(), scene.means3D.numpy(), cam.world_view_transform.numpy(),
                          cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx, cam.tanfovy, bg,
                          scales=scene.scales.numpy(), rotations=scene.rotations.numpy(), cov3D_precomp=None, shs=None,
                          sh_degree=0, tile_lo=lo, tile_hi=hi)
        want = gr if want is None else {k: want[k] + gr[k] for k in gr}
    empty = torch.Tensor([])
    dLd = dL.to(DEV)
    names = ["dL_dmean2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"]
    for mode in (0, 3):
        raster.set_backward_mode(mode)
        try:
            n, out, radii, geom, binn, img, _ = _render(s, c, C, W, H)
            got = raster.rasterize_backward(s.bg[:C], s.means3D, radii, s.features, s.scales, s.rotations, 1.0, empty,
                                            c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy, dLd, empty, 0,
                                            c.camera_center, geom, n, binn, img, False)
            got = [t.cpu().numpy() for t in got]
        finally:
            raster.set_backward_mode(0)
        for i, name in enumerate(names):
            w = want[name]
            if w.size == 0 or got[i].size == 0:
                continue
            scale = float(np.abs(w).max())
            err = float(np.abs(got[i].reshape(w.shape) - w).max())
            print(f"cfg3 backward vs oracle, mode {mode}, {name}: max|hip - oracle| = {err / scale:.2e} of the largest entry")
            assert scale > 0 and err <= 1e-4 * scale, (name, mode, err / scale)


def test_cfg3_pipelined_views_match_serial(cfg3):
    """Four views of the headline scene in flight on four HIP streams (what bench.py times) against the same
    views rendered alone: num_rendered, radii and the whole C = 512 feature map, bit for bit, 10 rounds."""
    import math
    from sgs_hip import raster, dist as sdist
    from sgs_hip.camera import make_camera, focal2fov
    from sgs_hip.synthetic import CONFIGS
    scene, _, (P, C, W, H) = cfg3
    s = scene.to(DEV)
    fx = CONFIGS["cfg3"][4]
    cams = []
    for i in range(4):   # bench.py's view_camera: slightly yawed / shifted views of the same slab
        a = 0.04 * i
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        cams.append(make_camera(R, np.array([0.02 * i, -0.01 * i, 0.0]), focal2fov(fx, W), focal2fov(fx, H), W, H).to(DEV))
    pool = raster.ScratchPool()
    e = torch.Tensor([])

    def render(c, slot):
        out = raster.rasterize_forward(s.bg[:C], s.means3D, s.features, s.opacities, s.scales, s.rotations, 1.0, e,
                                       c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy, H, W, e, 0,
                                       c.camera_center, False, False, C, False, pool=pool)
        return out[0], out[1].clone(), out[2].clone()

    serial = []
    for c in cams:
        serial.append(render(c, 0))
        torch.cuda.synchronize()
    assert len({n for n, _, _ in serial}) > 1          # the views differ
    for _ in range(10):
        piped = sdist.render_views_pipelined(render, cams, in_flight=4)
        for i, ((n0, c0, r0), (n1, c1, r1)) in enumerate(zip(serial, piped)):
            assert n0 == n1, (i, n0, n1)
            assert torch.equal(r0, r1), (i, "radii")
            assert torch.equal(c0, c1), (i, "color")
        del piped


def test_cfg3_deferred_count_and_the_drop_in_module_under_no_grad(cfg3):
    """The deferred count at the headline size: 1 M Gaussians, 245 workgroups in the sort's last pass (chained form), the last of them
    writes the count record.  On a fresh stream a blocking forward teaches the stream its capacity guess; a deferred forward must then
    return the same num_rendered and bits without a retry, and one whose capacity no frame fits must be rendered again.  Then the drop-in
    GaussianRasterizer under torch.no_grad() -- the path fusion.py and eval_segmentation.py take (deferred, resident inference pool) --
    must give the tracked call's image and radii bit for bit."""
    from sgs_hip import raster, _lib
    import channel_rasterization as chn
    scene, cam, (P, C, W, H) = cfg3
    s, c = scene.to(DEV), cam.to(DEV)
    st = torch.cuda.Stream(DEV)   # a fresh stream: no capacity guess yet
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        n, color, radii, *_ = _render(s, c, C, W, H)
        assert n > 10_000_000
        h = _render(s, c, C, W, H, fn=raster.rasterize_forward_deferred)
        o = h.result()
        assert not h.retried and o[0] == n and torch.equal(o[1], color) and torch.equal(o[2], radii)
        del o, h
        h = _render(s, c, C, W, H, fn=raster.rasterize_forward_deferred, _defer_mode=2)
        o = h.result()
        assert h.retried and o[0] == n and torch.equal(o[1], color) and torch.equal(o[2], radii)
        del o, h
        settings = chn.GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=s.bg[:C], scale_modifier=1.0,
            viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0, campos=c.camera_center,
            prefiltered=False, debug=False, num_channels=C)
        rasterizer = chn.GaussianRasterizer(settings)
        feats = torch.nn.Parameter(s.features.clone())
        kw = dict(means3D=s.means3D, means2D=torch.zeros_like(s.means3D, requires_grad=True), opacities=s.opacities,
                  colors_precomp=feats, scales=s.scales, rotations=s.rotations)
        tracked, tracked_radii = rasterizer(**kw)
        assert tracked.requires_grad and torch.equal(tracked.detach(), color) and torch.equal(tracked_radii, radii)
        deferred = raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS)
        with torch.no_grad():
            image, image_radii = rasterizer(**kw)
        assert raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS) == deferred + 1   # it did take the deferred path
        assert not image.requires_grad
        assert torch.equal(image, tracked.detach()) and torch.equal(image_radii, tracked_radii)
        del tracked, image
        raster.release_stream()
