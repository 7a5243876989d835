"""GPU parity tests proper: the HIP path, called through the C-ABI, against the CPU oracle on
the same seeded inputs.  Bar (north star): bit-exact on every integer output (radii, tiles
touched, offsets, 64-bit sort keys, sorted Gaussian lists, tile ranges, n_contrib) and
<= 1e-4 relative on the fp32 feature map -- the arithmetic contract in fact makes the floats
bit-identical as well, which is what these tests assert first."""
import os

import numpy as np
import pytest
import torch

from helpers import small_scene, oracle_forward, has_experiments, need_experiments

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _hip_forward(scene, cam, C=None, want_depth=False, colors=None, variant=0, debug=False,
                 shs=None, sh_degree=0, cov3D_precomp=None, bg=None):
    from sgs_hip import raster
    raster.set_blend_variant(variant)
    s = scene.to(DEV)
    cam = cam.to(DEV)
    empty = torch.Tensor([])
    feats = s.features if colors is None else colors.to(DEV)
    Cn = 3 if shs is not None else feats.shape[1]
    bgt = s.bg if bg is None else torch.as_tensor(bg).to(DEV)
    out = raster.rasterize_forward(
        bgt, s.means3D, empty if shs is not None else feats, s.opacities,
        empty if cov3D_precomp is not None else s.scales,
        empty if cov3D_precomp is not None else s.rotations, 1.0,
        empty if cov3D_precomp is None else torch.as_tensor(cov3D_precomp).to(DEV),
        cam.world_view_transform, cam.full_proj_transform, cam.tanfovx, cam.tanfovy,
        cam.image_height, cam.image_width, empty if shs is None else torch.as_tensor(shs).to(DEV),
        sh_degree, cam.camera_center, False, debug, Cn, want_depth)
    raster.set_blend_variant(0)
    return out


def _check_forward(orc, scene, cam, want_depth=False, variant=0, binning_mode=0, exact=None, two_term=None, **kw):
    from sgs_hip import raster
    if exact is None:   # the C >= 128 default (0) and variants 12-14 accumulate in split bf16; all else is bit-exact
        Cn = 3 if kw.get("shs") is not None else (scene.features.shape[1] if kw.get("colors") is None else kw["colors"].shape[1])
        # C >= 128: 0 (default) = six bf16 products of exact three-term splits ("f32-equivalent"), 14 / nibble 8 = round 2's
        # two-term split; both differ from the oracle's bits, everything else is bit-exact
        bf16 = variant in (0, 14) or (variant >= 16 and (variant & 15) in (6, 7, 8, 10, 12, 13, 14))
        exact = not (bf16 and Cn >= 128 and not want_depth)
    fw = oracle_forward(orc, scene, cam, want_depth=want_depth, **kw)
    raster.set_binning_mode(binning_mode)
    try:
        n, color, radii, geom, binn, img, depth = _hip_forward(scene, cam, want_depth=want_depth,
                                                               variant=variant, **kw)
    finally:
        raster.set_binning_mode(0)
    P = scene.means3D.shape[0]
    W, H = cam.image_width, cam.image_height
    assert n == fw["num_rendered"]
    assert np.array_equal(radii.cpu().numpy(), fw["radii"])
    g = {k: v.cpu().numpy() for k, v in raster.geometry_views(geom, P).items()}
    vis = fw["radii"] > 0
    assert np.array_equal(g["tiles_touched"].view(np.uint32), fw["tiles_touched"])
    if binning_mode == 1:   # mode 0 scans the tile counts in depth-sorted Gaussian order
        assert np.array_equal(g["point_offsets"].view(np.uint32), fw["point_offsets"])
    assert np.array_equal(g["depths"][vis].view(np.uint32), fw["depths"][vis].view(np.uint32))
    assert np.array_equal(g["means2D"][vis].view(np.uint32), fw["means2D"][vis].view(np.uint32))
    assert np.array_equal(g["conic_opacity"][vis].view(np.uint32), fw["conic_opacity"][vis].view(np.uint32))
    if binning_mode == 1:   # the reference order of operations: 64-bit keys emitted in index order
        b = {k: v.cpu().numpy() for k, v in raster.binning_views(binn, n).items()}
        assert np.array_equal(b["keys_unsorted"].view(np.uint64), fw["keys_unsorted"])
        assert np.array_equal(b["vals_unsorted"].view(np.uint32), fw["vals_unsorted"])
    else:                   # mode 0 sorts 32-bit tile ids; the 64-bit sorted keys are rebuilt on demand
        b = {k: v.cpu().numpy() for k, v in raster.binning_views(binn, n, geom, P, img, W, H).items()}
    assert np.array_equal(b["keys_sorted"].view(np.uint64), fw["keys_sorted"])
    assert np.array_equal(b["point_list"].view(np.uint32), fw["point_list"])
    im = {k: v.cpu().numpy() for k, v in raster.image_views(img, W, H).items()}
    assert np.array_equal(im["ranges"].view(np.uint32), fw["ranges"])
    assert np.array_equal(im["n_contrib"].view(np.uint32), fw["n_contrib"])
    assert np.array_equal(im["final_T"].view(np.uint32), fw["final_T"].view(np.uint32))
    out = color.cpu().numpy()
    # north-star tolerance first (1e-4 relative), then the stronger bit-exact claim
    scale = np.abs(fw["out"]).max() + 1e-30
    assert np.abs(out - fw["out"]).max() <= 1e-4 * scale
    if exact:
        assert np.array_equal(out.view(np.uint32), fw["out"].view(np.uint32))
    else:
        # split-bf16 accumulate: |error| <= 3 * 2^-16 (4.6e-5) of every |feature * weight| term
        # (two bf16 terms per operand, the lo*lo product dropped), i.e. bounded by the ABSOLUTE
        # composite (same weights, |features|, |bg|) -- immune to cancellation; measured max
        # 2.1e-5, mean 1.6e-6.  5e-5 is 2x inside the north star's 1e-4.
        sa = scene._replace(features=scene.features.abs(), bg=scene.bg.abs())
        fa = oracle_forward(orc, sa, cam, **kw)["out"]
        if two_term is None:
            two_term = variant == 14 or (variant >= 16 and (variant & 15) == 8)
        # six products: the difference to the oracle is the ORACLE's own fp32 rounding (tests/test_sweep2_gpu.py compares both
        # with the exact composite); two-term split: 3 * 2^-16 per term
        assert (np.abs(out - fw["out"]) <= (5e-5 if two_term else 4e-6) * fa + 1e-30).all()
        assert not np.array_equal(out, fw["out"]) or fa.max() == 0
    if want_depth:
        assert np.array_equal(depth.cpu().numpy().view(np.uint32), fw["depth"].view(np.uint32))
    return fw


def test_expf_contract_bit_exact(orc):
    from sgs_hip import raster
    x = np.concatenate([np.linspace(-25, 0, 4001), -np.logspace(-7, 2.2, 300), [0.0, -87.0, -88.5, -1e4]]).astype(np.float32)
    got = raster.debug_expf(torch.from_numpy(x).to(DEV)).cpu().numpy()
    want = orc.expf(x)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("variant", [15, 1, 2, 3, 4, 5, 6])
def test_forward_c128_all_variants(orc, variant):
    """Every bit-exact blend variant (15 = SGS_BLEND_EXACT: fp32 MFMA accumulate; 1-6 single-kernel forms)."""
    if 1 <= variant <= 5:
        need_experiments("single-kernel blend forms 1-5")
    scene, cam = small_scene(P=3000, C=128, W=200, H=120, fx=170.0, seed=1)
    fw = _check_forward(orc, scene, cam, variant=variant)
    assert fw["n_contrib"].max() > 20 and (fw["final_T"] < 1e-3).any()   # early stop exercised


def test_development_forms_are_not_in_the_product_library():
    """the default libsgs_hip.so holds the kernels that ship (default, exact, round 2's two-term sweep, the gated
    fallback, the remainder / RGB-D kernels, the N1 epilogues); sweep ablations, superseded sweeps and pre-passes, the single-kernel
    forms 1-5 and the two-kernel backward answer SGS_EINVAL unless the library was built with `make EXPERIMENTS=1`."""
    from sgs_hip import raster
    if has_experiments():
        pytest.skip("this library was built with make EXPERIMENTS=1")
    scene, cam = small_scene(P=500, C=128, W=64, H=48, fx=100.0, seed=2)
    for v in (1, 2, 3, 4, 5, 0x6A, 0x6D, 0x6E, 0x67, 0x65, 0x64, 0x69, 0x166, 0x266, 0x466, 0x4066, 0x8066, 0xC066):
        with pytest.raises(RuntimeError, match="EXPERIMENTS"):
            _hip_forward(scene, cam, variant=v)
    for v in (0x110006, 0x100066, 0x210064, 0x310004):   # store placements exist for the free-running x16 sweep only
        with pytest.raises(RuntimeError):
            _hip_forward(scene, cam, variant=v)
    for v in (0, 6, 14, 15, 0x66, 0x10066, 0x10006, 0x10064, 0x10004, 0x110004, 0x110064, 0x6B, 0x68, 0x16, 0x1066):   # what ships
        _hip_forward(scene, cam, variant=v)
    g = torch.Generator().manual_seed(1)
    dL = torch.randn(128, 48, 64, generator=g)
    n, color, radii, geom, binn, img, _ = _hip_forward(scene, cam)
    for mode in (4, 5):
        raster.set_backward_mode(mode)
        try:
            with pytest.raises(RuntimeError, match="EXPERIMENTS"):
                _hip_backward(scene, cam, scene.bg.numpy(), dL, n, radii, geom, binn, img)
        finally:
            raster.set_backward_mode(0)
    _hip_backward(scene, cam, scene.bg.numpy(), dL, n, radii, geom, binn, img)


@pytest.mark.parametrize("variant", [0, 14, 8 + 16 * 1, 14 + 16 * 1])
@pytest.mark.parametrize("C,W,H", [(128, 200, 120), (160, 208, 70), (512, 192, 100), (256, 48, 40), (128, 16, 16), (128, 400, 64)])
def test_forward_split_bf16_within_tolerance(orc, variant, C, W, H):
    """Split-bf16 row-sweep accumulate (default, and with forced 8-tile segments): integer state
    bit-exact, feature map within 5e-5 of the absolute composite.  Widths cover W % 32 == 16
    (staggered pairs), W % 32 == 0, ragged W and a single tile."""
    if variant == 14 + 16 * 1:
        need_experiments("round 3's sweep with 8-tile segments (0x1E)")
    scene, cam = small_scene(P=3000, C=C, W=W, H=H, fx=170.0, seed=C + W)
    _check_forward(orc, scene, cam, variant=variant)


def test_forward_sweep_long_lists(orc):
    """Dense scene, wide image: ~50 tiles per sweep segment with several hundred active entries each,
    so the sweep kernel's batch-table window (1024 batches) has to slide, chunk tables run past
    one chunk per tile and the id ring crosses many tile boundaries."""
    scene, cam = small_scene(P=40000, C=128, W=784, H=32, fx=600.0, seed=77)
    scene = scene._replace(scales=scene.scales * 3.0, opacities=scene.opacities * 0.05)
    _check_forward(orc, scene, cam)        # first frame: the work-list arena overflows, the gated fallback renders
    fw = _check_forward(orc, scene, cam)   # arena grown from the first frame's usage: the sweep renders
    ranges = fw["ranges"].reshape(-1, 2)
    assert (ranges[:, 1] - ranges[:, 0]).max() > 2000 and fw["n_contrib"].max() > 900
    _check_forward(orc, scene, cam, variant=8 + 16 * 6)   # one 49-tile segment: ~2900 batches, the window slides
    _check_forward(orc, scene, cam, variant=15)                  # and the exact path on the same lists


@pytest.mark.parametrize("C", [1, 3, 20, 21, 32, 33, 64, 160, 256, 768])
def test_forward_channel_counts(orc, C):
    scene, cam = small_scene(P=1200, C=C, W=100, H=70, fx=90.0, seed=C)
    _check_forward(orc, scene, cam)               # default arithmetic (split bf16 from 128 channels on)
    if C >= 128:
        _check_forward(orc, scene, cam, variant=15)   # SGS_BLEND_EXACT: bit-identical


@pytest.mark.parametrize("binning_mode", [0, 1, 2])
def test_binning_modes_bit_exact(orc, binning_mode):
    """Both binning algorithms give the oracle's sorted keys / lists / ranges; the reference-order
    mode additionally reproduces point_offsets and the emission-order (unsorted) arrays."""
    if binning_mode:
        need_experiments(f"binning mode {binning_mode} (the library scan / radix sort)")
    scene, cam = small_scene(P=6000, C=4, W=330, H=200, fx=300.0, seed=12)
    # exact duplicates: equal (tile, depth) keys must keep ascending Gaussian index
    m = scene.means3D.clone()
    m[1000:1400] = m[100:500]
    scene = scene._replace(means3D=m)
    fw = _check_forward(orc, scene, cam, binning_mode=binning_mode)
    ks = fw["keys_sorted"]
    assert (ks[1:] == ks[:-1]).sum() > 100      # ties really occur


def test_forward_rgbd_depth(orc):
    scene, cam = small_scene(P=2500, C=3, W=180, H=130, fx=150.0, seed=7)
    fw = _check_forward(orc, scene, cam, want_depth=True)
    assert (fw["depth"] != 15.0).all()
    # sparse scene: uncovered / never-below-0.5 pixels keep the 15.0 default (RR/forward.cu:308)
    scene, cam = small_scene(P=60, C=3, W=180, H=130, fx=150.0, seed=8)
    scene = scene._replace(scales=scene.scales / 3.0)
    d = _check_forward(orc, scene, cam, want_depth=True)["depth"]
    assert (d == 15.0).any() and (d != 15.0).any()     # default and median depths both occur


def test_forward_sh_colours_and_precomputed_cov(orc):
    scene, cam = small_scene(P=1500, C=3, W=128, H=96, fx=110.0, seed=11)
    g = torch.Generator().manual_seed(3)
    shs = (torch.randn(1500, 16, 3, generator=g) * 0.4).numpy()
    for deg in (0, 1, 2, 3):
        fw = _check_forward(orc, scene, cam, shs=shs, sh_degree=deg, want_depth=True)
    assert fw["clamped"].any()
    cov = fw["cov3D"]
    _check_forward(orc, scene, cam, cov3D_precomp=cov)


def test_forward_nonzero_background_and_ragged_image(orc):
    # W,H not multiples of 16: partial tiles on the right/bottom edges
    scene, cam = small_scene(P=900, C=40, W=93, H=51, fx=80.0, seed=4)
    bg = np.linspace(-1, 2, 40).astype(np.float32)
    _check_forward(orc, scene, cam, bg=bg)


def test_empty_scene_and_all_culled():
    from sgs_hip import raster
    scene, cam = small_scene(P=10, C=4, W=64, H=48, fx=60.0)
    empty = scene._replace(means3D=scene.means3D[:0], scales=scene.scales[:0],
                           rotations=scene.rotations[:0], opacities=scene.opacities[:0],
                           features=scene.features[:0], bg=torch.ones(4))
    n, color, radii, *_ = _hip_forward(empty, cam)
    assert n == 0 and color.shape == (4, 48, 64) and not color.any()     # zeros, not bg
    behind = scene._replace(means3D=scene.means3D * torch.tensor([1.0, 1.0, -1.0]), bg=torch.arange(4.0))
    n, color, radii, *_ = _hip_forward(behind, cam)
    assert n == 0 and (radii == 0).all()
    assert torch.equal(color.cpu(), torch.arange(4.0)[:, None, None].expand(4, 48, 64))


def test_debug_flag_and_errors():
    from sgs_hip import raster
    scene, cam = small_scene(P=500, C=8, W=64, H=48, fx=60.0)
    a = _hip_forward(scene, cam, debug=True)
    b = _hip_forward(scene, cam, debug=False)
    assert a[0] == b[0] and torch.equal(a[1], b[1])
    s = scene.to(DEV)
    c = cam.to(DEV)
    e = torch.Tensor([])
    with pytest.raises(RuntimeError, match="For non-RGB, provide precomputed Gaussian colors!"):
        raster.rasterize_forward(s.bg, s.means3D, e, s.opacities, s.scales, s.rotations, 1.0, e,
                                 c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy,
                                 48, 64, torch.zeros(500, 16, 3, device=DEV), 3, c.camera_center,
                                 False, False, 8, False)
    # a background shorter than C (view_viser.py passes a 3-vector with C ~ 20; the reference reads out of
    # bounds): missing channels are 0, with a warning -- or an error under SGS_STRICT_BG=1
    short_bg = torch.tensor([0.25, -0.5, 1.0], device=DEV)
    full_bg = torch.cat([short_bg, torch.zeros(5, device=DEV)])
    args = (s.means3D, s.features, s.opacities, s.scales, s.rotations, 1.0, e, c.world_view_transform,
            c.full_proj_transform, c.tanfovx, c.tanfovy, 48, 64, e, 0, c.camera_center, False, False, 8, False)
    raster._bg_warned = False
    with pytest.warns(UserWarning, match="bg has 3 entries"):
        padded = raster.rasterize_forward(short_bg, *args)[1]
    assert torch.equal(padded, raster.rasterize_forward(full_bg, *args)[1])
    raster.STRICT_BG = True
    try:
        with pytest.raises(RuntimeError, match="bg has 3 entries"):
            raster.rasterize_forward(short_bg, *args)
    finally:
        raster.STRICT_BG = False
    with pytest.raises(RuntimeError, match="prefiltered"):
        far = s.means3D.clone()
        far[0, 2] = -1.0
        raster.rasterize_forward(s.bg, far, s.features, s.opacities, s.scales, s.rotations, 1.0, e,
                                 c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy,
                                 48, 64, e, 0, c.camera_center, True, False, 8, False)


def test_mark_visible(orc):
    from sgs_hip import raster
    scene, cam = small_scene(P=4000, C=1, W=64, H=48, fx=60.0)
    pts = scene.means3D.clone()
    pts[::3, 2] -= 3.0
    got = raster.mark_visible(pts.to(DEV), cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV))
    want = orc.mark_visible(pts.numpy(), cam.world_view_transform.numpy(), cam.full_proj_transform.numpy())
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
    assert want.any() and not want.all()


@pytest.mark.parametrize("P", [1, 2, 3, 5, 64, 1000, 20000])
def test_dist2_bit_exact(orc, P):
    from simple_knn._C import distCUDA2
    g = torch.Generator().manual_seed(P)
    pts = torch.randn(P, 3, generator=g) * torch.tensor([3.0, 1.0, 0.3])
    if P >= 64:
        pts[10] = pts[20]                      # duplicates count at distance 0
        pts[::7] = (pts[::7] * 4).round() / 4  # ties
    got = distCUDA2(pts.to(DEV)).cpu().numpy()
    want = orc.dist2(pts.numpy())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _grad_close(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max() + 1e-20
    return np.abs(a - b).max() / scale <= tol, np.abs(a - b).max() / scale


@pytest.mark.parametrize("C,use_sh,precomp_cov", [(3, True, False), (3, False, False), (3, False, True),
                                                  (4, False, False), (32, False, False), (80, False, False),
                                                  (128, False, False), (160, False, False)])
def test_backward_parity(orc, C, use_sh, precomp_cov):
    """Backward (runtime C) against the oracle; fp32 atomics sum in unspecified order, so the
    bar is 1e-4 of the largest gradient entry (oracle accumulates in float64)."""
    from sgs_hip import raster
    scene, cam = small_scene(P=1500, C=C, W=96, H=80, fx=85.0, seed=20 + C)
    W, H = cam.image_width, cam.image_height
    g = torch.Generator().manual_seed(9)
    shs = (torch.randn(1500, 16, 3, generator=g) * 0.4).numpy() if use_sh else None
    bg = np.linspace(0.1, 0.9, C).astype(np.float32)
    fw = oracle_forward(orc, scene, cam, shs=shs, sh_degree=3, bg=bg)
    cov = fw["cov3D"] if precomp_cov else None
    if precomp_cov:
        fw = oracle_forward(orc, scene, cam, cov3D_precomp=cov, bg=bg)
    dL = torch.randn(C, H, W, generator=g)
    gr = orc.backward(fw, dL.numpy(), scene.means3D.numpy(), cam.world_view_transform.numpy(),
                      cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx,
                      cam.tanfovy, bg, scales=None if precomp_cov else scene.scales.numpy(),
                      rotations=None if precomp_cov else scene.rotations.numpy(), cov3D_precomp=cov,
                      shs=shs, sh_degree=3)
    n, color, radii, geom, binn, img, _ = _hip_forward(scene, cam, shs=shs, sh_degree=3,
                                                       cov3D_precomp=cov, bg=bg)
    s = scene.to(DEV)
    c = cam.to(DEV)
    e = torch.Tensor([])
    out = raster.rasterize_backward(
        torch.from_numpy(bg).to(DEV), s.means3D, radii, e if use_sh else s.features,
        e if precomp_cov else s.scales, e if precomp_cov else s.rotations, 1.0,
        e if not precomp_cov else torch.from_numpy(cov).to(DEV), c.world_view_transform,
        c.full_proj_transform, c.tanfovx, c.tanfovy, dL.to(DEV),
        e if not use_sh else torch.from_numpy(shs).to(DEV), 3, c.camera_center, geom, n, binn, img, False)
    names = ["dL_dmean2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
             "dL_dscales", "dL_drotations"]
    for name, t in zip(names, out):
        want = gr[name]
        got = t.cpu().numpy().reshape(want.shape)
        if want.size == 0:
            continue
        if name == "dL_dcolors" and use_sh:
            continue   # with SH colours dL_dcolors is the internal dL_dRGB; checked through dL_dsh
        ok, err = _grad_close(got, want, 1e-4)
        assert ok, (name, err)
    assert np.abs(gr["dL_dmeans3D"]).max() > 0


def _hip_backward(scene, cam, bg, dL, n, radii, geom, binn, img):
    from sgs_hip import raster
    s, c = scene.to(DEV), cam.to(DEV)
    e = torch.Tensor([])
    return raster.rasterize_backward(
        torch.from_numpy(bg).to(DEV), s.means3D, radii, s.features, s.scales, s.rotations, 1.0, e,
        c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy, dL.to(DEV), e, 3, c.camera_center,
        geom, n, binn, img, False)


@pytest.mark.parametrize("C,P,W,H,fx,dense", [(128, 1500, 96, 80, 85.0, False), (192, 2500, 100, 70, 90.0, False),
                                               (128, 12000, 150, 40, 300.0, True), (512, 1500, 64, 48, 60.0, False),
                                               (32, 2000, 101, 67, 90.0, False), (96, 1500, 64, 64, 70.0, False),
                                               (128, 12000, 272, 256, 500.0, True), (64, 9000, 333, 290, 300.0, False),
                                               (32, 8000, 331, 277, 300.0, False)])
def test_backward_worklist_mfma_path(orc, C, P, W, H, fx, dense):
    """C >= 32, C % 32 == 0: the backward blend as matrix products over the work list (blend_bwd_mfma.hip)
    against the oracle AND against the per-chunk kernel; ragged image edges (also a width that is not a
    multiple of 4), partial 128-channel groups, (dense) lists of several hundred active entries per tile =
    several arena chunks, and mode 2 = undersized arena: the device-side overflow flag hands over to the
    per-chunk kernel.  The last two cases have more tiles than the part has compute units: there the fused kernel runs as
    persistent workgroups that take tiles by ticket and prefetch the next tile's first loads (round 6)."""
    from sgs_hip import raster
    scene, cam = small_scene(P=P, C=C, W=W, H=H, fx=fx, seed=40 + C + P)
    if dense:
        scene = scene._replace(scales=scene.scales * 2.0, opacities=scene.opacities * 0.05)
    g = torch.Generator().manual_seed(5)
    bg = np.linspace(0.1, 0.9, C).astype(np.float32)
    dL = torch.randn(C, H, W, generator=g)
    fw = oracle_forward(orc, scene, cam, bg=bg)
    gr = orc.backward(fw, dL.numpy(), scene.means3D.numpy(), cam.world_view_transform.numpy(),
                      cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx,
                      cam.tanfovy, bg, scales=scene.scales.numpy(), rotations=scene.rotations.numpy(),
                      cov3D_precomp=None, shs=None, sh_degree=3)
    if dense:
        assert fw["n_contrib"].max() > 300
    outs = {}
    modes = (0, 1, 2, 3, 4, 5) if has_experiments() else (0, 1, 2, 3)
    for mode in modes:   # 0 fused kernel, split-bf16 products (default), 1 per-chunk kernel, 2 overflow fallback, 3 fused, fp32 products, 4 / 5 rounds 2-4's two kernels
        raster.set_backward_mode(mode)
        try:
            n, color, radii, geom, binn, img, _ = _hip_forward(scene, cam, bg=bg)
            outs[mode] = [t.cpu().numpy() for t in _hip_backward(scene, cam, bg, dL, n, radii, geom, binn, img)]
        finally:
            raster.set_backward_mode(0)
    names = ["dL_dmean2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
             "dL_dscales", "dL_drotations"]
    for i, name in enumerate(names):
        want = gr[name]
        if want.size == 0:
            continue
        for mode in modes:
            ok, err = _grad_close(outs[mode][i].reshape(want.shape), want, 1e-4)
            assert ok, (name, mode, err)
    assert np.abs(outs[0][1]).max() > 0


def test_backward_overflow_fallback_on_a_strided_grid():
    """The fallback behind the work-list path (blend_bwd.hip) is launched on a strided grid of 2 048 workgroups when it is gated -- 79 056
    workgroups that only read the gate word were 21 us of every cfg3 backward.  3 800 (tile, chunk) blocks here: mode 2 (undersized arena: the
    gate opens, every workgroup walks several blocks) against mode 1 (the same kernel, one workgroup per block, no gate)."""
    from sgs_hip import raster
    C, P, W, H, fx = 256, 20000, 400, 300, 350.0
    scene, cam = small_scene(P=P, C=C, W=W, H=H, fx=fx, seed=77)
    bg = np.linspace(0.1, 0.9, C).astype(np.float32)
    dL = torch.randn(C, H, W, generator=torch.Generator().manual_seed(6))
    from sgs_hip import _lib
    outs = {}
    overflows0 = raster.stream_stat(_lib.STAT_BWD_OVERFLOWS)
    for mode in (2, 0, 1):   # (the overflow of a backward is read back by the stream's next work-list backward: mode 0 in the middle)
        raster.set_backward_mode(mode)
        try:
            n, color, radii, geom, binn, img, _ = _hip_forward(scene, cam, bg=bg)
            outs[mode] = [t.cpu().numpy() for t in _hip_backward(scene, cam, bg, dL, n, radii, geom, binn, img)]
        finally:
            raster.set_backward_mode(0)
    assert raster.stream_stat(_lib.STAT_BWD_OVERFLOWS) - overflows0 >= 1   # the gate did open in mode 2
    assert ((W + 15) // 16) * ((H + 15) // 16) * (C // 32) > 2048
    for a, b in zip(outs[2], outs[1]):
        if b.size == 0:
            continue
        ok, err = _grad_close(a, b, 1e-5)
        assert ok, err
    assert np.abs(outs[1][1]).max() > 0


def test_channel_rasterization_call_pattern_matches_render_chn(orc):
    """Executes the exact kwargs of model/renderer.py:169-183,228-237 (render_chn) and of
    :54-69,111 (render) against the drop-in packages, with autograd through both."""
    import channel_rasterization as chn_rasterize
    from rgbd_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    scene, cam = small_scene(P=2000, C=16, W=128, H=96, fx=100.0, seed=3)
    s = scene.to(DEV)
    c = cam.to(DEV)
    fw = oracle_forward(orc, scene, cam)
    xyz = s.means3D.clone().requires_grad_(True)
    feats = s.features.clone().requires_grad_(True)
    screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device="cuda") + 0
    screenspace_points.retain_grad()
    raster_settings = chn_rasterize.GaussianRasterizationSettings(
        image_height=96, image_width=128, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=s.bg,
        scale_modifier=1.0, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform,
        sh_degree=3, campos=c.camera_center, prefiltered=False, debug=True, num_channels=16)
    rasterizer = chn_rasterize.GaussianRasterizer(raster_settings=raster_settings)
    # a non-contiguous column slice as override_color (eval_segmentation.py:383,392)
    wide = torch.cat([feats, feats], dim=1)
    rendered_image, radii = rasterizer.forward(
        means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=wide[:, :16],
        opacities=s.opacities, scales=s.scales, rotations=s.rotations, cov3D_precomp=None)
    assert rendered_image.shape == (16, 96, 128) and radii.dtype == torch.int32
    assert np.array_equal(rendered_image.detach().cpu().numpy(), fw["out"])
    assert np.array_equal((radii > 0).cpu().numpy(), fw["radii"] > 0)
    rendered_image.square().sum().backward()
    assert screenspace_points.grad.shape == (2000, 3) and screenspace_points.grad[:, :2].abs().sum() > 0
    assert xyz.grad.abs().sum() > 0 and feats.grad.abs().sum() > 0

    rs = GaussianRasterizationSettings(
        image_height=96, image_width=128, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(3, device=DEV),
        scale_modifier=1.0, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform,
        sh_degree=0, campos=c.camera_center, prefiltered=False, debug=False)
    rgb = torch.rand(2000, 3, device=DEV)
    img, radii, depth = GaussianRasterizer(raster_settings=rs)(
        means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=rgb,
        opacities=s.opacities, scales=s.scales, rotations=s.rotations, cov3D_precomp=None)
    assert img.shape == (3, 96, 128) and depth.shape == (1, 96, 128) and not depth.requires_grad
    vis = GaussianRasterizer(raster_settings=rs).markVisible(xyz)
    assert vis.dtype == torch.bool and vis.shape == (2000,)


def test_views_pipelined_on_two_streams_match_serial():
    """Two views in flight on two HIP streams (sgs_hip.dist.render_views_pipelined) give exactly the
    serial results: nothing in the library is shared between concurrent forwards except read-only inputs."""
    from sgs_hip import raster, dist as sdist
    from sgs_hip.camera import pinhole
    scene, cam0 = small_scene(P=5000, C=128, W=208, H=128, fx=170.0, seed=5)
    s = scene.to(DEV)
    cams = [pinhole(208, 128, fx).to(DEV) for fx in (150.0, 160.0, 170.0, 180.0, 190.0, 200.0)]
    e = torch.Tensor([])
    pool = raster.ScratchPool()   # one pool: scratch is keyed by stream

    def render(c, slot):
        out = raster.rasterize_forward(s.bg, s.means3D, s.features, s.opacities, s.scales, s.rotations, 1.0, e,
                                       c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy,
                                       128, 208, e, 0, c.camera_center, False, False, 128, False, pool=pool)
        return out[0], out[1].clone(), out[2].clone()

    serial = [render(c, 0) for c in cams]
    torch.cuda.synchronize()
    piped = sdist.render_views_pipelined(render, cams, in_flight=2)
    assert sum(n for n, _, _ in serial) > 0
    for i, ((n0, c0, r0), (n1, c1, r1)) in enumerate(zip(serial, piped)):
        assert n0 == n1, (i, n0, n1)
        assert torch.equal(r0, r1), (i, "radii")
        assert torch.equal(c0, c1), (i, "color", float((c0 - c1).abs().max()))
    # stress: 4 000 rounds (24 000 forwards, ~7 s: a 1-in-1000 event is missed with probability e^-24) with four views in flight.  Kernels of different views share CUs here; a forward
    # must not be disturbed by what runs beside it (the sweep's choice of MFMA instruction, DESIGN.md 5.4:
    # with v_mfma_f32_32x32x16_bf16 about one forward in a thousand came out with wrong radii).
    light = [(n, r) for n, _, r in serial]
    del serial, piped

    def render_light(c, slot):
        n, _, r = render(c, slot)
        return n, r

    bad = 0
    ROUNDS = 4000
    for _ in range(ROUNDS):
        for (n0, r0), (n1, r1) in zip(light, sdist.render_views_pipelined(render_light, cams, in_flight=4)):
            bad += int(n0 != n1 or not torch.equal(r0, r1))
    assert bad == 0, f"{bad} of {ROUNDS * len(cams)} pipelined forwards differ from the serial result"


def test_no_grad_with_parameters_uses_the_resident_pool():
    """fusion.py / eval_segmentation.py pass nn.Parameters under torch.no_grad(): the state buffers must come
    from the resident inference pool (same storage on the next frame), not from fresh allocations."""
    import channel_rasterization as chn
    from sgs_hip import raster
    scene, cam = small_scene(P=1500, C=8, W=64, H=48, fx=60.0)
    s, c = scene.to(DEV), cam.to(DEV)
    settings = chn.GaussianRasterizationSettings(
        image_height=48, image_width=64, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=s.bg, scale_modifier=1.0,
        viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0, campos=c.camera_center,
        prefiltered=False, debug=False, num_channels=8)
    xyz = torch.nn.Parameter(s.means3D.clone())
    feats = torch.nn.Parameter(s.features.clone())
    rast = chn.GaussianRasterizer(settings)
    raster.INFERENCE_POOL.clear()
    ptrs = []
    for _ in range(3):
        with torch.no_grad():
            color, radii = rast(means3D=xyz, means2D=torch.zeros_like(xyz), opacities=s.opacities,
                                colors_precomp=feats, scales=s.scales, rotations=s.rotations)
        assert not color.requires_grad
        ptrs.append(sorted(t.data_ptr() for t in raster.INFERENCE_POOL._t.values()))
    assert len(ptrs[0]) == 3 and ptrs[0] == ptrs[1] == ptrs[2]
    # with grad enabled the buffers belong to the autograd graph instead
    raster.INFERENCE_POOL.clear()
    color, _ = rast(means3D=xyz, means2D=torch.zeros_like(xyz, requires_grad=True), opacities=s.opacities,
                    colors_precomp=feats, scales=s.scales, rotations=s.rotations)
    assert color.requires_grad and len(raster.INFERENCE_POOL._t) == 0
    color.sum().backward()
    assert feats.grad is not None


def test_inference_calls_enqueue_the_frame_before_waiting_for_the_count(orc):
    """sgs_hip.api.SPECULATIVE_COUNT: under no_grad the drop-in module enqueues the whole frame against the stream's
    capacity guess and only then waits for num_rendered.  Same results as the tracked (classic) path bit for bit --
    also for a frame that outgrew the guess (rendered again) and with debug=True (model/renderer.py:181)."""
    import channel_rasterization as chn
    from sgs_hip import raster, api, _lib
    assert api.SPECULATIVE_COUNT
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        small, cam = small_scene(P=300, C=128, W=160, H=96, fx=120.0, seed=3)
        big, _ = small_scene(P=9000, C=128, W=160, H=96, fx=120.0, seed=4)
        big = big._replace(scales=big.scales * 2.5)
        c = cam.to(DEV)
        for debug in (False, True):
            settings = chn.GaussianRasterizationSettings(
                image_height=96, image_width=160, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=small.bg.to(DEV), scale_modifier=1.0,
                viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0, campos=c.camera_center,
                prefiltered=False, debug=debug, num_channels=128)
            rast = chn.GaussianRasterizer(settings)
            retries0 = raster.stream_stat(_lib.STAT_DEFERRED_RETRIES)
            deferred0 = raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS)
            for scene in (small, small, big, big, small):
                s = scene.to(DEV)
                kw = dict(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                          colors_precomp=s.features, scales=s.scales, rotations=s.rotations)
                with torch.no_grad():
                    color, radii = rast(**kw)
                tracked = dict(kw, colors_precomp=s.features.clone().requires_grad_(True))
                color_t, radii_t = rast(**tracked)
                assert torch.equal(color, color_t.detach()) and torch.equal(radii, radii_t)
                assert np.array_equal(radii.cpu().numpy(), oracle_forward(orc, scene, cam)["radii"])
            assert raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS) - deferred0 >= 3      # the path was really taken
            assert raster.stream_stat(_lib.STAT_DEFERRED_RETRIES) - retries0 >= 1        # small -> big outgrew the guess
    torch.cuda.synchronize()


def test_options_and_state_are_per_stream(orc):
    """Two callers in one process: stream A renders with the exact fp32 arithmetic and binning mode 1, stream B
    with the defaults, interleaved.  Each gets its own result and its own work-list state."""
    from sgs_hip import raster, _lib
    scene, cam = small_scene(P=2500, C=128, W=96, H=80, fx=85.0)
    want = oracle_forward(orc, scene, cam)["out"]
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        assert raster.set_stream_option(_lib.OPT_BLEND_VARIANT, 15) == 0x7fffffff
        if has_experiments():   # (binning mode 1 runs on the library scan / sort: make EXPERIMENTS=1)
            raster.set_stream_option(_lib.OPT_BINNING_MODE, 1)
    outs = {"a": [], "b": []}
    for _ in range(3):
        with torch.cuda.stream(sa):
            outs["a"].append(_hip_forward(scene, cam)[1])
        with torch.cuda.stream(sb):
            outs["b"].append(_hip_forward(scene, cam)[1])
    torch.cuda.synchronize()
    for o in outs["a"]:
        assert np.array_equal(o.cpu().numpy(), want)                      # exact arithmetic: the oracle's bits
    for o in outs["b"]:
        got = o.cpu().numpy()
        assert not np.array_equal(got, want)                              # default (split-bf16) arithmetic
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
    with torch.cuda.stream(sa):
        assert raster.stream_stat(_lib.STAT_FORWARDS) == 3
        assert raster.set_stream_option(_lib.OPT_BLEND_VARIANT, -1) == 15  # back to the process default
        assert raster.release_stream() == 1
    with torch.cuda.stream(sb):
        assert raster.stream_stat(_lib.STAT_FORWARDS) == 3 and raster.stream_stat(_lib.STAT_ARENA_SLOTS) > 0
        raster.release_stream()


def test_backward_worklist_feedback_is_per_stream(orc):
    """C = 64: the forward never builds a work list (below 128 channels), so the backward learns its capacity
    from its own feedback.  A backward whose work list overflowed (forced here with backward mode 2) is counted
    on ITS stream when the next backward reads the feedback, the per-chunk fallback and the MFMA path give the
    same gradients, and another stream's counters stay untouched."""
    from sgs_hip import raster, _lib
    scene, cam = small_scene(P=3000, C=64, W=64, H=48, fx=60.0)
    s, c = scene.to(DEV), cam.to(DEV)
    e = torch.Tensor([])
    st, other = torch.cuda.Stream(), torch.cuda.Stream()
    dL = torch.randn(64, 48, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
    torch.cuda.synchronize()

    def fwd_bwd():
        n, color, radii, geom, binn, img, _ = raster.rasterize_forward(
            s.bg, s.means3D, s.features, s.opacities, s.scales, s.rotations, 1.0, e, c.world_view_transform,
            c.full_proj_transform, c.tanfovx, c.tanfovy, 48, 64, e, 0, c.camera_center, False, False, 64, False)
        g = raster.rasterize_backward(s.bg, s.means3D, radii, s.features, s.scales, s.rotations, 1.0, e,
                                      c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy,
                                      dL, e, 0, c.camera_center, geom, n, binn, img, False)
        torch.cuda.current_stream().synchronize()
        return [t.clone() for t in g]

    with torch.cuda.stream(st):
        raster.set_stream_option(_lib.OPT_BACKWARD_MODE, 2)     # undersized work list: overflow -> fallback
        g_fallback = fwd_bwd()
        raster.set_stream_option(_lib.OPT_BACKWARD_MODE, -1)
        assert raster.stream_stat(_lib.STAT_BWD_OVERFLOWS) == 0   # not read back yet
        g_mfma = fwd_bwd()
        assert raster.stream_stat(_lib.STAT_BWD_OVERFLOWS) == 1
        g_again = fwd_bwd()
        assert raster.stream_stat(_lib.STAT_BWD_OVERFLOWS) == 1   # the default-capacity backward did not overflow
        raster.release_stream()
    with torch.cuda.stream(other):
        fwd_bwd()
        fwd_bwd()
        assert raster.stream_stat(_lib.STAT_BWD_OVERFLOWS) == 0
        raster.release_stream()
    for a, b, c2 in zip(g_fallback, g_mfma, g_again):
        if b.numel() == 0:   # (dL_dsh: no SH coefficients in this call)
            continue
        scale = b.abs().max().item() + 1e-20
        assert (a - b).abs().max().item() <= 2e-4 * scale
        assert (c2 - b).abs().max().item() <= 2e-4 * scale


@pytest.mark.parametrize("variant", [33, 35, 32, 34])
@pytest.mark.parametrize("C,W,H,P", [(128, 208, 160, 2500), (256, 200, 120, 2500), (512, 192, 100, 2500), (384, 100, 70, 2000)])
def test_fused_single_kernel_variants(orc, variant, C, W, H, P):
    if os.environ.get("SGS_WITH_FUSED", "0") != "1":
        pytest.skip("the fused single-kernel experiments are built only with `make FUSED=1` (set SGS_WITH_FUSED=1 to test them)")
    """The experimental single-kernel forward blends (blend_fused.hip: every wave autonomous, variants 32 / 33;
    blend_fused_pc.hip: one producer wave + C / 64 consumer waves per workgroup, 34 / 35).  Not the default -- both are
    slower than the two-kernel path (DESIGN.md 5.6) -- but they are complete renderers and must stay exact: the
    odd variants use fp32 MFMA and return the oracle's bits, the even ones the split-bf16 products."""
    scene, cam = small_scene(P=P, C=C, W=W, H=H, fx=90.0, seed=C)
    scene = scene._replace(bg=torch.linspace(-1.0, 1.0, C))
    _check_forward(orc, scene, cam, variant=variant, exact=bool(variant & 1), two_term=True)


@pytest.mark.parametrize("C,W,H", [(128, 205, 70), (256, 100, 52), (160, 49, 40), (128, 208, 64)])
def test_output_pitch_option(orc, C, W, H):
    """Opt-in row-padded output planes (sgs_hip.raster.OUTPUT_PITCH_ALIGN / SGS_OPT_OUT_PITCH): the (C,H,W) view of
    the padded tensor holds exactly the contiguous render's bits -- only the store addresses change -- in both
    arithmetic modes, for widths that are and are not multiples of 16."""
    from sgs_hip import raster
    scene, cam = small_scene(P=2500, C=C, W=W, H=H, fx=90.0, seed=W)
    scene = scene._replace(bg=torch.linspace(-1.0, 1.0, C))
    want = {v: _hip_forward(scene, cam, variant=v)[1].clone() for v in (0, 15)}
    raster.OUTPUT_PITCH_ALIGN = 32
    try:
        for v in (0, 15):
            out = _hip_forward(scene, cam, variant=v)[1]
            padded = W % 32 != 0
            assert out.shape == (C, H, W) and out.is_contiguous() == (not padded)
            if padded:
                assert out.stride() == (H * (-(-W // 32) * 32), -(-W // 32) * 32, 1)
            assert torch.equal(out, want[v])
    finally:
        raster.OUTPUT_PITCH_ALIGN = 0
    fw = oracle_forward(orc, scene, cam)
    assert np.array_equal(want[15].cpu().numpy(), fw["out"])


def _fwd_args(scene, cam, want_depth=False):
    s, c = scene.to(DEV), cam.to(DEV)
    e = torch.Tensor([])
    Cn = s.features.shape[1]
    return (s.bg, s.means3D, s.features, s.opacities, s.scales, s.rotations, 1.0, e, c.world_view_transform,
            c.full_proj_transform, c.tanfovx, c.tanfovy, c.image_height, c.image_width, e, 0, c.camera_center,
            False, False, Cn, want_depth)


@pytest.mark.gpu
@pytest.mark.parametrize("C,want_depth", [(128, False), (160, False), (16, False), (3, True)])
def test_deferred_count_forward_matches_blocking(C, want_depth):
    """SGS_OPT_DEFER_COUNT: the forward that never reads num_rendered back (buffers sized from the stream's previous
    frame, counts checked on the device) returns the blocking forward's bits -- feature map, depth, radii, final_T,
    n_contrib -- and its num_rendered; the first deferred call of a stream is an ordinary one (no guess yet); a frame
    that outgrows the guess aborts on the device and is rendered again; an all-culled frame works."""
    from sgs_hip import raster, _lib
    st = torch.cuda.Stream(DEV)   # a fresh stream: no capacity guess yet
    scene, cam = small_scene(P=3000, C=C, W=200, H=136, fx=120.0, seed=11 + C)
    args = _fwd_args(scene, cam, want_depth)
    H, W = 136, 200
    with torch.cuda.stream(st):
        want = raster.rasterize_forward(*args)
        iv = raster.image_views(want[5], W, H)
        want_T, want_nc = iv["final_T"].clone(), iv["n_contrib"].clone()
        want_color, want_depth_map = want[1].clone(), (want[6].clone() if want_depth else None)
        base = raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS)
        for k in range(3):
            h = raster.rasterize_forward_deferred(*args)
            assert h.layout_count >= want[0]
            out = h.result()
            assert not h.retried and out[0] == want[0]
            assert torch.equal(out[1], want_color) and torch.equal(out[2], want[2])
            iv = raster.image_views(out[5], W, H)
            assert torch.equal(iv["final_T"], want_T) and torch.equal(iv["n_contrib"], want_nc)
            if want_depth:
                assert torch.equal(out[6], want_depth_map)
        assert raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS) == base + 3
        # a capacity no frame fits: aborted on the device, rendered again by result()
        h = raster.rasterize_forward_deferred(*args, _defer_mode=2)
        out = h.result()
        assert h.retried and out[0] == want[0] and torch.equal(out[1], want_color)
        assert raster.stream_stat(_lib.STAT_DEFERRED_RETRIES) >= 1
        # a much larger frame on the same stream outgrows the guess learnt above
        big, bcam = small_scene(P=40000, C=C, W=200, H=136, fx=120.0, seed=5)
        big = big._replace(scales=big.scales * 1.5)
        bargs = _fwd_args(big, bcam, want_depth)
        bwant = raster.rasterize_forward(*_fwd_args(big, bcam, want_depth))
        bcolor = bwant[1].clone()
        raster.rasterize_forward(*args)   # (the guess follows the last frame: small again)
        h = raster.rasterize_forward_deferred(*bargs)
        out = h.result()
        assert out[0] == bwant[0] and torch.equal(out[1], bcolor)
        if bwant[0] > 2 * want[0] + (1 << 17):
            assert h.retried
        # nothing visible
        behind = scene._replace(means3D=scene.means3D * torch.tensor([1.0, 1.0, -1.0]))
        h = raster.rasterize_forward_deferred(*_fwd_args(behind, cam, want_depth))
        out = h.result()
        assert out[0] == 0 and (out[2] == 0).all()
        assert torch.equal(out[1], scene.bg.to(DEV)[:C, None, None].expand(C, H, W))
        raster.release_stream()


@pytest.mark.gpu
def test_pipelined_views_with_deferred_counts():
    """render_views_pipelined with deferred-count forwards: same images as serial blocking rendering."""
    from sgs_hip import raster, dist as sdist
    scene, cam = small_scene(P=6000, C=128, W=256, H=160, fx=140.0, seed=3)
    args = _fwd_args(scene, cam)
    want = raster.rasterize_forward(*args)[1].clone()
    pools = [raster.ScratchPool() for _ in range(3)]

    def fn(v, slot):
        return raster.rasterize_forward_deferred(*args, pool=pools[slot])

    outs = sdist.render_views_pipelined(fn, list(range(10)), in_flight=3)
    assert len(outs) == 10
    for o in outs:
        assert isinstance(o, tuple) and torch.equal(o[1], want)


def _sort_keys(P, kind, g):
    """Keys of one kind for the depth-sort tests (int64 holding the uint32 bit patterns)."""
    if kind == "random":
        return torch.randint(0, 2 ** 32, (P,), device=DEV, generator=g, dtype=torch.int64)
    if kind == "depth":
        return (0.2 + 60.0 * torch.rand(P, device=DEV, generator=g)).view(torch.int32).to(torch.int64)
    if kind == "equal":
        return torch.full((P,), 0x40490FDB, device=DEV, dtype=torch.int64)
    if kind == "planes":
        return torch.tensor([1.0, 1.5, 2.0, 2.0000002, 7.25], device=DEV)[
            torch.randint(0, 5, (P,), device=DEV, generator=g)].view(torch.int32).to(torch.int64)
    if kind.startswith("digit"):   # one random byte at that position, the other three fixed: three passes see a single bin
        b = 8 * int(kind[5:])
        return (0x3FA5C35A & ~(0xFF << b)) | (torch.randint(0, 256, (P,), device=DEV, generator=g, dtype=torch.int64) << b)
    if kind == "narrow-depth":     # the floats of [1, 2): the top byte is 0x3F throughout
        return 0x3F800000 | torch.randint(0, 1 << 23, (P,), device=DEV, generator=g, dtype=torch.int64)
    if kind == "all-culled":
        return torch.full((P,), 0xFFFFFFFF, device=DEV, dtype=torch.int64)
    assert kind == "culled", kind
    keys = (0.2 + 5.0 * torch.rand(P, device=DEV, generator=g)).view(torch.int32).to(torch.int64)
    keys[torch.rand(P, device=DEV, generator=g) < 0.9] = 0xFFFFFFFF
    return keys


@pytest.mark.gpu
@pytest.mark.parametrize("P,kind", [(1, "random"), (63, "random"), (4096, "random"), (4097, "random"),
                                    (300000, "random"), (1000003, "depth"), (200000, "equal"),
                                    (500000, "planes"), (150001, "culled"), (5000000, "depth"),
                                    # 32 tiles per group: one group -> two
                                    (131072, "random"), (131072, "narrow-depth"), (131073, "random"), (131073, "depth"),
                                    (131073, "digit0"),
                                    # 64 groups: the longest chained walk
                                    (8388608, "random"), (8388608, "depth"), (8388608, "narrow-depth"),
                                    # 65 groups: three levels, 3 super-groups, the last tile holds one key
                                    (8388609, "random"), (8388609, "depth"), (8388609, "digit1"), (8388609, "all-culled"),
                                    # 96 -> 97 groups: three super-groups -> four
                                    (12582912, "random"), (12582912, "culled"), (12582912, "digit2"),
                                    (12582913, "random"), (12582913, "narrow-depth"), (12582913, "digit3"),
                                    # BASELINE cfg5's size: 382 groups, 12 super-groups
                                    (50000000, "random"), (50000000, "depth"), (50000000, "digit0")])
def test_depth_sort_matches_stable_sort(P, kind):
    """csrc/depth_sort.hip (the forward's presort of the Gaussians) on bare keys against torch's stable sort:
    full-range random keys, depth-like float bit patterns, all keys equal (ties resolve by index), a handful of
    distinct values, mostly-culled (0xFFFFFFFF) and all-culled keys, keys in which a single byte varies (the other
    passes see one bin) or the top byte is constant (floats of [1, 2)); sizes around the 4096-key tile, the 32-tile
    group, the 64-group switch from the chained passes to three levels of count rows, a 32-group super-group, and
    BASELINE config 5's 50 M keys."""
    import ctypes as C
    from sgs_hip import _lib
    lib = _lib.load()
    g = torch.Generator(device=DEV).manual_seed(P)
    keys = _sort_keys(P, kind, g)
    want = torch.sort(keys, stable=True).indices.to(torch.int32)
    k32 = (keys & 0xFFFFFFFF).to(torch.int64)
    k32 = torch.where(k32 >= 2 ** 31, k32 - 2 ** 32, k32).to(torch.int32)   # same bits as uint32
    need = lib.sgs_debug_depth_sort(P, None, None, None, None)
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)
    perm = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(2):   # (twice: the count matrices must be cleared every time)
        rc = lib.sgs_debug_depth_sort(P, k32.data_ptr(), perm.data_ptr(), scratch.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(perm, want)


def test_output_pitch_is_consumed_by_one_forward(orc):
    """the per-stream output pitch must not outlive the call it was set for (a stale pitch on a later
    forward with a contiguous buffer is an out-of-bounds write).  The library consumes the override in the forward;
    an exception between the Python layer's set and its call cannot leave it behind either."""
    import ctypes as C
    from sgs_hip import raster, _lib
    lib = _lib.load()
    scene, cam = small_scene(P=1500, C=128, W=205, H=48, fx=90.0, seed=3)
    sp = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    with torch.cuda.device(DEV):
        lib.sgs_stream_set_option(sp, _lib.OPT_OUT_PITCH, 205)
        want = _hip_forward(scene, cam, variant=15)   # a contiguous forward: pitch == W, the override changes nothing but is consumed
    # (round 4: this used to set 224 -- wider than the contiguous buffer -- and so made the forward write 0.5 MB past its
    # end; harmless only while the allocator had mapped memory behind it: a GPU memory fault in a shorter test run.)  What
    # is checked is that the override is gone afterwards
    with torch.cuda.device(DEV):
        prev = lib.sgs_stream_set_option(sp, _lib.OPT_OUT_PITCH, -1)
    assert prev == 0x7fffffff
    del want
    raster.OUTPUT_PITCH_ALIGN = 32
    raster.STRICT_BG = True
    try:
        short_bg = scene._replace(bg=torch.zeros(3))
        with pytest.raises(RuntimeError, match="bg has 3 entries"):
            _hip_forward(short_bg, cam, variant=15)   # raises inside the Python layer, before the call
        with torch.cuda.device(DEV):
            assert lib.sgs_stream_set_option(sp, _lib.OPT_OUT_PITCH, -1) == 0x7fffffff
    finally:
        raster.OUTPUT_PITCH_ALIGN = 0
        raster.STRICT_BG = False
    fw = oracle_forward(orc, scene, cam)
    out = _hip_forward(scene, cam, variant=15)[1]
    assert np.array_equal(out.cpu().numpy(), fw["out"])


def test_forward_result_needs_a_forward_on_that_device_and_stream():
    """sgs_forward_result on a (device, stream) that never saw a forward is an error, not "0 rendered"."""
    import ctypes as C
    from sgs_hip import _lib
    lib = _lib.load()
    st = torch.cuda.Stream(device=DEV)
    n = C.c_int(-1)
    with torch.cuda.device(DEV):
        rc = lib.sgs_forward_result(C.c_void_p(st.cuda_stream), 1, C.byref(n))
    assert rc == _lib.SGS_EINVAL and "no forward" in _lib.last_error()


def _sparse_scene():
    """Few small Gaussians: empty tiles (range (0, 0), as the reference leaves them) in the middle of the image next to
    tiles whose lists start at small offsets -- the case in which an empty tile's work-list table index
    (range.x >> 7) + tile coincided with an early tile's (round 3 fix: chunk 0 never goes through the table)."""
    scene, cam = small_scene(P=60, C=128, W=208, H=96, fx=170.0, seed=5)
    g = torch.Generator().manual_seed(3)
    return scene._replace(bg=torch.randn(128, generator=g), scales=scene.scales * 0.3), cam


@pytest.mark.parametrize("variant", [0, 15, 0x6A, 0x6B, 0x6E, 0x66, 14])
def test_empty_tiles_get_the_background(orc, variant):
    if variant in (0x6A, 0x6E):
        need_experiments("round 3's sweep (0x6A / 0x6E)")
    scene, cam = _sparse_scene()
    fw = oracle_forward(orc, scene, cam)
    r = fw["ranges"].reshape(-1, 2)
    empty = r[:, 0] == r[:, 1]
    ne = np.nonzero(~empty)[0]
    assert empty.any() and np.isin((r[ne, 0] >> 7) + ne, np.nonzero(empty)[0]).any()   # an empty tile's old table index coincides with a non-empty tile's
    out = _hip_forward(scene, cam, variant=variant)[1].cpu().numpy()
    # 0 = round 2's two-term split (3 * 2^-16 of |f| w per term, the bg term included); the six-product paths carry the
    # operands exactly; 15 / 0x6B are the fp32 chain itself
    tol = 0 if variant in (15, 0x6B) else (2e-4 if variant == 14 else 1e-5)
    assert np.abs(out - fw["out"]).max() <= tol
    if variant == 14:
        return
    # every pixel of an empty tile is exactly the background
    gx = (208 + 15) // 16
    for t in np.nonzero(empty)[0]:
        ty, tx = divmod(int(t), gx)
        blk = out[:, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        assert np.array_equal(blk, np.broadcast_to(scene.bg.numpy()[:, None, None], blk.shape)), (t, variant)


def test_empty_tiles_backward(orc):
    """The work-list backward reads the same chunk table: gradients of a scene with empty tiles and a non-zero
    background against the oracle (the bg . g term of every empty tile's pixels flows nowhere, the others' must)."""
    from sgs_hip import raster
    scene, cam = _sparse_scene()
    C, H, W = 128, 96, 208
    bg = scene.bg.numpy()
    g = torch.Generator().manual_seed(5)
    dL = torch.randn(C, H, W, generator=g)
    fw = oracle_forward(orc, scene, cam, bg=bg)
    gr = orc.backward(fw, dL.numpy(), scene.means3D.numpy(), cam.world_view_transform.numpy(),
                      cam.full_proj_transform.numpy(), cam.camera_center.numpy(), W, H, cam.tanfovx,
                      cam.tanfovy, bg, scales=scene.scales.numpy(), rotations=scene.rotations.numpy(),
                      cov3D_precomp=None, shs=None, sh_degree=3)
    names = ["dL_dmean2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"]
    for mode in (0, 1, 3):
        raster.set_backward_mode(mode)
        try:
            n, color, radii, geom, binn, img, _ = _hip_forward(scene, cam, bg=bg)
            outs = [t.cpu().numpy() for t in _hip_backward(scene, cam, bg, dL, n, radii, geom, binn, img)]
        finally:
            raster.set_backward_mode(0)
        for i, name in enumerate(names):
            if gr[name].size == 0:
                continue
            ok, err = _grad_close(outs[i].reshape(gr[name].shape), gr[name], 1e-4)
            assert ok, (name, mode, err)


def test_tile_order_feedback_does_not_change_results(orc):
    """Round 4: the weights pre-pass takes its tiles longest-first by the work they had in the stream's PREVIOUS frame
    (BlendFwdArgs::tile_order, written by sweep_plan_kernel).  A scheduling hint only: on a fresh stream the first frame runs
    in tile order, the second with the first frame's order, a third frame of a DIFFERENT scene with the same tile grid runs
    with a stale order -- every integer output and the feature map are identical to the renders without any order."""
    from sgs_hip import raster
    a, cam = small_scene(P=6000, C=128, W=208, H=160, fx=170.0, seed=41)
    b, _ = small_scene(P=2500, C=128, W=208, H=160, fx=170.0, seed=42)
    b = b._replace(scales=b.scales * 2.5)

    def frame(scene):
        n, color, radii, geom, binn, img, _ = _hip_forward(scene, cam, variant=0)
        iv = raster.image_views(img, 208, 160)
        return n, color.clone(), radii.clone(), iv["n_contrib"].clone(), iv["final_T"].clone()

    fresh = [torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    with torch.cuda.stream(fresh[0]):
        a0 = frame(a)        # no order yet
        a1 = frame(a)        # a's own order
        b_stale = frame(b)   # a's order, b's scene
        b_own = frame(b)     # b's order
    with torch.cuda.stream(fresh[1]):
        b0 = frame(b)        # no order
    torch.cuda.synchronize()
    for x, y in ((a0, a1), (b0, b_stale), (b0, b_own)):
        assert x[0] == y[0]
        for u, v in zip(x[1:], y[1:]):
            assert torch.equal(u, v)
    fw = oracle_forward(orc, a, cam)
    assert a0[0] == fw["num_rendered"] and np.array_equal(a1[3].cpu().numpy().view(np.uint32), fw["n_contrib"])
    for st in fresh[:2]:
        with torch.cuda.stream(st):
            raster.release_stream()
