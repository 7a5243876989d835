"""fp16 feature tables (SGS_OPT_FEATURE_FORMAT, include/sgs_raster.h) on the N-channel forward.

The contract: rendering an fp16 table is BIT-IDENTICAL to rendering the same table converted to fp32 (fp16 -> fp32 is exact, and the
sweep's exact three-term bf16 split of such a value has a zero third term), with an fp32 background that keeps its full value -- on every
path a forward can take: the ping-pong sweep (default x16 form and its x8 fallback), the remainder channels and C < 128 (px1), the gated
overflow fallback and variants 6 / 15 (px4), band-major output, padded pitch, deferred counts and their retry.  For C >= 128 with C % 8 != 0
the promise is narrower: px4, bit-identical to the fp32 table under variant 6."""
import contextlib
import os
import subprocess
import sys

import pytest
import torch

from helpers import small_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "half_tables_child.py")


@contextlib.contextmanager
def fresh_stream():
    """A side stream whose library context (capacity guesses, counters) starts empty and is released again: torch hands out its
    streams from a small pool, so a stream another test used may come back -- with that test's context."""
    from sgs_hip import raster
    st = torch.cuda.Stream(DEV)
    with torch.cuda.stream(st):
        raster.release_stream()
    st.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.stream(st):
            yield st
    finally:
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            raster.release_stream()


def half_table(P, C, seed):
    """Random normals with fp16 subnormals, +-65504 and -0.0 sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(P, C, generator=g).half()
    flat = f.view(-1)
    n = flat.numel()
    idx = torch.randperm(n, generator=g)
    k = max(1, n // 64)
    sub = torch.randint(1, 1024, (k,), generator=g, dtype=torch.int16).view(torch.float16)   # bit patterns 0x0001 .. 0x03ff
    flat[idx[:k]] = sub * torch.where(torch.rand(k, generator=g) < 0.5, -1.0, 1.0).half()
    flat[idx[k:k + max(1, k // 4)]] = 65504.0
    flat[idx[k + max(1, k // 4):k + 2 * max(1, k // 4)]] = -65504.0
    flat[idx[k + 2 * max(1, k // 4):k + 3 * max(1, k // 4)]] = -0.0
    assert bool((flat.float().abs() < 6.2e-5).logical_and(flat.float() != 0).any()), "no subnormal in the table"
    return f


def fp32_background(C, seed):
    g = torch.Generator().manual_seed(seed + 1)
    bg = torch.randn(C, generator=g) * 0.3 + 0.1234567
    assert not torch.equal(bg.half().float(), bg), "the background must not be fp16-representable"
    return bg


def scene_for(C, W, H, seed=3, P=3000):
    fx = 0.9 * max(W, H)
    scene, cam = small_scene(P=P, C=1, W=W, H=H, fx=fx, seed=seed)
    F16 = half_table(P, C, seed)
    bg = fp32_background(C, seed)
    return scene.to(DEV), cam.to(DEV), F16.to(DEV), bg.to(DEV)


def render(s, c, feats, bg, W, H, mode="classic"):
    """-> (map, radii, final_T, n_contrib), cloned."""
    from sgs_hip import raster
    e = torch.Tensor([])
    args = (bg, s.means3D, feats, s.opacities, s.scales, s.rotations, 1.0, e, c.world_view_transform, c.full_proj_transform,
            c.tanfovx, c.tanfovy, H, W, e, 0, c.camera_center, False, False, feats.shape[1])
    if mode == "deferred":
        out = raster.rasterize_forward_deferred(*args, want_depth=False).result()
    elif mode == "retry":
        d = raster.rasterize_forward_deferred(*args, want_depth=False, _defer_mode=2)
        out = d.result()
    else:
        out = raster.rasterize_forward(*args, want_depth=False)
    iv = raster.image_views(out[5], W, H)
    return out[1].clone(), out[2].clone(), iv["final_T"].clone(), iv["n_contrib"].clone()


def assert_same(a, b, what):
    for x, y, name in zip(a, b, ("map", "radii", "final_T", "n_contrib")):
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name)
        assert torch.equal(x, y), (what, name, float((x.double() - y.double()).abs().max()) if x.is_floating_point() else None)


SHAPES = [(208, 96), (203, 77), (13, 11)]   # W % 32 == 16; W not a multiple of 16; a single tile


@contextlib.contextmanager
def stream_variant(v):
    """Blend variant v on the current stream only (None: leave it)."""
    from sgs_hip import raster, _lib
    if v is not None:
        raster.set_stream_option(_lib.OPT_BLEND_VARIANT, v)
    try:
        yield
    finally:
        if v is not None:
            raster.set_stream_option(_lib.OPT_BLEND_VARIANT, -1)


# C >= 128 with C % 8 != 0 (129 odd, 132 and 300 even): fp16 rows that are not 16-byte aligned, which the sweep's 16-byte LDS-DMA pieces
# cannot take -- the narrower promise for them: the px4 form, bit-identical to the fp32 table under variant 6
@pytest.mark.parametrize("C", [1, 21, 64, 127, 128, 129, 132, 200, 256, 300, 512, 640])
@pytest.mark.parametrize("W,H", SHAPES)
def test_fp16_table_renders_bit_identically_to_its_upcast(C, W, H, monkeypatch):
    from sgs_hip import raster
    s, c, F16, bg = scene_for(C, W, H, seed=C + W)
    F32 = F16.float()
    ref_variant = 6 if (C >= 128 and C % 8) else None
    with fresh_stream():
        for mode in ("classic", "deferred", "retry"):
            a = render(s, c, F16, bg, W, H, mode)
            with stream_variant(ref_variant):
                b = render(s, c, F32, bg, W, H, mode)
            assert_same(a, b, mode)
        if W % 32:
            monkeypatch.setattr(raster, "OUTPUT_PITCH_ALIGN", 32)
            a = render(s, c, F16, bg, W, H)
            with stream_variant(ref_variant):
                b = render(s, c, F32, bg, W, H)
            assert_same(a, b, "padded pitch")
            monkeypatch.setattr(raster, "OUTPUT_PITCH_ALIGN", 0)
        if C % 128 == 0:
            for w in (2, 3, 8):
                A16, T16, r16 = raster.render_partial(s.means3D, F16, s.opacities, s.scales, s.rotations, c.world_view_transform,
                                                      c.full_proj_transform, c.tanfovx, c.tanfovy, H, W, c.camera_center, bands=w)
                A32, T32, r32 = raster.render_partial(s.means3D, F32, s.opacities, s.scales, s.rotations, c.world_view_transform,
                                                      c.full_proj_transform, c.tanfovx, c.tanfovy, H, W, c.camera_center, bands=w)
                assert len(A16) == len(A32) == w
                assert all(torch.equal(x, y) for x, y in zip(A16, A32)), ("bands", w)
                assert torch.equal(T16, T32) and torch.equal(r16, r32)
    torch.cuda.synchronize()


@pytest.mark.parametrize("variant", [15, 6])
def test_fp16_under_variants_15_and_6_matches_their_own_fp32_render(variant):
    from sgs_hip import raster
    for C in (128, 200, 512):
        s, c, F16, bg = scene_for(C, 208, 96, seed=variant + C)
        prev = raster.set_blend_variant(variant)
        try:
            a = render(s, c, F16, bg, 208, 96)
            b = render(s, c, F16.float(), bg, 208, 96)
        finally:
            raster.set_blend_variant(prev)
        assert_same(a, b, (variant, C))


def test_fp16_under_variant_14_is_refused():
    from sgs_hip import raster
    s, c, F16, bg = scene_for(128, 64, 48)
    prev = raster.set_blend_variant(14)
    try:
        with pytest.raises(RuntimeError, match="fp16"):
            render(s, c, F16, bg, 64, 48)
        render(s, c, F16.float(), bg, 64, 48)   # (fp32 under 14 still renders)
    finally:
        raster.set_blend_variant(prev)
    a = render(s, c, F16, bg, 64, 48)   # the refused call consumed its option: the stream is clean
    assert_same(a, render(s, c, F16.float(), bg, 64, 48), "after a refusal")


def test_fp16_on_the_x8_sweep_in_a_fresh_process():
    """SGS_DEFAULT_SWEEP=6 (read once per process) selects the x8 lock-step sweep: its fp16 form against its fp32 render."""
    env = dict(os.environ, SGS_DEFAULT_SWEEP="6")
    r = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"child exited with {r.returncode}\n--- stderr ---\n{r.stderr[-6000:]}\n--- stdout ---\n{r.stdout[-2000:]}"
    assert "half tables x8: ok" in r.stdout


def test_fp16_through_the_overflow_fallback():
    """A fresh stream's first frame of a dense scene outgrows the work list: the gated px4 fallback renders it (tests/test_semantic.py)."""
    from sgs_hip import raster, _lib
    C, W, H = 128, 784, 32
    scene, cam = small_scene(P=120000, C=1, W=W, H=H, fx=600.0, seed=77)
    scene = scene._replace(scales=scene.scales * 3.0, opacities=scene.opacities * 0.02)
    s, c = scene.to(DEV), cam.to(DEV)
    F16 = half_table(120000, C, 77).to(DEV)
    bg = fp32_background(C, 77).to(DEV)
    maps = {}
    for name, feats in (("f16", F16), ("f32", F16.float())):
        with fresh_stream():   # (its first frame must start from the initial work-list capacity)
            first = render(s, c, feats, bg, W, H)
            second = render(s, c, feats, bg, W, H)
            overflows = raster.stream_stat(_lib.STAT_FWD_OVERFLOWS)
        torch.cuda.synchronize()
        assert overflows >= 1, name
        maps[name] = (first, second)
    assert_same(maps["f16"][0], maps["f32"][0], "first frame (fallback)")
    assert_same(maps["f16"][1], maps["f32"][1], "second frame (sweep)")


def _settings(c, bg, W, H, C):
    import channel_rasterization as cr
    return cr.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=bg, scale_modifier=1.0,
                                            viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0,
                                            campos=c.camera_center, prefiltered=False, debug=False, num_channels=C)


def test_fp16_norm_plane_and_normalised_similarity():
    from sgs_hip import semantic
    C, W, H = 256, 208, 96
    s, c, F16, bg = scene_for(C, W, H, seed=11)
    F16 = F16.clamp(-4, 4)   # (the norm of a +-65504 entry squared overflows fp32)
    F32 = F16.float()
    st = _settings(c, bg, W, H, C)
    n16 = semantic.render_norm2(st, s.means3D, s.opacities, s.scales, s.rotations, F16)
    n32 = semantic.render_norm2(st, s.means3D, s.opacities, s.scales, s.rotations, F32)
    assert float(((n16.double() - n32.double()).abs() / (n32.double().abs() + 1e-30)).max()) <= 1e-6
    text = torch.randn(20, C, device=DEV)
    proj16 = semantic.project_features(F16, text)
    assert proj16.dtype == torch.float32 and proj16.shape == (F16.shape[0], 20)
    assert torch.allclose(proj16, F32 @ text.t(), rtol=1e-5, atol=1e-4)
    sim16 = semantic.render_similarity(st, s.means3D, s.opacities, s.scales, s.rotations, F16, text, normalised=True, projected=proj16)
    sim32 = semantic.render_similarity(st, s.means3D, s.opacities, s.scales, s.rotations, F32, text, normalised=True, projected=proj16)
    assert float(((sim16.double() - sim32.double()).abs() / (sim32.double().abs() + 1e-6)).max()) <= 1e-6
    torch.cuda.synchronize()


def test_an_fp16_inference_forward_makes_no_fp32_copy_of_the_table():
    import channel_rasterization as cr
    from sgs_hip.camera import pinhole
    from sgs_hip.synthetic import make_scene
    P, C, W, H = 2_000_000, 128, 256, 256
    scene = make_scene(P, 1, W, H, 220.0, seed=5).to(DEV)
    cam = pinhole(W, H, 220.0).to(DEV)
    F16 = torch.randn(P, C, device=DEV, dtype=torch.float16)
    bg = torch.rand(C, device=DEV)
    rast = cr.GaussianRasterizer(_settings(cam, bg, W, H, C))

    def go():
        with torch.no_grad():
            return rast(means3D=scene.means3D, means2D=torch.zeros_like(scene.means3D), opacities=scene.opacities,
                        colors_precomp=F16, scales=scene.scales, rotations=scene.rotations)[0]
    go()
    go()   # (warm-up: the inference pool and the stream's capacity guesses settle)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    out = go()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    assert out.shape == (C, H, W)
    assert peak < P * C * 4, f"peak {peak / 2**20:.0f} MiB above the pre-call level: an fp32 copy of the table is {P * C * 4 / 2**20:.0f} MiB"


def test_fp16_leaf_under_autograd():
    import channel_rasterization as cr
    C, W, H = 128, 16, 16   # one tile: the backward's gradient sums have one order
    s, c, F16, bg = scene_for(C, W, H, seed=21, P=400)
    F16 = F16.clamp(-8, 8)
    G = torch.randn(C, H, W, device=DEV)
    rast = cr.GaussianRasterizer(_settings(c, bg, W, H, C))
    res = {}
    for name, table in (("f16", F16), ("f32", F16.float())):
        leaf = table.clone().requires_grad_(True)
        m = s.means3D.clone().requires_grad_(True)
        o = s.opacities.clone().requires_grad_(True)
        sc = s.scales.clone().requires_grad_(True)
        ro = s.rotations.clone().requires_grad_(True)
        color, _ = rast(means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=o, colors_precomp=leaf, scales=sc,
                        rotations=ro)
        (color * G).sum().backward()
        res[name] = (color.detach(), leaf.grad, m.grad, o.grad, sc.grad, ro.grad)
    f16, f32 = res["f16"], res["f32"]
    assert torch.equal(f16[0], f32[0])
    assert f16[1].dtype == torch.float16 and torch.equal(f16[1], f32[1].half())
    for k, name in zip(range(2, 6), ("means3D", "opacities", "scales", "rotations")):
        assert torch.equal(f16[k], f32[k]), name


def test_the_feature_format_is_a_per_stream_option():
    """At the C-ABI: the format armed on stream A is neither seen nor consumed by a forward on stream B (rasterize_forward arms and
    consumes it inside one call, so this is set by hand)."""
    from sgs_hip import raster, _lib
    C, W, H = 256, 208, 96
    s, c, F16, bg = scene_for(C, W, H, seed=51)
    F32 = F16.float()
    with fresh_stream():
        want = render(s, c, F32, bg, W, H)
    with fresh_stream() as A, fresh_stream() as B:
        with torch.cuda.stream(A):
            assert raster.set_stream_option(_lib.OPT_FEATURE_FORMAT, 1) == 0x7fffffff
        with torch.cuda.stream(B):
            got = render(s, c, F32, bg, W, H)   # an fp32 table on B: read as fp32
            got16 = render(s, c, F16, bg, W, H)
        with torch.cuda.stream(A):
            assert raster.set_stream_option(_lib.OPT_FEATURE_FORMAT, -1) == 1, "B's forwards consumed A's option"
    assert_same(got, want, "fp32 on stream B")
    assert_same(got16, want, "fp16 on stream B")


def test_fp32_and_fp16_forwards_interleaved_on_two_streams():
    C, W, H = 256, 208, 96
    s, c, F16, bg = scene_for(C, W, H, seed=31)
    F32b = (torch.randn_like(F16.float()) * 0.5)
    want16 = render(s, c, F16, bg, W, H)
    want32 = render(s, c, F32b, bg, W, H)
    got = []
    with fresh_stream() as s1, fresh_stream() as s2:
        for _ in range(4):
            with torch.cuda.stream(s1):
                got.append(("f32", render(s, c, F32b, bg, W, H)))
            with torch.cuda.stream(s2):
                got.append(("f16", render(s, c, F16, bg, W, H)))
    torch.cuda.synchronize()
    for name, r in got:
        assert_same(r, want16 if name == "f16" else want32, name)


def test_cfg3_frame_in_fp16():
    from sgs_hip.synthetic import make_config
    scene, cam = make_config("cfg3")
    W, H = cam.image_width, cam.image_height
    F16 = scene.features.half().to(DEV)
    s, c = scene._replace(features=scene.features[:, :1].contiguous()).to(DEV), cam.to(DEV)
    a = render(s, c, F16, s.bg, W, H)
    b = render(s, c, F16.float(), s.bg, W, H)
    assert_same(a, b, "cfg3")


def test_other_dtypes_and_unsupported_combinations_are_refused():
    import rgbd_rasterization as rr
    from sgs_hip import raster
    C, W, H = 128, 64, 48
    s, c, F16, bg = scene_for(C, W, H, seed=41)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(RuntimeError, match=f"expected scalar type torch.float32 for colors_precomp but found {dt}"):
            render(s, c, F16.to(dt), bg, W, H)
    e = torch.Tensor([])
    with pytest.raises(RuntimeError):   # the RGB-D variant: fp32 colours only
        raster.rasterize_forward(bg[:3].contiguous(), s.means3D, F16[:, :3].contiguous(), s.opacities, s.scales, s.rotations, 1.0, e,
                                 c.world_view_transform, c.full_proj_transform, c.tanfovx, c.tanfovy, H, W, e, 0, c.camera_center,
                                 False, False, 3, want_depth=True)
    st = rr.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=bg[:3].contiguous(),
                                          scale_modifier=1.0, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform,
                                          sh_degree=0, campos=c.camera_center, prefiltered=False, debug=False)
    with pytest.raises(RuntimeError):
        rr.GaussianRasterizer(st)(means3D=s.means3D, means2D=torch.zeros_like(s.means3D), opacities=s.opacities,
                                  colors_precomp=F16[:, :3].contiguous(), scales=s.scales, rotations=s.rotations)
    with pytest.raises(RuntimeError):   # SH input: fp32 only
        raster.rasterize_forward(bg[:3].contiguous(), s.means3D, e, s.opacities, s.scales, s.rotations, 1.0, e, c.world_view_transform,
                                 c.full_proj_transform, c.tanfovx, c.tanfovy, H, W, F16[:, :3].reshape(-1, 1, 3).contiguous(), 0,
                                 c.camera_center, False, False, 3, want_depth=False)
    a = render(s, c, F16, bg, W, H)   # nothing stale on the stream
    assert_same(a, render(s, c, F16.float(), bg, W, H), "after refusals")
