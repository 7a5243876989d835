"""fp32 feature table against the same table in fp16 (SGS_OPT_FEATURE_FORMAT): ms per view with one view and with four views in flight on
four HIP streams (deferred counts, as bench.py's headline), the device memory the table holds, the fp16 norm-plane frame, and -- under
`rocprofv3 --kernel-trace --stats -- python tools/bench_half_tables.py ...` -- the accumulate sweep's own time per format (the fp32 and fp16
forms are different instantiations of blend_accum_sweep3_kernel: the trailing template argument is the format).

The two formats are measured order-balanced (A B B A ... over --rounds rounds, the same box), each round --steps frames after --warmup.

usage: python tools/bench_half_tables.py [--configs cfg3,cfg4] [--channels C] [--rounds 4] [--steps 40] [--warmup 5] [--no-norm]
cfg4 is measured with raster.OUTPUT_PITCH_ALIGN = 32 (its width 1297 is not a multiple of 32).  --channels replaces the configuration's C (e.g.
516: fp16 rows that are not 16-byte aligned, which render on the px4 form -- include/sgs_raster.h SGS_OPT_FEATURE_FORMAT)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-gaussians_amd"))
import torch  # noqa: E402

from sgs_hip import dist, raster, semantic  # noqa: E402
from sgs_hip.synthetic import CONFIGS, make_config  # noqa: E402

DEV = "cuda:0"
E = torch.Tensor([])


def frame_fn(s, c, feats, bg, W, H, C, pools, deferred):
    def render(view, slot):
        args = (bg, s.means3D, feats, s.opacities, s.scales, s.rotations, 1.0, E, c.world_view_transform, c.full_proj_transform,
                c.tanfovx, c.tanfovy, H, W, E, 0, c.camera_center, False, False, C)
        if deferred:
            return raster.rasterize_forward_deferred(*args, want_depth=False, pool=pools[slot])
        return raster.rasterize_forward(*args, want_depth=False, pool=pools[slot])
    return render


def time_views(render, n_views, in_flight, steps, warmup):
    views = list(range(n_views))
    for _ in range(warmup):
        dist.render_views_pipelined(render, views, in_flight=in_flight)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        dist.render_views_pipelined(render, views, in_flight=in_flight)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / (steps * n_views)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg3,cfg4")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--channels", type=int, default=0)
    ap.add_argument("--no-norm", action="store_true")
    a = ap.parse_args()
    results = []
    for cfg in a.configs.split(","):
        P, C, W, H, _ = CONFIGS[cfg]
        C = a.channels or C
        raster.OUTPUT_PITCH_ALIGN = 32 if cfg == "cfg4" else 0
        scene, cam = make_config(cfg, features=False)
        s, c = scene._replace(features=torch.empty(0, C)).to(DEV), cam.to(DEV)
        g = torch.Generator(device=DEV).manual_seed(3)
        f32 = torch.randn(P, C, device=DEV, generator=g)
        f32 /= f32.norm(dim=1, keepdim=True)
        tables = {"fp32": f32, "fp16": f32.half()}
        bg = torch.rand(C, device=DEV, generator=g)
        pools = [raster.ScratchPool() for _ in range(4)]
        rec = {"config": cfg, "P": P, "C": C, "W": W, "H": H, "pitch_align": raster.OUTPUT_PITCH_ALIGN,
               "table_bytes": {k: v.numel() * v.element_size() for k, v in tables.items()}}
        # one view (blocking count read-back, the reference's order) and four views in flight (deferred counts)
        for name, n_views, in_flight, deferred in (("one_view_ms", 1, 1, False), ("four_in_flight_ms_per_view", 8, 4, True)):
            per = {"fp32": [], "fp16": []}
            for r in range(a.rounds):
                order = ("fp32", "fp16") if r % 2 == 0 else ("fp16", "fp32")
                for fmt in order:
                    fn = frame_fn(s, c, tables[fmt], bg, W, H, C, pools, deferred)
                    per[fmt].append(time_views(fn, n_views, in_flight, a.steps, a.warmup))
            rec[name] = {k: sorted(v) for k, v in per.items()}
            rec[name + "_median"] = {k: v[len(v) // 2] for k, v in rec[name].items()}
        if not a.no_norm and C % 128 == 0:
            import channel_rasterization as cr
            st = cr.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=bg,
                                                  scale_modifier=1.0, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform,
                                                  sh_degree=0, campos=c.camera_center, prefiltered=False, debug=False, num_channels=C)
            per = {"fp32": [], "fp16": []}
            for r in range(a.rounds):
                for fmt in (("fp32", "fp16") if r % 2 == 0 else ("fp16", "fp32")):
                    for _ in range(a.warmup):
                        semantic.render_norm2(st, s.means3D, s.opacities, s.scales, s.rotations, tables[fmt])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.steps):
                        semantic.render_norm2(st, s.means3D, s.opacities, s.scales, s.rotations, tables[fmt])
                    torch.cuda.synchronize()
                    per[fmt].append((time.perf_counter() - t0) * 1e3 / a.steps)
            rec["norm_plane_ms"] = {k: sorted(v) for k, v in per.items()}
            rec["norm_plane_ms_median"] = {k: v[len(v) // 2] for k, v in rec["norm_plane_ms"].items()}
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del tables, f32, s, pools
        torch.cuda.empty_cache()
    return results


if __name__ == "__main__":
    main()
