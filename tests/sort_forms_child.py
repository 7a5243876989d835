"""Child process of tests/test_sort_forms_gpu.py (not a test module): one form of the depth sort, selected by the parent through
SGS_DS_CHAIN / SGS_DS_WAVES -- csrc/depth_sort.hip reads them once per process -- checked on bare keys against torch's stable sort and
inside the forward against the oracle.  Exit status 0 when every check holds; an assertion's traceback goes to stderr."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "semantic-gaussians_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctypes as C  # noqa: E402

import torch  # noqa: E402

DEV = "cuda:0"


def sort_checks(lib):
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for P in (1_000_003, 5_000_000, 8_388_609):
        for kind in ("random", "depth"):
            g = torch.Generator(device=DEV).manual_seed(P)
            if kind == "random":
                keys = torch.randint(0, 2 ** 32, (P,), device=DEV, generator=g, dtype=torch.int64)
            else:   # depth-like float bits, 10 % culled
                keys = (0.2 + 60.0 * torch.rand(P, device=DEV, generator=g)).view(torch.int32).to(torch.int64)
                keys[torch.rand(P, device=DEV, generator=g) < 0.1] = 0xFFFFFFFF
            want = torch.sort(keys, stable=True).indices.to(torch.int32)
            k32 = torch.where(keys >= 2 ** 31, keys - 2 ** 32, keys).to(torch.int32)   # same bits as uint32
            scratch = torch.empty(lib.sgs_debug_depth_sort(P, None, None, None, None), dtype=torch.uint8, device=DEV)
            perm = torch.full((P,), -1, dtype=torch.int32, device=DEV)
            for _ in range(2):   # (twice: the count matrices must be cleared every time)
                assert lib.sgs_debug_depth_sort(P, k32.data_ptr(), perm.data_ptr(), scratch.data_ptr(), st) == 0
                torch.cuda.synchronize()
                assert torch.equal(perm, want), (P, kind)


def forward_checks():
    """A forward whose sort has 74 workgroups: integers against the oracle; then a deferred forward on the same stream (count record
    written by the last workgroup of this form's last pass) must return the same count and image."""
    import numpy as np
    from oracle import oracle as orc
    from sgs_hip import raster, _lib
    from helpers import small_scene
    from test_configs_gpu import _check_integers, _forward, _oracle_front
    P, C, W, H = 300_000, 32, 256, 192
    assert (P + 4095) // 4096 >= 70
    scene, cam = small_scene(P=P, C=C, W=W, H=H, fx=150.0, seed=17)
    orc.lib()
    pre, binn = _oracle_front(orc, scene, cam, W, H)
    s, c = scene.to(DEV), cam.to(DEV)
    st = torch.cuda.Stream(DEV)
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        out = _forward(s, c, s.features, s.bg, W, H)   # blocking: also the stream's capacity guess
        _check_integers(raster, out, pre, binn, P, W, H)
        n, color = out[0], out[1].clone()
        assert n > 0
        del out
        deferred = raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS)
        h = _forward(s, c, s.features, s.bg, W, H, fn=raster.rasterize_forward_deferred)
        o = h.result()
        assert raster.stream_stat(_lib.STAT_DEFERRED_FORWARDS) == deferred + 1
        assert not h.retried and o[0] == n and torch.equal(o[1], color)
        assert np.array_equal(o[2].cpu().numpy(), pre["radii"])
        del o, h
        raster.release_stream()


def main():
    from sgs_hip import _lib
    assert os.environ.get("SGS_DS_CHAIN") is not None and os.environ.get("SGS_DS_WAVES") is not None
    lib = _lib.load()
    sort_checks(lib)
    forward_checks()
    print(f"sort form SGS_DS_CHAIN={os.environ['SGS_DS_CHAIN']} SGS_DS_WAVES={os.environ['SGS_DS_WAVES']}: ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
