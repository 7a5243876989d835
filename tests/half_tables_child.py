"""Child process of tests/test_half_tables_gpu.py (not a test module): run with SGS_DEFAULT_SWEEP=6, which csrc/capi.hip reads once per
process, so that the default blend is the x8 lock-step sweep -- the form the default falls back to when its x16 form does not own its
compute unit.  The fp16 table must render bit-identically to its fp32 upcast there too.  Exit status 0 when every check holds."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "semantic-gaussians_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    from test_half_tables_gpu import assert_same, render, scene_for
    assert os.environ.get("SGS_DEFAULT_SWEEP") == "6"
    for C, W, H in ((128, 208, 96), (256, 203, 77), (640, 13, 11), (200, 208, 96)):
        s, c, F16, bg = scene_for(C, W, H, seed=C)
        for mode in ("classic", "deferred"):
            assert_same(render(s, c, F16, bg, W, H, mode), render(s, c, F16.float(), bg, W, H, mode), (C, W, H, mode))
    torch.cuda.synchronize()
    print("half tables x8: ok")


if __name__ == "__main__":
    main()
