"""The optimiser alone: one Adam step over
  six     the reference's six parameter groups at 500k Gaussians, SH degree 3: (P,3) (P,1,3) (P,15,3) (P,1) (P,3) (P,4), 59 floats a row
  table   one 1M x 512 feature table (2 GB; the distillation-style step of tools/bench_train_step.py)
with  torch.optim.Adam as the reference builds it (foreach),  torch.optim.Adam(fused=True),  sgs_hip.optim.GaussianAdam dense  and
GaussianAdam under a visibility mask of fraction 1.0, 0.3 and 0.05 -- the last two once with a random mask and once with a mask of
contiguous index ranges (RANGE rows each).

Each figure is the median of 5 timings of N steps after 3 warm-up steps; a timing is a host clock around N steps that end in a device
synchronise, and the variants alternate inside each of the 5 rounds.  GB/s counts 28 B per element of the WHOLE tensors (read param,
grad and both moments; write param and both moments), whatever the mask skips: for a masked step it is the dense-equivalent rate.
One JSON line per (case, variant) on stdout and, with --out, in that file.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-gaussians_amd"))
import torch  # noqa: E402

from sgs_hip.optim import GaussianAdam  # noqa: E402

RANGE = 4096


def make_mask(P, fraction, kind, gen, dev):
    if fraction >= 1.0:
        return torch.ones(P, dtype=torch.bool, device=dev)
    if kind == "random":
        return (torch.rand(P, generator=gen) < fraction).to(dev)
    m = torch.zeros(P, dtype=torch.bool)
    slots = P // RANGE
    for k in torch.randperm(slots, generator=gen)[:max(1, round(fraction * slots))].tolist():
        m[k * RANGE:(k + 1) * RANGE] = True
    return m.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="six,table")
    ap.add_argument("--gaussians", type=int, default=500_000)
    ap.add_argument("--table-rows", type=int, default=1_000_000)
    ap.add_argument("--table-width", type=int, default=512)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_adam needs a GPU"
    dev = "cuda:0"
    gen = torch.Generator().manual_seed(0)
    out = open(args.out, "a") if args.out else None
    for case in args.cases.split(","):
        if case == "six":
            P = args.gaussians
            shapes, N = [(P, 3), (P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4)], 100
        else:
            P = args.table_rows
            shapes, N = [(P, args.table_width)], 10
        elements = sum(torch.Size(s).numel() for s in shapes)
        grads = [torch.randn(s, device=dev) * 1e-3 for s in shapes]
        init = [torch.randn(s, device=dev) for s in shapes]
        variants = [("torch.optim.Adam", "torch", None, None), ("torch.optim.Adam(fused=True)", "fused", None, None),
                    ("GaussianAdam dense", "ours", None, None), ("GaussianAdam masked 1.0", "ours", 1.0, "all"),
                    ("GaussianAdam masked 0.3 random", "ours", 0.3, "random"), ("GaussianAdam masked 0.3 ranges", "ours", 0.3, "ranges"),
                    ("GaussianAdam masked 0.05 random", "ours", 0.05, "random"), ("GaussianAdam masked 0.05 ranges", "ours", 0.05, "ranges")]
        runs = []
        for label, kind, fraction, mask_kind in variants:
            params = [torch.nn.Parameter(p.clone()) for p in init]
            for p, g in zip(params, grads):
                p.grad = g          # (read only: every variant shares the gradients)
            groups = [{"params": [p]} for p in params]
            if kind == "ours":
                opt = GaussianAdam(groups, lr=1e-4, eps=1e-15)
            else:
                opt = torch.optim.Adam(groups, lr=1e-4, eps=1e-15, fused=(kind == "fused") or None)
            mask = make_mask(P, fraction, mask_kind, gen, dev) if fraction is not None else None
            step = (lambda o=opt, m=mask: o.step(visibility=m)) if kind == "ours" else opt.step
            for _ in range(3):
                step()
            runs.append(dict(label=label, step=step, mask=mask, opt=opt, ts=[]))
        torch.cuda.synchronize()
        for _ in range(5):
            for r in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(N):
                    r["step"]()
                torch.cuda.synchronize()
                r["ts"].append((time.perf_counter() - t0) / N)
        for r in runs:
            t = statistics.median(r["ts"])
            rec = dict(case=case, shapes=[list(s) for s in shapes], elements=elements, variant=r["label"],
                       visible_fraction=None if r["mask"] is None else round(float(r["mask"].float().mean()), 4),
                       launches=getattr(r["opt"], "last_launches", None), steps_per_timing=N,
                       ms=round(t * 1e3, 4), ms_min=round(min(r["ts"]) * 1e3, 4), ms_max=round(max(r["ts"]) * 1e3, 4),
                       gbps_28B_per_element=round(28.0 * elements / t / 1e9, 1))
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        del runs, grads, init
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
