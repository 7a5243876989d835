"""GPU tests of the fused Adam and the densification statistics (csrc/optim.hip, sgs_hip/optim.py).  The update is compared TO THE BIT
with tests/ref_adam.py, the arithmetic contract in float32 torch CPU ops (pinned to torch.optim.Adam by tests/test_optim.py): every
operation of the chain is one correctly rounded float32 operation on either side, so there is no tolerance to choose.

Gradients: randn * 10**U(-8, -2) per row, every 7th row exactly zero.  The host chain records its smallest nonzero intermediate and the
tests assert it is a normal float32 (>= 2^-126), so a flush-to-zero policy on either side cannot matter."""
import math

import pytest
import torch

import ref_adam
from sgs_hip.optim import GaussianAdam, accumulate_densification_stats

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = 2.0 ** -126
EPS = 1e-15          # the reference's torch.optim.Adam(l, lr=0.0, eps=1e-15)


def _bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _grad(shape, gen):
    rows = shape[0]
    scale = 10.0 ** torch.empty(rows, dtype=torch.float64).uniform_(-8, -2, generator=gen)
    g = torch.randn(shape, generator=gen) * scale.to(torch.float32).reshape([-1] + [1] * (len(shape) - 1))
    g[::7] = 0.0
    return g


class Host:
    """the host chain of one parameter: p, m, v and the step count"""

    def __init__(self, p, m=None, v=None, t=0):
        self.p = p.clone()
        self.m = torch.zeros_like(p) if m is None else m.clone()
        self.v = torch.zeros_like(p) if v is None else v.clone()
        self.t = t
        self.track = []

    def step(self, g, lr, mask=None):
        self.t += 1
        self.p, self.m, self.v = ref_adam.adam_step(self.p, g, self.m, self.v, self.t, lr, eps=EPS, mask=mask, track=self.track)

    def check(self, param, state, what=""):
        assert self.track and min(self.track) >= TINY, (what, min(self.track))
        assert float(state["step"]) == self.t and state["step"].device.type == "cpu" and state["step"].dtype == torch.float32, what
        for name, want, got in (("p", self.p, param), ("exp_avg", self.m, state["exp_avg"]), ("exp_avg_sq", self.v, state["exp_avg_sq"])):
            assert _bits_equal(want, got), f"{what}: {name} differs in {int((want != got.detach().cpu()).sum())} of {want.numel()} entries"


GUARD_ROWS = 4       # guard rows either side: a multiple of 16 bytes for every width, so a guarded tensor keeps its alignment


def _guard_pattern(n):
    return torch.full((n,), 0x7FC0BEEF, dtype=torch.int32).view(torch.float32)   # a quiet NaN with a payload


def _guarded(t):
    """t on the device as the middle of a larger allocation whose first and last GUARD_ROWS rows hold the NaN pattern"""
    w = t[0].numel()
    buf = _guard_pattern((t.shape[0] + 2 * GUARD_ROWS) * w).reshape((t.shape[0] + 2 * GUARD_ROWS,) + tuple(t.shape[1:])).to(DEV)
    buf[GUARD_ROWS:-GUARD_ROWS] = t.to(DEV)
    return buf, buf[GUARD_ROWS:-GUARD_ROWS]


def _guards_intact(buf):
    want = _guard_pattern(1).view(torch.int32).item()
    b = buf.detach().cpu().view(torch.int32)
    return bool((b[:GUARD_ROWS] == want).all()) and bool((b[-GUARD_ROWS:] == want).all())


def _run(shapes, base_lrs, steps, seed, mask_fn=None, guard=False, one_group=False, mask_dtype=torch.bool):
    """GaussianAdam over parameters of `shapes` (one group each unless one_group) against the host chain: `steps` steps, the lr of
    group k at step t is base_lrs[k] * 0.9**t, mask_fn(t) -> bool CPU mask or None.  Returns (optimiser, parameters, hosts)."""
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=gen) for s in shapes]
    hosts = [Host(p) for p in init]
    bufs = []
    params = []
    for p in init:
        if guard:
            buf, view = _guarded(p)
            bufs.append(buf)
            params.append(torch.nn.Parameter(view))
        else:
            params.append(torch.nn.Parameter(p.to(DEV)))
    if one_group:
        opt = GaussianAdam(params, lr=base_lrs[0], eps=EPS)
    else:
        opt = GaussianAdam([{"params": [p], "lr": lr} for p, lr in zip(params, base_lrs)], lr=0.0, eps=EPS)
    if guard:   # the moments too: put there before the first step, as a caller's state surgery would
        for p in params:
            st = {"step": torch.tensor(0.0)}
            for key in ("exp_avg", "exp_avg_sq"):
                buf, view = _guarded(torch.zeros(p.shape))
                bufs.append(buf)
                st[key] = view
            opt.state[p] = st
    for t in range(1, steps + 1):
        lrs = [lr * 0.9 ** t for lr in base_lrs]
        for k, group in enumerate(opt.param_groups):
            group["lr"] = lrs[k]
        mask = mask_fn(t) if mask_fn else None
        for k, (p, h) in enumerate(zip(params, hosts)):
            g = _grad(tuple(p.shape), gen) if p.shape[0] else torch.zeros(p.shape)
            p.grad = g.to(DEV)
            if p.numel():
                h.step(g, lrs[0 if one_group else k], mask)
            else:
                h.t += 1
        opt.step(visibility=mask.to(DEV, mask_dtype) if mask is not None else None)
    for k, (p, h) in enumerate(zip(params, hosts)):
        if p.numel():
            h.check(p, opt.state[p], f"tensor {k} {tuple(p.shape)}")
    assert all(_guards_intact(b) for b in bufs), "a guard row was written"
    return opt, params, hosts


def _shape(P, tail):
    return (P,) + tail


@pytest.mark.parametrize("tail", [(1,), (3,), (4,), (1, 3), (15, 3), (512,)], ids=lambda t: "x".join(map(str, t)))
@pytest.mark.parametrize("rows", [1, 5, 1003])
def test_dense_step_is_the_host_chain_to_the_bit(rows, tail):
    P = min(rows, 129) if tail == (512,) else rows
    opt, _, _ = _run([_shape(P, tail)], [1e-2], steps=12, seed=rows * 100 + len(tail) + tail[-1])
    assert opt.last_launches == 1


SIX = [(3,), (1, 3), (15, 3), (1,), (3,), (4,)]        # xyz, f_dc, f_rest, opacity, scaling, rotation
SIX_LRS = [1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3]


def test_six_reference_groups_in_one_launch():
    opt, _, _ = _run([_shape(1003, t) for t in SIX], SIX_LRS, steps=12, seed=11)
    assert opt.last_launches == 1


def test_misaligned_parameter_takes_the_scalar_path():
    """base[1:] of a (P+1, 3) tensor: contiguous, 12 bytes into its storage.  The gradient is an ordinary allocation."""
    gen = torch.Generator().manual_seed(12)
    P = 1003
    base = torch.randn(P + 1, 3, generator=gen)
    p = torch.nn.Parameter(base.to(DEV)[1:])
    assert p.is_contiguous() and p.data_ptr() % 16 == 12
    h = Host(base[1:])
    opt = GaussianAdam([p], lr=0.0, eps=EPS)
    for t in range(1, 13):
        opt.param_groups[0]["lr"] = lr = 1e-2 * 0.9 ** t
        g = _grad((P, 3), gen)
        p.grad = g.to(DEV)
        assert p.grad.data_ptr() % 16 == 0
        h.step(g, lr)
        opt.step()
    h.check(p, opt.state[p], "misaligned")
    assert opt.last_launches == 1


def test_grid_stride_loop_and_tail():
    """(70001, 45): 3 150 045 entries = 3077 chunks of 1024, more than the 2048 workgroups a launch is capped at, and numel % 4 == 1."""
    _run([(70001, 45)], [1e-2], steps=3, seed=13)


def test_launch_count_split_and_empty_tensor():
    from sgs_hip import _lib
    cap = _lib.load().sgs_adam_max_tensors()
    n = 2 * cap + 3
    shapes = [(5 + k, 3) for k in range(n)]
    shapes[cap // 2] = (0, 3)
    opt, params, _ = _run(shapes, [1e-2], steps=2, seed=14, one_group=True)
    assert opt.last_launches == math.ceil((n - 1) / cap)


def test_parameter_without_gradient_is_untouched_and_has_no_state():
    gen = torch.Generator().manual_seed(15)
    a0, b0 = torch.randn(9, 3, generator=gen), torch.randn(9, 4, generator=gen)
    a, b = torch.nn.Parameter(a0.to(DEV)), torch.nn.Parameter(b0.to(DEV))
    opt = GaussianAdam([{"params": [a]}, {"params": [b]}], lr=1e-2, eps=EPS)
    h = Host(a0)
    for _ in range(2):
        g = _grad((9, 3), gen)
        a.grad = g.to(DEV)
        h.step(g, 1e-2)
        opt.step()
    h.check(a, opt.state[a])
    assert _bits_equal(b, b0) and b not in opt.state and len(opt.state) == 1
    # a gradient later: b starts at step 1 while a is at 3
    hb = Host(b0)
    ga, gb = _grad((9, 3), gen), _grad((9, 4), gen)
    a.grad, b.grad = ga.to(DEV), gb.to(DEV)
    h.step(ga, 1e-2)
    hb.step(gb, 1e-2)
    opt.step()
    h.check(a, opt.state[a])
    hb.check(b, opt.state[b])
    assert opt.last_launches == 1


# ---- mask

MASK_SHAPES = [(1003, 3), (1003, 45), (129, 512)]


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_all_true_mask_is_the_dense_step(shape):
    _run([shape], [1e-2], steps=3, seed=21, mask_fn=lambda t: torch.ones(shape[0], dtype=torch.bool), guard=True)
    # (the host chain under an all-true mask is the dense chain: torch.where keeps nothing)
    opt_d, p_d, _ = _run([shape], [1e-2], steps=3, seed=21)
    opt_m, p_m, _ = _run([shape], [1e-2], steps=3, seed=21, mask_fn=lambda t: torch.ones(shape[0], dtype=torch.bool))
    for key in ("exp_avg", "exp_avg_sq"):
        assert _bits_equal(opt_d.state[p_d[0]][key], opt_m.state[p_m[0]][key])
    assert _bits_equal(p_d[0], p_m[0])


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=str)
def test_all_false_mask_changes_nothing_but_the_step(shape):
    gen = torch.Generator().manual_seed(22)
    p0 = torch.randn(shape, generator=gen)
    p = torch.nn.Parameter(p0.to(DEV))
    opt = GaussianAdam([p], lr=1e-2, eps=EPS)
    h = Host(p0)
    g = _grad(shape, gen)
    p.grad = g.to(DEV)
    h.step(g, 1e-2)
    opt.step()
    m1, v1, p1 = (x.detach().clone() for x in (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], p))
    p.grad = _grad(shape, gen).to(DEV)
    opt.step(visibility=torch.zeros(shape[0], dtype=torch.bool, device=DEV))
    assert _bits_equal(p, p1) and _bits_equal(opt.state[p]["exp_avg"], m1) and _bits_equal(opt.state[p]["exp_avg_sq"], v1)
    assert float(opt.state[p]["step"]) == 2 and opt.last_launches == 1
    h.check(p, {**opt.state[p], "step": torch.tensor(1.0)})


@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8])
def test_random_mask_fresh_per_step(dtype):
    """Widths 3 and 45 (16-byte groups straddle rows) and 512, one optimiser, a fresh 30 % mask at each of 12 steps; parameters and
    moments sit between guard rows of a NaN pattern that must survive."""
    P = 1003
    gen = torch.Generator().manual_seed(23)
    masks = {t: torch.rand(P, generator=gen) < 0.3 for t in range(1, 13)}
    # (the optimiser sees `dtype`, the host chain the same mask as bool)
    _run([(P, 3), (P, 45), (P, 512), (P, 1), (P, 4)], [1e-2, 2e-3, 5e-3, 1e-2, 1e-3], steps=12, seed=24,
         mask_fn=lambda t: masks[t], guard=True, mask_dtype=dtype)


def test_contiguous_range_mask():
    """visible index ranges with edges inside a 16-byte group and inside a wave"""
    P = 1003
    m = torch.zeros(P, dtype=torch.bool)
    for lo, hi in ((0, 1), (5, 70), (131, 133), (500, 777), (1002, 1003)):
        m[lo:hi] = True
    _run([(P, 3), (P, 45), (P, 512)], [1e-2, 2e-3, 5e-3], steps=3, seed=25, mask_fn=lambda t: m, guard=True)


# ---- state surgery (what replace_tensor_to_optimizer, _prune_optimizer and cat_tensors_to_optimizer do to an optimiser)

def _prune(opt, keep):
    out = []
    for group in opt.param_groups:
        old = group["params"][0]
        st = opt.state.get(old, None)
        st["exp_avg"] = st["exp_avg"][keep]
        st["exp_avg_sq"] = st["exp_avg_sq"][keep]
        del opt.state[old]
        group["params"][0] = torch.nn.Parameter(old[keep].requires_grad_(True))
        opt.state[group["params"][0]] = st
        out.append(group["params"][0])
    return out


def _cat(opt, extensions):
    out = []
    for group, ext in zip(opt.param_groups, extensions):
        old = group["params"][0]
        st = opt.state.get(old, None)
        st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
        st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
        del opt.state[old]
        group["params"][0] = torch.nn.Parameter(torch.cat((old, ext), dim=0).requires_grad_(True))
        opt.state[group["params"][0]] = st
        out.append(group["params"][0])
    return out


def _replace(opt, k, tensor):
    group = opt.param_groups[k]
    st = opt.state.get(group["params"][0], None)
    st["exp_avg"] = torch.zeros_like(tensor)
    st["exp_avg_sq"] = torch.zeros_like(tensor)
    del opt.state[group["params"][0]]
    group["params"][0] = torch.nn.Parameter(tensor.requires_grad_(True))
    opt.state[group["params"][0]] = st
    return group["params"][0]


def test_state_surgery_matches_the_host_chain():
    gen = torch.Generator().manual_seed(31)
    P = 301
    init = [torch.randn(_shape(P, t), generator=gen) for t in SIX]
    hosts = [Host(p) for p in init]
    params = [torch.nn.Parameter(p.to(DEV)) for p in init]
    opt = GaussianAdam([{"params": [p], "lr": lr, "name": str(k)} for k, (p, lr) in enumerate(zip(params, SIX_LRS))], lr=0.0, eps=EPS)
    count = [0]

    def steps(n):
        for _ in range(n):
            count[0] += 1
            with torch.no_grad():
                for k, (p, h) in enumerate(zip(params, hosts)):
                    opt.param_groups[k]["lr"] = lr = SIX_LRS[k] * 0.95 ** count[0]
                    g = _grad(tuple(p.shape), gen)
                    p.grad = g.to(DEV)
                    h.step(g, lr)
            opt.step()
            assert opt.last_launches == 1

    steps(4)
    keep = torch.rand(P, generator=gen) < 0.6
    params[:] = _prune(opt, keep.to(DEV))
    for h in hosts:
        h.p, h.m, h.v = h.p[keep], h.m[keep], h.v[keep]
    steps(2)
    ext = [torch.randn(_shape(77, t), generator=gen) for t in SIX]
    params[:] = _cat(opt, [e.to(DEV) for e in ext])
    for h, e in zip(hosts, ext):
        h.p, h.m, h.v = torch.cat((h.p, e)), torch.cat((h.m, torch.zeros_like(e))), torch.cat((h.v, torch.zeros_like(e)))
    steps(2)
    # the opacity reset: a new tensor for group 3, zeroed moments, the step count carried along
    new = torch.minimum(hosts[3].p, torch.full_like(hosts[3].p, -4.595))
    params[3] = _replace(opt, 3, new.to(DEV))
    hosts[3].p, hosts[3].m, hosts[3].v = new.clone(), torch.zeros_like(new), torch.zeros_like(new)
    steps(3)
    for k, (p, h) in enumerate(zip(params, hosts)):
        assert h.t == 11
        h.check(p, opt.state[p], f"group {k}")


# ---- state dict

def test_state_dict_loads_into_torch_adam():
    opt, params, hosts = _run([_shape(57, t) for t in SIX], SIX_LRS, steps=3, seed=41)
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    theirs = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(clones, SIX_LRS)], lr=0.0, eps=EPS)
    theirs.load_state_dict(opt.state_dict())
    for p, mine in zip(clones, params):
        st = theirs.state[p]
        assert float(st["step"]) == 3 and _bits_equal(st["exp_avg"], opt.state[mine]["exp_avg"])
        p.grad = torch.full_like(p, 1e-3)
    theirs.step()
    torch.cuda.synchronize()
    for p, mine in zip(clones, params):
        assert float(theirs.state[p]["step"]) == 4 and bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), mine.detach())


def test_state_dict_loads_from_torch_adam():
    gen = torch.Generator().manual_seed(42)
    init = [torch.randn(_shape(57, t), generator=gen) for t in SIX]
    tp = [torch.nn.Parameter(p.to(DEV)) for p in init]
    theirs = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(tp, SIX_LRS)], lr=0.0, eps=EPS)
    for _ in range(3):
        for p in tp:
            p.grad = _grad(tuple(p.shape), gen).to(DEV)
        theirs.step()
    ours_p = [torch.nn.Parameter(p.detach().clone()) for p in tp]
    ours = GaussianAdam([{"params": [p], "lr": lr} for p, lr in zip(ours_p, SIX_LRS)], lr=0.0, eps=EPS)
    ours.load_state_dict(theirs.state_dict())
    hosts = [Host(p.detach().cpu(), theirs.state[p]["exp_avg"].cpu(), theirs.state[p]["exp_avg_sq"].cpu(), int(theirs.state[p]["step"])) for p in tp]
    assert all(h.t == 3 for h in hosts)
    for k, (p, h) in enumerate(zip(ours_p, hosts)):
        g = _grad(tuple(p.shape), gen)
        p.grad = g.to(DEV)
        h.step(g, SIX_LRS[k])
    ours.step()
    assert ours.last_launches == 1
    for k, (p, h) in enumerate(zip(ours_p, hosts)):
        h.check(p, ours.state[p], f"group {k}")


# ---- accumulate_densification_stats

def _radii(P, gen):
    r = torch.randint(0, 4, (P,), generator=gen, dtype=torch.int32)                     # zeros and ones among them
    big = torch.randint(2, 2 ** 24, (P,), generator=gen, dtype=torch.int32)             # <= 2^24 - 1: exact in float32
    r = torch.where(torch.rand(P, generator=gen) < 0.3, big, r)
    if P > 8:
        r[0], r[1], r[2], r[3] = 0, 1, 2 ** 24 - 1, 0
    return r


@pytest.mark.parametrize("P", [1, 1003])
@pytest.mark.parametrize("form", ["radii", "mask"])
def test_densification_stats(P, form):
    gen = torch.Generator().manual_seed(50 + P)
    acc, den, mr = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
    d_acc, d_den, d_mr = (x.clone().to(DEV) for x in (acc, den, mr))   # ours
    t_acc, t_den, t_mr = (x.clone().to(DEV) for x in (acc, den, mr))   # the three indexed torch statements
    track = []
    for it in range(3):
        radii = _radii(P, gen)
        if P == 1:
            radii[0] = 0 if it == 1 else 7
        vg = _grad((P + 1, 3), gen)[1:]                                  # (the zero rows are 6, 13, ...: visible ones among them)
        vis = (radii > 0) if form == "radii" else (torch.rand(P, generator=gen) < 0.5)
        before = (d_acc.clone(), d_den.clone(), d_mr.clone())
        out = accumulate_densification_stats(d_acc, d_den, d_mr, vg.to(DEV), radii.to(DEV),
                                             visibility=None if form == "radii" else vis.to(DEV), return_visibility=True)
        assert out.dtype == torch.bool and torch.equal(out.cpu(), vis)
        if form == "radii":
            assert accumulate_densification_stats(d_acc.clone(), d_den.clone(), d_mr.clone(), vg.to(DEV), radii.to(DEV)) is None
        acc, den, mr = ref_adam.densify_stats(acc, den, mr, vg, radii, None if form == "radii" else vis, track=track)
        f, r_dev, g_dev = vis.to(DEV), radii.to(DEV), vg.to(DEV)
        t_mr[f] = torch.max(t_mr[f], r_dev[f].float())
        t_acc[f] += torch.norm(g_dev[f, :2], dim=-1, keepdim=True)
        t_den[f] += 1
        # rows that are not visible keep their bits
        for b, a in zip(before, (d_acc, d_den, d_mr)):
            assert _bits_equal(b[~f], a[~f])
    assert min(track) >= TINY
    assert torch.equal(d_den, t_den) and torch.equal(d_mr, t_mr)
    assert _bits_equal(d_acc, acc) and _bits_equal(d_den, den) and _bits_equal(d_mr, mr)
    # torch.norm is not held to the chain's bits, only to its neighbourhood: three sums of a few float32 roundings (6e-8) each
    assert torch.allclose(d_acc, t_acc, rtol=1e-5, atol=0)


def test_densification_stats_reads_a_pitched_gradient():
    """viewspace_grad as a (P, 2) column view of a wider tensor: read in place by its row pitch"""
    gen = torch.Generator().manual_seed(60)
    P = 130
    wide = _grad((P, 5), gen)
    radii = _radii(P, gen)
    acc, den, mr = torch.zeros(P, 1), torch.zeros(P, 1), torch.zeros(P)
    d = [x.clone().to(DEV) for x in (acc, den, mr)]
    accumulate_densification_stats(*d, wide.to(DEV)[:, :2], radii.to(DEV))
    acc, den, mr = ref_adam.densify_stats(acc, den, mr, wide[:, :2], radii)
    assert _bits_equal(d[0], acc) and _bits_equal(d[1], den) and _bits_equal(d[2], mr)


# ---- the training loop of tests/test_training_loop.py with GaussianAdam(visibility = radii > 0) and the stats call

def _fit(module, C, steps, with_depth):
    from test_training_loop import _params, _setup
    s, c = _setup(2500, C, 96, 64, 85.0, seed=31 + C)
    g = torch.Generator(device=DEV).manual_seed(0)
    kw = dict(image_height=64, image_width=96, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(C, device=DEV),
              scale_modifier=1.0, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=0,
              campos=c.camera_center, prefiltered=False, debug=False)
    if not with_depth:
        kw["num_channels"] = C
    rast = module.GaussianRasterizer(raster_settings=module.GaussianRasterizationSettings(**kw))

    def render(xyz, colors, opacity, scaling, rotation):
        screenspace_points = torch.zeros_like(xyz, dtype=xyz.dtype, requires_grad=True, device=DEV) + 0
        if screenspace_points.requires_grad:
            screenspace_points.retain_grad()
        out = rast(means3D=xyz, means2D=screenspace_points, shs=None, colors_precomp=colors,
                   opacities=torch.sigmoid(opacity), scales=torch.exp(scaling),
                   rotations=torch.nn.functional.normalize(rotation), cov3D_precomp=None)
        return out, screenspace_points

    with torch.no_grad():
        target = render(s.means3D, s.features, torch.logit(s.opacities.clamp(1e-3, 1 - 1e-3)), torch.log(s.scales), s.rotations)[0][0]
    xyz, opacity, scaling, rotation = _params(s, g, noise=1.0)
    colors = (s.features + 0.3 * torch.randn(s.features.shape, generator=g, device=DEV)).requires_grad_(True)
    opt = GaussianAdam([{"params": [xyz], "lr": 1e-3}, {"params": [colors], "lr": 2e-2}, {"params": [opacity], "lr": 5e-2},
                        {"params": [scaling], "lr": 5e-3}, {"params": [rotation], "lr": 1e-3}], eps=1e-15)
    xyz_gradient_accum = torch.zeros(xyz.shape[0], 1, device=DEV)
    denom = torch.zeros(xyz.shape[0], 1, device=DEV)
    max_radii2D = torch.zeros(xyz.shape[0], device=DEV)
    losses = []
    for it in range(steps):
        out, viewspace_point_tensor = render(xyz, colors, opacity, scaling, rotation)
        image, radii = out[0], out[1]
        loss = (image - target).abs().mean()
        loss.backward()
        with torch.no_grad():
            visibility_filter = accumulate_densification_stats(xyz_gradient_accum, denom, max_radii2D, viewspace_point_tensor.grad, radii,
                                                               return_visibility=True)
            opt.step(visibility=visibility_filter)
            assert opt.last_launches == 1
            opt.zero_grad()
        losses.append(float(loss.detach()))
    assert torch.equal(visibility_filter, radii > 0)
    assert float(xyz_gradient_accum.sum()) > 0 and int(denom.max()) == steps and float(max_radii2D.max()) > 0
    return losses


def test_rgbd_training_loop_converges_with_gaussian_adam():
    import rgbd_rasterization
    losses = _fit(rgbd_rasterization, 3, steps=80, with_depth=True)
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])


def test_feature_training_loop_converges_with_gaussian_adam():
    import channel_rasterization
    losses = _fit(channel_rasterization, 64, steps=80, with_depth=False)
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
