"""The arithmetic contract of csrc/optim.hip in torch CPU ops, one op per statement (no addcmul, addcdiv or lerp: they may fuse):

    b1 = beta1, c1 = 1 - beta1, b2 = beta2, c2 = 1 - beta2, r = sqrt(1 - beta2^t), e = eps, s = lr / (1 - beta1^t)
    m' = (b1*m) + (c1*g);   v' = (b2*v) + (c2*(g*g));   den = (sqrt(v') / r) + e;   p' = p - (s * (m' / den))

The seven scalars are computed in double.  In float32 they are rounded once and every tensor op is one correctly rounded float32
operation: that is what the kernels must reproduce to the bit.  In float64 the chain is torch.optim.Adam's update (no amsgrad,
weight_decay = 0), which tests/test_optim.py pins.  Also the host chain of the densification statistics."""
import math

import torch


def sqrt_rn(x):
    """The correctly rounded square root in x's dtype.  torch's CPU float32 sqrt goes through a vector maths library that is accurate
    to under 1 ulp but NOT correctly rounded (on long tensors about 0.7 % of the entries are one ulp off the IEEE result, while
    *, +, - and / are exact to the bit), so float32 takes the float64 sqrt and rounds once more: for a square root that second
    rounding cannot change the result, since 53 bits exceed 2 * 24 + 2 (and a sub-ulp error of the float64 sqrt still leaves the margin)."""
    if x.dtype == torch.float32:
        return torch.sqrt(x.to(torch.float64)).to(torch.float32)
    return torch.sqrt(x)


def scalars(lr, beta1, beta2, eps, t, dtype=torch.float32):
    """(b1, c1, b2, c2, r, e, s) as 0-dim tensors of `dtype`, each derived in double and rounded once"""
    vals = (beta1, 1.0 - beta1, beta2, 1.0 - beta2, math.sqrt(1.0 - beta2 ** t), eps, lr / (1.0 - beta1 ** t))
    return tuple(torch.tensor(v, dtype=torch.float64).to(dtype) for v in vals)


def smallest_nonzero(*tensors):
    m = math.inf
    for x in tensors:
        a = x.detach().abs()
        a = a[a > 0]
        if a.numel():
            m = min(m, float(a.min()))
    return m


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-15, mask=None, track=None, dtype=None):
    """One step, functional: returns (p', m', v') of `dtype` (default: p's).  `t` is the step count including this step.  mask: bool, one entry
    per row (leading index); rows with mask == False keep p, m and v.  track: a list that receives the smallest nonzero magnitude
    among the intermediates of this step (the tests assert it is a normal float32)."""
    if dtype is not None:   # the dtype the chain runs in; default: p's
        p, g, m, v = (x.to(dtype) for x in (p, g, m, v))
    b1, c1, b2, c2, r, e, s = scalars(lr, beta1, beta2, eps, t, p.dtype)
    t1 = b1 * m
    t2 = c1 * g
    m1 = t1 + t2
    t3 = g * g
    t4 = c2 * t3
    t5 = b2 * v
    v1 = t5 + t4
    t6 = sqrt_rn(v1)
    t7 = t6 / r
    den = t7 + e
    t8 = m1 / den
    t9 = s * t8
    p1 = p - t9
    if mask is not None:
        keep = ~mask.reshape([-1] + [1] * (p.dim() - 1))
        if track is not None:   # only what a visible row computes
            vis = (~keep).expand_as(p)
            track.append(smallest_nonzero(*[x[vis] for x in (t1, t2, m1, t3, t4, t5, v1, t6, t7, den, t8, t9)]))
        p1 = torch.where(keep, p, p1)
        m1 = torch.where(keep, m, m1)
        v1 = torch.where(keep, v, v1)
    elif track is not None:
        track.append(smallest_nonzero(t1, t2, m1, t3, t4, t5, v1, t6, t7, den, t8, t9))
    return p1, m1, v1


def densify_stats(accum, denom, max_radii2D, viewspace_grad, radii, visibility=None, track=None):
    """The host chain of sgs_densify_stats, functional: accum + sqrt((gx*gx) + (gy*gy)), denom + 1, max(max_radii2D, radii) on the
    visible rows (radii > 0 unless a mask is given), in the dtype of accum, one op per statement."""
    vis = (radii > 0) if visibility is None else visibility.bool()
    gx, gy = viewspace_grad[:, 0], viewspace_grad[:, 1]
    xx = gx * gx
    yy = gy * gy
    ss = xx + yy
    n = sqrt_rn(ss)
    if track is not None:
        track.append(smallest_nonzero(xx[vis], yy[vis], ss[vis], n[vis]))
    a1 = accum.reshape(-1) + n
    d1 = denom.reshape(-1) + 1.0
    r1 = torch.maximum(max_radii2D, radii.to(max_radii2D.dtype))
    return (torch.where(vis, a1, accum.reshape(-1)).reshape(accum.shape), torch.where(vis, d1, denom.reshape(-1)).reshape(denom.shape),
            torch.where(vis, r1, max_radii2D))
