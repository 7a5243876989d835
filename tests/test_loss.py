"""CPU tests of the fused L1 + D-SSIM loss (csrc/photometric_loss.hip, sgs_hip/loss.py): the float64 restatement the GPU tests
compare against (tests/ref_loss.py) is itself pinned by the reference's own run (tests/golden/photometric_loss.npz, written by
gen_loss_fixture.py from utils/loss_utils.py), the C-ABI exports and declares the new entry points and rejects bad arguments on the
host, and the Python layer raises its argument errors without a GPU.  No device work here."""
import ctypes as C

import numpy as np
import pytest
import torch

import ref_loss

CASES, WINDOW = ref_loss.load_fixture()
NEW_SYMBOLS = ("sgs_photometric_loss_scratch_bytes", "sgs_photometric_loss_window", "sgs_photometric_loss_forward",
               "sgs_photometric_loss_backward")


def _pair(c):
    x, y = c["image"], c["gt"]
    return (ref_loss.crop_of(x), ref_loss.crop_of(y)) if c["crop"] else (x, y)


def test_fixture_has_the_stated_cases():
    shapes = {n: tuple(c["image"].shape) for n, c in CASES.items()}
    assert sorted(shapes.values()) == sorted([(3, 61, 83), (3, 7, 9), (2, 3, 40, 56), (3, 120, 160)])
    assert [n for n, c in CASES.items() if c["crop"]] == ["crop120x160"]
    for n, c in CASES.items():
        x, y = _pair(c)
        assert c["grad64"].shape == tuple(x.shape), n
        assert 0.0 <= float(x.min()) and float(x.max()) <= 1.0
        assert int((x == y).sum()) > 0, "no image == gt block: sign(0) is not exercised"
        assert int(((x == 0) & (y == 0)).sum()) > 0, "no all-zero block: the variance-0 cancellation is not exercised"
        # the bounds the GPU tests build from these must mean something
        assert c["e_ref"] > 0 and all(c[k + "32"] != c[k + "64"] for k in ("loss", "ssim", "l1")), n


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref_loss_2d_form_reproduces_the_reference_float64(name):
    """The restatement with the window the reference builds (float32-rounded outer product), in float64, against the reference's
    own float64 run: loss, ssim, l1 and every gradient entry to 1e-12 relative (gradient: of its largest entry)."""
    c = CASES[name]
    x, y = _pair(c)
    v, s, l1, g = ref_loss.loss_and_grad(x, y, c["lam"], form="2d")
    errs = {"loss": abs(v - c["loss64"]) / abs(c["loss64"]), "ssim": abs(s - c["ssim64"]) / abs(c["ssim64"]),
            "l1": abs(l1 - c["l164"]) / abs(c["l164"]),
            "grad": np.abs(g.reshape(c["grad64"].shape) - c["grad64"]).max() / np.abs(c["grad64"]).max()}
    print(name, errs)
    assert all(e <= 1e-12 for e in errs.values()), errs
    if "ssim_per_image64" in c:
        sp, _ = ref_loss.terms(x.double(), y.double(), form="2d", per_image=True)
        assert np.abs(sp.numpy() - c["ssim_per_image64"]).max() <= 1e-12 * np.abs(c["ssim_per_image64"]).max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_ref_loss_separable_form_is_inside_the_reference_float32_error(name):
    """The separable form (what the kernels evaluate) uses the exact products w[i] * w[j] where the reference's window holds their
    float32 roundings, so in float64 it cannot meet the reference to 1e-12: it differs by one float32 rounding per window entry.
    That is one of the roundings the reference's float32 evaluation makes (it rounds every product and every sum besides), so the
    difference has to stay under that evaluation's own error, e_ref and |v32 - v64| of the fixture (measured: 1e-8 .. 1.1e-6 of the
    largest gradient entry against e_ref of 8e-7 .. 4.7e-5)."""
    c = CASES[name]
    x, y = _pair(c)
    v, s, l1, g = ref_loss.loss_and_grad(x, y, c["lam"], form="separable")
    e = np.abs(g.reshape(c["grad64"].shape) - c["grad64"]).max() / np.abs(c["grad64"]).max()
    print(name, "grad", e, "e_ref", c["e_ref"], "loss", abs(v - c["loss64"]), "ssim", abs(s - c["ssim64"]))
    assert e <= c["e_ref"]
    assert abs(v - c["loss64"]) <= abs(c["loss32"] - c["loss64"])
    assert abs(s - c["ssim64"]) <= abs(c["ssim32"] - c["ssim64"])
    assert abs(l1 - c["l164"]) <= 1e-12 * abs(c["l164"])      # no window in this term


def test_window_taps_are_the_reference_float32_taps():
    """The taps the kernels get (computed on the host by the library) and the restatement's, bit for bit the window
    gaussian(11, 1.5) produced when the fixture was written."""
    from sgs_hip import _lib
    lib = _lib.load()
    taps = (C.c_float * 11)()
    assert lib.sgs_photometric_loss_window(taps) == 0
    assert WINDOW.dtype == np.float32 and WINDOW.shape == (11,)
    assert np.array_equal(np.array(taps[:], dtype=np.float32), WINDOW)
    assert np.array_equal(ref_loss.taps(), WINDOW)


def test_new_symbols_are_exported_and_declared():
    from sgs_hip import _lib
    lib = _lib.load()
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(lib, s), s
        fn = getattr(lib, s)
        assert fn.argtypes is not None and fn.restype is not None, f"{s}: argtypes / restype not declared"
    assert len(lib.sgs_photometric_loss_forward.argtypes) == 21
    assert len(lib.sgs_photometric_loss_backward.argtypes) == 19


def test_scratch_size_is_host_only():
    from sgs_hip import _lib
    lib = _lib.load()
    # one pair of float64 sums per 32x32 tile of every (image, channel) plane
    assert lib.sgs_photometric_loss_scratch_bytes(1, 3, 968, 1296) == 3 * 31 * 41 * 16
    assert lib.sgs_photometric_loss_scratch_bytes(2, 3, 7, 9) == 6 * 16
    assert lib.sgs_photometric_loss_scratch_bytes(1, 3, 0, 9) == _lib.SGS_EINVAL
    assert "bad sizes" in _lib.last_error()


def test_host_side_argument_errors():
    """Non-positive sizes, null images, a pitch smaller than the row and missing buffers are SGS_EINVAL with a message, before any
    device work (the pointers below are host addresses that are never dereferenced)."""
    from sgs_hip import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)

    def fwd(B=1, Cn=3, H=7, W=9, img=a, gt=a, row=9, lam=0.2, out=a, ssim=a, dmaps=None, scratch=a, nbytes=48):
        return lib.sgs_photometric_loss_forward(B, Cn, H, W, img, row, H * row, Cn * H * row, gt, 9, 63, 189, lam, 1, out, ssim, a,
                                                dmaps, scratch, nbytes, None)

    def bwd(B=1, Cn=3, H=7, W=9, img=a, gt=a, row=9, w_ssim=-0.2, dmaps=a, g=a, out=a):
        return lib.sgs_photometric_loss_backward(B, Cn, H, W, img, row, H * row, Cn * H * row, gt, 9, 63, 189, w_ssim, 0.8, dmaps, g, 1,
                                                 out, None)

    for call, want in ((lambda: fwd(B=0), "bad sizes"), (lambda: fwd(Cn=-1), "bad sizes"), (lambda: fwd(H=0), "bad sizes"),
                       (lambda: fwd(W=0), "bad sizes"), (lambda: fwd(img=None), "null image"), (lambda: fwd(gt=None), "null image"),
                       (lambda: fwd(row=8), "row pitch"), (lambda: fwd(out=None), "null output"),
                       (lambda: fwd(ssim=None), "out_ssim"), (lambda: fwd(scratch=None), "scratch"),
                       (lambda: fwd(nbytes=47), "scratch"),
                       (lambda: bwd(B=0), "bad sizes"), (lambda: bwd(W=-3), "bad sizes"), (lambda: bwd(img=None), "null image"),
                       (lambda: bwd(row=8), "row pitch"), (lambda: bwd(g=None), "null gradient"), (lambda: bwd(out=None), "null gradient"),
                       (lambda: bwd(dmaps=None), "derivative maps")):
        assert call() == _lib.SGS_EINVAL
        assert want in _lib.last_error(), (want, _lib.last_error())
    assert lib.sgs_photometric_loss_window(None) == _lib.SGS_EINVAL


def test_python_layer_argument_errors():
    from sgs_hip import loss
    x, y = torch.rand(3, 20, 24), torch.rand(3, 20, 24)
    for fn in (loss.l1_loss, loss.ssim, loss.photometric_loss):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, y)
        with pytest.raises(RuntimeError, match="float32"):
            fn(x.half(), y.half())
        with pytest.raises(RuntimeError, match="float32"):
            fn(x, y.double())
        with pytest.raises(RuntimeError, match="same shape"):
            fn(x, y[:, :10])
        with pytest.raises(RuntimeError, match="second image requires grad"):
            fn(x, y.clone().requires_grad_(True))
        with pytest.raises(RuntimeError, match=r"\(C,H,W\) or \(B,C,H,W\)"):
            fn(x[0], y[0])
    with pytest.raises(RuntimeError, match="window_size must be 11"):
        loss.ssim(x, y, window_size=7)
    with pytest.raises(RuntimeError, match="window_size must be 11"):
        loss.ssim(x, y, 7, True)
