"""SGS_OPT_FEATURE_FORMAT (include/sgs_raster.h) at the C-ABI, host-only: the option is a ONE-SHOT stream option like the output pitch,
consumed by the next forward before its first early return, and only the formats that exist can be set.  Nothing here touches a device."""
import ctypes as C

NONE = 0x7fffffff   # sgs_stream_set_option's "there was no override"


def _lib():
    from sgs_hip import _lib
    return _lib, _lib.load()


def _forward(lib, _lib, P, with_callbacks, colors=True, depth=False, num_channels=128):
    @_lib.ALLOC_FN
    def alloc(user, n):
        return None
    cb = alloc if with_callbacks else _lib.ALLOC_FN()
    buf = (C.c_float * 4)()
    a = C.addressof(buf)
    return lib.sgs_rasterize_forward(cb, None, cb, None, cb, None, P, 0, 0, None, 16, 16, None, None, a if colors else None, None, None,
                                     1.0, None, None, None, None, None, 1.0, 1.0, 0, num_channels, a, a if depth else None, None,
                                     0, None)


def test_feature_format_is_consumed_by_a_forward_that_returns_early():
    _l, lib = _lib()
    assert _l.OPT_FEATURE_FORMAT == 9
    for P, with_callbacks, want_ok in ((0, True, True), (5, False, False), (-1, True, False)):
        assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, 1) == NONE
        rc = _forward(lib, _l, P, with_callbacks)
        assert (rc == 0) if want_ok else (rc < 0), (P, with_callbacks, rc)
        assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, -1) == NONE, "a stale feature format survived an early return"


def test_feature_format_values_outside_fp32_fp16_are_refused():
    _l, lib = _lib()
    for v in (2, 3, 255):
        assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, v) == _l.SGS_EINVAL, v
        assert b"SGS_OPT_FEATURE_FORMAT" in lib.sgs_last_error()
    assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, 0) == NONE   # (a refused value left nothing behind)
    assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, 1) == 0
    assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, -1) == 1
    assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, -1) == NONE
    assert lib.sgs_stream_set_option(None, 10, 0) == _l.SGS_EINVAL   # SGS_OPT_COUNT is 10


def test_fp16_features_are_refused_with_sh_input_and_with_a_depth_plane():
    _l, lib = _lib()
    for kw in (dict(colors=False, num_channels=3), dict(depth=True, num_channels=3)):
        assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, 1) == NONE
        assert _forward(lib, _l, 5, True, **kw) == _l.SGS_EINVAL, kw
        assert b"SGS_OPT_FEATURE_FORMAT" in lib.sgs_last_error(), lib.sgs_last_error()
        assert lib.sgs_stream_set_option(None, _l.OPT_FEATURE_FORMAT, -1) == NONE
    # the same calls in fp32 get past these checks (to the null-input check behind P == 0)
    assert _forward(lib, _l, 5, True, depth=True, num_channels=3) == _l.SGS_EINVAL
    assert b"SGS_OPT_FEATURE_FORMAT" not in lib.sgs_last_error()
