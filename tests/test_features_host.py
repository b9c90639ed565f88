"""CPU: the feature-blend entries of the C ABI (fdgs_feature_blend, fdgs_feature_blend_backward: exported, struct size, every argument
error -- nothing is launched) and the host side of fdgs.features (device check first, the shape logic)."""
import ctypes as C
import os

import pytest
import torch

from util import ROOT


def _valid():
    """A fdgs_feature_in that passes every check (the pointers are host memory: no test here gets as far as a launch) + its keep-alives."""
    from fdgs import _capi
    dummy = (C.c_float * 64)()
    cin = _capi.FdgsFeatureIn()
    cin.P, cin.W, cin.H, cin.C = 5, 16, 16, 3
    cin.geom_buffer = cin.binning_buffer = cin.image_buffer = cin.features = C.addressof(dummy)
    cin.num_rendered = 7
    return cin, dummy


def test_symbols_are_exported_and_the_struct_size_matches():
    from fdgs import _capi
    for sym in ("fdgs_feature_blend", "fdgs_feature_blend_backward"):
        assert sym in _capi.EXPORTED and hasattr(_capi.lib, sym)
    cin = _capi.FdgsFeatureIn()
    # include/fdgs.h on a 64-bit target: 5 x 4 bytes (+ padding), three pointers, an int32 (+ padding), a pointer
    assert cin.struct_size == C.sizeof(_capi.FdgsFeatureIn) == 64
    assert [f[0] for f in _capi.FdgsFeatureIn._fields_] == ["struct_size", "P", "W", "H", "C", "geom_buffer", "binning_buffer", "image_buffer",
                                                            "num_rendered", "features"]
    assert _capi.FDGS_FEATURE_MAX_CHANNELS == 256
    with open(os.path.join(ROOT, "include", "fdgs.h")) as f:
        assert "#define FDGS_FEATURE_MAX_CHANNELS 256" in f.read()
    # the library agrees with the size: with it, both calls get as far as the argument checks behind the size check
    cin.P, cin.W, cin.H, cin.C = 5, 16, 16, 0
    dummy = (C.c_float * 4)()
    assert _capi.lib.fdgs_feature_blend(C.byref(cin), C.addressof(dummy), None) == 1
    assert "struct_size" not in _capi.last_error() and "channels" in _capi.last_error()
    assert _capi.lib.fdgs_feature_blend_backward(C.byref(cin), C.addressof(dummy), C.addressof(dummy), None) == 1
    assert "struct_size" not in _capi.last_error() and "channels" in _capi.last_error()
    import fdgs.features  # noqa: F401


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_every_argument_error_is_reported_before_any_launch(which):
    from fdgs import _capi
    cin, dummy = _valid()
    out = C.addressof(dummy)

    def call(c, o=out, g=out):
        if which == "forward":
            return _capi.lib.fdgs_feature_blend(None if c is None else C.byref(c), o, None)
        return _capi.lib.fdgs_feature_blend_backward(None if c is None else C.byref(c), g, o, None)

    # NULL struct, NULL outputs
    assert call(None) == 1 and "must not be NULL" in _capi.last_error()
    assert call(cin, o=None) == 1 and "must not be NULL" in _capi.last_error()
    if which == "backward":
        assert call(cin, g=None) == 1 and "must not be NULL" in _capi.last_error()
    # a wrong struct_size
    for d in (-8, 8):
        cin.struct_size += d
        assert call(cin) == 1 and "fdgs_feature_in" in _capi.last_error() and "struct_size" in _capi.last_error()
        cin.struct_size -= d
    # sizes
    for P, W, H in ((-1, 16, 16), (1 << 26, 16, 16), (5, 0, 16), (5, 16, -3)):
        cin.P, cin.W, cin.H = P, W, H
        assert call(cin) == 1 and "bad sizes" in _capi.last_error(), (P, W, H)
    cin.P, cin.W, cin.H = 5, 16, 16
    # channels
    for Cn in (0, -2, _capi.FDGS_FEATURE_MAX_CHANNELS + 1):
        cin.C = Cn
        assert call(cin) == 1 and "channels" in _capi.last_error(), Cn
    cin.C = 3
    # P > 0 with a NULL scratch buffer: refused whatever num_rendered says
    for name in ("geom_buffer", "binning_buffer", "image_buffer"):
        keep = getattr(cin, name)
        setattr(cin, name, None)
        for R in (7, -1, 0):
            cin.num_rendered = R
            assert call(cin) == 1 and "must not be NULL" in _capi.last_error(), (name, R)
        setattr(cin, name, keep)
    cin.num_rendered = 7
    # NULL features: an error of the forward only (the backward does not read them)
    cin.features = None
    if which == "forward":
        assert call(cin) == 1 and "features must not be NULL" in _capi.last_error()
    else:
        cin.P = 0   # ... and with nothing to walk the backward returns without touching anything
        cin.geom_buffer = cin.binning_buffer = cin.image_buffer = None
        assert call(cin) == 0


def test_python_entry_points_check_the_device_first():
    from fdgs import features
    e = torch.empty(0, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        features.blend_pass(4, 8, 8, e, e, e, 0, torch.zeros(4, 3))
    # the device check comes before the shape checks: a CPU tensor of a bad shape is still the CPU error
    with pytest.raises(RuntimeError, match="no CPU path"):
        features.blend_pass(4, 8, 8, e, e, e, 0, torch.zeros(4, 1000))
    with pytest.raises(RuntimeError, match="no CPU path"):
        features.blend_backward_pass(4, 8, 8, e, e, e, 0, torch.zeros(3, 8, 8), torch.zeros(4, 3))

    class _M:
        get_xyz = torch.zeros(4, 3)

    class _Cam:
        image_width, image_height = 8, 8
    with pytest.raises(RuntimeError, match="no CPU path"):
        features.render_features(_Cam(), _M(), None, torch.zeros(4, 2))


def test_shape_logic():
    from fdgs import features
    v = torch.arange(6, dtype=torch.float32)
    m = features.as_feature_matrix(v, 6)
    assert m.shape == (6, 1) and m.data_ptr() == v.data_ptr()
    assert features.as_feature_matrix(torch.zeros(6, 17), 6).shape == (6, 17)
    assert features.as_feature_matrix(torch.zeros(6, features.MAX_CHANNELS), 6).shape == (6, 256)
    for bad in (torch.zeros(5), torch.zeros(5, 3), torch.zeros(6, 3, 1), torch.zeros(6, 0), torch.zeros(6, features.MAX_CHANNELS + 1)):
        with pytest.raises(ValueError):
            features.as_feature_matrix(bad, 6)
    with pytest.raises(ValueError, match="loss"):
        features.fit_features(None, [1], [torch.zeros(1, 2, 2)], None, iterations=1, loss="huber")
    with pytest.raises(ValueError, match="one target per camera"):
        features.fit_features(None, [1, 2], [torch.zeros(1, 2, 2)], None, iterations=1)
