"""ctypes signatures of include/fdgs_exposure.h (csrc/exposure.hip), applied to the library ``_capi`` loaded.

The table of ``_capi`` is pinned to include/fdgs.h; the entry points of the companion header are bound here, on the same ``lib``
object, and launched through the same ``_capi.call``."""
import ctypes as C

from . import _capi

_i, _d, _p = C.c_int32, C.c_double, C.c_void_p
_host_ints = C.POINTER(C.c_int32)

EXPOSURE_BLOCK_PIXELS, EXPOSURE_MAX_BLOCKS, EXPOSURE_MAX_VIEWS = 1024, 4096, 64       # include/fdgs_exposure.h FDGS_EXPOSURE_*

# every symbol include/fdgs_exposure.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "fdgs_exposure_apply": (C.c_int, [_i, _i, _p, _p, _i, _i, _p, _p]),
    "fdgs_exposure_num_partials": (_i, [_i, _i]),
    "fdgs_exposure_backward": (C.c_int, [_i, _i, _p, _p, _p, _i, _i, _p, _p, _p, _i, _p]),
    "fdgs_exposure_adam": (C.c_int, [_i, _p, _p, _p, _p, _i, _p, _host_ints, _d, _d, _d, _d, _p]),
    "fdgs_colour_fit_num_partials": (_i, [_i, _i]),
    "fdgs_colour_fit_moments": (C.c_int, [_i, _i, _p, _p, _i, _p, _p, _p]),
}
EXPORTED = tuple(SIGNATURES)

lib = _capi.lib
for _name, (_restype, _argtypes) in SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _restype, _argtypes

call = _capi.call


def host_ints(values):
    """Host int32s for a ``const int32_t*`` argument the library reads before it returns."""
    values = [int(v) for v in values]
    return (C.c_int32 * len(values))(*values)
