"""ctypes signatures of include/fdgs_seed.h (csrc/seed.hip), applied to the library ``_capi`` loaded.

The table of ``_capi`` is pinned to include/fdgs.h; the entry points of the companion header are bound here, on the same ``lib``
object, and launched through the same ``_capi.call``."""
import ctypes as C

from . import _capi

_i, _u32, _u64, _f, _p, _sz = C.c_int32, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p, C.c_size_t
_host_floats = C.POINTER(C.c_float)

SEED_AXIS_BITS, SEED_AXIS_CELLS = 16, 65536            # include/fdgs_seed.h FDGS_SEED_AXIS_*
SEED_BOX, SEED_SPHERE, SEED_TIME = 0, 1, 2             # FDGS_SEED_BOX / _SPHERE / _TIME

# every symbol include/fdgs_seed.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "fdgs_seed_thin_scratch_bytes": (_sz, [_i]),
    "fdgs_seed_thin": (C.c_int, [_i, _p, _p, _p, _host_floats, _host_floats, _i, _i] + [_p] * 9),
    "fdgs_seed_random": (C.c_int, [_i, _u64, _u32, _i, _host_floats, _p, _p, _p, _p]),
    "fdgs_seed_init": (C.c_int, [_i, _i, _i, _p, _p, _p, _p, _f, _f, _p, _p]),
}
EXPORTED = tuple(SIGNATURES)

lib = _capi.lib
for _name, (_restype, _argtypes) in SIGNATURES.items():
    _fn = getattr(lib, _name)
    _fn.restype, _fn.argtypes = _restype, _argtypes

call = _capi.call


def host_floats(values, n):
    """``n`` host floats for a ``const float*`` argument the library reads before it returns."""
    values = [float(v) for v in values]
    return (C.c_float * n)(*(values + [0.0] * (n - len(values))))
