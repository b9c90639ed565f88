"""ctypes signatures of include/fdgs_mcmc.h (csrc/mcmc.hip), applied to the library ``_capi`` loaded.

The table of ``_capi`` is pinned to include/fdgs.h; the entry points of the companion header are bound here, on the same ``lib``
object, and launched through the same ``_capi.call``."""
import ctypes as C

from . import _capi

_i, _i64, _u32, _u64, _f, _p, _sz = C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_void_p, C.c_size_t
_host_ints = C.POINTER(C.c_int32)

MCMC_WEIGHT_BITS, MCMC_MAX_MULTIPLICITY = 24, 51       # include/fdgs_mcmc.h FDGS_MCMC_*

# every symbol include/fdgs_mcmc.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "fdgs_mcmc_weights_scratch_bytes": (_sz, [_i]),
    "fdgs_mcmc_weights": (C.c_int, [_i, _p, _f, _p, _p, _p, _p, _p]),
    "fdgs_mcmc_draw": (C.c_int, [_i, _i, _p, _u64, _u32, _u64, _p, _p, _p, _p]),
    "fdgs_mcmc_copy_rows": (C.c_int, [_i, _host_ints, _i64, _i, _p, _p, _p, _p]),
    "fdgs_mcmc_zero_rows": (C.c_int, [_i, _host_ints, _i64, _i, _p, _p, _p, _p]),
    "fdgs_mcmc_update": (C.c_int, [_i, _i] + [_p] * 7),
    "fdgs_mcmc_noise": (C.c_int, [_i, _i, _i] + [_p] * 7 + [_f, _p, _u64, _u32, _u64, _p, _p, _p]),
    "fdgs_mcmc_regularize_num_partials": (_i, [_i]),
    "fdgs_mcmc_regularize": (C.c_int, [_i, _p, _p, _p, _f, _f, _f] + [_p] * 6),
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
