"""The ctypes face of the binding -- restype and argtypes of every exported function, size and field layout of every struct --
recorded from the commit BEFORE a change to how fdgs._capi declares them (never from the code under test):

    python tests/golden/make_golden_capi_signatures.py  ->  tests/golden/capi_signatures.json

tests/test_capi_host.py::test_signatures_did_not_move holds the binding to these values: a wrong argtype converts an argument silently
(a pointer cut to 32 bits, a float passed as an int).  Host only, no GPU."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def type_name(t):
    """A ctypes type as text: its name; a function pointer type with its own signature; None (unset, or void) as None."""
    if t is None:
        return None
    if issubclass(t, C._CFuncPtr):
        return "CFUNCTYPE(%s; %s)" % (type_name(t._restype_), ", ".join(str(type_name(a)) for a in t._argtypes_))
    return t.__name__


def describe(capi):
    """{"functions": {name: {"restype", "argtypes" (None where unset)}}, "structs": {name: {"sizeof", "fields": [[name, type, offset]]}}}"""
    functions = {}
    for name in capi.EXPORTED:
        fn = getattr(capi.lib, name)
        functions[name] = {"restype": type_name(fn.restype), "argtypes": None if fn.argtypes is None else [type_name(a) for a in fn.argtypes]}
    structs = {}
    for name, cls in sorted(vars(capi).items()):
        if isinstance(cls, type) and issubclass(cls, C.Structure):
            structs[name] = {"sizeof": C.sizeof(cls),
                             "fields": [[f[0], type_name(f[1]), getattr(cls, f[0]).offset] for f in getattr(cls, "_fields_", [])]}
    return {"functions": functions, "structs": structs}


if __name__ == "__main__":
    from fdgs import _capi
    table = describe(_capi)
    with open(os.path.join(HERE, "capi_signatures.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": {\n%s\n}' % (part, ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":")))
                                                                  for k, v in rows.items())) for part, rows in table.items()) + "\n}\n")
    print(len(table["functions"]), "functions,", len(table["structs"]), "structs")
