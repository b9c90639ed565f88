"""Exception type and text of every call in tests/cpu_rejection_cases.py, recorded from the commit BEFORE a change to the glue that
raises them (never from the code under test):

    python tests/golden/make_golden_cpu_rejections.py  ->  tests/golden/cpu_rejections.json

tests/test_capi_host.py::test_cpu_rejections_did_not_move holds the package to them, byte for byte.  Host only, no GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def record(call):
    """[exception type name, text] of ``call()``; a call that returns is a mistake in the table."""
    try:
        call()
    except Exception as e:  # noqa: BLE001 -- the type is what is recorded
        return [type(e).__name__, str(e)]
    raise AssertionError("the call did not raise")


if __name__ == "__main__":
    from cpu_rejection_cases import cases
    table = {name: record(call) for name, call in cases()}
    with open(os.path.join(HERE, "cpu_rejections.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in table.items()) + "\n}\n")
    print(len(table), "rejections")
