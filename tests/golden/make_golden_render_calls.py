"""The call trace of every case in tests/render_call_cases.py, recorded from the commit BEFORE a change to the layer between the
user and the native binding (never from the code under test):

    python tests/golden/make_golden_render_calls.py  ->  tests/golden/render_calls.json

tests/test_render_calls_host.py holds the package to it.  Host only, no GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


if __name__ == "__main__":
    import render_call_cases
    table = {case: render_call_cases.run(case, setattr) for case in render_call_cases.cases()}
    with open(os.path.join(HERE, "render_calls.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in table.items()) + "\n}\n")
    print(len(table), "cases,", sum(len(v["calls"]) for v in table.values()), "calls,", sum("raised" in v for v in table.values()), "raised")
