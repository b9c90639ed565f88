"""The model's description of itself (tests/model_layout_cases.py), recorded from the commit BEFORE a change to how the flat bucket is
stated (never from the code under test):

    python tests/golden/make_golden_model_layout.py  ->  tests/golden/model_layout.json

tests/test_model_layout_host.py holds the package to it.  Host only, no GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


if __name__ == "__main__":
    import model_layout_cases
    table = model_layout_cases.record()
    with open(os.path.join(HERE, "model_layout.json"), "w") as f:
        modes = ",\n".join('  "%s": {\n%s\n  }' % (mode, ",\n".join('    "%s": %s' % (k, json.dumps(v, sort_keys=True)) for k, v in entries.items()))
                          for mode, entries in table["modes"].items())
        f.write('{\n "compress.SEGMENTS": %s,\n "modes": {\n%s\n }\n}\n' % (json.dumps(table["compress.SEGMENTS"]), modes))
    print(len(table["modes"]), "modes,", sum(len(v) for v in table["modes"].values()), "entries")
