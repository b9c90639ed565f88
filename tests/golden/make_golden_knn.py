"""Golden values of simple-knn's distCUDA2 through the reference's OWN device code (oracle/_ref/liboracle_ref.so, built by
oracle/refbuild/build_ref.py where the reference is available), on the point clouds of tests/test_oracle_knn.py:
python tests/golden/make_golden_knn.py  ->  tests/golden/knn_ref.npz  (one array per case, named <P>_<kind>)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import pyoracle  # noqa: E402
from test_oracle_knn import PIN_CASES, _cloud  # noqa: E402

if not pyoracle.have_ref():
    raise SystemExit("needs oracle/_ref/liboracle_ref.so (oracle/refbuild/build_ref.py)")
out = {"%d_%s" % (P, kind): pyoracle.ref_dist2_knn3(_cloud(P, 100 + P, kind)) for P, kind in PIN_CASES}
np.savez_compressed(os.path.join(HERE, "knn_ref.npz"), **out)
print(len(out), "cases")
