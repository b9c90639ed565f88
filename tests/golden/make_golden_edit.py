"""Writes tests/golden/edit_render_psnr.json: how well the CPU oracle's render of a float64-transformed model (rounded to fp32), seen
through the transformed camera, matches its render of the original -- the figure tests/test_gpu_edit.py holds the HIP path to.

    python tests/golden/make_golden_edit.py

Per transform of edit_cases.RENDER_CASES: the PSNR of the two images (peak 1), the PSNR of depth' / s against depth (peak: the
original's largest depth), and that peak.  CPU only."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import edit_cases as ec  # noqa: E402
from oracle import pyoracle  # noqa: E402


def main():
    scene = ec.render_scene()
    model = ec.make_model(scene, "cpu")
    raw = ec.raw_numpy(model)
    side_a = ec.original_reference_scene(scene, raw)
    o = pyoracle.Oracle(side_a, kind="port")
    ref = o.forward()
    img_a, dep_a = ref["out_color"].copy(), ref["out_depth"].copy()
    visible = int((ref["radii"] > 0).sum())
    o.close()
    out = {}
    for name in ec.RENDER_CASES:
        s = ec.TRANSFORMS[name][2]
        assert ec.near_band_is_empty(scene, s), name
        o = pyoracle.Oracle(ec.transformed_reference_scene(side_a, raw, name), kind="port")
        res = o.forward()
        peak = float(dep_a.max())
        out[name] = {"psnr_image": round(ec.psnr(img_a, res["out_color"], 1.0), 3), "psnr_depth": round(ec.psnr(dep_a, res["out_depth"] / s, peak), 3),
                     "depth_peak": peak, "visible": visible, "visible_transformed": int((res["radii"] > 0).sum())}
        o.close()
        print(name, out[name])
    with open(os.path.join(HERE, ec.GOLDEN), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
