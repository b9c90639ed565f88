"""Records Pillow's own ``Image.resize(size)`` (default filter: BICUBIC) of the frames of tests/resize_cases.py into
tests/golden/resize/*.npz: what the reference's loader calls for every image (utils/general_utils.py:22-28 PILtoTorch).  Run once on
a machine that has Pillow; the tests read the files and need no Pillow.

    python tests/golden/make_golden_resize.py
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_cases as rc  # noqa: E402


def main():
    out_dir = os.path.join(HERE, "resize")
    os.makedirs(out_dir, exist_ok=True)
    for src, dst in rc.SHAPES:
        for C in (3, 4):
            u8 = rc.contents(src[0], src[1], C)
            mode = "RGB" if C == 3 else "RGBA"
            res = np.stack([np.array(Image.fromarray(f, mode).resize((dst[1], dst[0]))) for f in u8])
            assert res.shape == (len(u8), dst[0], dst[1], C) and res.dtype == np.uint8
            path = os.path.join(out_dir, rc.case_id(src, dst, C) + ".npz")
            np.savez_compressed(path, u8=u8, size=np.array([dst[1], dst[0]], np.int32), resized=res, pil_version=np.array(PIL.__version__))
            assert os.path.getsize(path) < (1 << 20), path
            print("%-28s %7d bytes" % (os.path.basename(path), os.path.getsize(path)))


if __name__ == "__main__":
    main()
