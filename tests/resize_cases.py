"""The shapes and contents the frame-resize tests share (tests/test_resize_host.py, tests/test_gpu_frame_resize.py) and the golden
files record PIL's results for (tests/golden/make_golden_resize.py): every frame is generated from a seed, nothing is read."""
import zlib

import numpy as np

# (Hs, Ws) -> (Hd, Wd): up-scale, down-scale, odd sizes, 1 x 1, one pass skipped, a copy, 33 and more taps, row bytes that are no
# multiple of 4 with sizes off any tile, and one shape of several tiles
SHAPES = [((1, 1), (3, 3)), ((7, 5), (3, 2)), ((5, 6), (11, 13)), ((13, 17), (6, 9)), ((9, 9), (9, 4)), ((9, 9), (4, 9)),
          ((9, 9), (9, 9)), ((3, 100), (3, 12)), ((64, 64), (8, 8)), ((33, 47), (11, 16)), ((203, 270), (102, 135))]
ALPHAS = np.array([0, 1, 2, 127, 254, 255], np.uint8)


def case_id(src, dst, C):
    return "%dx%d_to_%dx%d_c%d" % (src[0], src[1], dst[0], dst[1], C)


def contents(H, W, C):
    """uint8 [6, H, W, C]: uniform noise; a 0/255 checkerboard; 0/255 stripes of period 1 (columns) and 3 (rows) -- both clips of the
    filter's overshoot; all 255; all 0.  RGBA: alpha as noise over all bytes (frames 0, 4), in blocks of {0, 1, 2, 127, 254, 255}
    (frames 1, 3, 5) and as noise over that set (frame 2): the division, the alpha = 0 rule and the alpha = 255 rule."""
    rng = np.random.default_rng(zlib.crc32(("resize %d %d %d" % (H, W, C)).encode()))
    yy, xx = np.mgrid[0:H, 0:W]
    planes = [None, ((yy + xx) % 2) * 255, (xx % 2) * 255, ((yy // 3) % 2) * 255, np.full((H, W), 255), np.zeros((H, W))]
    f = np.empty((6, H, W, C), np.uint8)
    f[0, ..., :3] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    for i in range(1, 6):
        f[i, ..., :3] = planes[i].astype(np.uint8)[..., None]
    if C == 4:
        blocks = ALPHAS[((yy // 2) + (xx // 3)) % 6]
        f[0, ..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f[4, ..., 3] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        f[2, ..., 3] = ALPHAS[rng.integers(0, 6, (H, W))]
        f[1, ..., 3] = blocks
        f[3, ..., 3] = blocks[::-1, ::-1]
        f[5, ..., 3] = blocks
    return f
