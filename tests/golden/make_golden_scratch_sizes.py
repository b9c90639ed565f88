"""What every exported *_bytes / *_scratch* function returns over a small grid of sizes, recorded from a build of the commit BEFORE a
change to the scratch layouts (never from the code under test):

    FDGS_LIB=/path/to/the/earlier/libfdgs.so python tests/golden/make_golden_scratch_sizes.py  ->  tests/golden/scratch_sizes.json

tests/test_capi_host.py::test_scratch_sizes_did_not_move holds the library to these values: buffers a forward writes are read by a
later backward through the same layouts, so no offset or total may move.  Host arithmetic only, no GPU."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SIZES = (0, 1, 255, 256, 257, 100_000)
P_MAX = (1 << 26) - 1            # Gaussians (check_sizes)
MESH_MAX = (1 << 28) - 1         # vertices / faces (mesh_common.h)
SORT_MAX = (1 << 31) - 4097      # keys: the largest n for which sort_blocks(n) stays an int
IMAGES = ((1, 1), (16, 16), (17, 17), (16, 17), (17, 1), (1352, 1014))   # (W, H)


def pairs(a, b):
    return [list(x) for x in itertools.product(a, b)]


GRID = {
    "fdgs_geometry_bytes": [[p] for p in SIZES + (P_MAX,)],
    "fdgs_time_slice_scratch_bytes": [[p] for p in SIZES + (P_MAX,)],
    "fdgs_camera_backward_scratch": [[p] for p in SIZES + (P_MAX,)],
    "fdgs_knn_scratch_bytes": [[p] for p in SIZES + (P_MAX,)],
    "fdgs_debug_radix_sort_scratch_bytes": [[n] for n in SIZES + ((1 << 20), (1 << 20) + 1, SORT_MAX)],
    "fdgs_image_bytes": [list(i) for i in IMAGES],
    "fdgs_binning_bytes": [[r, w, h] for r in SIZES + ((1 << 31) - 1,) for (w, h) in IMAGES],
    "fdgs_debug_tile_bin_scratch_bytes": pairs(SIZES + ((1 << 24) - 1,), SIZES + ((1 << 31) - 1,)),
    "fdgs_knn_query_scratch_bytes": pairs(SIZES + (P_MAX,), SIZES + (1 << 24,)),
    "fdgs_rigid_motion_scratch_bytes": pairs(SIZES + (P_MAX,), (0, 1, 20, 31)),
    "fdgs_kmeans_scratch_bytes": pairs(SIZES + (P_MAX,), (0, 1, 255, 256, 257, 65536)),
    "fdgs_eval_metrics_scratch_bytes": [[c, h, w] for c in (1, 3) for (w, h) in IMAGES + ((176, 176), (175, 176), (0, 16))],
    "fdgs_frames_encode_gray_scratch_bytes": [[b, h, w] for b in (0, 1, 3, 65535, 65536) for (w, h) in IMAGES],
    "fdgs_frames_resize_scratch_bytes": [[b, hs, ws, hd, wd, c] for b in (1, 3, 65535) for c in (3, 4, 5) for (ws, hs) in IMAGES
                                         for (wd, hd) in ((1, 1), (16, 17), (676, 507), (1352, 1014), (2704, 2028))],
    "fdgs_surface_extract_scratch_bytes": [list(x) for x in itertools.product((1, 2, 3, 64), repeat=3)] + [[1024, 512, 511], [1024, 512, 512]],
    "fdgs_mesh_components_scratch_bytes": pairs(SIZES + (MESH_MAX, MESH_MAX + 1), SIZES + (MESH_MAX, MESH_MAX + 1)),
    "fdgs_mesh_compact_scratch_bytes": pairs(SIZES + (MESH_MAX, MESH_MAX + 1), SIZES + (MESH_MAX, MESH_MAX + 1)),
    "fdgs_mesh_smooth_scratch_bytes": pairs(SIZES + (MESH_MAX, MESH_MAX + 1), SIZES + (MESH_MAX, MESH_MAX + 1)),
    "fdgs_mesh_simplify_scratch_bytes": pairs(SIZES + (MESH_MAX, MESH_MAX + 1), SIZES + (MESH_MAX, MESH_MAX + 1)),
}

if __name__ == "__main__":
    from fdgs import _capi
    print("recording from", _capi.LIB_PATH)
    table = {name: [[args, int(getattr(_capi.lib, name)(*args))] for args in rows] for name, rows in GRID.items()}
    with open(os.path.join(HERE, "scratch_sizes.json"), "w") as f:
        f.write("{\n" + ",\n".join('"%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print(sum(len(v) for v in table.values()), "values of", len(table), "functions")
