"""``distCUDA2`` -- drop-in for ``simple_knn._C.distCUDA2`` (simple-knn/spatial.cu:15-27; used once, at initialisation,
scene/gaussian_model.py:274): mean squared distance of every point to its three nearest neighbours (csrc/knn.hip)."""
import torch

from . import _capi


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    if not points.is_cuda:
        raise RuntimeError("fdgs: distCUDA2 needs a GPU tensor; there is no CPU path")
    pts = points.contiguous().float()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise RuntimeError("fdgs: distCUDA2 expects a [P, 3] tensor")
    P, dev = int(pts.shape[0]), pts.device
    means = torch.zeros(P, dtype=torch.float32, device=dev)           # torch::full({P}, 0.0), spatial.cu:21
    if P == 0:
        return means
    scratch = _capi.scratch(_capi.lib.fdgs_knn_scratch_bytes(P), dev)
    _capi.call("fdgs_dist2_knn3", dev, P, pts.data_ptr(), means.data_ptr(), scratch.data_ptr())
    return means


KNN_MAX_K = 64  # include/fdgs.h FDGS_KNN_MAX_K: the k best of a query live in registers


def knn(x: torch.Tensor, src: torch.Tensor, k: int, transpose: bool = False):
    """Drop-in for the reference's ``utils.general_utils.knn`` (pointops2 ``knnquery``; utils/general_utils.py:170-184).

    ``x`` [b, n, 3] queries, ``src`` [b, m, 3] sources (``[b, 3, n]`` / ``[b, 3, m]`` with ``transpose=True``), on the GPU.
    Returns ``(idx int64 [b, n, k], dist2 float32 [b, n, k])``: the k nearest sources of every query, exact, each row sorted by
    (squared distance, source index); index 0 is the batch's first source; ``dist2`` is the SQUARED distance (the reference calls
    it ``dist``), a query that is also a source finds itself at 0.  Slots no source fills (m < k) hold 1e10 and index 0, as the
    reference's initial heap.  One difference: the reference breaks exact ties in an order that depends on its scan; here the
    lower source index wins, so duplicated points always come out in one order.  ``1 <= k <= 64``.  No CPU path."""
    if not x.is_cuda or not src.is_cuda:
        raise RuntimeError("fdgs: knn needs GPU tensors; there is no CPU path")
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("fdgs: knn supports 1 <= k <= %d (the k best are kept in registers); got k = %d" % (KNN_MAX_K, k))
    if transpose:
        x, src = x.transpose(1, 2), src.transpose(1, 2)
    if x.dim() != 3 or src.dim() != 3 or x.shape[2] != 3 or src.shape[2] != 3 or x.shape[0] != src.shape[0]:
        raise ValueError("fdgs: knn expects x [b, n, 3] and src [b, m, 3] with the same b; got %s and %s"
                         % (tuple(x.shape), tuple(src.shape)))
    xq, sq = x.detach().contiguous().float(), src.detach().contiguous().float()
    b, n, m, dev = int(xq.shape[0]), int(xq.shape[1]), int(sq.shape[1]), xq.device
    idx = torch.empty((b, n, k), dtype=torch.int64, device=dev)
    dist2 = torch.empty((b, n, k), dtype=torch.float32, device=dev)
    if b == 0 or n == 0:
        return idx, dist2
    scratch = _capi.scratch(_capi.lib.fdgs_knn_query_scratch_bytes(n, m), dev)
    _capi.call("fdgs_knn_query", dev, b, n, m, k, xq.data_ptr(), sq.data_ptr() if m > 0 else None, idx.data_ptr(), dist2.data_ptr(),
               scratch.data_ptr())
    return idx, dist2
