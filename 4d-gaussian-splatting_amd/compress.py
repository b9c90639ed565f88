"""A trained model stored small: an SH codebook plus quantised columns, and the way back to a flat-bucket model.

A 4D Gaussian is 17 geometry floats plus ``3 M`` SH floats (``M = 48``: 644 bytes), and 88 % of that is the non-DC SH coefficients
``_features[:, 1:, :]``.  ``compress`` replaces those rows by a k-means codebook (``kmeans``: assignment on the f32-input MFMA,
a reproducible weighted update; csrc/compress.hip) with one uint16 index per Gaussian, and stores every other segment per column as
8- or 16-bit integers over the column's range (or as float32, bit for bit).  ``decompress`` decodes straight into a new flat bucket
(``fdgs_compact_decode``) and returns a ``GaussianParams`` that renders like any other model.

* ``kmeans``                 -- weighted Lloyd iterations on the GPU, deterministic for a given seed.
* ``assign`` / ``update``    -- the two halves of an iteration (``fdgs_kmeans_assign`` / ``fdgs_kmeans_update``).
* ``quantize_columns`` / ``decode_into`` -- the column quantiser and the decode kernel.
* ``compress`` / ``decompress`` -- model -> ``CompressedModel`` (CPU tensors + a metadata dict) -> model.
* ``save`` / ``load`` / ``nbytes`` -- one ``.npz`` file with the metadata as a JSON string; these three are plain CPU code.

Quaternions are normalised before they are quantised over the fixed range [-1, 1]: every kernel normalises them on read (as the
reference's ``build_rotation`` / ``build_rotation_4d`` do with both of theirs), so only the quantisation itself changes the render.
There is no CPU path for anything that launches a kernel.  Not here: fine-tuning after quantisation, rendering from the compressed form,
entropy coding.
"""
import json
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _capi, layout

MAX_D = 192       # fdgs_kmeans_*: longest row
MAX_K = 65536     # ... and largest codebook: an index fits uint16
FORMAT_VERSION = 1

# the segments of a model besides the non-DC SH rows: name -> columns ("dc" is _features[:, 0, :])
SEGMENTS = tuple((s.name, s.tail[0]) for s in layout.GEOMETRY) + (("dc", layout.SEGMENTS[-1].head),)
DEFAULT_BITS = {"_xyz": 32, "_t": 16, "_scaling": 16, "_scaling_t": 16, "_opacity": 8, "dc": 16, "_rotation": 8, "_rotation_r": 8}
_QUATERNIONS = ("_rotation", "_rotation_r")


def _rows_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    _capi.need_gpu(t, name)
    if t.dim() != 2:
        raise ValueError("fdgs.compress: %s must be a matrix [rows, columns], got %s" % (name, tuple(t.shape)))
    return t.detach().to(torch.float32).contiguous()


def assign(x: torch.Tensor, codebook: torch.Tensor, *, want_dist: bool = False, scratch: Optional[torch.Tensor] = None):
    """``index`` [N] int32 = argmin_k |x_n - codebook_k|^2 (ties: the lowest k) and, with ``want_dist``, the winners' squared
    distances [N] (else None).  ``x`` [N, D], ``codebook`` [K, D] float32 on the GPU; D <= 192, K <= 65536."""
    x, c = _rows_f32(x, "x"), _rows_f32(codebook, "codebook")
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(c.shape[0])
    if int(c.shape[1]) != D or c.device != x.device:
        raise ValueError("fdgs.compress.assign: x is [%d, %d] on %s, the codebook %s on %s" % (N, D, x.device, tuple(c.shape), c.device))
    index = torch.empty((N,), dtype=torch.int32, device=x.device)
    dist = torch.empty((N,), dtype=torch.float32, device=x.device) if want_dist else None
    if scratch is None:
        scratch = _capi.scratch(_capi.lib.fdgs_kmeans_scratch_bytes(N, K), x.device, floor=1)
    _capi.call("fdgs_kmeans_assign", x.device, N, K, D, _capi._ptr(x), _capi._ptr(c), _capi._ptr(index), _capi._ptr(dist), scratch.data_ptr())
    return index, dist


def update(x: torch.Tensor, index: torch.Tensor, codebook: torch.Tensor, *, weights: Optional[torch.Tensor] = None,
           scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Replaces, IN PLACE, every row k of ``codebook`` [K, D] (contiguous float32) by the ``weights``-weighted mean of the rows of
    ``x`` with ``index == k``; a cluster without rows or without weight keeps its row.  Returns the rows per cluster, int32 [K].
    Bitwise reproducible."""
    x = _rows_f32(x, "x")
    _capi.need_gpu(codebook, "codebook")
    _capi.need_gpu(index, "index")
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(codebook.shape[0])
    if codebook.dtype != torch.float32 or not codebook.is_contiguous() or codebook.dim() != 2 or int(codebook.shape[1]) != D:
        raise ValueError("fdgs.compress.update: the codebook must be a contiguous float32 [K, %d] tensor" % D)
    if index.dtype != torch.int32 or index.numel() != N or not index.is_contiguous():
        raise ValueError("fdgs.compress.update: index must be a contiguous int32 tensor with %d elements" % N)
    w = None
    if weights is not None:
        w = _capi._dev_f32(weights.detach().reshape(-1), "weights")
        if w is None or w.numel() != N:
            raise ValueError("fdgs.compress.update: weights must have %d elements" % N)
    counts = torch.empty((K,), dtype=torch.int32, device=x.device)
    if scratch is None:
        scratch = _capi.scratch(_capi.lib.fdgs_kmeans_scratch_bytes(N, K), x.device, floor=1)
    _capi.call("fdgs_kmeans_update", x.device, N, K, D, _capi._ptr(x), _capi._ptr(index), _capi._ptr(w), _capi._ptr(codebook),
               _capi._ptr(counts), scratch.data_ptr())
    return counts


def kmeans(x: torch.Tensor, K: int, *, iters: int = 10, weights: Optional[torch.Tensor] = None, init: Optional[torch.Tensor] = None,
           seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """``iters`` Lloyd iterations over the rows ``x`` [N, D] (GPU): ``(codebook [K, D] float32, index [N] int32)``, ``index`` being
    the assignment against the RETURNED codebook.  ``init``: the [K, D] start (copied); None: K rows of ``x`` drawn with a CPU
    generator seeded with ``seed`` (N < K: the rows are cycled).  ``iters = 0`` assigns against ``init`` and returns it unchanged.
    ``weights`` [N] >= 0 weigh the means.  The same inputs and seed give bit-identical results."""
    x = _rows_f32(x, "x")
    N, D, K = int(x.shape[0]), int(x.shape[1]), int(K)
    if N < 1 or not (1 <= D <= MAX_D) or not (1 <= K <= MAX_K):
        raise ValueError("fdgs.compress.kmeans: need N >= 1, 1 <= D <= %d and 1 <= K <= %d (N=%d D=%d K=%d)" % (MAX_D, MAX_K, N, D, K))
    if init is not None:
        if tuple(init.shape) != (K, D):
            raise ValueError("fdgs.compress.kmeans: init must be [%d, %d], got %s" % (K, D, tuple(init.shape)))
        codebook = init.detach().to(device=x.device, dtype=torch.float32).contiguous().clone()
    else:
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))
        codebook = x[perm[torch.arange(K) % N].to(x.device)].contiguous()
    scratch = _capi.scratch(_capi.lib.fdgs_kmeans_scratch_bytes(N, K), x.device, floor=1)
    for _ in range(int(iters)):
        index, _d = assign(x, codebook, scratch=scratch)
        update(x, index, codebook, weights=weights, scratch=scratch)
    index, _d = assign(x, codebook, scratch=scratch)
    return codebook, index


def column_ranges(lo: np.ndarray, hi: np.ndarray, bits: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(step, inv)`` of columns spanning [lo, hi] at ``bits`` (8 / 16), in float32: (hi - lo) / qmax and qmax / (hi - lo), both 0
    where hi == lo."""
    qmax = np.float32((1 << int(bits)) - 1)
    span = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        step = np.where(span > 0, span / qmax, np.float32(0)).astype(np.float32)
        inv = np.where(span > 0, qmax / span, np.float32(0)).astype(np.float32)
    return step, inv


def quantize_columns(x: torch.Tensor, lo, inv, bits: int) -> torch.Tensor:
    """``min(max(rintf((x - lo) * inv), 0), qmax)`` per column of ``x`` [P, C] (GPU) as uint8 (``bits`` 8) or -- the same 16 bits in
    torch's int16 -- uint16 (``bits`` 16); ``lo`` / ``inv``: C float32 values."""
    x = _rows_f32(x, "x")
    if bits not in (8, 16):
        raise ValueError("fdgs.compress.quantize_columns: bits must be 8 or 16, got %r" % (bits,))
    P, C = int(x.shape[0]), int(x.shape[1])
    lo_d = torch.as_tensor(np.asarray(lo, np.float32).reshape(C)).to(x.device)
    inv_d = torch.as_tensor(np.asarray(inv, np.float32).reshape(C)).to(x.device)
    q = torch.empty((P, C), dtype=torch.uint8 if bits == 8 else torch.int16, device=x.device)
    _capi.call("fdgs_quantize_columns", x.device, P, C, _capi._ptr(x), lo_d.data_ptr(), inv_d.data_ptr(), (1 << bits) - 1, _capi._ptr(q))
    return q


def decode_into(out: torch.Tensor, P: int, C: int, bits: int, q: Optional[torch.Tensor], lo=None, step=None, *,
                rows: Optional[torch.Tensor] = None, index: Optional[torch.Tensor] = None) -> None:
    """Fills ``out`` (contiguous float32, P * (C + D) elements, GPU) row by row: the C columns of ``q`` [P, C] -- uint8 / 16-bit /
    float32 by ``bits``, dequantised as ``lo + q * step`` -- then row ``index[p]`` (int32; None: row p) of ``rows`` [K, D]."""
    _capi.need_gpu(out, "out")
    D = 0 if rows is None else int(rows.shape[1])
    if out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != int(P) * (int(C) + D):
        raise ValueError("fdgs.compress.decode_into: out must be a contiguous float32 tensor of %d elements" % (int(P) * (int(C) + D)))
    for name, t in (("q", q), ("rows", rows), ("index", index)):
        if t is not None and (not t.is_cuda or t.device != out.device or not t.is_contiguous()):
            raise RuntimeError("fdgs: tensor '%s' must be contiguous on %s (got %s); there is no CPU path" % (name, out.device, t.device))
    if q is not None and q.element_size() * 8 != int(bits):
        raise ValueError("fdgs.compress.decode_into: q holds %d-bit values, bits says %d" % (q.element_size() * 8, int(bits)))
    if index is not None and index.dtype != torch.int32:
        raise ValueError("fdgs.compress.decode_into: index must be int32")
    dev = out.device
    lo_d = step_d = None
    if int(bits) != 32 and int(C) > 0:
        lo_d = torch.as_tensor(np.asarray(lo, np.float32).reshape(int(C))).to(dev)
        step_d = torch.as_tensor(np.asarray(step, np.float32).reshape(int(C))).to(dev)
    _capi.call("fdgs_compact_decode", dev, int(P), int(C), int(bits), _capi._ptr(q), _capi._ptr(lo_d), _capi._ptr(step_d), D, _capi._ptr(rows),
               _capi._ptr(index), 0 if rows is None else int(rows.shape[0]), out.data_ptr())


@dataclass
class CompressedModel:
    """``tensors`` (CPU): per segment of ``SEGMENTS`` a [P, C] uint8 / uint16 / float32 tensor, plus ``sh_codebook`` [K, D] float32 with
    ``sh_index`` [P] uint16, or ``sh_rest`` [P, D] float32 without a codebook (neither with M == 1).  ``meta``: P, M, the SH degrees,
    time_duration, gaussian_dim, rot_4d, force_sh_3d, prefilter_var, and per segment ``bits``, ``lo`` and ``step`` (float32 values)."""
    tensors: Dict[str, torch.Tensor] = field(default_factory=dict)
    meta: Dict[str, object] = field(default_factory=dict)


def _segment_source(model, name: str) -> torch.Tensor:
    if name == "dc":
        return model._features.detach()[:, 0, :]
    return getattr(model, name).detach()


@torch.no_grad()
def compress(model, *, codebook_size: Optional[int] = 4096, iters: int = 10, weights: Optional[torch.Tensor] = None,
             bits: Optional[Dict[str, int]] = None, seed: int = 0, init: Optional[torch.Tensor] = None) -> CompressedModel:
    """``model`` (fdgs.train_host.GaussianParams on the GPU) as a ``CompressedModel``.  ``_features[:, 1:, :]`` becomes a codebook of
    ``codebook_size`` rows (``kmeans`` with ``iters``, ``weights`` [P] -- e.g. ``ContributionStats.weight_sum`` --, ``seed``,
    ``init``) plus uint16 indices; ``codebook_size = None`` keeps the rows as float32.  Every other segment is stored with
    ``bits[name]`` in {8, 16, 32} over its columns' [min, max] (quaternions: normalised, over [-1, 1]); 32 keeps the float32 values bit
    for bit.  ``bits`` overrides ``DEFAULT_BITS`` per name."""
    _capi.need_gpu(model.flat, "model.flat")
    P, M = int(model.P), int(model.M)
    if P < 1:
        raise ValueError("fdgs.compress: the model has no Gaussians")
    if not bool(torch.isfinite(model.flat.detach()).all()):
        raise ValueError("fdgs.compress: the model holds non-finite parameters")
    use = dict(DEFAULT_BITS)
    for k, v in (bits or {}).items():
        if k not in use or int(v) not in (8, 16, 32):
            raise ValueError("fdgs.compress: bits[%r] = %r; the names are %s, the widths 8, 16 and 32" % (k, v, sorted(use)))
        use[k] = int(v)
    cm = CompressedModel()
    lo_meta, step_meta = {}, {}
    for name, C in SEGMENTS:
        x = _segment_source(model, name).reshape(P, C).to(torch.float32).contiguous()
        b = use[name]
        if b == 32:
            cm.tensors[name] = x.cpu().clone()
            continue
        if name in _QUATERNIONS:
            x = F.normalize(x)
            lo, hi = np.full((C,), -1.0, np.float32), np.full((C,), 1.0, np.float32)
        else:
            lo, hi = x.min(dim=0).values.cpu().numpy().astype(np.float32), x.max(dim=0).values.cpu().numpy().astype(np.float32)
        step, inv = column_ranges(lo, hi, b)
        q = quantize_columns(x, lo, inv, b).cpu()
        cm.tensors[name] = q if b == 8 else q.view(torch.uint16)
        lo_meta[name], step_meta[name] = [float(v) for v in lo], [float(v) for v in step]
    D = 3 * (M - 1)
    K = None
    if M > 1:
        rest = model._features.detach()[:, 1:, :].reshape(P, D).to(torch.float32).contiguous()
        if codebook_size is None:
            cm.tensors["sh_rest"] = rest.cpu().clone()
        else:
            K = int(codebook_size)
            if not (1 <= K <= MAX_K) or D > MAX_D:
                raise ValueError("fdgs.compress: codebook_size must be within 1..%d and 3 (M - 1) <= %d (got %d, M = %d)" % (MAX_K, MAX_D, K, M))
            w = None
            if weights is not None:
                w = weights.detach().reshape(-1).to(device=rest.device, dtype=torch.float32)
                if w.numel() != P or not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
                    raise ValueError("fdgs.compress: weights must be %d finite values >= 0" % P)
            codebook, index = kmeans(rest, K, iters=iters, weights=w, init=init, seed=seed)
            cm.tensors["sh_codebook"] = codebook.cpu()
            cm.tensors["sh_index"] = torch.from_numpy(index.cpu().numpy().astype(np.uint16))
    cm.meta = {
        "format": FORMAT_VERSION, "P": P, "M": M, "codebook_size": K,
        **layout.settings_of(model), "bits": use, "lo": lo_meta, "step": step_meta,
    }
    cm.meta["time_duration"] = list(cm.meta["time_duration"])
    return cm


def _upload(t: torch.Tensor, device) -> torch.Tensor:
    t = t.contiguous()
    if t.dtype == torch.uint16:
        t = t.view(torch.int16)   # the same bits in a type every backend copies
    return t.to(device)


@torch.no_grad()
def decompress(cm: CompressedModel, device):
    """A ``GaussianParams`` on ``device`` (a GPU) from ``cm``: every segment is decoded straight into its place in a new flat bucket."""
    from .train_host import GaussianParams
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("fdgs: decompress needs a GPU device (got %s); there is no CPU path" % device)
    meta, T = cm.meta, cm.tensors
    P, M = int(meta["P"]), int(meta["M"])
    D = 3 * (M - 1)
    model = GaussianParams.empty(P, M, device)
    flat = model.flat.detach()
    for name, C in SEGMENTS:
        b = int(meta["bits"][name])
        q = _upload(T[name], device)
        lo, step = meta["lo"].get(name), meta["step"].get(name)
        if name != "dc":
            o0, o1 = model.offsets[name]
            decode_into(flat[o0:o1], P, C, b, q, lo, step)
            continue
        o0, o1 = model.offsets["_features"]
        if M == 1:
            decode_into(flat[o0:o1], P, C, b, q, lo, step)
        elif "sh_codebook" in T:
            index = torch.from_numpy(T["sh_index"].numpy().astype(np.int32)).to(device)
            decode_into(flat[o0:o1], P, C, b, q, lo, step, rows=_upload(T["sh_codebook"], device), index=index)
        else:
            decode_into(flat[o0:o1], P, C, b, q, lo, step, rows=_upload(T["sh_rest"], device))
    return model.apply_settings(**{k: meta[k] for k in layout.SETTINGS})


def _meta_bytes(cm: CompressedModel) -> bytes:
    return json.dumps(cm.meta, sort_keys=True).encode("utf-8")


def nbytes(cm: CompressedModel) -> int:
    """Bytes of payload ``save`` writes: every tensor plus the metadata's JSON text (not the container's own headers)."""
    return sum(int(t.numel()) * int(t.element_size()) for t in cm.tensors.values()) + len(_meta_bytes(cm))


def save(path, cm: CompressedModel) -> None:
    """One uncompressed ``.npz``: the tensors under their names, the metadata as JSON text in the uint8 array ``meta``."""
    arrays = {k: t.detach().cpu().contiguous().numpy() for k, t in cm.tensors.items()}
    if "meta" in arrays:
        raise ValueError("fdgs.compress.save: 'meta' is not a tensor name")
    arrays["meta"] = np.frombuffer(_meta_bytes(cm), dtype=np.uint8)
    with open(path, "wb") as fh:
        np.savez(fh, **arrays)


def load(path) -> CompressedModel:
    with np.load(path, allow_pickle=False) as z:
        meta = json.loads(bytes(z["meta"]).decode("utf-8"))
        tensors = {k: torch.from_numpy(np.ascontiguousarray(z[k])) for k in z.files if k != "meta"}
    if int(meta.get("format", -1)) != FORMAT_VERSION:
        raise ValueError("fdgs.compress.load: %s is format %r, this code reads %d" % (path, meta.get("format"), FORMAT_VERSION))
    return CompressedModel(tensors, meta)
