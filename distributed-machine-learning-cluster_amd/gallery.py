"""An HBM-resident gallery of embeddings with nearest-neighbour search (the
Python face of csrc/runtime/gallery.cpp and csrc/kernels/sim_topk.hip).

Reference counterpart: none, the reference answers with a class name only.
This is what ``InferenceEngine.embed`` is for: retrieval, de-duplication and
k-NN labelling against stored images, without a [B, N] score matrix in HBM.
"""
from __future__ import annotations

import torch

from . import native, ops
from .runtime import require_gpu


class Gallery:
    """Up to ``capacity`` embeddings of length ``dim`` on one GPU, stored as
    bf16 rows (dim % 32 == 0, 32 <= dim <= 4096).

    metric "dot": score = the dot product of the bf16-rounded query and row;
    "cosine": that divided by both L2 norms (of the rounded vectors, each
    clamped at 1e-12 as ``F.normalize`` does). All device memory, the search
    workspace for ``max_batch`` queries included, is allocated here.

    dtype "e4m3": rows are stored as one-byte OCP e4m3 codes with one fp32
    scale per row (dim % 128 == 0, 128 <= dim <= 4096) and searched on the
    block-scaled fp8 MFMA: half the bytes, half the MFMA cycles. A row (and
    each query) is multiplied by the largest power of two that keeps its
    largest magnitude <= 448 and rounded to e4m3 (``ops.gallery_pack8``);
    "dot" is then the dot product of the dequantised vectors, "cosine" that
    of the codes divided by both L2 norms of the codes. Every method behaves
    as on a bf16 gallery."""

    def __init__(self, dim: int, capacity: int, device: int = 0, metric: str = "cosine", max_batch: int = 256,
                 dtype: str = "bf16"):
        require_gpu()
        if metric not in ("cosine", "dot"):
            raise ValueError(f"metric is 'cosine' or 'dot', got {metric!r}")
        if dtype not in ("bf16", "e4m3"):
            raise ValueError(f"dtype is 'bf16' or 'e4m3', got {dtype!r}")
        self.device = torch.device("cuda", device)
        self._g = native().Gallery(dim, capacity, device, metric, max_batch, dtype)
        self.dim, self.capacity, self.metric, self.max_batch = dim, capacity, metric, max_batch
        self.dtype = dtype
        self.max_topk = native().MAX_TOPK

    def __len__(self) -> int:
        return self._g.size

    def clear(self) -> None:
        """Forget every row, label and removal; the next ``add`` starts at id 0 again."""
        self._g.clear()

    @property
    def live(self) -> int:
        """Rows a search can return: ``len(self)`` less the removed ones."""
        return self._g.live

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def add(self, features: torch.Tensor, labels=None) -> range:
        """Append contiguous float32 [M, dim] rows on this gallery's GPU (what
        ``InferenceEngine.embed`` returns); the new rows' ids. ``labels``: an
        int tensor or sequence [M], all >= 0 (default: 0 each)."""
        if features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] != self.dim \
                or features.device != self.device or not features.is_contiguous():
            raise ValueError(f"add: expected contiguous torch.float32 [M,{self.dim}] on {self.device}, got "
                             f"{features.dtype} {tuple(features.shape)} on {features.device}")
        M = features.shape[0]
        if len(self) + M > self.capacity:
            raise ValueError(f"add: {len(self)} + {M} rows exceed the capacity {self.capacity}")
        lab = None
        if labels is not None:
            lab = self._ints(labels, M, "add: labels")
            if M and (int(lab.min()) < 0 or int(lab.max()) > 2 ** 31 - 1):
                raise ValueError("add: labels must lie in 0..2^31 - 1 (a negative label marks a removed row)")
            lab = lab.to(device=self.device, dtype=torch.int32).contiguous()
        first = self._g.add(features.data_ptr(), M, self._stream(), labels=0 if lab is None else lab.data_ptr())
        return range(first, first + M)

    @staticmethod
    def _ints(values, n: int, what: str) -> torch.Tensor:
        """An int tensor or sequence as an integer tensor [n]."""
        t = values if isinstance(values, torch.Tensor) else torch.as_tensor(list(values))
        if t.numel() == 0 and n == 0:
            t = t.to(torch.int64)
        if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool or tuple(t.shape) != (n,):
            raise ValueError(f"{what}: expected {n} integers, got {t.dtype} {tuple(t.shape)}")
        return t

    def remove(self, ids) -> None:
        """Take rows out of every later search. ``ids``: ints in
        0..len(self)-1 (a sequence, range or int tensor); one bad id raises and
        removes nothing. Removing a removed row is a no-op; ids are not reused,
        ``len(self)`` stays and ``live`` drops."""
        ids = ids.tolist() if isinstance(ids, torch.Tensor) else list(ids)
        for i in ids:
            if not isinstance(i, int) or isinstance(i, bool) or not 0 <= i < len(self):
                raise ValueError(f"remove: id {i!r} outside 0..{len(self) - 1}")
        self._g.remove(ids, self._stream())

    def labels(self) -> torch.Tensor:
        """int32 [len(self)]: every row's label, -1 for a removed row."""
        out = torch.empty(len(self), dtype=torch.int32, device=self.device)
        self._g.read_labels(out.data_ptr(), self._stream())
        return out

    def _queries(self, queries, k, what):
        qdt = ops.query_rows(queries, self.dim, self.device, what)
        B = queries.shape[0]
        if B > self.max_batch:
            raise ValueError(f"{what}: {B} queries exceed max_batch = {self.max_batch}")
        if len(self) == 0:
            raise ValueError(f"{what}: the gallery is empty")
        if not isinstance(k, int) or not 1 <= k <= min(len(self), self.max_topk):
            raise ValueError(f"{what}: k = {k} outside 1..min(len = {len(self)}, {self.max_topk})")
        return qdt, B

    def search(self, queries: torch.Tensor, k: int = 1, out=None, where=None):
        """The k nearest rows of each query: (idx int32 [B,k], score f32
        [B,k]), best first, equal scores by ascending id. queries: contiguous
        float32 or bfloat16 [B, dim] on this GPU, B <= max_batch. ``out``: the
        (idx, score) pair to write instead of new tensors. ``where``: an int,
        or an int [B] tensor: query b sees only rows labelled where[b] (a
        negative entry: any row). Removed rows are never returned; with
        ``where`` or after a removal a query with fewer than k candidates gets
        idx = -1, score = -inf at the ranks left over."""
        qdt, B = self._queries(queries, k, "search")
        want = None
        if where is not None:
            if isinstance(where, int) and not isinstance(where, bool):
                where = torch.full((B,), where, dtype=torch.int64)
            elif not isinstance(where, torch.Tensor):
                raise ValueError(f"search: where is an int or an int [B] tensor, got {type(where).__name__}")
            where = self._ints(where, B, "search: where")
            if B and (int(where.max()) > 2 ** 31 - 1 or int(where.min()) < -2 ** 31):
                raise ValueError("search: where outside int32")
            want = where.to(device=self.device, dtype=torch.int32).contiguous()
        idx, score = ops.topk_out(out, B, k, self.device, "search")
        self._g.search(queries.data_ptr(), qdt, B, k, idx.data_ptr(), score.data_ptr(), self._stream(),
                       q_want=0 if want is None else want.data_ptr())
        return idx, score

    def classify(self, queries: torch.Tensor, k: int = 5, weighted: bool = False, out=None):
        """k-NN labelling: (label int32 [B], share f32 [B]), the vote of each
        query's k nearest live rows (``ops.knn_vote``'s rule: weight 1 or,
        ``weighted``, max(score, 0); the largest total wins, equal totals by
        the best rank; share = the winner's part of all weights). queries as
        for ``search``; ``out``: the (label, share) pair to write."""
        qdt, B = self._queries(queries, k, "classify")
        label, share = ops.vote_out(out, B, self.device, "classify")
        self._g.classify(queries.data_ptr(), qdt, B, k, bool(weighted), label.data_ptr(), share.data_ptr(),
                         self._stream())
        return label, share
