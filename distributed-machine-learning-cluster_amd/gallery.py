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
    workspace for ``max_batch`` queries included, is allocated here."""

    def __init__(self, dim: int, capacity: int, device: int = 0, metric: str = "cosine", max_batch: int = 256):
        require_gpu()
        if metric not in ("cosine", "dot"):
            raise ValueError(f"metric is 'cosine' or 'dot', got {metric!r}")
        self.device = torch.device("cuda", device)
        self._g = native().Gallery(dim, capacity, device, metric, max_batch)
        self.dim, self.capacity, self.metric, self.max_batch = dim, capacity, metric, max_batch
        self.max_topk = native().MAX_TOPK

    def __len__(self) -> int:
        return self._g.size

    def clear(self) -> None:
        """Forget every row; the next ``add`` starts at id 0 again."""
        self._g.clear()

    def add(self, features: torch.Tensor) -> range:
        """Append contiguous float32 [M, dim] rows on this gallery's GPU (what
        ``InferenceEngine.embed`` returns); the new rows' ids."""
        if features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] != self.dim \
                or features.device != self.device or not features.is_contiguous():
            raise ValueError(f"add: expected contiguous torch.float32 [M,{self.dim}] on {self.device}, got "
                             f"{features.dtype} {tuple(features.shape)} on {features.device}")
        M = features.shape[0]
        if len(self) + M > self.capacity:
            raise ValueError(f"add: {len(self)} + {M} rows exceed the capacity {self.capacity}")
        first = self._g.add(features.data_ptr(), M, torch.cuda.current_stream(self.device).cuda_stream)
        return range(first, first + M)

    def search(self, queries: torch.Tensor, k: int = 1, out=None):
        """The k nearest rows of each query: (idx int32 [B,k], score f32
        [B,k]), best first, equal scores by ascending id. queries: contiguous
        float32 or bfloat16 [B, dim] on this GPU, B <= max_batch. ``out``: the
        (idx, score) pair to write instead of new tensors."""
        qdt = ops.query_rows(queries, self.dim, self.device, "search")
        B = queries.shape[0]
        if B > self.max_batch:
            raise ValueError(f"search: {B} queries exceed max_batch = {self.max_batch}")
        if len(self) == 0:
            raise ValueError("search: the gallery is empty")
        if not isinstance(k, int) or not 1 <= k <= min(len(self), self.max_topk):
            raise ValueError(f"search: k = {k} outside 1..min(len = {len(self)}, {self.max_topk})")
        idx, score = ops.topk_out(out, B, k, self.device, "search")
        self._g.search(queries.data_ptr(), qdt, B, k, idx.data_ptr(), score.data_ptr(),
                       torch.cuda.current_stream(self.device).cuda_stream)
        return idx, score
