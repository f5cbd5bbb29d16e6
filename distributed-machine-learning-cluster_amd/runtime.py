"""GPU inference engine (Python face of csrc/runtime/engine.cpp).

Reference counterpart: ``Member::predict`` (src/services.rs:475-497) — one
image per call, CPU libtorch, model mutex. Here one call classifies a whole
batch of u8 images already resident in HBM: on-device preprocess, the
hand-written MFMA conv stack, fused softmax+top-1, all replayed from a
hipGraph captured on first use.
"""
from __future__ import annotations

import torch

from . import native, ops
from .models import build, state_dict_f32


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("dmlc GPU engine needs a ROCm GPU (torch.cuda.is_available() is False)")


class InferenceEngine:
    """Batched classifier on one GPU.

    weights: None (random init of ``arch`` with ``seed``), a state dict, or a
    path to a ``.ot`` checkpoint. options: kernel-path switches by name
    (csrc/runtime/engine.h EngineOptions, e.g. {"fused_block": False}); the
    defaults are the fastest measured paths.
    """

    def __init__(self, arch: str = "resnet18", weights=None, device: int = 0, max_batch: int = 256,
                 num_classes: int = 1000, image_size: int = 224, seed: int = 0, options: dict | None = None):
        require_gpu()
        C = native()
        self.arch = arch
        self.device = torch.device("cuda", device)
        if isinstance(weights, str):
            self._e = C.Engine.from_ot(arch, weights, device, num_classes, image_size, dict(options or {}))
        else:
            sd = weights if weights is not None else state_dict_f32(build(arch, num_classes, seed=seed))
            self._e = C.Engine(arch, {k: v.detach().cpu().float().numpy() for k, v in sd.items()},
                               device, num_classes, image_size, dict(options or {}))
        self._e.reserve(max_batch)
        self.max_batch = max_batch
        self.num_classes = num_classes
        self.image_size = image_size
        self.max_topk = min(num_classes, C.MAX_TOPK)  # largest predict(topk=)
        # length of the vector the last fc reads: 512 (ResNet18/34), 2048 (ResNet50), 4096 (AlexNet)
        self.feature_dim = self._e.feature_dim
        self._scratch = None  # embed(): idx / prob nobody reads
        self._features = None  # index() / search(): the embeddings on their way to a gallery

    @property
    def gflop_per_image(self) -> float:
        return self._e.gflop_per_image

    @property
    def weight_bytes(self) -> int:
        return self._e.weight_bytes

    def predict(self, images: torch.Tensor, use_graph: bool = True, out=None, return_logits: bool = False,
                topk: int = 1, return_features: bool = False, normalize_features: bool = False):
        """images: uint8 [B,H,W,3] on this engine's GPU. Returns (idx int32 [B],
        prob f32 [B]) (+ logits f32 [B,num_classes] if return_logits). topk > 1:
        idx and prob are [B,topk], the best classes in descending order (equal
        logits by ascending class), and ``out`` must be contiguous tensors of
        that shape; 1 <= topk <= min(num_classes, MAX_TOPK).

        images may instead be a float32 / float16 / bfloat16 tensor
        [B,3,image_size,image_size], contiguous or ``torch.channels_last``: the
        tensor a torch model takes. It is used as given (rounded to bf16): the
        caller resizes and normalises, with whatever mean/std the weights were
        trained with. topk, out, return_logits and use_graph work the same.

        return_features: ``features`` f32 [B,feature_dim] is appended to the
        returned tuple (after logits): the vector the last fc reads, i.e. the
        pooled feature of a ResNet or AlexNet's ``classifier.4`` output, widened
        from the bf16 the fc multiplies; normalize_features: each row scaled to
        unit L2 norm (``F.normalize``). One more kernel after the forward's
        own; idx, prob and logits are the same bits with and without it."""
        if normalize_features and not return_features:
            raise ValueError("normalize_features needs return_features")
        feats = (None, bool(normalize_features)) if return_features else None
        return self._predict(images, use_graph, out, return_logits, topk, feats)

    def embed(self, images: torch.Tensor, normalize: bool = False, use_graph: bool = True,
              out: torch.Tensor | None = None) -> torch.Tensor:
        """The ``features`` of ``predict(images, return_features=True,
        normalize_features=normalize)`` alone: f32 [B,feature_dim]. images as
        for ``predict``. ``out``: a contiguous float32 [B,feature_dim] tensor
        on this engine's GPU to write instead of a new one. The forward's class
        answer goes to a scratch pair."""
        B = images.shape[0]
        if out is not None and (out.device != self.device or out.dtype != torch.float32
                                or tuple(out.shape) != (B, self.feature_dim) or not out.is_contiguous()):
            raise ValueError(f"out: expected contiguous torch.float32 [{B},{self.feature_dim}] on {self.device}, got "
                             f"{out.dtype} {tuple(out.shape)} on {out.device}")
        if self._scratch is None:
            self._scratch = (torch.empty(self.max_batch, dtype=torch.int32, device=self.device),
                             torch.empty(self.max_batch, dtype=torch.float32, device=self.device))
        answer = (self._scratch[0][:B], self._scratch[1][:B])
        return self._predict(images, use_graph, answer, False, 1, (out, bool(normalize)))[-1]

    def _check_gallery(self, gallery, what: str) -> None:
        if getattr(gallery, "dim", None) != self.feature_dim or getattr(gallery, "device", None) != self.device:
            raise ValueError(f"{what}: expected a dmlc.Gallery of dim {self.feature_dim} on {self.device}, got dim "
                             f"{getattr(gallery, 'dim', None)} on {getattr(gallery, 'device', None)}")

    def index(self, images: torch.Tensor, gallery, use_graph: bool = True, labels=None) -> range:
        """``gallery.add(self.embed(images), labels)``: store the images'
        embeddings in a ``dmlc.Gallery`` of this engine's ``feature_dim`` on
        this GPU; the new rows' ids. images as for ``predict``."""
        self._check_gallery(gallery, "index")
        return gallery.add(self._embed_into_buffer(images, use_graph), labels)

    def search(self, images: torch.Tensor, gallery, k: int = 1, use_graph: bool = True, out=None, where=None):
        """The k stored rows nearest to each image: ``gallery.search(
        self.embed(images), k)``, the same bits, with the embeddings in a
        buffer the engine keeps and the search launched on the same stream
        after the forward (whose plan and graphs are what ``embed`` uses).
        ``where``: ``Gallery.search``'s label filter. Returns (idx int32
        [B,k], score f32 [B,k])."""
        self._check_gallery(gallery, "search")
        return gallery.search(self._embed_into_buffer(images, use_graph), k, out, where)

    def classify_knn(self, images: torch.Tensor, gallery, k: int = 5, weighted: bool = False, use_graph: bool = True,
                     out=None):
        """k-NN labelling against a gallery: ``gallery.classify(
        self.embed(images), k, weighted)``, the same bits. Returns (label
        int32 [B], share f32 [B])."""
        self._check_gallery(gallery, "classify_knn")
        return gallery.classify(self._embed_into_buffer(images, use_graph), k, weighted, out)

    def _embed_into_buffer(self, images, use_graph):
        B = images.shape[0]
        if B > self.max_batch:
            raise ValueError(f"{B} images exceed max_batch = {self.max_batch}")
        if self._features is None:
            self._features = torch.empty(self.max_batch, self.feature_dim, dtype=torch.float32, device=self.device)
        return self.embed(images, use_graph=use_graph, out=self._features[:B])

    def _predict(self, images, use_graph, out, return_logits, topk, feats):
        """feats: None, or (features buffer or None for a new one, normalise)."""
        if images.is_floating_point():
            if images.device != self.device:
                raise ValueError(f"expected a float tensor on {self.device}, got one on {images.device}")
            dt, channels_last = ops.tensor_input(images, self.image_size)
            return self._forward(("tensor", images.data_ptr(), dt, channels_last), images.shape[0], use_graph, out,
                                 return_logits, topk, feats)
        if images.device != self.device or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"expected uint8 [B,H,W,3] on {self.device}, got {images.dtype} {tuple(images.shape)} "
                             f"on {images.device}")
        if not images.is_contiguous():
            raise ValueError("images must be contiguous")
        B, H, W, _ = images.shape
        return self._forward(("u8", images.data_ptr(), H, W), B, use_graph, out, return_logits, topk, feats)

    def _forward(self, src, B, use_graph, out, return_logits, topk, feats=None):
        if not isinstance(topk, int) or not 1 <= topk <= self.max_topk:
            raise ValueError(f"topk = {topk} outside 1..{self.max_topk}")
        if out is None:
            shape = (B,) if topk == 1 else (B, topk)
            idx = torch.empty(shape, dtype=torch.int32, device=self.device)
            prob = torch.empty(shape, dtype=torch.float32, device=self.device)
        else:
            idx, prob = out
            if topk > 1:
                for t, dt in ((idx, torch.int32), (prob, torch.float32)):
                    if (t.device != self.device or t.dtype != dt or tuple(t.shape) != (B, topk)
                            or not t.is_contiguous()):
                        raise ValueError(f"out: expected contiguous {dt} [{B},{topk}] on {self.device}, got "
                                         f"{t.dtype} {tuple(t.shape)} on {t.device}")
        logits = torch.empty(B, self.num_classes, dtype=torch.float32, device=self.device) if return_logits else None
        features, l2norm = None, False
        if feats is not None:
            features, l2norm = feats
            if features is None:
                features = torch.empty(B, self.feature_dim, dtype=torch.float32, device=self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        lp = 0 if logits is None else logits.data_ptr()
        fp = 0 if features is None else features.data_ptr()
        if src[0] == "tensor":
            _, ptr, dt, channels_last = src
            self._e.forward_tensor(ptr, dt, channels_last, B, topk, idx.data_ptr(), prob.data_ptr(), lp, stream,
                                   use_graph, fp, l2norm)
        else:  # positionally: keyword arguments cost a batch-1 query most of a microsecond in the binding
            _, ptr, H, W = src
            self._e.forward_topk(ptr, B, H, W, topk, idx.data_ptr(), prob.data_ptr(), lp, stream, use_graph, fp, l2norm)
        return tuple(t for t in (idx, prob, logits, features) if t is not None)

    def profile(self, images: torch.Tensor) -> list[tuple[str, float]]:
        """Per-op GPU time (ms) of one eager forward (hipEvent pairs)."""
        B, H, W, _ = images.shape
        return self._e.profile(images.data_ptr(), B, H, W, torch.cuda.current_stream(self.device).cuda_stream)
