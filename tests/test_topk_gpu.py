"""Softmax + top-k: the kernel (csrc/kernels/softmax_topk.hip, ops.softmax_topk)
and the engine path (Engine::forward_topk, InferenceEngine.predict(topk=)).

Reference: the fp64 softmax of the logits gathered at the first k columns of
a stable descending sort (torch.topk promises no order among equal values).
idx must match exactly; prob within rtol 1e-4 / atol 1e-6, test_softmax_top1's
bar for the same arithmetic. Rank 0 must be bit-equal to ops.softmax_top1.
"""
import pytest
import torch

from dmlc import ops
from dmlc.models import build, state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-6


def _reference(logits, k, n=None):
    """logits: [B, ld] on any device -> (idx int64 [B,k], prob f64 [B,k]) on the CPU over the first n columns."""
    x = logits.detach().cpu()[:, :n]
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
    return order, torch.softmax(x.double(), -1).gather(1, order)


def _check(logits, k, n=None):
    """ops.softmax_topk on device logits against the reference and against ops.softmax_top1."""
    idx, prob = ops.softmax_topk(logits, k, n)
    i1, p1 = ops.softmax_top1(logits, n)
    torch.cuda.synchronize()
    B = logits.shape[0]
    assert idx.shape == (B, k) and idx.dtype == torch.int32
    assert prob.shape == (B, k) and prob.dtype == torch.float32
    ridx, rprob = _reference(logits, k, n)
    assert torch.equal(idx.cpu().long(), ridx)
    assert not torch.isnan(prob).any()
    torch.testing.assert_close(prob.cpu().double(), rprob, rtol=RTOL, atol=ATOL)
    assert torch.equal(idx[:, 0], i1)
    assert torch.equal(prob[:, 0], p1)  # bit-equal: the same max, the same summation order
    return idx.cpu(), prob.cpu()


def _randn(B, N, seed):
    return torch.randn(B, N, generator=torch.Generator().manual_seed(seed)) * 3


# ragged last workgroup / N no multiple of 64; one lane with two values and
# the 64 / 65 boundary; k == N with most lanes empty; the last register-
# resident row length, the first rereading one, and a longer rereading row
@pytest.mark.parametrize("B,N,k", [
    (37, 1000, 5), (5, 1000, 16), (1, 1000, 1), (3, 65, 8), (2, 64, 8), (4, 5, 5), (4, 16, 16),
    (3, 1024, 16), (3, 1025, 16), (2, 4100, 16)])
def test_topk_shapes(gpu, B, N, k):
    _check(_randn(B, N, 1000 * B + N + k).to(gpu), k)


def test_topk_ignores_padding(gpu):
    N, pad = 1000, 24
    x = torch.full((6, N + pad), 1e30)
    x[:, :N] = _randn(6, N, 3)
    _check(x.to(gpu), 5, n=N)


@pytest.mark.parametrize("N", [1000, 1100])  # register-resident and rereading rows
def test_topk_one_lane_owns_all_winners(gpu, N):
    x = torch.randn(5, N, generator=torch.Generator().manual_seed(4))
    for j in range(8):
        x[:, 3 + 64 * j] = 50 - j
    idx, _ = _check(x.to(gpu), 8)
    assert idx.tolist() == [[3 + 64 * j for j in range(8)]] * 5


@pytest.mark.parametrize("N", [1000, 1100])
def test_topk_ties(gpu, N):
    zeros = torch.zeros(3, N)
    idx, prob = _check(zeros.to(gpu), 8)
    assert idx.tolist() == [list(range(8))] * 3
    torch.testing.assert_close(prob, torch.full((3, 8), 1.0 / N), rtol=RTOL, atol=ATOL)
    # 3, 67 and 131 share a lane, 900 does not
    x = torch.randn(5, N, generator=torch.Generator().manual_seed(5))
    for c in (900, 3, 67, 131):
        x[:, c] = 7.0
    idx, _ = _check(x.to(gpu), 4)
    assert idx.tolist() == [[3, 67, 131, 900]] * 5


def test_topk_magnitude(gpu):
    _check((_randn(9, 1000, 6) + 1e4).to(gpu), 5)
    x = torch.randn(4, 1000, generator=torch.Generator().manual_seed(7))
    x[:, 321] += 100  # the lower ranks' probabilities are ~e-100: 0, not NaN
    idx, prob = _check(x.to(gpu), 5)
    assert (idx[:, 0] == 321).all() and torch.equal(prob[:, 0], torch.ones(4))
    assert (prob[:, 1:] >= 0).all() and (prob[:, 1:] < 1e-30).all()


def test_topk_argument_checks(gpu):
    x = torch.zeros(2, 20, device=gpu)
    for k in (0, 17, 21):
        with pytest.raises(ValueError):
            ops.softmax_topk(x, k)
    with pytest.raises(ValueError):
        ops.softmax_topk(x[:, :8].contiguous(), 9)  # k = N + 1
    with pytest.raises(ValueError):
        ops.softmax_topk(x, 6, n=5)
    with pytest.raises(ValueError):
        ops.softmax_topk(x.bfloat16(), 5)
    with pytest.raises(ValueError):
        ops.softmax_topk(x[0], 5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- engine
# one case per tail the top-k step follows
ENGINE_CASES = [("resnet18", 4, "HeadFused"), ("resnet18", 64, "HeadPooled"), ("alexnet", 3, "SoftmaxTop1"),
                ("resnet50", 32, "HeadPooled")]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(arch):
        if arch not in cache:
            model = build(arch, seed=5) if arch == "resnet50" else calibrated(arch, seed=11)
            cache[arch] = InferenceEngine(arch, state_dict_f32(model), max_batch=64)
        return cache[arch]
    return get


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("arch,B,tail", ENGINE_CASES, ids=[f"{a}-b{b}" for a, b, _ in ENGINE_CASES])
def test_engine_topk(gpu, engines, arch, B, tail, use_graph):
    eng = engines(arch)
    kernels = [k for k, _, _, _ in eng._e.plan(B, 224, 224, topk=5)]
    assert kernels[-1] == "SoftmaxTopK" and kernels[-2] == tail
    if arch == "resnet50":
        assert kernels[-3] == "AvgPoolGlobal"
    img = mixed_images(B, seed=40 + B).to(gpu)

    # against the engine's own logits
    idx, prob, logits = eng.predict(img, topk=5, return_logits=True, use_graph=use_graph)
    torch.cuda.synchronize()
    assert idx.shape == (B, 5) and idx.dtype == torch.int32 and prob.shape == (B, 5) and prob.dtype == torch.float32
    ridx, rprob = _reference(logits, 5)
    assert torch.equal(idx.cpu().long(), ridx)
    torch.testing.assert_close(prob.cpu().double(), rprob, rtol=RTOL, atol=ATOL)

    # without a logits buffer (the step reads the logits activation)
    idx_n, prob_n = eng.predict(img, topk=5, use_graph=use_graph)
    torch.cuda.synchronize()
    assert torch.equal(idx_n, idx)
    torch.testing.assert_close(prob_n, prob, rtol=1e-5, atol=0)

    # against topk = 1
    i1, p1 = eng.predict(img, use_graph=use_graph)
    i1k, p1k = eng.predict(img, topk=1, use_graph=use_graph)
    torch.cuda.synchronize()
    assert i1.shape == (B,) and p1.shape == (B,) and i1k.shape == (B,) and p1k.shape == (B,)
    assert torch.equal(i1k, i1) and torch.equal(p1k, p1)
    assert torch.equal(idx_n[:, 0], i1)
    torch.testing.assert_close(prob_n[:, 0], p1, rtol=1e-5, atol=0)


@pytest.mark.parametrize("arch,B", [("resnet18", 4), ("alexnet", 3)])
def test_engine_topk_graph_key(gpu, engines, arch, B):
    """Same images, same idx / prob pointers, another k: never the other k's graph."""
    eng = engines(arch)
    img = mixed_images(B, seed=50 + B).to(gpu)
    fresh = {k: eng.predict(img, topk=k) for k in (5, 3)}
    torch.cuda.synchronize()
    fresh = {k: (i.clone(), p.clone()) for k, (i, p) in fresh.items()}
    fi = torch.empty(B * 8, dtype=torch.int32, device=gpu)
    fp = torch.empty(B * 8, dtype=torch.float32, device=gpu)
    for k in (5, 3, 5):
        fi.fill_(-1)
        fp.fill_(-1)
        out = (fi[:B * k].view(B, k), fp[:B * k].view(B, k))
        assert out[0].data_ptr() == fi.data_ptr() and out[1].data_ptr() == fp.data_ptr()
        idx, prob = eng.predict(img, out=out, topk=k)
        torch.cuda.synchronize()
        assert idx.data_ptr() == fi.data_ptr()
        assert torch.equal(idx, fresh[k][0]), k
        assert torch.equal(prob, fresh[k][1]), k
        assert (fi[B * k:] == -1).all() and (fp[B * k:] == -1).all()  # nothing past [B, k]


def test_engine_topk_argument_checks(gpu, engines):
    eng = engines("alexnet")
    B = 3
    img = mixed_images(B, seed=60).to(gpu)
    for k in (0, 17):
        with pytest.raises(ValueError):
            eng.predict(img, topk=k)
    flat = (torch.empty(B, dtype=torch.int32, device=gpu), torch.empty(B, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        eng.predict(img, out=flat, topk=5)
    wrong = (torch.empty(B, 5, dtype=torch.int64, device=gpu), torch.empty(B, 5, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        eng.predict(img, out=wrong, topk=5)
    strided = (torch.empty(B, 10, dtype=torch.int32, device=gpu)[:, ::2],
               torch.empty(B, 5, dtype=torch.float32, device=gpu))
    with pytest.raises(ValueError):
        eng.predict(img, out=strided, topk=5)
    # topk > num_classes, below MAX_TOPK (the engine takes class counts that are multiples of 4: 12, not 10)
    small = InferenceEngine("resnet18", None, max_batch=2, num_classes=12)
    with pytest.raises(ValueError):
        small.predict(img[:2], topk=13)
    with pytest.raises(ValueError):  # the native check, past the Python one
        small._e.forward_topk(img.data_ptr(), 2, 224, 224, 13, flat[0].data_ptr(), flat[1].data_ptr(), 0,
                              torch.cuda.current_stream().cuda_stream, False)
    idx, prob, logits = small.predict(img[:2], topk=12, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu().long(), _reference(logits, 12)[0])
    torch.testing.assert_close(prob.sum(-1).cpu(), torch.ones(2), rtol=1e-5, atol=0)
