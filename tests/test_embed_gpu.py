"""Penultimate-layer embeddings: the kernel (csrc/kernels/embed.hip,
ops.embed_rows) and the engine path (Engine::forward_topk / forward_tensor
with a features buffer, InferenceEngine.predict(return_features=) / embed()).

Kernel. The plain output is exact by construction, so it is compared bit for
bit: with x.float() for rows (HW == 1), with ops.avgpool_global for bf16
images, and with a CPU emulation in torch fp32 that performs avgpool_global's
stated order literally (part p = pixels p, p + 8, ... summed in order onto 0,
the parts combined as ((0+1)+(2+3))+((4+5)+(6+7)), one multiply by
(scale or 1) / HW, rounded to bf16). A reference pooled in plain pixel order
must be rejected by the same comparison. The normalised output is compared
with float64 on the kernel's own plain output v: rtol = C 2^-24, atol = 0.
That is the first-order worst case of an fp32 sum of C non-negative terms in
any order; the square root halves it, and the other half covers the roundings
of the squares, the root and the quotient (about 3 2^-24 together).

Engine. The features are (1) bit-equal to the vector the engine itself holds
or would have pooled, (2) what the fc reads: the logits of the same forward
lie within K 2^-23 mag (tests/_kernel_bar.py's summation term; the output is
fp32 and the operand rounding is already in the features) of the float64 fc
of the returned features with the bf16-rounded fc weights, (3) within the
project's whole-model bf16 bar, 3e-2 relative L2, of the fp32 model's
penultimate features on images with >= 8 distinct fp32 top-1 classes, where a
batch rolled by one image misses that bar, (4) leave idx, prob and logits bit
for bit as they are without them, (5) never replay another forward's graph,
and (6) are what embed() returns.
"""
import pytest
import torch

from _kernel_bar import bound, fc_ref
from dmlc import native, ops
from dmlc.models import build, penultimate_features, state_dict_f32
from dmlc.models.calibrated import calibrated, mixed_images, normalize
from dmlc.runtime import InferenceEngine

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 64  # sentinel elements past [B, C]

# (B, HW, C, e4m3 scale or None): one lane of one wave; rows of 2, 1 and 4
# groups per lane (4096 = 2 x 256 x 8, 8192 the widest) with an odd batch; the
# engine's pooled shapes below and above avgpool_global's B = 32 switch; HW no
# multiple of 8 or 24 with a part-filled wave (C = 64); e4m3 at the engine's
# shape and with a partial last block of pixels (36 = 24 + 12)
KERNEL_CASES = [(1, 1, 8, None), (3, 1, 4096, None), (37, 1, 2048, None), (2, 1, 8192, None), (5, 49, 512, None),
                (33, 49, 512, None), (31, 50, 64, None), (2, 49, 2048, 0.37), (40, 36, 256, 1.0 / 7)]


def _case_id(c):
    B, HW, C, scale = c
    return f"b{B}-hw{HW}-c{C}" + ("-e4m3" if scale is not None else "")


def _input(B, HW, C, scale, seed, cancelling=False):
    """CPU input of a case: bf16 randn, or random e4m3 bytes without the two NaN encodings.

    fp32 sums of 49 bf16 randn values (8 significant bits within a few binades) are exact, and so are sums of
    e4m3 values: every summation order gives the same bits. cancelling: pixel 0 scaled by 2^20 and pixel 9 its
    negative, so the small pixels added in between lose low bits to the large one before it cancels, and the
    result depends on the order well above a bf16 ulp."""
    g = torch.Generator().manual_seed(seed)
    if scale is None:
        x = torch.randn(B, HW, C, generator=g).bfloat16()
        if cancelling:
            x[:, 0] *= 2.0 ** 20
            x[:, 9] = -x[:, 0]
        return x[:, 0].contiguous() if HW == 1 else x
    b = torch.randint(0, 256, (B, HW, C), dtype=torch.uint8, generator=g)
    b[(b & 0x7F) == 0x7F] = 0x38  # 0x7f / 0xff are NaN: 1.0 instead
    return b


def _widen(x_cpu):
    return x_cpu.view(ops.FP8).float() if x_cpu.dtype == torch.uint8 else x_cpu.float()


def _pool_emulated(xf, scale, sequential=False):
    """avgpool_global's order in torch fp32 on the CPU. xf: fp32 [B, HW, C]. sequential: plain pixel order instead."""
    B, HW, C = xf.shape
    parts = []
    for p in range(1 if sequential else 8):
        s = torch.zeros(B, C, dtype=torch.float32)
        for i in range(p, HW, 1 if sequential else 8):
            s = s + xf[:, i]
        parts.append(s)
    tot = parts[0] if sequential else \
        ((parts[0] + parts[1]) + (parts[2] + parts[3])) + ((parts[4] + parts[5]) + (parts[6] + parts[7]))
    inv = torch.tensor(1.0 if scale is None else scale, dtype=torch.float32) / torch.tensor(float(HW))
    return (tot * inv).bfloat16().float()


def _embed_with_tail(x, normalize, scale):
    """ops.embed_rows into a buffer with a sentinel tail; the tail must stay untouched."""
    B, C = x.shape[0], x.shape[-1]
    buf = torch.full((B * C + PAD,), SENTINEL, dtype=torch.float32, device=x.device)
    out = ops.embed_rows(x, normalize=normalize, scale=scale, out=buf[:B * C].view(B, C))
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr()
    assert (buf[B * C:] == SENTINEL).all()
    return out


def _assert_normalised(got, v):
    """got = normalised rows of the kernel's own plain output v: float64 reference, rtol C 2^-24, atol 0."""
    C = v.shape[1]
    v64 = v.double().cpu()
    ref = v64 / v64.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    err = (got.double().cpu() - ref).abs()
    assert not torch.isnan(got).any()
    worst = (err / ref.abs().clamp_min(1e-300)).max().item() / (C * 2.0 ** -24)
    print(f"normalised: worst |err| / (C 2^-24 |ref|) = {worst:.3f}")
    assert (err <= C * 2.0 ** -24 * ref.abs()).all(), worst


@pytest.mark.parametrize("case", KERNEL_CASES, ids=_case_id)
def test_embed_rows(gpu, case):
    B, HW, C, scale = case
    x_cpu = _input(B, HW, C, scale, seed=1000 * B + HW + C)
    x = x_cpu.to(gpu)
    v = _embed_with_tail(x, False, scale)
    assert v.shape == (B, C) and v.dtype == torch.float32
    if HW == 1:
        assert torch.equal(v, x.float())
    else:
        assert torch.equal(v.cpu(), _pool_emulated(_widen(x_cpu), scale))
        if scale is None:  # both of avgpool_global's kernels (B < 32 and B >= 32 across the cases)
            assert torch.equal(v, ops.avgpool_global(x.view(B, HW, 1, C)).float())
    _assert_normalised(_embed_with_tail(x, True, scale), v)
    if HW > 1 and scale is None:  # an input whose mean depends on the summation order
        x_cpu = _input(B, HW, C, None, seed=1000 * B + HW + C, cancelling=True)
        x = x_cpu.to(gpu)
        v = _embed_with_tail(x, False, None)
        assert torch.equal(v.cpu(), _pool_emulated(x_cpu.float(), None))
        assert torch.equal(v, ops.avgpool_global(x.view(B, HW, 1, C)).float())


def test_embed_rows_rejects_sequential_pooling(gpu):
    """The negative control of the bit comparison: the same mean summed in plain pixel order differs."""
    B, HW, C = 5, 49, 512
    x_cpu = _input(B, HW, C, None, seed=1000 * B + HW + C, cancelling=True)
    seq = _pool_emulated(x_cpu.float(), None, sequential=True)
    differ = (seq != _pool_emulated(x_cpu.float(), None)).float().mean().item()
    assert differ > 0.5, differ  # (76 % of the elements for this seed; none without the cancelling pixels)
    v = ops.embed_rows(x_cpu.to(gpu))
    torch.cuda.synchronize()
    assert not torch.equal(v.cpu(), seq)
    assert torch.equal(v.cpu(), _pool_emulated(x_cpu.float(), None))


def test_embed_rows_zero_row(gpu):
    for HW, C in ((1, 512), (49, 512)):
        x = torch.randn(6, HW, C, generator=torch.Generator().manual_seed(HW)).bfloat16()
        x[2] = 0
        x = (x[:, 0].contiguous() if HW == 1 else x).to(gpu)
        out = _embed_with_tail(x, True, None)
        assert not torch.isnan(out).any() and not torch.isinf(out).any()
        assert (out[2] == 0).all()
        norms = out.double().norm(dim=-1).cpu()
        assert norms[2] == 0 and ((norms[[0, 1, 3, 4, 5]] - 1).abs() <= C * 2.0 ** -24).all()


def test_embed_rows_argument_checks(gpu):
    bf = torch.zeros(2, 64, dtype=torch.bfloat16, device=gpu)
    u8 = torch.zeros(2, 4, 64, dtype=torch.uint8, device=gpu)
    bad = [
        lambda: ops.embed_rows(bf.float()),                          # dtype
        lambda: ops.embed_rows(bf.half()),
        lambda: ops.embed_rows(bf[0]),                               # rank
        lambda: ops.embed_rows(bf.view(1, 2, 8, 8)),
        lambda: ops.embed_rows(u8[:, 0], scale=1.0),                 # e4m3 rows
        lambda: ops.embed_rows(torch.zeros(2, 12, dtype=torch.bfloat16, device=gpu)),  # C % 8
        lambda: ops.embed_rows(torch.zeros(2, 3, 12, dtype=torch.uint8, device=gpu), scale=1.0),
        lambda: ops.embed_rows(torch.zeros(1, 8200, dtype=torch.bfloat16, device=gpu)),  # C > 8192
        lambda: ops.embed_rows(u8),                                  # e4m3 without its scale
        lambda: ops.embed_rows(bf, out=torch.empty(2, 64, dtype=torch.float64, device=gpu)),
        lambda: ops.embed_rows(bf, out=torch.empty(2, 128, device=gpu)[:, ::2]),
        lambda: ops.embed_rows(bf, out=torch.empty(3, 64, device=gpu)),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):  # the native check, past the Python one
        native().embed_rows(bf.data_ptr(), torch.empty(2, 12, device=gpu).data_ptr(), 2, 1, 12, False, 1.0, False, 0)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- engine
# (arch, B, the plan's tail before Embed): the pooling form, the epilogue-pooled row, the AvgPoolGlobal row,
# AlexNet's classifier.4, the e4m3 pooling form
ENGINE_CASES = [("resnet18", 4, ["HeadFused"]), ("resnet18", 64, ["None", "HeadPooled"]),
                ("resnet50", 32, ["AvgPoolGlobal", "HeadPooled"]), ("alexnet", 3, ["SoftmaxTop1"]),
                ("resnet50_fp8", 4, ["HeadFused"])]
ENGINE_IDS = [f"{a}-b{b}" for a, b, _ in ENGINE_CASES]


@pytest.fixture(scope="module")
def engines():
    """key -> (fp32 model, engine), max_batch 64. resnet18 / alexnet: calibrated(seed=11); the resnet50s:
    build(seed=5), one model for both; "resnet50:calibrated": the discriminating model of the fp32 comparison."""
    models, cache = {}, {}

    def get(key):
        if key not in cache:
            arch, _, how = key.partition(":")
            mkey = (arch.replace("_fp8", ""), how)
            if mkey not in models:
                models[mkey] = build(mkey[0], seed=5) if mkey == ("resnet50", "") else calibrated(mkey[0], seed=11)
            cache[key] = (models[mkey], InferenceEngine(arch, state_dict_f32(models[mkey]), max_batch=64))
        return cache[key]
    return get


def _fc(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.Linear)][-1]


def _read(eng, act, B, dtype):
    """The first B images of a stored activation: [B, H * W, C]."""
    H, W, C, f32 = eng._e.activation_shape(act)
    assert not f32
    t = torch.empty(B, H * W, C, dtype=dtype, device=eng.device)
    eng._e.read_activation(act, B, t.data_ptr(), torch.cuda.current_stream(eng.device).cuda_stream)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("arch,B,tail", ENGINE_CASES, ids=ENGINE_IDS)
def test_engine_features(gpu, engines, arch, B, tail, use_graph):
    model, eng = engines(arch)
    D = eng.feature_dim
    assert D == _fc(model).in_features
    plan = eng._e.plan(B, 224, 224, features=True)
    kernels = [k for k, _, _, _ in plan]
    assert kernels[-1] == "Embed" and kernels[-1 - len(tail):-1] == tail and kernels.count("Embed") == 1
    assert plan[:-1] == eng._e.plan(B, 224, 224)
    img = mixed_images(B, seed=40 + B).to(gpu)

    idx, prob, logits, feats = eng.predict(img, return_logits=True, return_features=True, use_graph=use_graph)
    torch.cuda.synchronize()
    assert feats.shape == (B, D) and feats.dtype == torch.float32 and feats.is_contiguous()
    assert not torch.isnan(feats).any() and feats.abs().max() > 0

    # 1. the engine's own vector, after an eager forward (which stores every activation)
    eng.predict(img, use_graph=False)
    ops_ = eng._e.op_list()
    (fc,) = [op for op in ops_ if op[2] == ops_[-1][1]]
    detail = dict(f.split("=") for f in plan[-1][3].split())
    if tail == ["HeadFused"]:
        (pool,) = [op for op in ops_ if op[0] == "avgpool"]
        (src,) = [op for op in ops_ if op[2] == pool[1]]
        assert detail == {"in": src[0], "hw": "49"}
        fp8, scale = eng._e.activation_quant(pool[1])
        assert fp8 == arch.endswith("_fp8")
        H, W, C, _ = eng._e.activation_shape(pool[1])
        assert (H * W, C) == (49, D)
        if fp8:
            act = _read(eng, pool[1], B, torch.uint8)
            assert torch.equal(feats, ops.embed_rows(act, scale=scale))
            assert torch.equal(feats.cpu(), _pool_emulated(_widen(act.cpu()), scale))
        else:
            act = _read(eng, pool[1], B, torch.bfloat16)
            assert torch.equal(feats, ops.embed_rows(act))
            assert torch.equal(feats, ops.avgpool_global(act.view(B, H, W, C)).float())
    else:
        (src,) = [op for op in ops_ if op[2] == fc[1]]
        assert detail == {"in": src[0]}
        act = _read(eng, fc[1], B, torch.bfloat16)
        assert act.shape == (B, 1, D)
        assert torch.equal(feats, act[:, 0].float())

    # 2. what the fc reads: the forward's logits against the float64 fc of the features. The fc has no BN
    # to fold; its weights are packed as bf16 for the e4m3 arch too (no alpha region: the head stays bf16)
    if arch.endswith("_fp8"):
        sd = {k: v.numpy() for k, v in state_dict_f32(model).items()}
        regions, _ = native().pack_audit(arch, sd)
        assert {kind for layer, kind, _, _ in regions if layer == "fc"} == {"w", "b"}
    lin = _fc(model)
    ref, mag = fc_ref(feats.cpu(), lin.weight.detach().bfloat16(), lin.bias.detach())
    bar = bound(ref, mag, D, out_bf16=False)
    err = (logits.double().cpu() - ref).abs()
    print(f"{arch} b{B}: logits vs fp64 fc of the features, worst |err| / bar = {(err / bar).max().item():.3f}")
    assert (err <= bar).all(), (err / bar).max().item()

    # 6. embed()
    assert torch.equal(eng.embed(img, use_graph=use_graph), feats)
    fn = eng.predict(img, return_features=True, normalize_features=True, use_graph=use_graph)[-1]
    assert torch.equal(eng.embed(img, normalize=True, use_graph=use_graph), fn)
    torch.cuda.synchronize()
    _assert_normalised(fn, feats)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("arch,B,tail", ENGINE_CASES, ids=ENGINE_IDS)
def test_engine_features_move_nothing_else(gpu, engines, arch, B, tail, use_graph):
    """4. idx, prob and logits are the same bits with and without features: topk 1 and 5, u8 and fp32 tensors."""
    _, eng = engines(arch)
    u8 = mixed_images(B, seed=40 + B)
    for img in (u8.to(gpu), normalize(u8).to(gpu)):
        for k in (1, 5):
            base = eng.predict(img, topk=k, return_logits=True, use_graph=use_graph)
            plain = eng.predict(img, topk=k, return_logits=True, return_features=True, use_graph=use_graph)
            norm = eng.predict(img, topk=k, return_logits=True, return_features=True, normalize_features=True,
                               use_graph=use_graph)
            torch.cuda.synchronize()
            assert len(base) == 3 and len(plain) == 4 and len(norm) == 4
            for got in (plain, norm):
                for a, b in zip(base, got):
                    assert torch.equal(a, b), (k, img.dtype)
            _assert_normalised(norm[3], plain[3])
    # the same features from both kinds of input only where the packed image is the same: not asserted


REFERENCE_CASES = [("resnet18", 16, "HeadFused"), ("resnet18", 32, "HeadPooled"), ("resnet50:calibrated", 32, "HeadPooled"),
                   ("alexnet", 16, "SoftmaxTop1")]


@pytest.mark.parametrize("key,B,tail", REFERENCE_CASES, ids=[f"{k.split(':')[0]}-b{b}" for k, b, _ in REFERENCE_CASES])
def test_engine_features_match_fp32(gpu, engines, key, B, tail):
    """3. against the fp32 model's penultimate features, on a discriminating batch."""
    model, eng = engines(key)
    assert eng._e.plan(B, 224, 224, features=True)[-2][0] == tail
    img = mixed_images(B, seed=70 + B)
    x = normalize(img)
    with torch.no_grad():
        n_cls = len(set(model(x).argmax(-1).tolist()))
    ref = penultimate_features(model, x)
    feats = eng.embed(img.to(gpu)).cpu()
    rel = ((feats - ref).norm() / ref.norm()).item()
    rolled = ((feats.roll(1, 0) - ref).norm() / ref.norm()).item()
    print(f"{key} b{B}: {n_cls} fp32 top-1 classes, features rel L2 {rel:.4f} (rolled {rolled:.3f})")
    assert n_cls >= 8, n_cls
    assert rel <= 3e-2, rel
    assert rolled > 3e-2, rolled


@pytest.mark.parametrize("arch,B", [("resnet18", 4), ("resnet18", 64), ("alexnet", 3)])
def test_engine_features_graph_key(gpu, engines, arch, B):
    """5. same images, same idx / prob / logits / features pointers: plain, normalised, no features, plain."""
    _, eng = engines(arch)
    D = eng.feature_dim
    img = mixed_images(B, seed=50 + B).to(gpu)
    i0, p0, l0, plain = eng.predict(img, return_logits=True, return_features=True)
    normed = eng.predict(img, return_features=True, normalize_features=True)[-1]
    torch.cuda.synchronize()
    assert not torch.equal(plain, normed)
    norms = normed.double().norm(dim=-1).cpu()
    assert ((norms - 1).abs() <= D * 2.0 ** -24).all(), norms
    idx = torch.empty(B, dtype=torch.int32, device=gpu)
    prob = torch.empty(B, dtype=torch.float32, device=gpu)
    logits = torch.empty(B, eng.num_classes, dtype=torch.float32, device=gpu)
    fbuf = torch.empty(B * D + PAD, dtype=torch.float32, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for want in ("plain", "normalised", "none", "plain"):
        idx.fill_(-1)
        prob.fill_(-1)
        logits.fill_(SENTINEL)
        fbuf.fill_(SENTINEL)
        eng._e.forward_topk(img.data_ptr(), B, 224, 224, 1, idx.data_ptr(), prob.data_ptr(), logits.data_ptr(), stream,
                            True, features=0 if want == "none" else fbuf.data_ptr(), l2norm=want == "normalised")
        torch.cuda.synchronize()
        assert torch.equal(idx, i0) and torch.equal(prob, p0) and torch.equal(logits, l0), want
        got = fbuf[:B * D].view(B, D)
        if want == "none":
            assert (got == SENTINEL).all()
        else:
            assert torch.equal(got, plain if want == "plain" else normed), want
        assert (fbuf[B * D:] == SENTINEL).all(), want


def test_engine_embed_argument_checks(gpu, engines):
    _, eng = engines("alexnet")
    B, D = 3, eng.feature_dim
    img = mixed_images(B, seed=60).to(gpu)
    out = torch.empty(B, D, device=gpu)
    got = eng.embed(img, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(out, eng.predict(img, return_features=True)[-1])
    for bad in (torch.empty(B, D), torch.empty(B, D, dtype=torch.float64, device=gpu),
                torch.empty(B, D, dtype=torch.bfloat16, device=gpu), torch.empty(B + 1, D, device=gpu),
                torch.empty(B, D + 8, device=gpu), torch.empty(B * D, device=gpu),
                torch.empty(B, 2 * D, device=gpu)[:, ::2], torch.empty(D, B, device=gpu).t()):
        with pytest.raises(ValueError):
            eng.embed(img, out=bad)
    with pytest.raises(ValueError):
        eng.predict(img, normalize_features=True)
    torch.cuda.synchronize()
