"""Rotary-embedding and SwiGLU kernels (csrc/decoder.hip) against float64 math on the same bf16 inputs.

Tolerance: the kernels do fp32 math and ONE bf16 rounding -- half a bf16 ulp (2**-8 relative) plus
fp32 cancellation noise (in x1*cos - x2*sin, and near silu'(g) = 0 at g = -1.278) below 1e-5 for
unit-scale data -- so rtol = 2**-7, atol = 1e-4 holds with a factor two to spare, while a
composition that rounds to bf16 between steps does not.  Every element is checked."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL, ATOL = 2 ** -7, 1e-4
BF = torch.bfloat16


def rope_ref(x, cos, sin, backward=False):
    """float64 rotary of x [B,H,T,D] (or, with ``backward``, its gradient map) for cos/sin [Bc,T,D]."""
    x, c, s = x.double(), cos.double().unsqueeze(1), sin.double().unsqueeze(1)
    h = x.shape[-1] // 2
    if backward:  # transpose of the forward map
        return x * c + torch.cat(((x * s)[..., h:], -(x * s)[..., :h]), -1)
    return x * c + torch.cat((-x[..., h:], x[..., :h]), -1) * s


def swiglu_ref(g, u, dy):
    g, u, dy = g.double(), u.double(), dy.double()
    s = torch.sigmoid(g)
    return g * s * u, dy * u * s * (1 + g * (1 - s)), dy * g * s


ROPE_SHAPES = [(2, 4, 2, 5, 64), (1, 14, 7, 33, 64), (2, 6, 3, 7, 128), (1, 8, 8, 4, 128)]  # (B, H, Hkv, T, D)
ROPE_CASES = [(*shp, shared, dt, False) for shp in ROPE_SHAPES for shared in (True, False)
              for dt in (torch.float32, BF)] + [(1, 14, 7, 33, 64, True, BF, True)]


@pytest.mark.parametrize("B,H,Hkv,T,D,shared,cs_dtype,packed", ROPE_CASES)
def test_rotary_vs_float64(B, H, Hkv, T, D, shared, cs_dtype, packed):
    from determined_amd.ops.rotary import apply_rotary

    torch.manual_seed(B * 1000 + H * 10 + T)
    if packed:  # q, k as slices of one [B, T, (H + 2 Hkv) * D] projection output
        qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device="cuda", dtype=BF)
        q = qkv[..., :H * D].view(B, T, H, D).transpose(1, 2)
        k = qkv[..., H * D:(H + Hkv) * D].view(B, T, Hkv, D).transpose(1, 2)
    else:  # transposed views of [B, T, H, D] buffers
        q = torch.randn(B, T, H, D, device="cuda", dtype=BF).transpose(1, 2)
        k = torch.randn(B, T, Hkv, D, device="cuda", dtype=BF).transpose(1, 2)
    # independent over the full D: a kernel that assumes cos[:h] == cos[h:] fails
    cos, sin = (torch.randn(1 if shared else B, T, D, device="cuda").to(cs_dtype) for _ in range(2))
    q.requires_grad_(True), k.requires_grad_(True)
    qr, kr = apply_rotary(q, k, cos, sin)
    assert qr.shape == q.shape and kr.shape == k.shape and qr.dtype == BF
    assert qr.transpose(1, 2).is_contiguous() and kr.transpose(1, 2).is_contiguous()  # [B,T,H,D] memory
    for out, x in ((qr, q), (kr, k)):
        torch.testing.assert_close(out.double(), rope_ref(x.detach(), cos, sin), rtol=RTOL, atol=ATOL)
    # non-contiguous upstream gradients (the first D columns of [B,H,T,2D] buffers)
    gq = torch.randn(B, H, T, 2 * D, device="cuda", dtype=BF)[..., :D]
    gk = torch.randn(B, Hkv, T, 2 * D, device="cuda", dtype=BF)[..., :D]
    torch.autograd.backward((qr, kr), (gq, gk))
    for x, g in ((q, gq), (k, gk)):
        # (autograd re-lays the gradient of a leaf that is a slice of a larger buffer: the packed case)
        assert packed or x.grad.transpose(1, 2).is_contiguous()
        torch.testing.assert_close(x.grad.double(), rope_ref(g, cos, sin, backward=True), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("M,I,packed", [(1, 8, False), (67, 264, False), (5, 4096, False), (67, 264, True)])
def test_swiglu_vs_float64(M, I, packed):
    from determined_amd.ops.fused import swiglu

    torch.manual_seed(M + I)
    gu = torch.randn(M, 2 * I, device="cuda")
    gu[:, :I] *= 3
    gu[0, :7] = torch.tensor([-100., -30., -1.278, 0., 1e-3, 30., 100.], device="cuda")
    gu = gu.to(BF)
    gate, up = (gu[:, :I], gu[:, I:]) if packed else (gu[:, :I].contiguous(), gu[:, I:].contiguous())
    gate.requires_grad_(True), up.requires_grad_(True)
    dy = torch.randn(M, I, device="cuda", dtype=BF)
    y = swiglu(gate, up)
    y.backward(dy)
    refs = swiglu_ref(gate.detach(), up.detach(), dy)
    for got, ref in zip((y, gate.grad, up.grad), refs):
        assert got.dtype == BF and torch.isfinite(got).all()
        torch.testing.assert_close(got.double(), ref, rtol=RTOL, atol=ATOL)


def test_hf_llama_rope_swiglu(monkeypatch):
    transformers = pytest.importorskip("transformers")
    from determined_amd.ops import rotary
    from determined_amd.transformers import accelerate
    from determined_amd.utils.graphs import GraphedStep

    kernel_ran = []  # per apply_rotary call of the accelerated forwards: did rope_qk produce the outputs

    def spy(*args, real=rotary.apply_rotary):
        out = real(*args)
        kernel_ran.append(all(type(o.grad_fn).__name__ == "_RotaryFnBackward" and o.transpose(1, 2).is_contiguous()
                              for o in out))
        return out

    monkeypatch.setattr(rotary, "apply_rotary", spy)
    torch.manual_seed(4)
    cfg = transformers.LlamaConfig(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, num_hidden_layers=2,
                                   intermediate_size=512, vocab_size=512)
    stock = transformers.LlamaForCausalLM(cfg).cuda().eval()
    x = torch.randint(0, 512, (2, 100), device="cuda")
    with torch.no_grad():
        ref = stock(x).logits
    m = accelerate(copy.deepcopy(stock).bfloat16())
    names = {(type(mod).__name__, mod.forward.__func__.__name__) for mod in m.modules()
             if type(mod).__name__.endswith(("MLP", "Attention"))}
    assert names == {("LlamaMLP", "_swiglu_mlp_forward"), ("LlamaAttention", "_rope_attention_forward")}

    captured = accelerate(copy.deepcopy(stock).bfloat16())  # first run inside GraphedStep, as a captured model's is

    # detached outputs: a live autograd graph would keep the eager run's gradient accumulators (and
    # the stream they were created on) attached to the parameters (see GraphedStep)
    def step(model, **kw):
        model.zero_grad(set_to_none=False)
        logits = model(x, **kw).logits
        loss = logits.float().square().mean()
        loss.backward()
        return logits.detach(), loss.detach()

    # HF's default (use_cache=True: every layer is handed a fresh DynamicCache, in training too) and no cache
    for n, kw in enumerate(({}, {"use_cache": False}), 1):
        logits, eager_loss = step(m, **kw)
        assert kernel_ran == [True] * (2 * n)  # one rope_qk per layer
        torch.testing.assert_close(logits.float(), ref, rtol=2e-2, atol=2e-2 * ref.abs().max().item())
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    graphed = GraphedStep(lambda: step(captured), warmup=2)
    for _ in range(3):  # several replays, each the eager step again: the same kernels on the same inputs (a GEMM
        # that orders its sums differently moves a few bf16 logits by an ulp: ~1e-7 of the mean)
        torch.testing.assert_close(graphed()[1], eager_loss, rtol=1e-4, atol=0)
    assert len(kernel_ran) == 4 + 2 * 3 and all(kernel_ran)  # two warm-up runs and the capture ran rope_qk too
