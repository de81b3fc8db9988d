"""Fused per-head RMSNorm + rotary embedding (csrc/decoder.hip rope_norm) against float64 math on the same
bf16 inputs, and a Qwen3 model through transformers.accelerate().

out / dq / dk: the kernel is fp32 math plus ONE bf16 rounding, so test_rope_swiglu_gpu.py's rtol = 2**-7,
atol = 1e-4 applies (derived in that file's docstring); every element is checked.  dw: a sum over all
(batch, token, head) rows accumulated in fp32, so |err_i| <= rtol_w * |ref_i| + 1e-5 * S_i with S_i the
float64 sum of |gy_i * x_i * r| over the rows -- what an fp32 accumulation can lose scales with the terms, not
with the cancelled sum -- and rtol_w the rounding of the weight dtype (2**-7 for bf16, 1e-5 for fp32).  Measured
on an MI355X with fp32 weights: max err_i / S_i = 1.3e-8 at the 9000-token case and 9.8e-8 (about one fp32 ulp
of a single term) at the small shapes, where few rows are summed; each term gy * x * r carries a few fp32
roundings, so 1e-5 keeps a factor ~20 over the worst case of the arithmetic and was left as it is."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL, ATOL = 2 ** -7, 1e-4
BF, F32 = torch.bfloat16, torch.float32
EPS = 1e-6


def reference(x, w, cos, sin, g):
    """float64 (out, dx, dw, S) of rope(w * x * rsqrt(mean(x^2) + EPS)) for x, g [B,H,T,D], w [D], cos / sin [Bc,T,D]."""
    x, w = x.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    g, c, s = g.double(), cos.double().unsqueeze(1), sin.double().unsqueeze(1)
    h = x.shape[-1] // 2

    def rot(v):
        return torch.cat((-v[..., h:], v[..., :h]), -1)

    r = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
    out = w * x * r
    out = out * c + rot(out) * s
    dx, dw = torch.autograd.grad(out, (x, w), g)
    gy = g * c - rot(g * s)  # rope^T(g): the transpose of rot is -rot
    return out.detach(), dx, dw, (gy * x * r).abs().sum((0, 1, 2)).detach()


# (B, H, Hkv, T, D, weight dtype, shared cos / sin -- fp32 when shared, bf16 per batch --, packed projection);
# 9000 tokens: more than the backward's resident grid covers in one sweep (at most 8 workgroups x 4 tokens per CU)
CASES = [(2, 4, 2, 5, 64, BF, True, False), (2, 4, 2, 5, 64, F32, False, False),
         (1, 14, 7, 33, 64, BF, False, False), (1, 14, 7, 33, 64, F32, True, True),
         (2, 6, 3, 7, 128, BF, False, False), (2, 6, 3, 7, 128, F32, True, False),
         (1, 8, 8, 4, 128, BF, True, False), (1, 8, 8, 4, 128, F32, False, False),
         (1, 2, 1, 9000, 64, BF, False, False), (1, 2, 1, 9000, 64, F32, True, False)]


@pytest.mark.parametrize("B,H,Hkv,T,D,w_dtype,shared,packed", CASES)
def test_norm_rotary_vs_float64(B, H, Hkv, T, D, w_dtype, shared, packed):
    from determined_amd.ops.rotary import apply_rotary

    torch.manual_seed(B * 1000 + H * 10 + T)
    qkv = torch.randn(B, T, (H + 2 * Hkv) * D, device="cuda")
    for lo in (0, H * D):  # head 0 of q and of k: all zeros at the first token, mean(x^2) close to EPS at the last
        qkv[0, 0, lo:lo + D] = 0
        qkv[-1, -1, lo:lo + D] *= 1e-3
    qkv = qkv.to(BF)
    q = qkv[..., :H * D].view(B, T, H, D).transpose(1, 2)
    k = qkv[..., H * D:(H + Hkv) * D].view(B, T, Hkv, D).transpose(1, 2)
    if not packed:  # transposed views of [B, T, H, D] buffers
        q, k = q.transpose(1, 2).contiguous().transpose(1, 2), k.transpose(1, 2).contiguous().transpose(1, 2)
    cos, sin = (torch.randn(1 if shared else B, T, D, device="cuda").to(F32 if shared else BF) for _ in range(2))
    wq, wk = ((1 + 0.5 * torch.randn(D, device="cuda")).to(w_dtype).requires_grad_() for _ in range(2))
    q.requires_grad_(True), k.requires_grad_(True)
    qr, kr = apply_rotary(q, k, cos, sin, wq, wk, EPS)
    assert type(qr.grad_fn).__name__ == "_NormRotaryFnBackward" and qr.dtype == BF and kr.dtype == BF
    assert qr.transpose(1, 2).is_contiguous() and kr.transpose(1, 2).is_contiguous()  # [B,T,H,D] memory
    # non-contiguous upstream gradients (the first D columns of [B,H,T,2D] buffers)
    gq = torch.randn(B, H, T, 2 * D, device="cuda", dtype=BF)[..., :D]
    gk = torch.randn(B, Hkv, T, 2 * D, device="cuda", dtype=BF)[..., :D]
    grads = [torch.autograd.grad((qr, kr), (q, k, wq, wk), (gq, gk), retain_graph=True) for _ in range(2)]
    rtol_w = 2 ** -7 if w_dtype == BF else 1e-5
    for i, (out, x, w, g) in enumerate(((qr, q, wq, gq), (kr, k, wk, gk))):
        ref_out, ref_dx, ref_dw, S = reference(x, w, cos, sin, g)
        dx, dw = grads[0][i], grads[0][2 + i]
        assert torch.equal(out[0, 0, 0], torch.zeros_like(out[0, 0, 0])) and torch.isfinite(dx).all()
        torch.testing.assert_close(out.double(), ref_out, rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(dx.double(), ref_dx, rtol=RTOL, atol=ATOL)
        assert dw.dtype == w_dtype and torch.equal(dw, grads[1][2 + i])  # deterministic: bit-identical reruns
        err, bound = (dw.double() - ref_dw).abs(), rtol_w * ref_dw.abs() + 1e-5 * S
        print(f"dw max err {err.max().item():.3e}, max err / S {(err / S).max().item():.3e}")
        assert (err <= bound).all(), (err.max().item(), bound.min().item())


def test_hf_qwen3(monkeypatch):
    transformers = pytest.importorskip("transformers")
    from determined_amd.ops import rotary
    from determined_amd.transformers import accelerate

    kernel_ran = []  # per apply_rotary call of the accelerated forwards: did rope_norm produce the outputs

    def spy(*args, real=rotary.apply_rotary):
        out = real(*args)
        kernel_ran.append(len(args) == 7 and all(type(o.grad_fn).__name__ == "_NormRotaryFnBackward" for o in out))
        return out

    monkeypatch.setattr(rotary, "apply_rotary", spy)
    torch.manual_seed(4)
    cfg = transformers.Qwen3Config(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                                   num_hidden_layers=2, intermediate_size=512, vocab_size=512)
    stock = transformers.Qwen3ForCausalLM(cfg).cuda().eval()
    for name, p in stock.named_parameters():  # norm weights off their all-ones initial value
        if "norm" in name:
            torch.nn.init.normal_(p, 1.0, 0.5)
    x = torch.randint(0, 512, (2, 100), device="cuda")
    stock_bf = copy.deepcopy(stock).bfloat16()
    m = accelerate(copy.deepcopy(stock).bfloat16())
    classes = {type(mod).__name__: mod.forward.__func__.__name__ for mod in m.modules()}
    assert classes["Qwen3Attention"] == "_rope_attention_forward" and "Qwen3RMSNorm" not in classes

    def qk_norm_grads(model):
        model.zero_grad()
        logits = model(x, use_cache=False).logits
        logits.float().square().mean().backward()
        return logits.detach(), {n: p.grad.float() for n, p in model.named_parameters() if n.endswith(("q_norm.weight", "k_norm.weight"))}

    ref, ref_grads = qk_norm_grads(stock)
    _, bf_grads = qk_norm_grads(stock_bf)
    logits, grads = qk_norm_grads(m)
    assert kernel_ran == [True, True]  # one fused norm + rotary per layer
    tol = dict(rtol=2e-2, atol=2e-2 * ref.abs().max().item())
    torch.testing.assert_close(logits.float(), ref, **tol)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert len(grads) == 4  # q_norm and k_norm of two layers
    for n, r in ref_grads.items():  # yardstick: what the stock bf16 model loses against fp32
        err, stock_err = (grads[n] - r).abs().max().item(), (bf_grads[n] - r).abs().max().item()
        print(f"{n}: accelerated err {err:.3e}, stock bf16 err {stock_err:.3e}, max |ref| {r.abs().max().item():.3e}")
        assert err <= 2 * stock_err + 1e-3 * r.abs().max().item()
    with torch.no_grad():  # the cache must receive normalised, rotated keys
        past = m(x[:, :20], use_cache=True).past_key_values
        nxt = m(x[:, 20:40], past_key_values=past, use_cache=True).logits
        torch.testing.assert_close(nxt.float(), stock(x[:, :40]).logits[:, 20:], **tol)
