"""The PyTorch fallbacks of ops.fused.lm_cross_entropy / token_cross_entropy (fp32 / CPU tensors) vs
an fp64 reference with the fused kernels' label rules, and that reference itself
(tests/test_fused_loss_gelu_gpu.py holds the HIP kernels to the same one)."""

import pytest
import torch
import torch.nn.functional as F

from determined_amd.ops.fused import lm_cross_entropy, token_cross_entropy


def ce_reference(logits, labels, V, ignore_index=-100, shift=False, upstream=1.0):
    """fp64 mean cross-entropy over the first ``V`` columns of ``logits [..., Vp]`` (taken as they
    are: round them to the kernel's input dtype first) and its logits gradient.

    ``shift``: the LM form, ``logits[:, t]`` against ``labels[:, t + 1]``.  A label equal to
    ``ignore_index``, ``< 0`` or ``>= V`` is masked out; the mean is over ``max(n_valid, 1)``.
    Returns ``(loss, grad, n_valid)``: ``grad`` is autograd's gradient of ``loss * upstream`` in the
    shape of ``logits`` (zero in pad columns, ignored rows and the last position of the LM form)."""
    x = logits.detach().double().requires_grad_(True)
    lg, tgt = (x[:, :-1, :V], labels[:, 1:]) if shift else (x[..., :V], labels)
    lg, tgt = lg.reshape(-1, V), tgt.reshape(-1).to(x.device)
    valid = (tgt != ignore_index) & (tgt >= 0) & (tgt < V)
    picked = torch.log_softmax(lg, -1).gather(1, tgt.clamp(0, V - 1).unsqueeze(1)).squeeze(1)
    n_valid = int(valid.sum())
    loss = -torch.where(valid, picked, torch.zeros_like(picked)).sum() / max(n_valid, 1)
    (loss * upstream).backward()
    return loss.detach(), x.grad, n_valid


def lm_labels(B, T, V, ignore_index):
    """Deterministic LM labels ``[B, T]`` (needs ``B * (T - 1) >= 8``): the targets ``labels[:, 1:]``
    hold column 0, V - 1, both sides of the 16-byte-vector / scalar-tail boundary, V (the first pad
    column), a negative non-ignore value and ``ignore_index``; the rest are spread over ``[1, V)``.
    ``labels[:, 0]`` (never a target) holds valid labels no neighbour shares, so reading
    ``labels[b, t]`` for position ``t`` changes the loss."""
    tail = 8 * (V // 8)
    placed = [0, V - 1, tail - 1, tail, V, -7, ignore_index, V // 2]
    n = B * (T - 1)
    vals = placed + [1 + (37 * i) % (V - 1) for i in range(n - len(placed))]
    labels = torch.empty(B, T, dtype=torch.long)
    labels[:, 1:] = torch.tensor(vals[:n]).view(B, T - 1)
    for b in range(B):
        taken = set(labels[b, 1:].tolist()) | {ignore_index}
        labels[b, 0] = next(v for v in range(V - 2, 0, -1) if v not in taken)
    return labels


def test_reference_matches_torch_on_plain_labels():
    """With every label in range the reference is F.cross_entropy in fp64 (to fp64 rounding)."""
    torch.manual_seed(0)
    x = torch.randn(3, 6, 16).double() * 3
    labels = torch.randint(0, 13, (3, 6))
    labels[1, 2] = -100
    for shift in (False, True):
        loss, grad, n_valid = ce_reference(x, labels, 13, shift=shift, upstream=0.37)
        xr = x.clone().requires_grad_(True)
        lg, tgt = (xr[:, :-1, :13], labels[:, 1:]) if shift else (xr[..., :13], labels)
        rl = F.cross_entropy(lg.reshape(-1, 13), tgt.reshape(-1), ignore_index=-100)
        (rl * 0.37).backward()
        assert n_valid == int((tgt != -100).sum())
        torch.testing.assert_close(loss, rl.detach(), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(grad, xr.grad, rtol=1e-12, atol=1e-14)


def test_lm_labels_cover_the_edges():
    for V, ii in ((13, -100), (13, 0), (8, -100), (4099, 0)):
        labels = lm_labels(2, 5, V, ii)
        tgt = set(labels[:, 1:].reshape(-1).tolist())
        assert {0, V - 1, V, -7, ii, min(8 * (V // 8), V), 8 * (V // 8) - 1} <= tgt
        for b in range(2):
            first = int(labels[b, 0])
            assert 0 <= first < V and first != ii and first not in labels[b, 1:].tolist()


# fp32 log-softmax of <= 16 columns: a few fp32 eps (6e-8) relative on the loss and on every
# gradient entry; p - 1 at the label column leaves a few eps of `scale = |upstream| / n_valid` absolute
def _check_fp32(loss, grad, ref_loss, ref_grad, upstream, n_valid):
    torch.testing.assert_close(loss.detach().double(), ref_loss, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(grad.double(), ref_grad, rtol=1e-4, atol=1e-6 * abs(upstream) / max(n_valid, 1))


@pytest.mark.parametrize("ignore_index", [-100, 0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lm_fallback_matches_reference(ignore_index, dtype):
    """fp32 / bf16 CPU logits with Vp > V: the shift, pad columns, labels >= V and negative
    non-ignore labels (ignored as on the fused path, no exception), upstream gradient 0.37."""
    torch.manual_seed(1)
    B, T, V, Vp = 2, 5, 13, 16
    base = (torch.randn(B, T, Vp) * 3).to(dtype)
    labels = lm_labels(B, T, V, ignore_index)
    x = base.clone().requires_grad_(True)
    loss = lm_cross_entropy(x, labels, V, ignore_index=ignore_index)
    (loss * 0.37).backward()
    ref_loss, ref_grad, n_valid = ce_reference(base, labels, V, ignore_index, shift=True, upstream=0.37)
    assert n_valid == (5 if ignore_index == -100 else 4)
    if dtype == torch.float32:
        _check_fp32(loss, x.grad, ref_loss, ref_grad, 0.37, n_valid)
    else:  # fp32 arithmetic, the gradient rounded to bf16 (2^-9) by autograd's cast back
        torch.testing.assert_close(loss.detach().double(), ref_loss, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(x.grad.double(), ref_grad, rtol=2.0 ** -8, atol=1e-6 * 0.37 / n_valid)
    assert float(x.grad[:, :, V:].abs().sum()) == 0.0 and float(x.grad[:, -1].abs().sum()) == 0.0
    ignored = ~((labels[:, 1:] != ignore_index) & (labels[:, 1:] >= 0) & (labels[:, 1:] < V))
    assert float(x.grad[:, :-1][ignored].abs().sum()) == 0.0


@pytest.mark.parametrize("B,T,fill", [(2, 5, "ignore"), (2, 5, "out_of_range"), (3, 1, "valid")])
def test_lm_fallback_without_a_valid_label_is_zero(B, T, fill):
    torch.manual_seed(2)
    V, Vp = 13, 16
    x = torch.randn(B, T, Vp, requires_grad=True)
    labels = {"ignore": torch.full((B, T), -100), "out_of_range": torch.tensor([V, -1, 99, V + 2, -5]).repeat(B, 1),
              "valid": torch.randint(0, V, (B, T))}[fill]
    labels[:, 0] = 3  # never a target
    loss = lm_cross_entropy(x, labels, V)
    loss.backward()
    assert loss.item() == 0.0 and float(x.grad.abs().sum()) == 0.0


@pytest.mark.parametrize("ignore_index", [-100, 0])
def test_token_fallback_matches_reference(ignore_index):
    """Odd V (never fused): labels on 0, V - 1, V, beyond, negative and ignore_index."""
    torch.manual_seed(3)
    B, T, V = 3, 4, 11
    base = torch.randn(B, T, V) * 3
    labels = torch.tensor([0, V - 1, V, V + 5, -7, ignore_index, 5, 1, 9, -100, 2, 10]).view(B, T)
    x = base.clone().requires_grad_(True)
    loss = token_cross_entropy(x, labels, ignore_index=ignore_index)
    (loss * 0.37).backward()
    ref_loss, ref_grad, n_valid = ce_reference(base, labels, V, ignore_index, upstream=0.37)
    assert n_valid == (7 if ignore_index == -100 else 6)
    _check_fp32(loss, x.grad, ref_loss, ref_grad, 0.37, n_valid)
    ignored = ~((labels != ignore_index) & (labels >= 0) & (labels < V))
    assert float(x.grad[ignored].abs().sum()) == 0.0


def test_token_fallback_without_a_valid_label_is_zero():
    x = torch.randn(2, 3, 11, requires_grad=True)
    loss = token_cross_entropy(x, torch.tensor([[-100, 11, -1], [-100, -100, 40]]))
    loss.backward()
    assert loss.item() == 0.0 and float(x.grad.abs().sum()) == 0.0
