"""The loss and activation kernels of csrc/fused.hip (lm_ce, ce, gelu_fwd, gelu_bwd_bias, sum_rows)
vs fp64 references of the same operations computed from the bf16-rounded inputs, at the label,
vocabulary and shape edges where they take another path.

Tolerances of the cross-entropy tests: the loss is an fp32 sum of a few rows: rtol = atol = 1e-4.  The
logits gradient is written in bf16: rtol = 2e-2 (2^-9 output rounding with margin).  Its atol,
``1e-5 * scale`` with ``scale = |upstream| / n_valid``, covers the one entry that rtol cannot,
``p - 1`` at the label column as ``p -> 1``: ``p = exp(x - lse)`` with an fp32 ``lse`` that was
rounded twice (``max + log(sum)`` and ``x - lse``), 2^-23 |lse| in all, so the entry is off by
``scale * 2^-23 |lse|``: 7e-6 * scale at the +-60 logits of the saturating cases."""

import pytest
import torch
import torch.nn.functional as F

from tests.test_fused_loss_cpu import ce_reference, lm_labels

pytestmark = pytest.mark.gpu

LM_FN = "_LMCrossEntropyFnBackward"
TOKEN_FN = "_TokenCEFnBackward"


def _randn(*shape, seed, std=3.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).bfloat16().cuda()


def _check_ce(loss, grad, base, labels, V, ignore_index, shift, upstream):
    ref_loss, ref_grad, n_valid = ce_reference(base, labels, V, ignore_index, shift=shift, upstream=upstream)
    atol = 1e-5 * abs(upstream) / max(n_valid, 1)
    torch.testing.assert_close(loss.double(), ref_loss, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(grad.double(), ref_grad, rtol=2e-2, atol=atol,
                               msg=lambda m: f"{m}\nn_valid {n_valid}, atol {atol:.3e}, ref max {ref_grad.abs().max().item():.3e}")
    return n_valid


# ------------------------------------------------------------------------------------ lm_cross_entropy
LM_VOCABS = [(8, 8), (13, 16), (2048, 2048), (2055, 2056), (4099, 4104)]


def _lm_run(base, labels, V, ignore_index=-100, upstream=1.0, inplace=True):
    """(loss, gradient at the leaf, the logits tensor the kernel was given, after the backward)."""
    from determined_amd.ops.fused import lm_cross_entropy

    lg = base.clone().requires_grad_(True)
    x = lg * 1  # a non-leaf (the in-place gradient overwrites it)
    loss = lm_cross_entropy(x, labels, V, ignore_index=ignore_index, inplace_grad=inplace)
    assert type(loss.grad_fn).__name__ == LM_FN
    (loss * upstream).backward()
    return loss.detach(), lg.grad, x.detach()


def _lm_ignored(labels, V, ignore_index):
    """[B, T] mask of the positions that contribute nothing: ignored targets and the last position."""
    tgt = labels[:, 1:]
    m = torch.ones_like(labels, dtype=torch.bool)
    m[:, :-1] = (tgt == ignore_index) | (tgt < 0) | (tgt >= V)
    return m


@pytest.mark.parametrize("V,Vp", LM_VOCABS)
@pytest.mark.parametrize("ignore_index,upstream", [(-100, 1.0), (-100, 0.37), (0, 0.37)])
def test_lm_ce_placed_labels(V, Vp, ignore_index, upstream):
    """Labels on 0, V - 1, both sides of the vector / tail boundary, the pad range, a negative value
    and ignore_index; labels[:, 0] would change the loss if the t -> t + 1 shift were wrong."""
    B, T = 2, 5
    base = _randn(B, T, Vp, seed=V)
    labels = lm_labels(B, T, V, ignore_index).cuda()
    loss, grad, _ = _lm_run(base, labels, V, ignore_index, upstream)
    n_valid = _check_ce(loss, grad, base, labels, V, ignore_index, True, upstream)
    assert 3 <= n_valid <= 5
    assert float(grad[:, :, V:].abs().sum()) == 0.0, "pad columns"
    assert float(grad[_lm_ignored(labels, V, ignore_index)].abs().sum()) == 0.0, "ignored rows"


@pytest.mark.parametrize("V,Vp", [(13, 16), (4099, 4104)])
@pytest.mark.parametrize("B,T,fill", [(2, 5, "ignore"), (2, 5, "out_of_range"), (3, 1, "valid")])
def test_lm_ce_without_a_valid_label_is_zero(V, Vp, B, T, fill):
    base = _randn(B, T, Vp, seed=1)
    labels = {"ignore": torch.full((B, T), -100), "out_of_range": torch.tensor([V, -1, V + 99, Vp, -5]).repeat(B, 1),
              "valid": torch.full((B, T), 2)}[fill].cuda()
    labels[:, 0] = 3  # never a target
    loss, grad, _ = _lm_run(base, labels, V, upstream=0.37)
    assert loss.item() == 0.0 and float(grad.abs().sum()) == 0.0


@pytest.mark.parametrize("V,Vp", LM_VOCABS)
def test_lm_ce_out_of_place_gradient(V, Vp):
    """inplace_grad=False leaves the logits as they were and writes the same bits elsewhere."""
    B, T = 2, 5
    base = _randn(B, T, Vp, seed=V + 1)
    labels = lm_labels(B, T, V, -100).cuda()
    loss_i, grad_i, x_i = _lm_run(base, labels, V, upstream=0.37, inplace=True)
    loss_o, grad_o, x_o = _lm_run(base, labels, V, upstream=0.37, inplace=False)
    assert torch.equal(x_o, base) and torch.equal(loss_i, loss_o)
    assert torch.equal(grad_i.view(torch.int16), grad_o.view(torch.int16))
    assert torch.equal(x_i.view(torch.int16), grad_i.view(torch.int16))  # in place: over the logits
    _check_ce(loss_o, grad_o, base, labels, V, -100, True, 0.37)


@pytest.mark.parametrize("V,Vp", LM_VOCABS)
def test_lm_ce_saturating_logits(V, Vp):
    """Logits scaled to +-60: the softmax saturates; one target sits on its row's arg-max (p -> 1)."""
    B, T = 2, 5
    base = _randn(B, T, Vp, seed=V + 2).float()
    base = (base * (60.0 / base.abs().max())).bfloat16()
    labels = lm_labels(B, T, V, -100).cuda()
    labels[0, 4] = base[0, 3, :V].argmax()
    loss, grad, _ = _lm_run(base, labels, V, upstream=0.37)
    _check_ce(loss, grad, base, labels, V, -100, True, 0.37)
    assert float(grad[:, :, V:].abs().sum()) == 0.0


def test_lm_ce_neg_inf_vocabulary_range():
    """A masked vocabulary range: columns 2048..2055 (one whole 16-byte vector, the second one of
    thread 0, which holds a finite maximum by then) and 4096..4098 are -inf in every row."""
    B, T, V = 2, 5, 4104
    base = _randn(B, T, V, seed=5)
    masked = torch.zeros(V, dtype=torch.bool, device="cuda")
    masked[2048:2056] = True
    masked[4096:4099] = True
    base[:, :, masked] = float("-inf")
    labels = lm_labels(B, T, V, -100).cuda()
    labels[labels == V // 2] = 2060  # lm_labels' mid-vocabulary label is a masked column here
    assert not masked[labels[:, 1:].clamp(0, V - 1)].any()
    loss, grad, _ = _lm_run(base, labels, V, upstream=0.37)
    assert torch.isfinite(loss), loss
    _check_ce(loss, grad, base, labels, V, -100, True, 0.37)
    assert float(grad[:, :, masked].abs().sum()) == 0.0


def _at_offset(base, offset):
    """A contiguous view with ``base``'s values that starts ``offset`` elements into its storage."""
    buf = torch.zeros(base.numel() + 16, device="cuda", dtype=base.dtype)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + base.numel()].view(base.shape)
    v.copy_(base)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + offset * base.element_size()
    return v.requires_grad_(True)


@pytest.mark.parametrize("offset,fused", [(1, False), (4, False), (8, True)])
def test_lm_ce_dispatch_checks_alignment(offset, fused):
    """Logits that do not start on a 16-byte boundary take the PyTorch path (dispatch only: no
    misaligned vector load is launched); labels in range, so that path cannot assert."""
    from determined_amd.ops.fused import lm_cross_entropy

    B, T, V, Vp = 2, 5, 13, 16
    base = _randn(B, T, Vp, seed=6)
    labels = lm_labels(B, T, V, -100).clamp_(min=-100, max=V - 1).cuda()
    labels[labels < 0] = -100
    x = _at_offset(base, offset)
    loss = lm_cross_entropy(x, labels, V, inplace_grad=False)
    assert (type(loss.grad_fn).__name__ == LM_FN) == fused
    ref_loss = ce_reference(base, labels, V, shift=True)[0]
    torch.testing.assert_close(loss.detach().double(), ref_loss, rtol=1e-4, atol=1e-4)


# --------------------------------------------------------------------------------- token_cross_entropy
TOKEN_VOCABS = [2, 10, 12, 14, 514, 1030, 30522]  # V % 8: 2, 2, 4, 6, 2, 6, 2
TB, TT = 4, 16


def _token_labels(V, ignore_index, density):
    """[TB, TT] labels: ``density`` of the rows labelled at random, then the first rows placed on 0,
    1, V - 2, V - 1, V and beyond (ignored), a negative value, ignore_index and, where V reaches it,
    both sides of column 512 (the second pair of thread 0)."""
    g = torch.Generator().manual_seed(11)
    labels = torch.randint(0, V, (TB * TT,), generator=g)
    labels[torch.rand(TB * TT, generator=g) > density] = ignore_index
    placed = [0, 1, V - 2, V - 1, V, V + 5, -7, ignore_index] + ([511, 512, 513, 514] if V > 514 else [])
    labels[:len(placed)] = torch.tensor(placed)
    return labels.view(TB, TT).cuda()


def _token_run(base, labels, ignore_index=-100, upstream=1.0, inplace=False):
    from determined_amd.ops.fused import token_cross_entropy

    lg = base.clone().requires_grad_(True)
    x = lg * 1  # a non-leaf (the in-place gradient overwrites it)
    loss = token_cross_entropy(x, labels, ignore_index=ignore_index, inplace_grad=inplace)
    assert type(loss.grad_fn).__name__ == TOKEN_FN
    (loss * upstream).backward()
    return loss.detach(), lg.grad, x.detach()


def _token_ignored(labels, V, ignore_index):
    return (labels == ignore_index) | (labels < 0) | (labels >= V)


@pytest.mark.parametrize("V", TOKEN_VOCABS)
@pytest.mark.parametrize("ignore_index,upstream,inplace", [(-100, 1.0, False), (-100, 0.37, True), (0, 0.37, False)])
def test_token_ce_placed_labels(V, ignore_index, upstream, inplace):
    base = _randn(TB, TT, V, seed=V)
    labels = _token_labels(V, ignore_index, 0.15)
    loss, grad, _ = _token_run(base, labels, ignore_index, upstream, inplace)
    n_valid = _check_ce(loss, grad, base, labels, V, ignore_index, False, upstream)
    assert 2 <= n_valid < TB * TT // 2
    assert float(grad[_token_ignored(labels, V, ignore_index)].abs().sum()) == 0.0, "ignored rows"


@pytest.mark.parametrize("V", TOKEN_VOCABS)
def test_token_ce_every_row_labelled(V):
    base = _randn(TB, TT, V, seed=V + 1)
    labels = torch.randint(0, V, (TB, TT), generator=torch.Generator().manual_seed(12)).cuda()
    loss, grad, _ = _token_run(base, labels, upstream=0.37)
    assert _check_ce(loss, grad, base, labels, V, -100, False, 0.37) == TB * TT


@pytest.mark.parametrize("V", TOKEN_VOCABS)
@pytest.mark.parametrize("inplace", [False, True])
def test_token_ce_without_a_valid_label_is_zero(V, inplace):
    base = _randn(TB, TT, V, seed=2)
    labels = torch.tensor([-100, V, -1, V + 7]).repeat(TB, TT // 4).cuda()
    loss, grad, _ = _token_run(base, labels, upstream=0.37, inplace=inplace)
    assert loss.item() == 0.0 and float(grad.abs().sum()) == 0.0


@pytest.mark.parametrize("V", TOKEN_VOCABS)
def test_token_ce_out_of_place_gradient(V):
    base = _randn(TB, TT, V, seed=V + 3)
    labels = _token_labels(V, -100, 0.15)
    loss_i, grad_i, x_i = _token_run(base, labels, upstream=0.37, inplace=True)
    loss_o, grad_o, x_o = _token_run(base, labels, upstream=0.37, inplace=False)
    assert torch.equal(x_o, base) and torch.equal(loss_i, loss_o)
    assert torch.equal(grad_i.view(torch.int16), grad_o.view(torch.int16))
    assert torch.equal(x_i.view(torch.int16), grad_i.view(torch.int16))


@pytest.mark.parametrize("V", TOKEN_VOCABS)
def test_token_ce_saturating_logits(V):
    base = _randn(TB, TT, V, seed=V + 4).float()
    base = (base * (60.0 / base.abs().max())).bfloat16()
    labels = _token_labels(V, -100, 0.15)
    labels[1, 0] = base[1, 0].argmax()
    loss, grad, _ = _token_run(base, labels, upstream=0.37)
    _check_ce(loss, grad, base, labels, V, -100, False, 0.37)


def test_token_ce_neg_inf_pair():
    """Columns 512 and 513 (one aligned bf16 pair, the second one of thread 0) are -inf in every row."""
    V = 1030
    base = _randn(TB, TT, V, seed=7)
    base[:, :, 512:514] = float("-inf")
    labels = _token_labels(V, -100, 0.15)
    labels[(labels == 512) | (labels == 513)] = 515
    loss, grad, _ = _token_run(base, labels, upstream=0.37)
    assert torch.isfinite(loss), loss
    _check_ce(loss, grad, base, labels, V, -100, False, 0.37)
    assert float(grad[:, :, 512:514].abs().sum()) == 0.0


@pytest.mark.parametrize("offset,fused", [(1, False), (3, False), (2, True)])
def test_token_ce_dispatch_checks_alignment(offset, fused):
    """Logits that do not start on a 4-byte boundary take the PyTorch path (dispatch only; labels
    in range); rows that are 4-byte but not 16-byte aligned are the kernel's ordinary case."""
    from determined_amd.ops.fused import token_cross_entropy

    V = 10
    base = _randn(TB, TT, V, seed=8)
    labels = torch.randint(0, V, (TB, TT), generator=torch.Generator().manual_seed(13)).cuda()
    labels[0, :5] = -100
    x = _at_offset(base, offset)
    loss = token_cross_entropy(x, labels)
    assert (type(loss.grad_fn).__name__ == TOKEN_FN) == fused
    ref_loss = ce_reference(base, labels, V)[0]
    torch.testing.assert_close(loss.detach().double(), ref_loss, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------------------------ GELU
# Forward: the output is rounded to bf16, one ulp (2^-8 relative at most to nearest, 2^-7 with a flip
# at a rounding boundary): rtol = 2^-7.  atol = 1e-5: tanh_fast / erff form 1 + t by cancellation with
# an absolute error of a few fp32 eps (about 1e-7), multiplied by 0.5 |x| <= 8 on the sweep.
# Backward: the same for gelu'(h) * dg, atol scaled by max |dg|.
GELU_RTOL, GELU_ATOL = 2.0 ** -7, 1e-5


def _bf16_sweep():
    """Every bf16 value in [-16, 16] (both zeros, the subnormals) and +-1e4, padded with zeros to a
    multiple of 8."""
    pos = torch.arange(0, 0x4180 + 1, dtype=torch.int16).view(torch.bfloat16)  # bit patterns of +0 .. 16
    assert float(pos[-1]) == 16.0 and float(pos[0]) == 0.0
    x = torch.cat([pos, -pos, torch.tensor([1e4, -1e4]).bfloat16()])
    return torch.cat([x, torch.zeros(-x.numel() % 8, dtype=torch.bfloat16)]).cuda()


def _gelu_ref(h, exact, dg=None):
    """fp64 gelu(h), and with ``dg`` its fp64 gradient gelu'(h) * dg."""
    h64 = h.double().requires_grad_(dg is not None)
    y = F.gelu(h64, approximate="none" if exact else "tanh")
    if dg is None:
        return y
    y.backward(dg.double())
    return y.detach(), h64.grad


@pytest.mark.parametrize("exact", [False, True], ids=["tanh", "erf"])
def test_gelu_fwd_dense_sweep(exact):
    from determined_amd import ops

    h = _bf16_sweep()
    assert h.numel() % 8 == 0 and h.numel() > 33000
    g = ops.ext().gelu_fwd(h, exact)
    assert g.dtype == torch.bfloat16 and g.shape == h.shape
    torch.testing.assert_close(g.double(), _gelu_ref(h, exact), rtol=GELU_RTOL, atol=GELU_ATOL)


def _check_gelu_bwd(h, dg, exact, bias_dtype):
    """dh against fp64; db against the column sums of the kernel's own bf16 dh (what it documents)
    and against the fp64 bias gradient.  Twice: the column partials' workspace is shared."""
    from determined_amd import ops

    N = h.shape[-1]
    _, ref_dh = _gelu_ref(h, exact, dg)
    ref_db = ref_dh.reshape(-1, N).sum(0)
    for _ in range(2):
        dh, db = ops.ext().gelu_bwd_bias(dg, h, bias_dtype, exact)
        assert dh.dtype == torch.bfloat16 and dh.shape == h.shape and db.dtype == bias_dtype and db.shape == (N,)
        atol = GELU_ATOL * dg.float().abs().max().item()
        own = dh.double().reshape(-1, N).sum(0)
        own_abs = dh.double().reshape(-1, N).abs().sum(0)
        tol = 1e-5 * own_abs + (own.abs() * 2.0 ** -7 if bias_dtype == torch.bfloat16 else 0.0)
        rel = ((db.double() - ref_db).norm() / ref_db.norm()).item()
        torch.testing.assert_close(dh.double(), ref_dh, rtol=GELU_RTOL, atol=atol)
        over = ((db.double() - own).abs() / tol.clamp(min=1e-300)).max().item()
        assert over <= 1.0, f"db vs the column sums of dh: max err / tol {over:.3f}"
        assert rel < 2e-2, f"db vs the fp64 bias gradient: relative norm error {rel:.3e}"


@pytest.mark.parametrize("exact", [False, True], ids=["tanh", "erf"])
@pytest.mark.parametrize("bias_dtype", [torch.bfloat16, torch.float32])
def test_gelu_bwd_bias_dense_sweep(exact, bias_dtype):
    h = _bf16_sweep().view(-1, 8)
    dg = _randn(*h.shape, seed=20, std=1.0)
    _check_gelu_bwd(h, dg, exact, bias_dtype)


# one row; a partial column block (136 = 128 + 8) of one split; 2 splits (M > 128) of one and three
# column blocks, the last of them partial; 32 splits of 125 rows with a short last one (94 rows)
GELU_SHAPES = [(1, 8), (15, 136), (17, 128), (129, 8), (130, 264), (3969, 1024)]


@pytest.mark.parametrize("M,N", GELU_SHAPES)
@pytest.mark.parametrize("exact", [False, True], ids=["tanh", "erf"])
@pytest.mark.parametrize("bias_dtype", [torch.bfloat16, torch.float32])
def test_gelu_bwd_bias_shapes(M, N, exact, bias_dtype):
    h = _randn(M, N, seed=M + N)
    dg = _randn(M, N, seed=M + N + 1, std=1.0)
    _check_gelu_bwd(h, dg, exact, bias_dtype)


@pytest.mark.parametrize("M,N", GELU_SHAPES)
@pytest.mark.parametrize("exact", [False, True], ids=["tanh", "erf"])
def test_gelu_fwd_shapes(M, N, exact):
    from determined_amd import ops

    h = _randn(M, N, seed=M + N + 2)
    g = ops.ext().gelu_fwd(h, exact)
    torch.testing.assert_close(g.double(), _gelu_ref(h, exact), rtol=GELU_RTOL, atol=GELU_ATOL)


# ------------------------------------------------------------------------------------ grid-stride loops
@pytest.mark.parametrize("exact", [False, True], ids=["tanh", "erf"])
def test_gelu_fwd_grid_stride(exact):
    """8192 * 256 vectors fill the largest grid once; 257 more enter the stride loop."""
    from determined_amd import ops

    n = 8192 * 256 * 8 + 8 * 257
    h = (torch.randn(n, device="cuda", generator=torch.Generator("cuda").manual_seed(30)) * 3).bfloat16()
    g = ops.ext().gelu_fwd(h, exact)
    ref = F.gelu(h.float(), approximate="none" if exact else "tanh")
    torch.testing.assert_close(g.float(), ref, rtol=GELU_RTOL, atol=GELU_ATOL)


def test_sum_rows_into_grid_stride():
    """16384 * 256 float4 columns fill the largest grid once; 300 more enter the stride loop.  Two
    rows: one fp32 addition per element, which has one correctly rounded result."""
    from determined_amd import ops

    W, H = 2, 16384 * 1024 + 4 * 300
    part = torch.randn(W, H, device="cuda", generator=torch.Generator("cuda").manual_seed(31))
    out = torch.full((H,), 5.0, device="cuda")
    ops.ext().sum_rows_into(part, out)
    torch.testing.assert_close(out, part.sum(0), rtol=0, atol=0)
