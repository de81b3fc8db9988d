"""The float64 reference of tests/optim_ref.py against torch.optim, and the fused optimizers' own
fp32 CPU path against that reference on the inputs the GPU tests (test_optim_kernels_gpu.py) use."""

import pytest
import torch

from determined_amd.ops.optim import FusedAdamW, FusedSGD
from tests import optim_ref as R

# float64 round-off: values are O(1), eps is 2.2e-16, a step is a dozen operations.  Where p - lr*u
# cancels to a result far below |p| the relative error of the difference grows, so a few ulps of
# O(1) are allowed absolutely.
F64 = dict(rtol=1e-12, atol=1e-14)
# the tolerance of the existing fused-optimizer tests, which the GPU tests apply as well
F32 = dict(rtol=1e-5, atol=1e-6)

SMALL = (5, 64, 33, 7)
SMALL_GROUP = (0, 1, 0, 1)


def _torch_run(cls, hyper, extra, params64, grads):
    ps = [torch.nn.Parameter(p.clone()) for p in params64]
    groups = []
    for gi, h in enumerate(hyper):
        d = {k: v for k, v in h.items() if k not in ("maximize", "adam_w_mode")}
        d["params"] = [p for p, g in zip(ps, SMALL_GROUP) if g == gi]
        groups.append(d)
    opt = cls(groups, lr=1.0, **extra)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.double()
        opt.step()
    return ps, opt


@pytest.mark.parametrize("adam_w_mode", [True, False])
@pytest.mark.parametrize("maximize", [False, True])
def test_reference_adam_equals_torch_float64(adam_w_mode, maximize):
    params, grads = R.make_inputs(11, SMALL)
    hyper = R.adam_hyper(adam_w_mode, maximize, n_groups=2)
    ref = R.Ref("adam", params, SMALL_GROUP, hyper)
    for gs in grads:
        ref.step(gs)
    cls = torch.optim.AdamW if adam_w_mode else torch.optim.Adam
    ps, opt = _torch_run(cls, hyper, dict(maximize=maximize), R.to64(params), grads)
    for i, p in enumerate(ps):
        torch.testing.assert_close(ref.w[i], p.detach(), **F64)
        torch.testing.assert_close(ref.s0[i], opt.state[p]["exp_avg"], **F64)
        torch.testing.assert_close(ref.s1[i], opt.state[p]["exp_avg_sq"], **F64)


SGD_VARIANTS = {
    "momentum": [dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=False),
                 dict(lr=0.02, momentum=0.8, dampening=0.0, weight_decay=0.0, nesterov=False)],
    "nesterov": [dict(lr=0.05, momentum=0.9, dampening=0.0, weight_decay=1e-3, nesterov=True),
                 dict(lr=0.02, momentum=0.7, dampening=0.0, weight_decay=1e-2, nesterov=False)],
    "dampening": [dict(lr=0.05, momentum=0.9, dampening=0.1, weight_decay=1e-3, nesterov=False),
                  dict(lr=0.02, momentum=0.8, dampening=0.3, weight_decay=0.0, nesterov=False)],
    "plain": [dict(lr=0.05, momentum=0.0, dampening=0.0, weight_decay=1e-3, nesterov=False),
              dict(lr=0.02, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)],
    "mixed_momentum": R.mixed_momentum_hyper(),
}


@pytest.mark.parametrize("variant", sorted(SGD_VARIANTS))
@pytest.mark.parametrize("maximize", [False, True])
def test_reference_sgd_equals_torch_float64(variant, maximize):
    params, grads = R.make_inputs(12, SMALL)
    hyper = [dict(h, maximize=maximize) for h in SGD_VARIANTS[variant]]
    ref = R.Ref("sgd", params, SMALL_GROUP, hyper)
    for gs in grads:
        ref.step(gs)
    ps, opt = _torch_run(torch.optim.SGD, hyper, dict(maximize=maximize), R.to64(params), grads)
    for i, p in enumerate(ps):
        torch.testing.assert_close(ref.w[i], p.detach(), **F64)
        buf = opt.state[p].get("momentum_buffer")
        if buf is not None:
            torch.testing.assert_close(ref.s0[i], buf, **F64)
        else:  # torch keeps no buffer for a momentum-free group; the reference leaves its own untouched
            assert hyper[SMALL_GROUP[i]]["momentum"] == 0 and not ref.s0[i].any()


def test_reference_clipping_equals_torch_float64():
    params, grads = R.make_inputs(13, SMALL, steps=1)
    gs = R.to64(grads[0])
    ps = [torch.nn.Parameter(p.double()) for p in params]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    norm = R.global_norm(gs)
    for max_norm in (norm / 3.0, norm * 2.0):
        for p, g in zip(ps, gs):
            p.grad.copy_(g)
        n_t = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        torch.testing.assert_close(torch.tensor(norm, dtype=torch.float64), n_t, **F64)
        coef = R.clip_coef(norm, max_norm)
        assert (coef == 1.0) == (max_norm > norm)
        for p, g in zip(ps, gs):
            torch.testing.assert_close(g * coef, p.grad, **F64)
    # weights and replicas enter the sum of squares, not the norm
    assert R.global_norm(gs, [0.5] * len(gs), replicas=2) == pytest.approx(norm, rel=1e-14)


# ---------------------------------------------------------------------------------- project CPU path
STORED = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _fused_cpu(kind, hyper, n_steps, sizes, group_of, seed, max_norm=None, change=None, stored="fp32"):
    """Run the fused optimizer's fp32 CPU path and the float64 reference on the GPU tests' inputs:
    the values as the GPU tests store them (rounded to ``stored``), held in fp32 like a master."""
    params, grads = R.make_inputs(seed, sizes)
    params = [p.to(STORED[stored]).float() for p in params]
    grads = [[g.to(STORED[stored]).float() for g in gs] for gs in grads]
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    groups = R.param_groups(ps, group_of, hyper)
    if kind == "adam":
        opt = FusedAdamW(groups, adam_w_mode=hyper[0]["adam_w_mode"], maximize=hyper[0]["maximize"])
    else:
        opt = FusedSGD(groups, maximize=hyper[0]["maximize"])
    opt.set_grad_clipping(max_norm)
    ref = R.Ref(kind, params, group_of, hyper)
    for s in range(n_steps):
        if change is not None and s == change[0]:
            for k, v in change[2].items():
                opt.param_groups[change[1]][k] = v
                hyper[change[1]][k] = v
        for p, g in zip(ps, grads[s]):
            p.grad = g.clone()
        opt.step()
        ref.step(grads[s], max_norm=max_norm)
    return ps, opt, ref


def _check_fp32(ps, opt, ref, state_keys):
    for i, p in enumerate(ps):
        torch.testing.assert_close(p.detach().double(), ref.w[i], **F32)
        for k, s in zip(state_keys, (ref.s0, ref.s1)):
            torch.testing.assert_close(opt.state[p][k].double(), s[i], **F32)


@pytest.mark.parametrize("adam_w_mode", [True, False])
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("stored", sorted(STORED))
def test_cpu_path_adam_on_gpu_inputs(adam_w_mode, maximize, stored):
    ps, opt, ref = _fused_cpu("adam", R.adam_hyper(adam_w_mode, maximize), R.STEPS, R.SIZES, R.GROUP_OF, 21,
                              stored=stored)
    _check_fp32(ps, opt, ref, ("exp_avg", "exp_avg_sq"))


@pytest.mark.parametrize("stored", sorted(STORED))
@pytest.mark.parametrize("seed,sizes,n_groups", [(21, R.SIZES, 3), (24, R.SIZES + (1023, 16385), 10)])
def test_gpu_inputs_keep_adams_first_step_well_conditioned(stored, seed, sizes, n_groups):
    """g + wd * p of the first step stays far above eps for either sign of g (see make_inputs)."""
    params, grads = R.make_inputs(seed, sizes)
    hyper = R.adam_hyper(False, n_groups=n_groups)
    group_of = R.GROUP_OF if n_groups == 3 else list(range(10))
    for p, g, gi in zip(params, grads[0], group_of):
        p, g = p.to(STORED[stored]).double(), g.to(STORED[stored]).double()
        wd = hyper[gi]["weight_decay"]
        assert float(torch.minimum((g + wd * p).abs(), (-g + wd * p).abs()).min()) > 0.1


@pytest.mark.parametrize("momentum", [True, False])
@pytest.mark.parametrize("maximize", [False, True])
@pytest.mark.parametrize("stored", sorted(STORED))
def test_cpu_path_sgd_on_gpu_inputs(momentum, maximize, stored):
    ps, opt, ref = _fused_cpu("sgd", R.sgd_hyper(momentum, maximize), R.STEPS, R.SIZES, R.GROUP_OF, 21,
                              stored=stored)
    _check_fp32(ps, opt, ref, ("momentum_buffer",) if momentum else ())


def test_cpu_path_mixed_momentum_on_gpu_inputs():
    ps, opt, ref = _fused_cpu("sgd", R.mixed_momentum_hyper(), 3, R.SIZES, [i % 2 for i in range(len(R.SIZES))], 23)
    for i, p in enumerate(ps):
        torch.testing.assert_close(p.detach().double(), ref.w[i], **F32)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_cpu_path_ten_groups_clip_and_hyper_change_on_gpu_inputs(kind):
    sizes = R.SIZES + (1023, 16385)
    hyper = R.adam_hyper(True, n_groups=10) if kind == "adam" else R.sgd_hyper(True, n_groups=10)
    ps, opt, ref = _fused_cpu(kind, hyper, 4, sizes, list(range(10)), 24, max_norm=50.0,
                              change=(2, 9, dict(lr=0.004, weight_decay=0.05)))
    _check_fp32(ps, opt, ref, ("exp_avg", "exp_avg_sq") if kind == "adam" else ("momentum_buffer",))
    assert float(opt.last_grad_norm) == pytest.approx(ref.last_norm, rel=1e-5)


def _clip_case(kind, stored, max_norm_of, n_steps, weighted=False, replicas=1):
    """The clipping cases of the GPU tests: ``max_norm`` is a multiple of the first step's (weighted,
    replicated) norm, the hyperparameters are the three-group ones, the seed is 21."""
    params, grads = R.make_inputs(21, R.SIZES)
    params = [p.to(STORED[stored]).float() for p in params]
    grads = [[g.to(STORED[stored]).float() for g in gs] for gs in grads]
    hyper = R.adam_hyper(True) if kind == "adam" else R.sgd_hyper(True)
    ps = [torch.nn.Parameter(p.clone()) for p in params]
    cls = FusedAdamW if kind == "adam" else FusedSGD
    opt = cls(R.param_groups(ps, R.GROUP_OF, hyper))
    weights = None
    if weighted:
        half = {id(p) for p in ps[::2]}
        weights = [0.5 if id(p) in half else 1.0 for p in ps]
        opt._norm_weight = lambda t: 0.5 if id(t) in half else 1.0
    if replicas == 2:
        opt._partial_reducer = lambda t: t.mul_(2.0)
    norm = R.global_norm(grads[0], weights, replicas)
    max_norm = norm * max_norm_of
    opt.set_grad_clipping(max_norm)
    ref = R.Ref(kind, params, R.GROUP_OF, hyper)
    for s in range(n_steps):
        for p, g in zip(ps, grads[s]):
            p.grad = g.clone()
        opt.step()
        ref.step(grads[s], max_norm=max_norm, norm_weights=weights, replicas=replicas)
        assert float(opt.last_grad_norm) == pytest.approx(ref.last_norm, rel=1e-5)
    _check_fp32(ps, opt, ref, ("exp_avg", "exp_avg_sq") if kind == "adam" else ("momentum_buffer",))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("stored", sorted(STORED))
@pytest.mark.parametrize("max_norm_of", [1.0 / 3.0, 2.0], ids=["below", "above"])
def test_cpu_path_clipping_on_gpu_inputs(kind, stored, max_norm_of):
    _clip_case(kind, stored, max_norm_of, 2)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("stored", ["fp32", "bf16"])
def test_cpu_path_weighted_norm_on_gpu_inputs(kind, stored):
    _clip_case(kind, stored, 1.0 / 3.0, 1, weighted=True)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
@pytest.mark.parametrize("stored", ["fp32", "bf16"])
def test_cpu_path_two_replicas_on_gpu_inputs(kind, stored):
    _clip_case(kind, stored, 1.0 / 3.0, 1, replicas=2)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_cpu_path_mixed_copy_dtypes_on_gpu_inputs(kind):
    """bf16 and fp16 parameters with fp32 gradients and fp32 masters (seed 41), three steps."""
    p32, g32 = R.make_inputs(41, R.MIXED_COPY_SIZES)
    ps = [torch.nn.Parameter(p.to(STORED[d]), requires_grad=False) for p, d in zip(p32, R.MIXED_COPY_DTYPES)]
    for p in ps:
        if hasattr(p, "grad_dtype"):
            p.grad_dtype = None
    hyper = R.single_group_hyper(kind)
    cls = FusedAdamW if kind == "adam" else FusedSGD
    opt = cls(R.param_groups(ps, [0] * len(ps), hyper), master_weights=True)
    ref = R.Ref(kind, [p.detach() for p in ps], [0] * len(ps), hyper)
    for s in range(3):
        for p, g in zip(ps, g32[s]):
            p.grad = g.clone()
        opt.step()
        ref.step(g32[s])
    for i, p in enumerate(ps):
        master = opt.state[p]["master"]
        torch.testing.assert_close(master.double(), ref.w[i], **F32)
        assert torch.equal(p.detach(), master.to(p.dtype))
