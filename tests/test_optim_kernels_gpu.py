"""The fused optimizer kernels (csrc/optim.hip) against the float64 reference of tests/optim_ref.py,
over gradient / parameter dtypes, operand alignment, chunk shapes and parameter groups.

Every operand is a ``narrow()`` view into a flat buffer (as the ZeRO engine hands them over), at an
element offset that decides between the vector and the scalar path; the gaps between the views hold a
sentinel that no kernel may touch.  Every comparison covers every element.

Operand names follow the kernels: ``p`` is what the kernel updates in fp32 or in place (the fp32
master when there is one, else the parameter), ``lp`` the 16-bit copy of a master, ``g`` the gradient,
``s`` the fp32 state tensors.

Known divergences from torch.optim that are out of scope here (neither tested nor changed):

* the step count is shared per device, so a parameter whose first gradient arrives late uses the
  global step for Adam's bias correction;
* for SGD with dampening, such a late parameter has its buffer initialised as ``(1-damp)*g``, not ``g``.
"""

import math

import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu

F32 = dict(rtol=1e-5, atol=1e-6)
DT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
# one unit in the last place, relative: 8 significand bits for bf16, 11 for fp16
ULP = {torch.bfloat16: 2.0**-7, torch.float16: 2.0**-10}
SENTINEL = 1234.0

# (parameter, gradient, master_weights)
ROWS = [
    ("fp32", "fp32", False),
    ("bf16", "bf16", True),
    ("fp16", "fp16", True),
    ("bf16", "fp32", True),
    ("fp16", "fp32", True),
    ("bf16", "bf16", False),
    ("fp16", "fp16", False),
    ("bf16", "fp32", False),
]
VARIANTS = ["adamw", "adam_l2", "sgd_mom", "sgd_plain"]
ALIGNED = dict(p=0, g=0, lp=0, s=0)
ALIGN = {"aligned": ALIGNED, "all1": dict(p=1, g=1, lp=1, s=1)}
for _r in ("p", "g", "lp", "s"):
    for _o in (1, 4, 8):
        ALIGN[f"{_r}{_o}"] = dict(ALIGNED, **{_r: _o})


@pytest.fixture(scope="module")
def ops():
    import determined_amd.ops as ops

    ops.ext()  # must load: these tests exist to exercise the native path
    return ops


def _kind(variant):
    return "adam" if variant.startswith("adam") else "sgd"


def _hyper(variant, maximize=False, n_groups=3):
    if variant == "adamw":
        return R.adam_hyper(True, maximize, n_groups)
    if variant == "adam_l2":
        return R.adam_hyper(False, maximize, n_groups)
    if variant == "sgd_mom":
        return R.sgd_hyper(True, maximize, n_groups)
    if variant == "sgd_plain":
        return R.sgd_hyper(False, maximize, n_groups)
    assert variant == "sgd_mixed"
    return R.mixed_momentum_hyper()


def _n_states(variant, hyper):
    if _kind(variant) == "adam":
        return 2
    return 1 if any(h["momentum"] != 0 for h in hyper) else 0


_INPUTS = {}


def _inputs(seed, sizes, dtype_p, dtype_g):
    """The shared CPU inputs as stored: parameters cast to the parameter dtype, gradients to the gradient dtype."""
    key = (seed, sizes)
    if key not in _INPUTS:
        _INPUTS[key] = R.make_inputs(seed, sizes)
    ck = key + (dtype_p, dtype_g)
    if ck not in _INPUTS:
        p32, g32 = _INPUTS[key]
        _INPUTS[ck] = ([p.to(dtype_p) for p in p32], [[g.to(dtype_g) for g in gs] for gs in g32])
    return _INPUTS[ck]


class Flat:
    """Views at element offset ``off`` from 16-element-aligned slots of one flat buffer, with sentinel gaps."""

    def __init__(self, sizes, dtype, off):
        cur, starts = 16, []
        for n in sizes:
            cur = (cur + 15) // 16 * 16 + 16
            starts.append(cur + off)
            cur += off + n
        total = (cur + 15) // 16 * 16 + 16
        self.buf = torch.full((total,), SENTINEL, dtype=dtype, device="cuda")
        assert self.buf.data_ptr() % 64 == 0
        self.views = [self.buf.narrow(0, s, n) for s, n in zip(starts, sizes)]
        gap = torch.ones(total, dtype=torch.bool)
        for s, n in zip(starts, sizes):
            gap[s:s + n] = False
        self.gap = gap.cuda()
        self.before = None

    def bits(self):
        return self.buf.view(BITS[self.buf.dtype])

    def snapshot(self):
        self.before = self.bits().clone()

    def assert_gaps_untouched(self, what):
        changed = (self.bits() != self.before) & self.gap
        assert not bool(changed.any()), f"{what}: {int(changed.sum())} elements outside the views were written"

    def assert_unchanged(self, what):
        assert torch.equal(self.bits(), self.before), f"{what}: changed"


class Case:
    """A fused optimizer over flat-buffer views, and the float64 reference fed with the same stored values."""

    def __init__(self, ops, variant, row, offs=ALIGNED, sizes=R.SIZES, group_of=R.GROUP_OF, seed=21,
                 maximize=False, hyper=None):
        pd, gd, master = row
        self.pd, self.gd, self.master = DT[pd], DT[gd], master
        self.variant, self.kind = variant, _kind(variant)
        self.sizes, self.group_of = tuple(sizes), list(group_of)
        self.hyper = hyper if hyper is not None else _hyper(variant, maximize, max(group_of) + 1)
        self.params_in, self.grads_in = _inputs(seed, self.sizes, self.pd, self.gd)
        self.P = Flat(sizes, self.pd, offs["lp"] if master else offs["p"])
        self.G = Flat(sizes, self.gd, offs["g"])
        self.M = Flat(sizes, torch.float32, offs["p"]) if master else None
        self.S = [Flat(sizes, torch.float32, offs["s"]) for _ in range(_n_states(variant, self.hyper))]
        self.ps = []
        for v, g, src in zip(self.P.views, self.G.views, self.params_in):
            v.copy_(src)
            p = torch.nn.Parameter(v, requires_grad=self.pd == self.gd)
            if self.pd != self.gd and hasattr(p, "grad_dtype"):
                p.grad_dtype = None
            p.grad = g
            self.ps.append(p)
        groups = R.param_groups(self.ps, self.group_of, self.hyper)
        if self.kind == "adam":
            self.opt = ops.FusedAdamW(groups, adam_w_mode=self.hyper[0]["adam_w_mode"],
                                      maximize=self.hyper[0]["maximize"], master_weights=master)
        else:
            self.opt = ops.FusedSGD(groups, maximize=self.hyper[0]["maximize"], master_weights=master)
        # move the optimizer's state into flat-buffer views of its own
        for i, p in enumerate(self.ps):
            st = self.opt.state[p]
            self.opt._init_state(p, st)
            for k, flat in zip(self.opt._state_keys, self.S):
                st[k] = flat.views[i].zero_()
            if master:
                st["master"] = self.M.views[i].copy_(self.opt._master(p, st))
        assert len(self.opt._state_keys) == len(self.S)
        self.flats = [self.P, self.G] + ([self.M] if master else []) + self.S
        for f in self.flats:
            f.snapshot()
        self.ref = R.Ref(self.kind, self.params_in, self.group_of, self.hyper)
        self.n = 0

    def load_grads(self, s):
        for v, g in zip(self.G.views, self.grads_in[s]):
            v.copy_(g)
        return self.grads_in[s]

    def step(self, ref=True, max_norm=None, **kw):
        gs = self.load_grads(self.n)
        self.n += 1
        self.opt.step(**kw)
        if ref:
            self.ref.step(gs, max_norm=max_norm)

    def check(self, ref=None):
        ref = ref or self.ref
        what = f"{self.variant} p={self.pd} g={self.gd} master={self.master}"
        for i, p in enumerate(self.ps):
            st = self.opt.state[p]
            tag = lambda m, i=i: f"{what} tensor {i} (n={self.sizes[i]}, group {self.group_of[i]}): {m}"
            for k, s in zip(self.opt._state_keys, (ref.s0, ref.s1)):
                torch.testing.assert_close(st[k].cpu().double(), s[i], msg=lambda m, k=k: tag(f"{k}: {m}"), **F32)
            if self.master:
                torch.testing.assert_close(st["master"].cpu().double(), ref.w[i],
                                           msg=lambda m: tag(f"master: {m}"), **F32)
                # the 16-bit parameter is bit for bit the round-to-nearest-even cast of its own master
                want = st["master"].to(self.pd)
                assert p.dtype == self.pd and torch.equal(p.detach().view(torch.int16), want.view(torch.int16)), \
                    tag("16-bit parameter is not the exact cast of its master")
            elif self.pd == torch.float32:
                torch.testing.assert_close(p.detach().cpu().double(), ref.w[i], msg=lambda m: tag(f"param: {m}"), **F32)
            else:
                _assert_within_ulp(p.detach(), ref.w[i], tag("param"))
        for f, name in zip(self.flats, ["param", "grad"] + (["master"] if self.master else []) + ["s0", "s1"]):
            f.assert_gaps_untouched(f"{what} {name} buffer")

    def assert_grads_untouched(self, s):
        for v, g in zip(self.G.views, self.grads_in[s]):
            assert torch.equal(v.cpu().view(BITS[g.dtype]), g.view(BITS[g.dtype])), "step() changed a gradient"


def _assert_within_ulp(stored, ref64, what):
    """``stored`` (16-bit) within one unit in the last place of the float64 value rounded to its dtype."""
    want = ref64.to(stored.dtype).double()
    err = (stored.cpu().double() - want).abs()
    bad = ~(err <= ULP[stored.dtype] * want.abs())
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond one ulp, worst {float(err.max())}"


def _steps_for(row):
    # a 16-bit parameter without a master diverges by its own rounding over several steps: one step
    return R.STEPS if (row[0] == "fp32" or row[2]) else 1


def _matrix_cases():
    out = []
    for variant in VARIANTS:
        for row in ROWS:
            for name, offs in ALIGN.items():
                if name.startswith("lp") and not row[2]:
                    continue  # no 16-bit copy without a master
                if name.startswith("s") and variant == "sgd_plain":
                    continue  # no state tensor
                out.append(pytest.param(variant, row, name, id=f"{variant}-{row[0]}-{row[1]}-{'m' if row[2] else 'n'}-{name}"))
    return out


class FrozenRef:
    """A copy of a finished reference's tensors: shared between the alignment cases, owned by none."""

    def __init__(self, ref):
        self.w, self.s0, self.s1 = ([t.clone() for t in ts] for ts in (ref.w, ref.s0, ref.s1))


_REF_CACHE = {}


@pytest.mark.parametrize("variant,row,align", _matrix_cases())
def test_dtype_alignment_matrix(ops, variant, row, align):
    c = Case(ops, variant, row, ALIGN[align])
    n = _steps_for(row)
    key = (variant, row)
    have = key in _REF_CACHE  # the reference does not depend on the alignment: computed once
    for _ in range(n):
        c.step(ref=not have)
    if not have:
        _REF_CACHE[key] = FrozenRef(c.ref)
    c.check(_REF_CACHE[key])


@pytest.mark.parametrize("variant", ["adamw", "sgd_mom"])
@pytest.mark.parametrize("row", [ROWS[0], ROWS[1]], ids=["fp32", "bf16m"])
def test_ten_groups_second_launch(ops, variant, row):
    sizes = R.SIZES + (1023, 16385)
    c = Case(ops, variant, row, ALIGN["all1"], sizes=sizes, group_of=list(range(10)), seed=24)
    assert len(c.opt.param_groups) == 10
    for _ in range(R.STEPS):
        c.step()
    assert len([k for k in c.opt._plans if k != "__fast__"]) == 2  # groups 8 and 9 are a launch of their own
    c.check()


@pytest.mark.parametrize("row", [ROWS[0], ROWS[1]], ids=["fp32", "bf16m"])
def test_sgd_mixed_momentum_groups(ops, row):
    """A momentum-free group next to a momentum group ignores its dampening (torch semantics)."""
    c = Case(ops, "sgd_mixed", row, group_of=[i % 2 for i in range(len(R.SIZES))], seed=23)
    for _ in range(3):
        c.step()
    c.check()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("row", [ROWS[0], ROWS[1], ROWS[4]], ids=["fp32", "bf16m", "fp16-fp32m"])
def test_maximize(ops, variant, row):
    c = Case(ops, variant, row, ALIGN["g1"], maximize=True)
    for _ in range(R.STEPS):
        c.step()
    c.check()


@pytest.mark.parametrize("variant", ["adamw", "adam_l2", "sgd_mom"])
def test_hyperparameters_changed_between_steps(ops, variant):
    c = Case(ops, variant, ROWS[0])
    c.step()
    c.step()
    for k, v in dict(lr=0.004, weight_decay=0.05).items():
        c.opt.param_groups[1][k] = v
        c.hyper[1][k] = v  # the reference reads the same list
    c.step()
    c.step()
    c.check()


# ---------------------------------------------------------------------------------- clipping
CLIP_ROWS = [ROWS[0], ROWS[1], ROWS[2]]


def _norm_close(got, want):
    assert float(got) == pytest.approx(want, rel=1e-5), (float(got), want)


@pytest.mark.parametrize("variant", ["adamw", "sgd_mom"])
@pytest.mark.parametrize("row", CLIP_ROWS, ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("align", ["aligned", "all1", "g1", "g4", "g8"])
@pytest.mark.parametrize("above", [False, True])
def test_clipping_inside_step(ops, variant, row, align, above):
    c = Case(ops, variant, row, ALIGN[align])
    norm = R.global_norm(c.grads_in[0])
    max_norm = norm * 2.0 if above else norm / 3.0
    c.opt.set_grad_clipping(max_norm)
    c.step(max_norm=max_norm)
    _norm_close(c.opt.last_grad_norm, norm)
    assert (R.clip_coef(norm, max_norm) == 1.0) == above
    c.step(max_norm=max_norm)
    _norm_close(c.opt.last_grad_norm, c.ref.last_norm)
    c.check()
    c.assert_grads_untouched(1)  # the clip is applied inside the update


@pytest.mark.parametrize("gdtypes", [("fp32",), ("bf16",), ("fp16",), ("fp32", "bf16")], ids=lambda g: "+".join(g))
@pytest.mark.parametrize("off", [0, 1, 4, 8])
@pytest.mark.parametrize("above", [False, True])
def test_fused_clip_grad_norm(ops, gdtypes, off, above):
    flats, params, stored = [], [], []
    for j, gd in enumerate(gdtypes):
        _, grads = _inputs(31 + j, R.SIZES, DT[gd], DT[gd])
        G = Flat(R.SIZES, DT[gd], off)
        for v, g in zip(G.views, grads[0]):
            v.copy_(g)
            p = torch.nn.Parameter(torch.zeros_like(v))
            p.grad = v
            params.append(p)
        stored += grads[0]
        G.snapshot()
        flats.append(G)
    norm = R.global_norm(stored)
    max_norm = norm * 2.0 if above else norm / 2.0
    got = ops.fused_clip_grad_norm_(params, max_norm)
    _norm_close(got, norm)
    coef = R.clip_coef(norm, max_norm)
    assert (coef == 1.0) == above
    for G in flats:
        G.assert_gaps_untouched("gradient buffer")
        if above:
            G.assert_unchanged("gradients under a max_norm above their norm")
    for i, (p, g) in enumerate(zip(params, stored)):
        want = g.double() * coef
        if g.dtype == torch.float32:
            torch.testing.assert_close(p.grad.cpu().double(), want, **F32)
        else:
            _assert_within_ulp(p.grad, want, f"clipped {g.dtype} gradient {i}")


@pytest.mark.parametrize("variant", ["adamw", "sgd_mom"])
@pytest.mark.parametrize("row", [ROWS[0], ROWS[1]], ids=["fp32", "bf16m"])
def test_weighted_norm(ops, variant, row):
    c = Case(ops, variant, row, ALIGN["g1"])
    half = {id(p) for p in c.ps[::2]}
    weights = [0.5 if id(p) in half else 1.0 for p in c.ps]
    c.opt._norm_weight = lambda t: 0.5 if id(t) in half else 1.0
    norm = R.global_norm(c.grads_in[0], weights)
    assert norm < 0.95 * R.global_norm(c.grads_in[0])
    max_norm = norm / 3.0
    c.opt.set_grad_clipping(max_norm)
    c.load_grads(0)
    c.opt.step()
    c.ref.step(c.grads_in[0], max_norm=max_norm, norm_weights=weights)
    _norm_close(c.opt.last_grad_norm, norm)
    c.check()


@pytest.mark.parametrize("variant", ["adamw", "sgd_mom"])
@pytest.mark.parametrize("row", [ROWS[0], ROWS[1]], ids=["fp32", "bf16m"])
def test_partial_reducer_two_identical_ranks(ops, variant, row):
    c = Case(ops, variant, row, ALIGN["g1"])
    c.opt._partial_reducer = lambda t: t.mul_(2.0)
    local = R.global_norm(c.grads_in[0])
    max_norm = local / 3.0
    c.opt.set_grad_clipping(max_norm)
    c.load_grads(0)
    c.opt.step()
    c.ref.step(c.grads_in[0], max_norm=max_norm, replicas=2)
    _norm_close(c.opt.last_grad_norm, math.sqrt(2.0) * local)
    c.check()


# ---------------------------------------------------------------------------------- non-finite gradients
# (tensor index into R.SIZES, element, gradient offset)
PLACES = {
    "first": (4, 0, 0),
    "chunk_end": (4, 16383, 0),
    "tail_end": (7, 40000, 0),      # 40001 - 2 * 16384 = 7233 elements, not a multiple of 4
    "single": (5, 16384, 0),        # the n == 1 chunk of the 16385-element tensor
    "misaligned": (6, 5, 1),
}


@pytest.mark.parametrize("row", [ROWS[0], ROWS[1], ROWS[2]], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("place", sorted(PLACES))
@pytest.mark.parametrize("value", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_skips_the_step(ops, row, place, value):
    ti, ei, off = PLACES[place]
    assert R.SIZES[ti] > ei
    c = Case(ops, "adamw", row, dict(ALIGNED, g=off))
    c.load_grads(0)
    c.G.views[ti][ei] = value
    held = [f for f in c.flats if f is not c.G]
    for f in held:
        f.snapshot()
    c.opt.step(check_finite=True)
    dev = c.ps[0].device
    assert int(c.opt._aux[dev]["found_inf"].item()) == 1
    for f in held:
        f.assert_unchanged("parameter / state buffer after a skipped step")
    assert float(c.opt._step_tensor(dev).item()) == 0.0
    # a clean step then updates normally, with the bias correction of step 1
    c.step(check_finite=True)
    assert int(c.opt._aux[dev]["found_inf"].item()) == 0
    assert float(c.opt._step_tensor(dev).item()) == 1.0
    c.check()


# ---------------------------------------------------------------------------------- dispatch
def _one_chunk_table(ops, g_dtype, lp_dtype):
    n = 64
    p = torch.ones(n, device="cuda")
    g = torch.zeros(n, device="cuda", dtype=g_dtype)
    s0, s1 = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    lp = torch.zeros(n, device="cuda", dtype=lp_dtype)
    keep = (p, g, s0, s1, lp)
    return ops.ext().build_chunk_table([p], [g], [s0], [s1], [lp], [0], 16384), keep


BAD_DTYPES = [(0, 1, 2), (0, 2, 1), (3, 0, 0), (-1, 0, 0), (0, 3, 0), (0, -1, 0), (0, 0, 3), (0, 0, -1),
              (1, 2, 0), (2, 1, 0), (1, 1, 1), (2, 0, 2)]


@pytest.mark.parametrize("codes", BAD_DTYPES, ids=lambda c: "p%d_g%d_lp%d" % c)
def test_unserved_dtype_combinations_raise(ops, codes):
    e = ops.ext()
    pd, gd, lp = codes
    step = torch.ones(1, device="cuda")
    tables = [torch.empty(0, dtype=torch.uint8, device="cuda")]
    keep = None
    if codes in ((0, 1, 2), (0, 2, 1)):  # every operand of these is what the table says: a real table too
        t, keep = _one_chunk_table(ops, DT["bf16"] if gd == 1 else DT["fp16"], DT["fp16"] if lp == 2 else DT["bf16"])
        tables.append(t)
    for table in tables:
        with pytest.raises(RuntimeError):
            e.adam_step(table, [1e-3], [0.1], [0.9], [0.99], [1e-8], [1], None, None, step, False, pd, gd, lp, None)
        for mom in (True, False):
            with pytest.raises(RuntimeError):
                e.sgd_step(table, [1e-3], [0.1], [0.9], [0.0], [0], None, None, step, False, pd, gd, lp, mom, None)
    if keep is not None:
        torch.cuda.synchronize()
        # refused before any launch: the decay alone would have moved the parameter
        assert bool((keep[0] == 1).all()) and all(not bool(t.any()) for t in keep[1:])


@pytest.mark.parametrize("g_dtype", [3, -1])
def test_unknown_gradient_dtype_code_raises(ops, g_dtype):
    e = ops.ext()
    table = torch.empty(0, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        e.l2norm_partial(table, torch.zeros(1, device="cuda"), g_dtype)
    with pytest.raises(RuntimeError):
        e.scale_grads(table, torch.ones(1, device="cuda"), g_dtype)


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_bf16_and_fp16_copies_in_one_model(ops, kind):
    """One bf16 and one fp16 parameter, both with fp32 gradients: each copy is written in its own format."""
    sizes, dts = R.MIXED_COPY_SIZES, [DT[d] for d in R.MIXED_COPY_DTYPES]
    p32, g32 = _inputs(41, sizes, torch.float32, torch.float32)
    ps = []
    for src, dt in zip(p32, dts):
        p = torch.nn.Parameter(src.to(dt).cuda(), requires_grad=False)
        if hasattr(p, "grad_dtype"):
            p.grad_dtype = None
        ps.append(p)
    hyper = R.single_group_hyper(kind)
    cls = ops.FusedAdamW if kind == "adam" else ops.FusedSGD
    opt = cls(R.param_groups(ps, [0] * len(ps), hyper), master_weights=True)
    ref = R.Ref(kind, [p.detach() for p in ps], [0] * len(ps), hyper)
    for s in range(3):
        for p, g in zip(ps, g32[s]):
            p.grad = g.cuda()
        opt.step()
        ref.step(g32[s])
    for i, p in enumerate(ps):
        master = opt.state[p]["master"]
        torch.testing.assert_close(master.cpu().double(), ref.w[i], **F32)
        assert torch.equal(p.detach().view(torch.int16), master.to(p.dtype).view(torch.int16)), \
            f"{p.dtype} parameter {i} is not the exact cast of its master"
