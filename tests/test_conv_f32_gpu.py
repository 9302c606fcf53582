"""The fp32 backbone convolutions of include/pd_conv_f32.h against torch on the CPU in float64.

The tolerance is derived, not measured.  An output that sums n products in any order of f32 fma accumulation with S partial sums obeys
    |got - exact| <= gamma * M,   gamma = (n + S + 4) u / (1 - (n + S + 4) u),   u = 2^-24,
M = the same expression in float64 on absolute values (conv(|x|, |w|) |scale| + |bias| + |residual|, likewise for the gradients); the 4
covers the epilogue's multiply and adds.  S is stated as 64, the largest partition the filter gradient uses (it only loosens the bound
harmlessly for the kernels that keep one sum).  Asserted elementwise with no extra margin: at these sizes the bound is ~1e-5 relative
while a missing tap or term is ~1e-2."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
S_MAX = 64
INVALID = -1

# (batch, hi, wi, ci, co, k, stride)
CASES = [
    (2, 5, 7, 64, 64, 1, 1),
    (2, 5, 7, 128, 192, 1, 1),          # several K-steps and N-tiles
    (2, 9, 6, 64, 64, 1, 2),            # -> 5 x 3
    (2, 8, 8, 64, 128, 1, 2),
    (2, 5, 7, 64, 64, 3, 1),
    (2, 1, 1, 64, 64, 3, 1),            # eight of nine taps outside
    (1, 33, 35, 64, 64, 3, 1),          # several pixel tiles, ragged last tile
    (2, 9, 6, 64, 128, 3, 2),
    (2, 8, 7, 64, 128, 3, 2),
    (2, 5, 7, 128, 128, 1, 1),          # the 128-wide tiles of forward and filter gradient
    (1, 6, 5, 128, 128, 3, 1),          # ... with taps
]
STEM_CASES = [(2, 17, 22, 64), (2, 8, 8, 64)]         # (batch, hi, wi, co): -> 9 x 11 and 4 x 4
IDS = ["b%d_%dx%d_%dto%d_k%ds%d" % c for c in CASES]
STEM_IDS = ["b%d_%dx%d_co%d" % c for c in STEM_CASES]


def gamma(n):
    e = (n + S_MAX + 4) * U
    return e / (1 - e)


def L():
    from partdistillation_amd import lib
    return lib.load()


def stream():
    from partdistillation_amd import lib
    return lib.current_stream()


def out_size(h, k, s):
    return (h + 2 * (k // 2) - k) // s + 1


def normal(shape, seed, exact):
    g = torch.Generator().manual_seed(seed)
    if exact:                                           # small integers: every sum below 2^24 is exact in f32 in any order
        return torch.randint(-2, 3, shape, generator=g).float()
    return torch.randn(shape, generator=g)


def nchw(t):
    """NHWC-shaped float32 tensor -> NCHW-shaped float64"""
    return t.double().permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_refs(x, w, dz, k, s, p):
    """float64: (conv(x, w), its gradient w.r.t. x given dz, its gradient w.r.t. w given dz), all in the kernels' layouts"""
    x64 = nchw(x).requires_grad_(True)
    w64 = w.double().permute(0, 3, 1, 2).requires_grad_(True)             # [co][k][k][ci] -> [co][ci][k][k]
    y = F.conv2d(x64, w64, None, s, p)
    dx, dw = torch.autograd.grad(y, (x64, w64), nchw(dz))
    return nhwc(y.detach()), nhwc(dx), nhwc(dw)


@functools.lru_cache(maxsize=None)
def problem(case, exact=False):
    """operands (CPU float32, kernel layouts) and the float64 references of one case: computed once, shared, never modified"""
    B, hi, wi, ci, co, k, s = case
    p, ho, wo = k // 2, out_size(hi, k, s), out_size(wi, k, s)
    o = dict(B=B, hi=hi, wi=wi, ci=ci, co=co, k=k, s=s, p=p, ho=ho, wo=wo)
    o["x"] = normal((B, hi, wi, ci), 1, exact)
    o["w"] = normal((co, k, k, ci), 2, exact)                              # asymmetric: independent draws per (co, tap, ci)
    o["dz"] = normal((B, ho, wo, co), 3, exact)
    o["res"] = normal((B, ho, wo, co), 4, exact)
    o["add"] = normal((B, hi, wi, ci), 5, exact)
    g = torch.Generator().manual_seed(6)
    o["scale"] = torch.randint(1, 4, (co,), generator=g).float() if exact else 0.5 + torch.rand(co, generator=g)
    o["bias"] = normal((co,), 7, exact)
    o["y"], o["dx"], o["dw"] = conv_refs(o["x"], o["w"], o["dz"], k, s, p)
    o["y_abs"], o["dx_abs"], o["dw_abs"] = conv_refs(o["x"].abs(), o["w"].abs(), o["dz"].abs(), k, s, p)
    return o


@functools.lru_cache(maxsize=None)
def stem_problem(case, exact=False):
    B, hi, wi, co = case
    ho, wo = out_size(hi, 7, 2), out_size(wi, 7, 2)
    o = dict(B=B, hi=hi, wi=wi, co=co, ho=ho, wo=wo)
    o["x"] = normal((B, hi, wi, 3), 11, exact)
    o["w"] = normal((co, 7, 7, 3), 12, exact)
    o["dz"] = normal((B, ho, wo, co), 13, exact)
    g = torch.Generator().manual_seed(16)
    o["scale"] = torch.randint(1, 4, (co,), generator=g).float() if exact else 0.5 + torch.rand(co, generator=g)
    o["bias"] = normal((co,), 17, exact)
    o["y"], _, o["dw"] = conv_refs(o["x"], o["w"], o["dz"], 7, 2, 3)
    o["y_abs"], _, o["dw_abs"] = conv_refs(o["x"].abs(), o["w"].abs(), o["dz"].abs(), 7, 2, 3)
    return o


def ptr(t):
    return t.data_ptr() if t is not None else None


def run_fwd(o, scale, bias, res, relu):
    x, w = o["x"].to(DEV), o["w"].to(DEV)
    sc, bi, rs = (t.to(DEV) if t is not None else None for t in (scale, bias, res))
    y = torch.full((o["B"], o["ho"], o["wo"], o["co"]), float("nan"), device=DEV)
    rc = L().pd_conv_f32_fwd(x.data_ptr(), w.data_ptr(), ptr(sc), ptr(bi), ptr(rs), y.data_ptr(), o["B"], o["hi"], o["wi"], o["ci"], o["ho"], o["wo"],
                             o["co"], o["k"], o["s"], o["p"], int(relu), stream())
    assert rc == 0
    return y.cpu()


def run_dgrad(o, addend, alias=False):
    dz = o["dz"].to(DEV)
    wt = o["w"].permute(3, 1, 2, 0).contiguous().to(DEV)                   # [ci][k][k][co]
    ad = addend.to(DEV) if addend is not None else None
    dx = ad if alias else torch.full((o["B"], o["hi"], o["wi"], o["ci"]), float("nan"), device=DEV)
    rc = L().pd_conv_f32_dgrad(dz.data_ptr(), wt.data_ptr(), ptr(ad), dx.data_ptr(), o["B"], o["hi"], o["wi"], o["ci"], o["ho"], o["wo"], o["co"],
                               o["k"], o["s"], o["p"], stream())
    assert rc == 0
    return dx.cpu()


def run_wgrad(o, scale, fill=float("nan")):
    dz, x = o["dz"].to(DEV), o["x"].to(DEV)
    sc = scale.to(DEV) if scale is not None else None
    n = int(L().pd_conv_f32_wgrad_workspace_floats(o["B"], o["ho"], o["wo"], o["ci"], o["co"], o["k"]))
    total = o["co"] * o["k"] * o["k"] * o["ci"]
    assert n % total == 0 and 1 <= n // total <= S_MAX
    ws = torch.full((n,), fill, device=DEV)                                 # whatever the workspace held must not matter
    dw = torch.full((o["co"], o["k"], o["k"], o["ci"]), float("nan"), device=DEV)
    rc = L().pd_conv_f32_wgrad(dz.data_ptr(), x.data_ptr(), ptr(sc), dw.data_ptr(), ws.data_ptr(), n, o["B"], o["hi"], o["wi"], o["ci"], o["ho"],
                               o["wo"], o["co"], o["k"], o["s"], o["p"], stream())
    assert rc == 0
    return dw.cpu()


def run_stem_fwd(o, scale, bias, relu):
    x, w = o["x"].to(DEV), o["w"].to(DEV)
    sc, bi = (t.to(DEV) if t is not None else None for t in (scale, bias))
    y = torch.full((o["B"], o["ho"], o["wo"], o["co"]), float("nan"), device=DEV)
    rc = L().pd_stem7x7_f32_fwd(x.data_ptr(), w.data_ptr(), ptr(sc), ptr(bi), y.data_ptr(), o["B"], o["hi"], o["wi"], o["ho"], o["wo"], o["co"],
                                int(relu), stream())
    assert rc == 0
    return y.cpu()


def run_stem_wgrad(o, scale, fill=float("nan")):
    dz, x = o["dz"].to(DEV), o["x"].to(DEV)
    sc = scale.to(DEV) if scale is not None else None
    n = int(L().pd_conv_f32_wgrad_workspace_floats(o["B"], o["ho"], o["wo"], 3, o["co"], 7))
    assert n % (o["co"] * 147) == 0 and 1 <= n // (o["co"] * 147) <= S_MAX
    ws = torch.full((n,), fill, device=DEV)
    dw = torch.full((o["co"], 7, 7, 3), float("nan"), device=DEV)
    rc = L().pd_stem7x7_f32_wgrad(dz.data_ptr(), x.data_ptr(), ptr(sc), dw.data_ptr(), ws.data_ptr(), n, o["B"], o["hi"], o["wi"], o["ho"], o["wo"],
                                  o["co"], stream())
    assert rc == 0
    return dw.cpu()


def check(got, ref, mag, n, exact, what):
    assert got.shape == ref.shape, what
    assert torch.isfinite(got).all(), what
    err = (got.double() - ref).abs()
    if exact:
        assert torch.equal(got.double(), ref), f"{what}: {int((err > 0).sum())} elements differ, max {float(err.max())}"
        return
    bound = gamma(n) * mag
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, max err/bound {worst:.3f}, gamma {gamma(n):.3e}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} elements past the bound, worst err/bound {worst:.3f}"


# (scale, bias, residual, relu)
FWD_VARIANTS = [(False, False, False, False), (True, True, True, True), (True, True, False, True), (False, False, True, False),
                (True, False, False, False)]


def fwd_ref(o, sc, bi, rs, relu):
    y, m = o["y"], o["y_abs"]
    if sc:
        y, m = y * o["scale"].double(), m * o["scale"].double().abs()
    if bi:
        y, m = y + o["bias"].double(), m + o["bias"].double().abs()
    if rs:
        y, m = y + o["res"].double(), m + o["res"].double().abs()
    return (y.clamp_min(0) if relu else y), m                            # |relu(a) - relu(b)| <= |a - b|: the bound survives the ReLU


def all_fwd(o, exact, n):
    for sc, bi, rs, relu in FWD_VARIANTS:
        got = run_fwd(o, o["scale"] if sc else None, o["bias"] if bi else None, o["res"] if rs else None, relu)
        ref, m = fwd_ref(o, sc, bi, rs, relu)
        check(got, ref, m, n, exact, f"fwd scale={sc} bias={bi} residual={rs} relu={relu}")


def all_dgrad(o, exact, n):
    check(run_dgrad(o, None), o["dx"], o["dx_abs"], n, exact, "dgrad")
    ref, m = o["dx"] + o["add"].double(), o["dx_abs"] + o["add"].double().abs()
    check(run_dgrad(o, o["add"]), ref, m, n, exact, "dgrad + addend")
    check(run_dgrad(o, o["add"].clone(), alias=True), ref, m, n, exact, "dgrad + addend, dx aliases it")


def all_wgrad(o, exact, n):
    check(run_wgrad(o, None), o["dw"], o["dw_abs"], n, exact, "wgrad")
    sc = o["scale"].double().view(-1, 1, 1, 1)
    check(run_wgrad(o, o["scale"]), o["dw"] * sc, o["dw_abs"] * sc.abs(), n, exact, "wgrad * scale")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward(case):
    o = problem(case)
    all_fwd(o, False, o["k"] ** 2 * o["ci"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_dgrad(case):
    o = problem(case)
    all_dgrad(o, False, o["k"] ** 2 * o["co"])
    if o["k"] == 1 and o["s"] == 2:                                        # pixels that no tap reaches: zeros, not garbage
        dx = run_dgrad(o, None)
        assert (dx[:, 1::2] == 0).all() and (dx[:, :, 1::2] == 0).all()
        assert (dx[:, 0::2, 0::2] != 0).any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad(case):
    o = problem(case)
    all_wgrad(o, False, o["B"] * o["ho"] * o["wo"])


@pytest.mark.parametrize("case", STEM_CASES, ids=STEM_IDS)
def test_stem(case):
    o = stem_problem(case)
    for sc, bi, relu in [(False, False, False), (True, True, True), (True, False, False)]:
        got = run_stem_fwd(o, o["scale"] if sc else None, o["bias"] if bi else None, relu)
        y, m = o["y"], o["y_abs"]
        if sc:
            y, m = y * o["scale"].double(), m * o["scale"].double().abs()
        if bi:
            y, m = y + o["bias"].double(), m + o["bias"].double().abs()
        check(got, y.clamp_min(0) if relu else y, m, 147, False, f"stem fwd scale={sc} bias={bi} relu={relu}")
    n = o["B"] * o["ho"] * o["wo"]
    check(run_stem_wgrad(o, None), o["dw"], o["dw_abs"], n, False, "stem wgrad")
    sc = o["scale"].double().view(-1, 1, 1, 1)
    check(run_stem_wgrad(o, o["scale"]), o["dw"] * sc, o["dw_abs"] * sc.abs(), n, False, "stem wgrad * scale")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_data(case):
    """small-integer operands: every sum is exact in f32 whatever its order, so the result equals the float64 reference bit for bit —
    a swapped row / column or a wrong tap cannot hide inside a bound"""
    o = problem(case, True)
    all_fwd(o, True, 0)
    all_dgrad(o, True, 0)
    all_wgrad(o, True, 0)


@pytest.mark.parametrize("case", STEM_CASES, ids=STEM_IDS)
def test_exact_data_stem(case):
    o = stem_problem(case, True)
    y = o["y"] * o["scale"].double() + o["bias"].double()
    check(run_stem_fwd(o, o["scale"], o["bias"], True), y.clamp_min(0), None, 0, True, "stem fwd")
    check(run_stem_fwd(o, None, None, False), o["y"], None, 0, True, "stem fwd, bare")
    check(run_stem_wgrad(o, o["scale"]), o["dw"] * o["scale"].double().view(-1, 1, 1, 1), None, 0, True, "stem wgrad * scale")


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[6], CASES[8], CASES[10]], ids=[IDS[i] for i in (1, 3, 6, 8, 10)])
def test_repeatable(case):
    """two launches on the same operands give identical bits; the filter gradient's result does not depend on what its workspace held"""
    o = problem(case)
    assert torch.equal(run_fwd(o, o["scale"], o["bias"], o["res"], True), run_fwd(o, o["scale"], o["bias"], o["res"], True))
    assert torch.equal(run_dgrad(o, o["add"]), run_dgrad(o, o["add"]))
    assert torch.equal(run_wgrad(o, o["scale"], fill=float("nan")), run_wgrad(o, o["scale"], fill=3.0))


def test_repeatable_stem():
    o = stem_problem(STEM_CASES[0])
    assert torch.equal(run_stem_fwd(o, o["scale"], o["bias"], True), run_stem_fwd(o, o["scale"], o["bias"], True))
    assert torch.equal(run_stem_wgrad(o, o["scale"], fill=float("nan")), run_stem_wgrad(o, o["scale"], fill=3.0))


@pytest.mark.parametrize("ci,co,k,s,p", [(32, 64, 3, 1, 1), (64, 96, 3, 1, 1), (64, 64, 5, 1, 2), (64, 64, 3, 3, 1), (64, 64, 3, 1, 0), (64, 64, 1, 1, 1)],
                         ids=["ci32", "co96", "k5", "stride3", "k3pad0", "k1pad1"])
def test_guards(ci, co, k, s, p):
    """an unsupported convolution is refused by every entry point, says no in pd_conv_f32_supported, and no buffer is written"""
    lib = L()
    assert lib.pd_conv_f32_supported(ci, co, k, s, p) == 0
    B, hi, wi = 1, 6, 6
    ho = wo = (hi + 2 * p - k) // s + 1
    big = 4096 * 64
    x, w, dz, ws = (torch.ones(big, device=DEV) for _ in range(4))
    out = torch.full((big,), -7.0, device=DEV)
    st = stream()
    assert lib.pd_conv_f32_fwd(x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), B, hi, wi, ci, ho, wo, co, k, s, p, 1, st) == INVALID
    assert lib.pd_conv_f32_dgrad(dz.data_ptr(), w.data_ptr(), None, out.data_ptr(), B, hi, wi, ci, ho, wo, co, k, s, p, st) == INVALID
    assert lib.pd_conv_f32_wgrad(dz.data_ptr(), x.data_ptr(), None, out.data_ptr(), ws.data_ptr(), big, B, hi, wi, ci, ho, wo, co, k, s, p, st) == INVALID
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (ws == 1.0).all()
    assert b"pd_conv_f32" in lib.pd_last_error()


def test_supported_says_yes():
    lib = L()
    for ci, co, k, s in [(64, 64, 1, 1), (256, 64, 1, 1), (64, 64, 3, 1), (128, 128, 3, 2), (256, 512, 1, 2), (1024, 2048, 1, 2), (512, 512, 3, 1)]:
        assert lib.pd_conv_f32_supported(ci, co, k, s, k // 2) == 1


def test_sizes_that_do_not_belong_together_are_refused():
    lib = L()
    x, w = torch.ones(64 * 64 * 16, device=DEV), torch.ones(64 * 64 * 9, device=DEV)
    out = torch.full((64 * 64 * 16,), -7.0, device=DEV)
    assert lib.pd_conv_f32_fwd(x.data_ptr(), w.data_ptr(), None, None, None, out.data_ptr(), 1, 4, 4, 64, 5, 4, 64, 3, 1, 1, 0, stream()) == INVALID
    assert lib.pd_stem7x7_f32_fwd(x.data_ptr(), w.data_ptr(), None, None, out.data_ptr(), 1, 8, 8, 4, 4, 32, 0, stream()) == INVALID
    assert lib.pd_conv_f32_wgrad(x.data_ptr(), x.data_ptr(), None, out.data_ptr(), w.data_ptr(), 8, 1, 4, 4, 64, 4, 4, 64, 3, 1, 1, stream()) == INVALID
    torch.cuda.synchronize()
    assert (out == -7.0).all()


# ---------------------------------------------------------------------------------------------- the autograd Functions
def test_function_conv_bn_act():
    """functions/conv_f32.conv_bn_act: forward, and a backward whose pieces are the float64 gradients taken with the forward's own ReLU mask"""
    from partdistillation_amd.functions import conv_f32
    o = problem(CASES[8])                                                   # 3 x 3 stride 2, 64 -> 128
    k, s, p = o["k"], o["s"], o["p"]
    cl = lambda t: t.permute(0, 3, 1, 2).to(DEV)                            # NCHW-shaped view of NHWC storage = channels-last
    x, res = cl(o["x"]).requires_grad_(True), cl(o["res"]).requires_grad_(True)
    weight = o["w"].permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True)
    scale, bias = o["scale"].to(DEV), o["bias"].to(DEV)
    y = conv_f32.conv_bn_act(x, weight, scale, bias, res, True, s, p)
    assert y.is_contiguous(memory_format=torch.channels_last)
    ref, m = fwd_ref(o, True, True, True, True)
    check(y.detach().permute(0, 2, 3, 1).cpu(), ref, m, k * k * o["ci"], False, "Function forward")
    dy = cl(o["dz"])
    dx, dw, dres = torch.autograd.grad(y, (x, weight, res), dy)
    assert dw.shape == weight.shape
    mask = (y.detach() > 0).permute(0, 2, 3, 1).cpu()
    dz = o["dz"] * mask                                                     # exact in f32
    assert torch.equal(dres.permute(0, 2, 3, 1).cpu(), dz)
    g = dz * o["scale"]                                                     # the Function's own rounding of dz * scale, reproduced
    _, dx_ref, _ = conv_refs(o["x"], o["w"], g, k, s, p)
    _, dx_abs, _ = conv_refs(o["x"].abs(), o["w"].abs(), g.abs(), k, s, p)
    check(dx.permute(0, 2, 3, 1).cpu(), dx_ref, dx_abs, k * k * o["co"], False, "Function dx")
    _, _, dw_ref = conv_refs(o["x"], o["w"], dz, k, s, p)
    _, _, dw_abs = conv_refs(o["x"].abs(), o["w"].abs(), dz.abs(), k, s, p)
    sc = o["scale"].double().view(-1, 1, 1, 1)
    check(dw.permute(0, 2, 3, 1).cpu(), dw_ref * sc, dw_abs * sc, o["B"] * o["ho"] * o["wo"], False, "Function dw")


def test_function_stem_conv():
    from partdistillation_amd.functions import conv_f32
    o = stem_problem(STEM_CASES[0])
    x = o["x"].permute(0, 3, 1, 2).to(DEV)
    weight = o["w"].permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True)
    y = conv_f32.StemConvF32.apply(x, weight, o["scale"].to(DEV), o["bias"].to(DEV), True)
    pre = o["y"] * o["scale"].double() + o["bias"].double()
    check(y.detach().permute(0, 2, 3, 1).cpu(), pre.clamp_min(0), o["y_abs"] * o["scale"].double() + o["bias"].double().abs(), 147, False, "stem Function forward")
    dw, = torch.autograd.grad(y, weight, o["dz"].permute(0, 3, 1, 2).to(DEV))
    assert dw.shape == weight.shape
    dz = o["dz"] * (y.detach() > 0).permute(0, 2, 3, 1).cpu()
    _, _, dw_ref = conv_refs(o["x"], o["w"], dz, 7, 2, 3)
    _, _, dw_abs = conv_refs(o["x"].abs(), o["w"].abs(), dz.abs(), 7, 2, 3)
    sc = o["scale"].double().view(-1, 1, 1, 1)
    check(dw.permute(0, 2, 3, 1).cpu(), dw_ref * sc, dw_abs * sc, o["B"] * o["ho"] * o["wo"], False, "stem Function dw")
