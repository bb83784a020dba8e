"""GPU: every launch branch of the detector's convolutions (csrc/conv_kernels.hip) -- the rows of tests/conv_cases.py, at the shapes its ladder
finds for this device's compute units -- element by element against a float64 convolution of the same operand values.

Per row (test_branch):
 1. the branch ran: bf_last_conv2d_plan after the launch equals the row's tuple, and the whole plan equals what bf_plan_conv2d said;
 2. every output element is within the bound derived below of the float64 result, and the project's max-norm bars hold besides
    (5e-6 of the layer's largest output in float32, 2e-3 in float16);
 3. the same bits from the kernels that promise them: the register-staged kernel on every float16 / float32-native LDS-DMA tile, the patch
    kernel against the register-staged one (and, in float32, the LDS-DMA one), two sources / an upsampled source against the materialised
    concatenation (every family and mode).  The bfloat16 split meets the native kernels only through 2;
 4. nothing outside the output: ldy - N guard channels per pixel and one pixel row before and after the tensor keep their sentinel.
Then the split's part products on exact data (test_part_products_are_all_there) and float32's exponent range (test_exponent_range).

The bound of 2.  K = KH KW C products per output, u = 2^-24.  p = bias + sum x w in float64; S = |bias| + sum |x| |w|; r the residual.
  * accumulation: products of float16 operands are exact in float32, v_mfma_f32_32x32x2_f32 rounds product and sum once each step, and any order of
    K float32 additions plus the bias's errs by at most (K + 2) u S to first order.  The split keeps six of the nine bfloat16 part products of each
    x w; the three dropped ones are below 3 u |x w| together, so (K + 5) u S.
  * SiLU: slope at most 1.1 scales that; silu_f's own evaluation adds (2 |p| + 8) u |silu(p)| -- the rounding of -p log2 e inside __expf is
    worth |p| u relative in the exponential (twice: the product and the argument reduction), v_exp_f32, the add, the refined reciprocal and
    the multiply an ulp or so each.  A float16 layer skips the Newton step on v_rcp_f32 (its result is rounded to 11 bits next): 2^-22 for u there.
  * the output rounding: u_out |want|, u_out = 2^-24 (float32; the conversion is exact and only the residual's add rounds) or 2^-11 (float16).
    A residual is added to the ROUNDED activation in float32 and the sum rounded again: u_out (|silu(p)| + |r|) more.
  * a term the list above lacks, added after reading the epilogue: a float16 result below 2^-14 is subnormal and rounds to a multiple of 2^-24
    whatever its size (SiLU of a very negative p lands there), so each float16 rounding may also err by 2^-25 absolutely.
No constant is fitted to what the kernels give; the largest error / bound ratios seen are printed (-s) and recorded in DESIGN.md section 2."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import conv_cases as cc

SENTINEL = 7.5
U24 = 2.0 ** -24


@contextlib.contextmanager
def switches(native, dma, mode):
    d0, m0 = native.lib.bf_conv2d_use_dma_kernel(dma), native.lib.bf_conv2d_f32_mode(mode)
    try:
        yield
    finally:
        native.lib.bf_conv2d_use_dma_kernel(d0)
        native.lib.bf_conv2d_f32_mode(m0)


@pytest.fixture(scope="module")
def n_cus(native):
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _dtype(row):
    import torch
    return torch.float16 if row.branch.eb == cc.F16 else torch.float32


class Case(object):
    """The operands of a row at a shape: drawn once on the CPU in the row's type, uploaded once; the float64 reference computed once."""

    def __init__(self, row, shape, scale_exponents=None, seed=None):
        import torch
        self.row, (self.B, self.H, self.W) = row, shape
        B, H, W = shape
        dt = _dtype(row)
        g = torch.Generator(device="cpu").manual_seed(1000 + row.index if seed is None else seed)
        x = torch.randn((B, row.c, H, W), generator=g) * 1.5
        w = torch.randn((row.n, row.c, row.kh, row.kw), generator=g) / row.K ** 0.5
        if scale_exponents is not None:                  # channel c of the input times 2^e(c), of the weights times 2^-e(c): exact in float32
            e = torch.tensor(scale_exponents, dtype=torch.float64)
            x = (x.double() * torch.pow(2.0, e)[None, :, None, None]).float()
            w = (w.double() * torch.pow(2.0, -e)[None, :, None, None]).float()
        self.x, self.w = x.to(dt), w.to(dt)
        # (float32 for the kernel, but drawn in the row's type: a float16 module rounds its bias before HipConv takes it)
        self.bias = (torch.randn((row.n,), generator=g) * 0.5).to(dt).float() if row.bias else None
        self.ho, self.wo = row.out_hw(H, W)
        self.M = B * self.ho * self.wo
        self.res = torch.randn((B, row.n, self.ho, self.wo), generator=g).to(dt) if row.residual else None
        self._dev = None
        self._ref = None

    def conv(self):
        """HipConv of the layer (the weights repacked to the kernels' rows)"""
        import torch
        from image_detection.model import yolov5s
        r = self.row
        m = torch.nn.Conv2d(r.c, r.n, (r.kh, r.kw), r.stride, r.pad, bias=self.bias is not None)
        with torch.no_grad():
            m.weight.copy_(self.w.float())
            if self.bias is not None:
                m.bias.copy_(self.bias)
        m = m.cuda().to(_dtype(r))
        hc = yolov5s.HipConv(m, bool(r.silu))
        if self.bias is not None:
            assert torch.equal(hc.bias.cpu(), self.bias)              # (the reference adds the very values the kernel reads)
        return hc

    def device_inputs(self):
        """x dense, and for two-source rows the channel slices a (of a buffer E channels wider, base E channels in) and b (2 E wider)."""
        import torch
        if self._dev is None:
            r, cl = self.row, torch.channels_last
            d = {"x": self.x.cuda().contiguous(memory_format=cl), "res": None if self.res is None else self.res.cuda().contiguous(memory_format=cl)}
            if r.src in ("two", "up"):
                xa = self.x[:, :r.c1, ::2, ::2] if r.src == "up" else self.x[:, :r.c1]
                big_a = torch.full((self.B, r.c1 + r.E) + tuple(xa.shape[2:]), 3.0, dtype=self.x.dtype).contiguous(memory_format=cl)
                big_b = torch.full((self.B, r.c - r.c1 + 2 * r.E, self.H, self.W), -3.0, dtype=self.x.dtype).contiguous(memory_format=cl)
                big_a[:, r.E:] = xa
                big_b[:, r.E:r.E + r.c - r.c1] = self.x[:, r.c1:]
                d["big_a"], d["big_b"] = big_a.cuda(), big_b.cuda()
                d["a"], d["b"] = d["big_a"][:, r.E:], d["big_b"][:, r.E:r.E + r.c - r.c1]
                assert d["a"].stride(3) == r.ld1 and d["b"].stride(3) == r.ld2
            self._dev = d
        return self._dev

    def full_input(self):
        """What the layer convolves, [B, C, H, W] on the CPU in the row's type: for an upsampled first source the 2x nearest upsampling of what it holds."""
        import torch
        r = self.row
        if r.src != "up":
            return self.x
        up = torch.nn.functional.interpolate(self.x[:, :r.c1, ::2, ::2].float(), scale_factor=2, mode="nearest").to(self.x.dtype)
        return torch.cat((up, self.x[:, r.c1:]), 1)

    def reference(self):
        """(p, S) in float64: the convolution plus bias before the activation, and the same of the absolute values."""
        import torch
        if self._ref is None:
            r = self.row
            x, w = self.full_input().double(), self.w.double()
            b = None if self.bias is None else self.bias.double()
            p = torch.nn.functional.conv2d(x, w, b, r.stride, r.pad)
            S = torch.nn.functional.conv2d(x.abs(), w.abs(), None if b is None else b.abs(), r.stride, r.pad)
            self._ref = (p, S)
        return self._ref


def run(native, case, hc, dma, mode, materialised=False):
    """One launch into a fresh guarded buffer -> (the whole buffer [M + 2 Wo][ldy] on the CPU, the plan of the launch)"""
    import torch
    r, d = case.row, case.device_inputs()
    dt = _dtype(r)
    rows = case.M + 2 * case.wo
    flat = torch.full((rows * r.ldy,), SENTINEL, dtype=dt, device="cuda")
    out = flat.as_strided((case.B, r.n, case.ho, case.wo), (case.ho * case.wo * r.ldy, 1, case.wo * r.ldy, r.ldy), case.wo * r.ldy)
    with switches(native, dma, mode):
        if r.src in ("two", "up") and not materialised:
            y = hc(d["a"], x2=d["b"], up=r.src == "up", out=out, residual=d["res"])
        elif r.src == "up":
            y = hc(case.full_input().cuda().contiguous(memory_format=torch.channels_last), out=out, residual=d["res"])
        else:
            y = hc(d["x"], out=out, residual=d["res"])
        plan = (C.c_longlong * cc.OUT_LEN)()
        assert native.lib.bf_last_conv2d_plan(plan) == 0, native.lib.bf_last_error()
    assert y.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    return flat.cpu().reshape(rows, r.ldy), list(plan), out.data_ptr()


def bound(case, split):
    """(want, bound) in float64, [B, N, Ho, Wo] -- the module docstring's derivation."""
    import torch
    r = case.row
    p, S = case.reference()
    f16 = r.branch.eb == cc.F16
    u_out, tiny = (2.0 ** -11, 2.0 ** -25) if f16 else (U24, 2.0 ** -150)
    err = (r.K + (5 if split else 2)) * U24 * S
    act = p
    if r.silu:
        act = p * torch.sigmoid(p)
        err = 1.1 * err + (2.0 * p.abs() + 8.0) * (2.0 ** -22 if f16 else U24) * act.abs()
    want = act
    if case.res is not None:
        rr = case.res.double()
        want = act + rr
        err = err + u_out * (act.abs() + rr.abs()) + tiny
    err = err + u_out * want.abs() + tiny
    return want, err


def check_against_float64(case, buf, split, what):
    """Assertion 2 (and 4) on a buffer `run` returned; returns the largest error / bound."""
    import torch
    r = case.row
    want, err = bound(case, split)
    got = buf[case.wo:case.wo + case.M, :r.n].double().reshape(case.B, case.ho, case.wo, r.n).permute(0, 3, 1, 2)
    assert bool(torch.isfinite(got).all()), what
    diff = (got - want).abs()
    ratio = float((diff / err).max())
    top = float(want.abs().max())
    norm = float(diff.max()) / top
    print("conv-branch-ratio %s %-7s error/bound %.4f max-norm %.3g  M=%d N=%d K=%d  %s" % (
        "f16" if r.branch.eb == cc.F16 else "f32", "split" if split else "native", ratio, norm, case.M, r.n, r.K, what))
    assert ratio <= 1.0, (what, ratio, "worst element", int(torch.argmax(diff / err)))
    assert norm < (2e-3 if r.branch.eb == cc.F16 else 5e-6), (what, norm)
    guards_untouched(case, buf, what)
    return ratio


def guards_untouched(case, buf, what):
    r = case.row
    assert bool((buf[:case.wo] == SENTINEL).all()) and bool((buf[case.wo + case.M:] == SENTINEL).all()), what + ": a pixel row outside the tensor was written"
    assert bool((buf[:, r.n:] == SENTINEL).all()), what + ": channels past N were written"


@pytest.fixture(scope="module")
def shapes(native, n_cus):
    return {r.index: cc.find_shape(native.lib, r, n_cus) for r in cc.ROWS}


@pytest.mark.gpu
@pytest.mark.parametrize("row", cc.ROWS, ids=[r.id for r in cc.ROWS])
def test_branch(native, n_cus, shapes, row):
    import torch
    found = shapes[row.index]
    assert found is not None, "the ladder of conv_cases.find_shape reaches no shape for %s at %d compute units" % (row.id, n_cus)
    shape, _ = found
    b = row.branch
    case = Case(row, shape)
    hc = case.conv()
    buf, plan, y_ptr = run(native, case, hc, row.dma, row.mode)
    # 1. the branch, and the plan the planner gives for the very same call
    assert cc.branch_of(plan) == b, (row.id, plan)
    rc, said = cc.plan(native.lib, row, *shape, n_cus, y_misaligned=bool(y_ptr & 15))
    assert rc == 0 and said == plan and plan[15] == n_cus
    # 2. (and 4.) float64
    check_against_float64(case, buf, bool(b.split), row.id)
    # 3. the same bits
    if b.family == cc.DMA and not b.split:
        other, p2, _ = run(native, case, hc, 0, 0)
        assert p2[1] == cc.REG and torch.equal(buf, other), row.id + ": the register-staged kernel gives other bits"
    if b.family == cc.PATCH:
        other, p2, _ = run(native, case, hc, 0, 0)
        assert p2[1] == cc.REG and torch.equal(buf, other), row.id + ": the register-staged kernel gives other bits"
        if b.eb == cc.F32:
            other, p2, _ = run(native, case, hc, 1, 0)
            assert p2[1] == cc.DMA and torch.equal(buf, other), row.id + ": the LDS-DMA kernel gives other bits"
    if row.src in ("two", "up"):
        other, p2, _ = run(native, case, hc, row.dma, row.mode, materialised=True)
        assert p2[5] == 1 and torch.equal(buf, other), row.id + ": the materialised concatenation gives other bits"


def _special_row(base, c, n, src=None, c1=0, silu=False, bias=False):
    """A row outside the table (its own layer on one of the table's branches): dense output, no residual."""
    b = base._replace(wide=int(n % (16 // base.eb) == 0))
    r = cc.Row(b, c, n, 1 if b.cat else 3, 1, 0 if b.cat else 1, src, c1=c1)
    r.index, r.sliced, r.residual, r.bias, r.silu = 900, False, False, bias, silu
    return r


PARTS = [(1.0 + 2.0 ** -9 + 2.0 ** -17, 1.0), (1.0, 1.0 + 2.0 ** -9 + 2.0 ** -17), (1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["native", "split"])
@pytest.mark.parametrize("tile", [(64, 64), (128, 128)], ids=["64x64", "128x128"])
def test_part_products_are_all_there(native, n_cus, tile, mode):
    """f32_split.h: "each part product exact, six of nine kept".  A 1x1 layer, K = 16, no bias, no activation, constant operands whose bfloat16
    parts are h = 1, m = 2^-9, l = 2^-17: (a = 1 + m + l, b = 1) needs hh + mh + lh, (a = 1, b = 1 + m + l) needs hh + hm + hl,
    (a = b = 1 + m) needs hh + mh + hm + mm -- every one of the six kept products is needed by one of them, every dropped product is zero, and
    16 a b has at most 19 significant bits: the output equals the float64 value bit for bit.  Both ways round (a the input or the weight),
    with either sign, on the smallest tile and on the 128 x 128 one; the float32 instruction is held to the same."""
    import torch
    from image_detection.model import yolov5s
    row = _special_row(cc.Branch(cc.F32, cc.DMA, tile[0], tile[1], 4, 1, mode, 0, 1), 16, 72 if tile[1] == 64 else 200, "dense")
    found = cc.find_shape(native.lib, row, n_cus)
    assert found is not None
    (B, H, W), _ = found
    x = torch.empty((B, 16, H, W), dtype=torch.float32, device="cuda").contiguous(memory_format=torch.channels_last)
    plan = (C.c_longlong * cc.OUT_LEN)()
    for a, b in PARTS:
        for x_val, w_val in ((a, b), (b, a)):
            for sign in (1.0, -1.0):
                want = np.float32(16.0 * x_val * w_val * sign)
                assert float(want) == 16.0 * x_val * w_val * sign              # representable: nothing for the kernel to round
                conv = torch.nn.Conv2d(16, row.n, 1, bias=False)
                with torch.no_grad():
                    conv.weight.fill_(w_val * sign)
                assert float(conv.weight.detach()[0, 0, 0, 0]) == w_val * sign
                hc = yolov5s.HipConv(conv.cuda(), False)
                x.fill_(x_val)
                with switches(native, 1, mode):
                    y = hc(x)
                    assert native.lib.bf_last_conv2d_plan(plan) == 0 and cc.branch_of(list(plan)) == row.branch, list(plan)
                bad = int((y != float(want)).sum())
                assert bad == 0, (x_val, w_val, sign, bad, float(y.flatten()[0]), float(want))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["native", "split"])
@pytest.mark.parametrize("kind", ["window", "cat"])
def test_exponent_range(native, n_cus, kind, mode):
    """The split is exact over float32's exponent range because bfloat16 shares it: input channel c times 2^e(c), the matching weight channel
    times 2^-e(c), e over [-40, 40] (every product stays between 2^-100 and 2^100, clear of the 2^-118 f32_split.h names).  The products are
    the unscaled layer's, so is S, and the bound of test_branch holds unchanged -- in both modes, on a window layer and on a two-source 1x1."""
    base = cc.Branch(cc.F32, cc.DMA, 64, 64, 4, int(kind == "cat"), mode, int(kind == "window"), 1)
    row = _special_row(base, 64 if kind == "cat" else 16, 72, "two" if kind == "cat" else None, c1=16 if kind == "cat" else 0, silu=True, bias=True)
    row.dma, row.mode = 1, mode
    found = cc.find_shape(native.lib, row, n_cus)
    assert found is not None
    e = np.round(np.linspace(-40, 40, row.c)).astype(np.int64)
    e = e[np.random.default_rng(5).permutation(row.c)]                    # (neighbouring channels far apart in scale)
    case = Case(row, found[0], scale_exponents=e.tolist(), seed=77)
    x = case.x.double().abs()
    assert float(x[x > 0].min()) > 2.0 ** -80 and float(x.max()) < 2.0 ** 80
    buf, plan, _ = run(native, case, case.conv(), 1, mode)
    assert cc.branch_of(plan) == row.branch, plan
    check_against_float64(case, buf, bool(mode), "exponent-range-%s-%s" % (kind, "split" if mode else "native"))
