"""Every hand-written path of the 1-2 channel output heads (csrc/heads.hip) on data whose fp32 sums are exact in any order, against
the float64 model and the derived bounds of tests/heads_ref.py (checked without a GPU by tests/test_heads_ref_cpu.py):

  1. the window, straddling and tail paths on every geometry of heads_ref.GEOMETRIES, linear mode, one head per launch: bit equality;
  2. the lane loop over channel vectors (C / VN = 64, 65, 128) and the second blockIdx.x of the backward launch;
  3. column slices of wider buffers (NaN beside X, a pattern beside dX) and guard elements around every output;
  4. exp mode (z exact, out and the gradients inside their bounds), dscale into a strided sink with 1, 3 and 4 levels;
  5. two heads per launch, of equal and of unequal geometry, in both orders: the bits of each head launched alone;
  6. accumulate_dx and accumulate_dw;
  7. the workspace contract of drn_heads_bwd (exactly drn_heads_ws_elems floats);
  8. the autograd wrapper (drn_amd.functional.head_out): an unused head, a partial column cover, the K > 2 slices of model/fcos.py;
  9. rejected arguments: DrnError, and nothing written.

Linear mode asserts EQUALITY with the float64 value (a bf16 dX: that value rounded to nearest-even).  Exp mode asserts the bounds
of heads_ref.py, the gradients against the model fed the device's own `out`; they are loose on many_blocks (gamma_4472 = 2.7e-4) --
the linear-mode run of the same geometry pins that reduction exactly.  Every output buffer carries sentinel guards on both sides.
With -s every exp-mode check prints its err / bound; the module prints the largest per group when it is done (DESIGN.md quotes one
MI355X run)."""
import functools
import types

import pytest
import torch

import heads_ref as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
TAG = {F32: "f32", BF16: "bf16"}
DTS = pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
NAMES = list(H.GEOMETRIES)
SENT = -777.25            # what every fp32 output buffer holds before a launch
DX_FILL = 123.5           # ... and every dX buffer (exact in bf16)
GUARD = 16
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIOS):
        print("\n[heads] %-16s largest err / bound = %.3g" % (k, RATIOS[k]), end="")
    print()


def code_of(dt):
    from drn_amd import ops
    return ops.BF16 if dt == BF16 else ops.F32


def small_c(dt):
    return H.vn_of(dt)                    # one channel vector: fp32 C = 4, bf16 C = 8


def bits(t):
    """the stored bits, NaN-safe"""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


@functools.lru_cache(maxsize=None)
def case_of(name, C, N, taps, exp, dt, seed=0):
    """(the exact case, its forward model): computed once per parameter set, never modified"""
    c = H.exact_case(name, C, N, taps, exp, dt, seed)
    return c, H.forward_ref(c["xs"], c["W"], c["bias"], c["scales"])


class Guarded:
    """An fp32 device buffer of `shape` with GUARD sentinel floats on either side.  step > 1 (1-D only): the live elements are every
    step-th float of `slots` slots; the floats between them and the slots past the last live element are guards as well."""

    def __init__(self, shape, step=1, slots=None):
        n = 1
        for s in shape:
            n *= s
        slots = n if slots is None else slots
        assert slots >= n and (step == 1 or len(shape) == 1)
        self.whole = torch.full((2 * GUARD + slots * step,), SENT, dtype=torch.float32, device=DEV)
        self.live = torch.zeros(self.whole.numel(), dtype=torch.bool, device=DEV)
        self.live[GUARD:GUARD + n * step:step] = True
        self.view = self.whole[GUARD:GUARD + n * step:step].view(shape) if step > 1 else self.whole[GUARD:GUARD + n].view(shape)
        self.sent = bits(torch.full((1,), SENT, dtype=torch.float32, device=DEV))

    def guards_intact(self):
        return bool((bits(self.whole)[~self.live] == self.sent).all())

    def untouched(self):
        return bool((bits(self.whole) == self.sent).all())


class Head:
    """The device side of one head on an exact case: X in columns [c0, c0 + C) of (B, L, ld) buffers (its own, NaN beside the slice, or
    the caller's), dX likewise (DX_FILL everywhere, or the old values in the slice under accumulate_dx), guarded outputs."""

    def __init__(self, case, dt, c0=0, ld=None, xbuf=None, dxbuf=None, acc_dx=False, acc_dw=False, ds_step=3):
        from drn_amd import ops
        c = self.c = case
        self.dt, self.c0, self.acc_dx, self.acc_dw = dt, c0, acc_dx, acc_dw
        B, Ls, C, N, taps, R = c["B"], c["Ls"], c["C"], c["N"], c["taps"], c["R"]
        if xbuf is None:
            ld = C if ld is None else ld
            xbuf = [torch.full((B, L, ld), float("nan"), dtype=dt, device=DEV) for L in Ls]
            dxbuf = [torch.full((B, L, ld), DX_FILL, dtype=dt, device=DEV) for L in Ls]
        self.xbuf, self.dxbuf = xbuf, dxbuf
        for l in range(len(Ls)):
            xbuf[l][:, :, c0:c0 + C] = c["xs"][l].to(DEV, dt)
            if acc_dx:
                dxbuf[l][:, :, c0:c0 + C] = c["dx0"][l].to(DEV, dt)
        self.Wt = c["W"].permute(0, 2, 1).contiguous().float().to(DEV)               # [N][taps][C]
        self.bias = c["bias"].float().to(DEV)
        self.scales = c["scales"].float().to(DEV) if c["exp"] else None
        self.dout = c["dout"].float().to(DEV)
        self.out, self.z = Guarded((R, N)), Guarded((R, N)) if c["exp"] else None
        self.dW, self.db = Guarded((N, C, taps)), Guarded((N,))
        self.ds = Guarded((len(Ls),), step=ds_step, slots=H.MAX_GROUPS) if c["exp"] else None
        if acc_dw:
            self.dW.view.copy_(c["dW0"].float())
            self.db.view.copy_(c["db0"].float())
            if c["exp"]:
                self.ds.view.copy_(c["ds0"].float())
        xsl = [(x[:, :, c0:c0 + C], x.stride(1), B * L, L) for x, L in zip(xbuf, Ls)]
        self.xsl = xsl
        self.g_fwd = ops.head_groups(xsl, scales=self.scales)
        self.g_bwd = ops.head_groups(xsl, dxs=[d[:, :, c0:c0 + C] for d in dxbuf], scales=self.scales)

    def fwd_call(self):
        c = self.c
        return dict(groups=self.g_fwd, W=self.Wt, bias=self.bias, N=c["N"], C=c["C"], taps=c["taps"], exp_mode=c["exp"],
                    out=self.out.view, z=self.z.view if c["exp"] else None)

    def bwd_call(self):
        c = self.c
        return dict(groups=self.g_bwd, W=self.Wt, dout=self.dout, out=self.out.view, z=self.z.view if c["exp"] else None, N=c["N"],
                    C=c["C"], taps=c["taps"], exp_mode=c["exp"], accumulate_dx=int(self.acc_dx), accumulate_dw=int(self.acc_dw),
                    dW=self.dW.view, dbias=self.db.view, dscale=self.ds.view if c["exp"] else None)

    def outputs(self):
        """every output as the device holds it (clones)"""
        C, c0 = self.c["C"], self.c0
        r = dict(out=self.out.view.clone(), dW=self.dW.view.clone(), dbias=self.db.view.clone())
        for l, d in enumerate(self.dxbuf):
            r["dX%d" % l] = d[:, :, c0:c0 + C].clone()
        if self.c["exp"]:
            r.update(z=self.z.view.clone(), dscale=self.ds.view.clone())
        return r

    def buffers(self):
        return [b for b in (self.out, self.z, self.dW, self.db, self.ds) if b is not None]

    def assert_guards(self, covered=None):
        """no output buffer written outside its live elements; dX columns outside `covered` (default: this head's slice) keep DX_FILL"""
        for b in self.buffers():
            assert b.guards_intact(), "a guard element was overwritten"
        covered = [(self.c0, self.c0 + self.c["C"])] if covered is None else covered
        fill = bits(torch.full((1,), DX_FILL, dtype=self.dt, device=DEV))
        for d in self.dxbuf:
            spare = torch.ones(d.shape[2], dtype=torch.bool, device=DEV)
            for a, b in covered:
                spare[a:b] = False
            assert bool((bits(d)[:, :, spare] == fill).all()), "a spare column of dX was overwritten"

    def assert_untouched(self):
        for b in self.buffers():
            assert b.untouched(), "a rejected call wrote an output"
        fill = bits(torch.full((1,), DX_FILL, dtype=self.dt, device=DEV))
        for d in self.dxbuf:
            assert bool((bits(d) == fill).all()), "a rejected call wrote dX"


def launch(heads, dt, fwd=True, bwd=True):
    from drn_amd import ops
    if fwd:
        ops.heads_fwd([h.fwd_call() for h in heads], code_of(dt))
    if bwd:
        ops.heads_bwd([h.bwd_call() for h in heads], code_of(dt))
    torch.cuda.synchronize()


def same(what, got, want):
    """bit equality with the float64 value"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, what
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        i = [int(j) for j in bad.nonzero()[0]]
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %.9g, want %.9g"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[tuple(i)]), float(want[tuple(i)])))


def within(group, what, got, want, bound):
    """|got - want| <= bound elementwise; records the largest err / bound of the group"""
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), "%s / %s: shape, or a NaN / Inf (an element nobody wrote?)" % (group, what)
    err = (got - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    RATIOS[group] = max(RATIOS.get(group, 0.0), worst)
    print("[heads] %s / %s: err / bound = %.3g" % (group, what, worst))
    if not worst <= 1.0:
        i = int(ratio.argmax())
        raise AssertionError("%s / %s: err %.6g > bound %.6g at flat index %d (got %.9g, want %.9g)"
                             % (group, what, float(err.flatten()[i]), float(bound.flatten()[i]), i, float(got.flatten()[i]),
                                float(want.flatten()[i])))


def verify(h, fwd_ref, covered=None, what=""):
    """every output of a launched head against the model: equality in linear mode, the bounds of heads_ref.py in exp mode"""
    c, dt = h.c, h.dt
    tag = TAG[dt]
    got = h.outputs()
    B, Ls, N, taps, R = c["B"], c["Ls"], c["N"], c["taps"], c["R"]
    old = dict(dx0=c["dx0"] if h.acc_dx else None, dW0=c["dW0"] if h.acc_dw else None, db0=c["db0"] if h.acc_dw else None,
               ds0=c["ds0"] if h.acc_dw else None)
    if not c["exp"]:
        same(what + "out", got["out"], fwd_ref["out"])
        b = H.backward_ref(c["xs"], c["W"], c["dout"], **old)
        for l in range(len(Ls)):
            same(what + "dX level %d" % l, got["dX%d" % l], H.rne(b["dX"][l], dt))
        same(what + "dW", got["dW"], b["dW"])
        same(what + "dbias", got["dbias"], b["dbias"])
    else:
        same(what + "z", got["z"], fwd_ref["z"])
        within("exp out " + tag, what + c["name"], got["out"], fwd_ref["out"], H.out_bound(fwd_ref["sz"]))
        dev_out = got["out"].double().cpu()
        b = H.backward_ref(c["xs"], c["W"], c["dout"], out=dev_out, z=fwd_ref["z"], scales=c["scales"], **old)
        acc = int(h.acc_dw)
        for l in range(len(Ls)):
            within("exp dX " + tag, what + "%s level %d" % (c["name"], l), got["dX%d" % l], b["dX"][l],
                   H.dx_bound(b["dX_abs"][l], b["dX"][l], N, taps, dt))
        within("exp dW " + tag, what + c["name"], got["dW"], b["dW"], H.sum_bound(b["dW_abs"], R + 2, acc))
        within("exp dbias " + tag, what + c["name"], got["dbias"], b["dbias"], H.sum_bound(b["dbias_abs"], R + 1, acc))
        bound = torch.stack([H.sum_bound(b["dscale_abs"][l], N * B * Ls[l] + 2, acc) for l in range(len(Ls))])
        within("exp dscale " + tag, what + c["name"], got["dscale"], b["dscale"], bound)
    h.assert_guards(covered)


def run_alone(key, dt, **kw):
    c, f = case_of(*key)
    h = Head(c, dt, **kw)
    launch([h], dt)
    verify(h, f)
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. paths, exactly
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,taps", [(1, 1), (1, 3), (2, 1), (2, 3)])
@pytest.mark.parametrize("dt,C", [(F32, 4), (F32, 64), (BF16, 8), (BF16, 64)], ids=["f32-4", "f32-64", "bf16-8", "bf16-64"])
@pytest.mark.parametrize("name", NAMES)
def test_paths_exact(name, dt, C, N, taps):
    """linear mode, one head per launch: out, dX, dW, dbias equal the float64 model bit for bit, and a second run gives the same bits"""
    h = run_alone((name, C, N, taps, False, dt), dt)
    h2 = Head(h.c, dt)
    launch([h2], dt)
    a, b = h.outputs(), h2.outputs()
    for k in a:
        assert same_bits(a[k], b[k]), "%s differs between two runs" % k


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. channel loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,C", [(F32, 256), (F32, 260), (F32, 512), (BF16, 512), (BF16, 520)],
                         ids=["f32-256", "f32-260", "f32-512", "bf16-512", "bf16-520"])
@pytest.mark.parametrize("name", ["ragged3", "four"])
def test_channel_loop_exact(name, dt, C):
    """64, 65 and 128 channel vectors: one full lane pass, a second pass with one live lane (and a second blockIdx.x in backward),
    two full passes"""
    assert C // H.vn_of(dt) in (64, 65, 128)
    run_alone((name, C, 2, 3, False, dt), dt)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. column slices and guards
# ---------------------------------------------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("exp", [False, True], ids=["linear", "exp"])
@pytest.mark.parametrize("name", ["ragged3", "four"])
def test_column_slice_of_a_wider_buffer(name, exp, dt):
    """X = wide[:, :, c0 : c0 + C], NaN in the spare columns on both sides; dX's spare columns keep their pattern; out, z, dW, dbias
    and the strided dscale keep their guards (verify -> assert_guards)"""
    vn = H.vn_of(dt)
    C = 2 * vn
    h = run_alone((name, C, 2, 3, exp, dt, 5), dt, c0=vn, ld=C + 3 * vn)
    assert all(bool(torch.isnan(x[:, :, :vn]).all()) and bool(torch.isnan(x[:, :, vn + C:]).all()) for x in h.xbuf)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. exp mode
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,taps", [(1, 1), (1, 3), (2, 1), (2, 3)])
@DTS
@pytest.mark.parametrize("name", NAMES)
def test_exp_mode_inside_bounds(name, dt, N, taps):
    """z exact; out, dX, dW, dbias, dscale inside the derived bounds; dscale goes to every third float of a 4-slot sink (1, 3 and 4
    levels among the geometries): the slots of absent levels and the floats in between stay untouched"""
    h = run_alone((name, small_c(dt), N, taps, True, dt), dt)
    assert h.ds.view.stride(0) == 3 and int(h.ds.live.sum()) == len(h.c["Ls"])


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. two heads per launch
# ---------------------------------------------------------------------------------------------------------------------------------
def _pair_equals_alone(make):
    """make() -> two fresh heads; launched together (in both orders) every output has the bits of the same head launched alone"""
    alone = make()
    for h in alone:
        launch([h], h.dt)
    ref = [h.outputs() for h in alone]
    for order in ((0, 1), (1, 0)):
        pair = make()
        launch([pair[i] for i in order], pair[0].dt)
        for i, h in enumerate(pair):
            got = h.outputs()
            for k in got:
                assert same_bits(got[k], ref[i][k]), "head %d, %s: launched with the other head (order %s) != launched alone" % (i, k, order)
    return alone


@DTS
@pytest.mark.parametrize("name", ["ragged3", "four"])
def test_two_heads_on_the_halves_of_one_buffer(name, dt):
    """cls (N = 1, linear) + bbox (N = 2, exp) on the two halves of one 2C-wide buffer, as model/fcos.py launches them"""
    C = small_c(dt)
    (c0, f0), (c1, f1) = case_of(name, C, 1, 3, False, dt, 7), case_of(name, C, 2, 3, True, dt, 8)

    def make():
        B, Ls = c0["B"], c0["Ls"]
        xbuf = [torch.full((B, L, 2 * C), float("nan"), dtype=dt, device=DEV) for L in Ls]
        dxbuf = [torch.full((B, L, 2 * C), DX_FILL, dtype=dt, device=DEV) for L in Ls]
        return [Head(c0, dt, c0=0, xbuf=xbuf, dxbuf=dxbuf), Head(c1, dt, c0=C, xbuf=xbuf, dxbuf=dxbuf)]
    _pair_equals_alone(make)
    pair = make()
    launch(pair, dt)
    verify(pair[0], f0, covered=[(0, 2 * C)])
    verify(pair[1], f1, covered=[(0, 2 * C)])


@pytest.mark.parametrize("dt,C", [(F32, 260), (BF16, 520)], ids=["f32-260", "bf16-520"])
def test_two_heads_of_unequal_geometry(dt, C):
    """head 0: `four`, the smallest C, taps = 1, N = 1, linear; head 1: `ragged3`, 65 channel vectors, taps = 3, N = 2, exp.  The
    grid is sized by the maxima (rows, channel blocks, row blocks, outputs): each set returns on its own bounds."""
    (c0, f0), (c1, f1) = case_of("four", small_c(dt), 1, 1, False, dt, 9), case_of("ragged3", C, 2, 3, True, dt, 9)
    alone = _pair_equals_alone(lambda: [Head(c0, dt), Head(c1, dt)])
    verify(alone[0], f0)
    verify(alone[1], f1)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. accumulate
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acc_dx,acc_dw", [(True, False), (False, True), (True, True)], ids=["dx", "dw", "dx+dw"])
@pytest.mark.parametrize("exp", [False, True], ids=["linear", "exp"])
@pytest.mark.parametrize("N,taps", [(1, 1), (2, 3)])
@DTS
@pytest.mark.parametrize("name", ["short_tail", "ragged3"])
def test_accumulate(name, dt, N, taps, exp, acc_dx, acc_dw):
    """accumulate_dx: dx0 + dX (bf16: the sum rounded once); accumulate_dw: dW0 + dW, db0 + db, ds0 + ds -- exact in linear mode,
    inside the bounds in exp mode (verify models the old values as further terms of the sums)"""
    run_alone((name, small_c(dt), N, taps, exp, dt, 11), dt, acc_dx=acc_dx, acc_dw=acc_dw)


def test_accumulate_dw_many_blocks():
    """the final kernel's unrolled trip, its remainder loop and the old values together"""
    run_alone(("many_blocks", 4, 2, 3, False, F32, 12), F32, acc_dw=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. workspace contract
# ---------------------------------------------------------------------------------------------------------------------------------
@DTS
def test_workspace_is_exactly_ws_elems(dt):
    """drn_heads_bwd called directly with a workspace of exactly drn_heads_ws_elems floats, 64 NaN behind it: the results of
    test_paths_exact, the NaN intact, and every workspace float written (the final kernel reads all of them)"""
    from drn_amd import ops
    from drn_amd._lib import check, lib
    c, f = case_of("many_blocks", 64, 2, 3, False, dt)
    h = Head(c, dt)
    launch([h], dt, bwd=False)
    n = int(lib().drn_heads_ws_elems(c["R"], c["N"], c["C"], c["taps"]))
    assert n == 70 * (2 * 3 * 64 + 8)
    ws = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=DEV)
    call = h.bwd_call()
    call["ws"] = ws
    check(lib().drn_heads_bwd(ops._head_calls([call]), 1, code_of(dt), ops._stream()), "drn_heads_bwd")
    torch.cuda.synchronize()
    verify(h, f)
    assert bool(torch.isnan(ws[n:]).all()), "the launch wrote past drn_heads_ws_elems floats"
    assert not bool(torch.isnan(ws[:n]).any()), "a workspace element the final kernel sums was never written"


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. the autograd wrapper
# ---------------------------------------------------------------------------------------------------------------------------------
def _conv(c):
    m = torch.nn.Conv1d(c["C"], c["N"], c["taps"], padding=(c["taps"] - 1) // 2).to(DEV)
    with torch.no_grad():
        m.weight.copy_(c["W"].float())
        m.bias.copy_(c["bias"].float())
    return m


def _wide(cases, dt, width):
    """per-level (B, L, width) leaves holding the cases' X side by side from column 0 (zeros in the rest)"""
    xs = []
    for l, L in enumerate(cases[0]["Ls"]):
        x = torch.zeros((cases[0]["B"], L, width), dtype=dt, device=DEV)
        c0 = 0
        for c in cases:
            x[:, :, c0:c0 + c["C"]] = c["xs"][l].to(DEV, dt)
            c0 += c["C"]
        xs.append(x.requires_grad_())
    return xs


class _Ctx:
    """what _HeadOutFn.forward / backward use of an autograd context, for calling them directly"""

    def save_for_backward(self, *ts):
        self.saved_tensors = ts


@DTS
@pytest.mark.parametrize("how", ["autograd", "direct"])
@pytest.mark.parametrize("used", [0, 1], ids=["cls-only", "bbox-only"])
def test_wrapper_unused_head(dt, used, how):
    """Only one of the two outputs has an upstream gradient: the other head's dW, db, dscale and its dx slice are zero, the used
    head is exact (cls) / inside the bounds (bbox).  "autograd": the other output never reaches the loss (autograd hands backward a
    zero gradient for it); "direct": _HeadOutFn.backward is called with None in its place, the branch that allocates the zeros
    itself and clears the slice of the uninitialised dx buffers."""
    from drn_amd import functional as DF
    C = small_c(dt)
    (c0, f0), (c1, f1) = case_of("four", C, 1, 3, False, dt, 13), case_of("four", C, 2, 3, True, dt, 14)
    m0, m1 = _conv(c0), _conv(c1)
    sh = c1["scales"].float().to(DEV).requires_grad_()
    xs = _wide([c0, c1], dt, 2 * C)
    cu = c0 if used == 0 else c1
    dout = cu["dout"].float().to(DEV)
    if how == "autograd":
        logits, reg = DF.head_out(xs, [(m0, None), (m1, sh)], cols=[0, C], dtype=dt)
        ((logits if used == 0 else reg) * dout).sum().backward()
        g = dict(dW0=m0.weight.grad, db0=m0.bias.grad, dW1=m1.weight.grad, db1=m1.bias.grad, ds=sh.grad, dxs=[x.grad for x in xs])
    else:
        ctx = _Ctx()
        meta = {"nheads": 2, "nl": len(xs), "dtype": dt, "cols": [0, C]}
        with torch.no_grad():
            logits, reg = DF._HeadOutFn.forward(ctx, meta, m0.weight, m0.bias, None, m1.weight, m1.bias, sh, *xs)
            r = DF._HeadOutFn.backward(ctx, *((dout, None) if used == 0 else (None, dout)))
        assert len(r) == 7 + len(xs) and r[0] is None and r[3] is None
        g = dict(dW0=r[1], db0=r[2], dW1=r[4], db1=r[5], ds=r[6], dxs=list(r[7:]))
    torch.cuda.synchronize()
    same("logits", logits, f0["out"])
    within("exp out " + TAG[dt], "wrapper", reg, f1["out"], H.out_bound(f1["sz"]))
    assert all(v is not None for v in g.values()) and all(d.dtype == dt and d.shape == x.shape for d, x in zip(g["dxs"], xs))
    idle = ("dW1", "db1", "ds") if used == 0 else ("dW0", "db0")
    for k in idle:
        assert not bool(g[k].any()), "%s of the head without a gradient" % k
    lo, hi = (C, 2 * C) if used == 0 else (0, C)
    for d in g["dxs"]:
        assert not bool(d[:, :, lo:hi].any()), "dx of the columns of the head without a gradient"
    if used == 0:
        b = H.backward_ref(c0["xs"], c0["W"], c0["dout"])
        for l, d in enumerate(g["dxs"]):
            same("dx level %d" % l, d[:, :, :C], H.rne(b["dX"][l], dt))
        same("dW", g["dW0"], b["dW"])
        same("db", g["db0"], b["dbias"])
    else:
        R, N, taps = c1["R"], 2, 3
        b = H.backward_ref(c1["xs"], c1["W"], c1["dout"], out=reg.detach().double().cpu(), z=f1["z"], scales=c1["scales"])
        tag = TAG[dt]
        for l, d in enumerate(g["dxs"]):
            within("exp dX " + tag, "wrapper level %d" % l, d[:, :, C:], b["dX"][l], H.dx_bound(b["dX_abs"][l], b["dX"][l], N, taps, dt))
        within("exp dW " + tag, "wrapper", g["dW1"], b["dW"], H.sum_bound(b["dW_abs"], R + 2))
        within("exp dbias " + tag, "wrapper", g["db1"], b["dbias"], H.sum_bound(b["dbias_abs"], R + 1))
        bound = torch.stack([H.sum_bound(b["dscale_abs"][l], N * c1["B"] * c1["Ls"][l] + 2) for l in range(4)])
        within("exp dscale " + tag, "wrapper", g["ds"], b["dscale"], bound)


@DTS
def test_wrapper_partial_column_cover(dt):
    """one head on columns [0, C) of a 2C-wide input: dx[:, :, C:] is exactly zero, the rest exact"""
    from drn_amd import functional as DF
    C = small_c(dt)
    c, f = case_of("four", C, 2, 3, False, dt, 15)
    m = _conv(c)
    xs = _wide([c], dt, 2 * C)
    (out,) = DF.head_out(xs, [(m, None)], cols=[0], dtype=dt)
    same("out", out, f["out"])
    (out * c["dout"].float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    b = H.backward_ref(c["xs"], c["W"], c["dout"])
    for l, x in enumerate(xs):
        assert x.grad.shape == x.shape and not bool(x.grad[:, :, C:].any()), "dx beyond the head's columns"
        same("dx level %d" % l, x.grad[:, :, :C], H.rne(b["dX"][l], dt))
    same("dW", m.weight.grad, b["dW"])
    same("db", m.bias.grad, b["dbias"])


@DTS
def test_wrapper_class_slices(dt):
    """The K > 2 call pattern of model/fcos.py with K = 5: two-row slices of one weight as SimpleNamespace heads (the last slice has
    N = 1), the first sharing its launch with bbox_pred.  Logits and the weight / bias gradients equal the float64 convolution with
    the full 5-row weight."""
    from drn_amd import functional as DF
    C, K = small_c(dt), 5
    parts = [case_of("four", C, n, 3, False, dt, 20 + i) for i, n in enumerate((2, 2, 1))]
    cb, fb = case_of("four", C, 2, 3, True, dt, 24)
    x0 = parts[0][0]["xs"]                                              # every class slice reads the same activations
    Wf = torch.cat([p[0]["W"] for p in parts])
    bf = torch.cat([p[0]["bias"] for p in parts])
    dout = torch.cat([p[0]["dout"] for p in parts], dim=1)              # (R, 5)
    assert Wf.shape == (K, C, 3)
    full = H.forward_ref(x0, Wf[:2], bf[:2])["out"], H.forward_ref(x0, Wf[2:4], bf[2:4])["out"], H.forward_ref(x0, Wf[4:], bf[4:])["out"]
    want = torch.cat(full, dim=1)
    W = torch.nn.Parameter(Wf.float().to(DEV))
    b = torch.nn.Parameter(bf.float().to(DEV))
    bbox, sh = _conv(cb), cb["scales"].float().to(DEV).requires_grad_()
    xs = []
    for l, L in enumerate(cb["Ls"]):
        xs.append(torch.cat([x0[l], cb["xs"][l]], dim=2).to(DEV, dt).requires_grad_())
    part = lambda k0: types.SimpleNamespace(weight=W[k0:k0 + 2], bias=b[k0:k0 + 2])
    l0, reg = DF.head_out(xs, [(part(0), None), (bbox, sh)], cols=[0, C], dtype=dt)
    rest = [DF.head_out(xs, [(part(k0), None)], cols=[0], dtype=dt)[0] for k0 in range(2, K, 2)]
    logits = torch.cat([l0] + rest, dim=1)
    same("logits", logits, want)
    (logits * dout.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    dW = torch.cat([H.backward_ref(x0, Wf[k0:k0 + 2], dout[:, k0:k0 + 2])["dW"] for k0 in range(0, K, 2)])
    db = dout.sum(0)
    same("dW of the full weight", W.grad, dW)
    same("db of the full bias", b.grad, db)
    assert not bool(bbox.weight.grad.any()) and not bool(sh.grad.any())


# ---------------------------------------------------------------------------------------------------------------------------------
# 9. rejected arguments
# ---------------------------------------------------------------------------------------------------------------------------------
def _bad_c(h, fc, bc):
    fc["C"] = bc["C"] = h.c["C"] - 2


def _bad_taps(h, fc, bc):
    fc["taps"] = bc["taps"] = 2


def _bad_n(h, fc, bc):
    fc["N"] = bc["N"] = 3


def _five_groups(h, fc, bc):
    from drn_amd import ops
    xsl = h.xsl + h.xsl[:1]
    dsl = [d[:, :, :h.c["C"]] for d in h.dxbuf] + [h.dxbuf[0][:, :, :h.c["C"]]]
    sc5 = torch.ones(5, dtype=torch.float32, device=DEV)
    fc["groups"], bc["groups"] = ops.head_groups(xsl, scales=sc5), ops.head_groups(xsl, dxs=dsl, scales=sc5)


def _bad_m(h, fc, bc):
    from drn_amd import ops
    x, ld, M, L = h.xsl[0]
    xsl = [(x, ld, M + 1, L)] + h.xsl[1:]
    dsl = [d[:, :, :h.c["C"]] for d in h.dxbuf]
    fc["groups"], bc["groups"] = ops.head_groups(xsl, scales=h.scales), ops.head_groups(xsl, dxs=dsl, scales=h.scales)


def _no_scales(h, fc, bc):
    from drn_amd import ops
    dsl = [d[:, :, :h.c["C"]] for d in h.dxbuf]
    fc["groups"], bc["groups"] = ops.head_groups(h.xsl), ops.head_groups(h.xsl, dxs=dsl)


@DTS
@pytest.mark.parametrize("spoil", [_bad_c, _bad_taps, _bad_n, _five_groups, _bad_m, _no_scales],
                         ids=["C-not-16-bytes", "taps-2", "N-3", "five-groups", "M-not-multiple-of-L", "exp-without-scales"])
def test_rejected_arguments(spoil, dt):
    """DrnError from both entry points, and every output buffer keeps its sentinel"""
    from drn_amd import ops
    from drn_amd._lib import DrnError
    c, _ = case_of("four", 2 * small_c(dt), 2, 3, True, dt, 30)
    h = Head(c, dt)
    fc, bc = h.fwd_call(), h.bwd_call()
    spoil(h, fc, bc)
    with pytest.raises(DrnError):
        ops.heads_fwd([fc], code_of(dt))
    with pytest.raises(DrnError):
        ops.heads_bwd([bc], code_of(dt))
    torch.cuda.synchronize()
    h.assert_untouched()


@DTS
def test_three_heads_in_one_call_rejected(dt):
    """drn_heads_fwd / drn_heads_bwd take at most two heads per launch (ops.heads_fwd chunks its list; the entry points refuse)"""
    from drn_amd import ops
    from drn_amd._lib import DrnError, check, lib
    c, _ = case_of("four", small_c(dt), 1, 3, False, dt, 31)
    hs = [Head(c, dt) for _ in range(3)]
    ws = torch.full((3 * 4096,), SENT, dtype=torch.float32, device=DEV)
    bcs = [h.bwd_call() for h in hs]
    for i, bc in enumerate(bcs):
        bc["ws"] = ws[i * 4096:(i + 1) * 4096]
    with pytest.raises(DrnError):
        check(lib().drn_heads_fwd(ops._head_calls([h.fwd_call() for h in hs]), 3, code_of(dt), ops._stream()), "drn_heads_fwd")
    with pytest.raises(DrnError):
        check(lib().drn_heads_bwd(ops._head_calls(bcs), 3, code_of(dt), ops._stream()), "drn_heads_bwd")
    torch.cuda.synchronize()
    for h in hs:
        h.assert_untouched()
    assert bool((ws == SENT).all())
