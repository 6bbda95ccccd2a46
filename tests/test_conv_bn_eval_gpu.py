"""drn_conv_bn_eval / drn_conv_bn_eval_splitk (Conv1d -> eval BatchNorm -> [ReLU] in one launch) against a float64 model built from
tests/launch_ref.py, on every kernel kind an eval conv lands on, and -- fp32 -- bit for bit against drn_gemm_nt (or
drn_gemm_nt_splitk) followed by drn_bn_apply_multi on the same operands.

Bounds.  E = gemm_nt_ref(..., out_dtype=float32)["C"] gives the accumulator acc and its bound e_acc (E.bound minus the fp32 rounding
term).  With pre = acc*sc + sh, r = relu(pre) (ReLU is 1-Lipschitz: nothing near zero is left out), the bound on `out` is
u|r| + e_acc|sc| + 2^-23 (|acc*sc| + |sh|), u = unit(dtype); on `gated` the same times |gate| with u|r*gate|.  Relative L2: REL_L2.

Shapes: the smallest at which each path can go wrong (ragged M / N, sequence edges inside a tile, stride 2 with a gate, k = 1, the
pyramid launch of three groups, the 256-wide tile, gemm_nt_w4h_kernel plain / k = 3 on both walks, gemm_nt_w4c_kernel, both in-launch
K-splits), put on their kernels with drn_tune and confirmed with the plan entry points.  gemm_nt_w4h_kernel takes no launch with fewer
than two K-steps of 64 and stages a channel block once only when there are at least two of them, so its cases use Cin = 128."""
import ctypes

import pytest
import torch

import launch_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, BF16 = torch.float32, torch.bfloat16
DEFAULTS = {"exp0": 0, "nt_w4h": 160, "nt_w4c": 1, "w4h_halo": 1}
T128, T256, W4C, W4H = 0, 1, 3, 4


@pytest.fixture
def tune():
    from drn_amd import _lib
    touched = []

    def setter(**kv):
        for k, v in kv.items():
            _lib.check(_lib.lib().drn_tune(k.encode(), int(v)), "drn_tune")
            touched.append(k)
    yield setter
    for k in touched:
        _lib.lib().drn_tune(k.encode(), DEFAULTS[k])


def rnd(shape, seed, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(DEV)


class Group(object):
    """One problem: operands, the scale/shift table, an optional gate, outputs with row strides wider than N behind a sentinel."""

    def __init__(self, seed, dtype, B, L, Cin, N, k, stride, gate):
        self.B, self.L, self.Cin, self.N, self.k, self.stride, self.dtype = B, L, Cin, N, k, stride, dtype
        self.pad = (k - 1) // 2
        self.Lo = (L + 2 * self.pad - k) // stride + 1
        self.M = B * self.Lo
        self.x = rnd((B * L, Cin), seed, dtype)
        self.w = rnd((N, k * Cin), seed + 1, dtype, (k * Cin) ** -0.5)
        self.ss = torch.cat([rnd((1, N), seed + 2).abs() + 0.25, rnd((1, N), seed + 3, scale=0.5)]).contiguous()
        self.ss[0, ::7] *= -1.0                              # (a negative gamma is legal)
        self.gate = rnd((B, N + 8), seed + 4) if gate else None
        self.ld = N + 16

    def fresh(self):
        out = torch.full((self.M, self.ld), 7.0, dtype=self.dtype, device=DEV)
        return out, (torch.full_like(out, 7.0) if self.gate is not None else None)

    def desc(self, C=None):
        from drn_amd import ops
        return ops.gemm_desc(self.x, self.w, C, self.M, self.N, self.Cin, taps=self.k, stride=self.stride, pad=self.pad, Lout=self.Lo,
                             Lsrc=self.L)

    def level(self, out, gated, raw=None):
        return dict(raw=raw, ld_raw=self.N, ss=self.ss, out=out, ld_out=self.ld, M=self.M, L=self.Lo, gate=self.gate, gated=gated,
                    ld_gated=self.ld)

    def expects(self, relu):
        E = LR.gemm_nt_ref(self.x, self.w, self.M, self.N, self.Cin, taps=self.k, stride=self.stride, pad=self.pad, Lout=self.Lo,
                           Lsrc=self.L, out_dtype=F32)["C"]
        acc = E.ref
        e_acc = E.bound - LR.U_F32 * acc.abs()
        sc, sh = self.ss[0].double(), self.ss[1].double()
        pre = acc * sc + sh
        r = pre.clamp_min(0) if relu else pre
        u = LR.unit(self.dtype)
        slack = e_acc * sc.abs() + LR.U_F32 * ((acc * sc).abs() + sh.abs())
        out = {"out": LR.Expect("out", r, u * r.abs() + slack, LR.REL_L2[self.dtype], E.where)}
        if self.gate is not None:
            g = self.gate[:, :self.N].double().repeat_interleave(self.Lo, dim=0)
            out["gated"] = LR.Expect("gated", r * g, u * (r * g).abs() + slack * g.abs(), LR.REL_L2[self.dtype], E.where)
        return out


def run_case(groups, relu, ksplit, kind):
    from drn_amd import _lib, ops
    from drn_amd._lib import GemmDesc, lib
    dtype = groups[0].dtype
    code = ops.dtype_code(groups[0].x)
    outs = [g.fresh() for g in groups]
    descs = [g.desc() for g in groups]
    levels = [g.level(o, gd) for g, (o, gd) in zip(groups, outs)]
    arr, barr = (GemmDesc * len(descs))(*descs), ops._bn_apply_descs(levels)
    stream = ops._stream()
    dev = torch.device(DEV)
    if ksplit > 1:
        g0 = groups[0]
        ws = torch.empty(ksplit * max(256 * 128 * ((g0.M + 255) // 256) * ((g0.N + 127) // 128), 1), dtype=torch.float32, device=DEV)
        assert lib().drn_conv_bn_eval_splitk_plan(arr, barr, ksplit, code) == kind
        rc = lib().drn_conv_bn_eval_splitk(arr, barr, ksplit | (ops.KSPLIT_EVAL_RELU if relu else 0), ops._p(ws), ops._p(ops._counters(dev)),
                                           code, stream)
    else:
        assert lib().drn_conv_bn_eval_plan(arr, barr, len(descs), code) == kind
        rc = lib().drn_conv_bn_eval(arr, barr, len(descs), int(relu), code, stream)
    _lib.check(rc, "drn_conv_bn_eval")
    torch.cuda.synchronize()
    for g, (o, gd) in zip(groups, outs):
        exp = g.expects(relu)
        for name, t in (("out", o), ("gated", gd)):
            if t is None:
                continue
            mx, rel = LR.compare("conv_bn_eval %s" % name, exp[name], t[:, :g.N])
            print("%s kind %d ksplit %d %s: err/bound %.3f rel-L2 %.2e" % (str(dtype)[6:], kind, ksplit, name, mx, rel))
            assert bool((t[:, g.N:] == 7.0).all()), "columns beyond N were written (%s)" % name
    if dtype != F32:
        return
    # fp32: the raw tensor of the separate launches IS the accumulator, both paths apply one fmaf and one fmaxf to it
    raws = [torch.empty((g.M, g.N), dtype=F32, device=DEV) for g in groups]
    descs2 = [g.desc(r) for g, r in zip(groups, raws)]
    arr2 = (GemmDesc * len(descs2))(*descs2)
    outs2 = [g.fresh() for g in groups]
    if ksplit > 1:
        assert lib().drn_gemm_nt_splitk_plan(arr2, 1, ksplit, code) == kind
        _lib.check(lib().drn_gemm_nt_splitk(arr2, ksplit, ops._p(ws), ops._p(ops._counters(dev)), code, stream), "drn_gemm_nt_splitk")
    else:
        assert lib().drn_gemm_nt_plan(arr2, len(descs2), code) == kind
        _lib.check(lib().drn_gemm_nt(arr2, len(descs2), code, stream), "drn_gemm_nt")
    ops.bn_apply_multi([g.level(o, gd, r) for g, (o, gd), r in zip(groups, outs2, raws)], groups[0].N, code, relu=relu)
    torch.cuda.synchronize()
    for (o, gd), (o2, gd2) in zip(outs, outs2):
        assert torch.equal(o, o2)
        assert gd is None or torch.equal(gd, gd2)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("k,stride,gate,relu", [(3, 1, False, True), (3, 2, True, True), (1, 1, False, False), (3, 1, True, False)])
def test_general_kernel_ragged_tiles(dtype, k, stride, gate, relu):
    """B = 3, L = 40, N = 96: ragged M and N, sequence edges inside a tile; stride 2 with a gate as in the backbone's conv1 / conv2."""
    run_case([Group(10, dtype, 3, 40, 64, 96, k, stride, gate)], relu, 1, T128)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_general_kernel_pyramid_launch(dtype):
    run_case([Group(20 + 10 * i, dtype, 2, L, 64, 128, 3, 1, False) for i, L in enumerate((64, 32, 16))], True, 1, T128)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_general_kernel_256_wide_tile(dtype, tune):
    tune(exp0=1)
    run_case([Group(50, dtype, 4, 128, 64, 256, 1, 1, True)], True, 1, T256)


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("k,B,L,halo", [(1, 8, 32, 1), (3, 8, 32, 1), (3, 4, 64, 1), (3, 4, 64, 0)])
def test_w4h_kernel(k, B, L, halo, gate, tune):
    """M = 256: as 8 x 32 one wave's 128 rows span four sequences (the non-uniform gate rows); k = 3 on the old walk (L = 32, or the
    staged-once walk switched off) and on the staged-once walk (L = 64)."""
    tune(nt_w4h=1, w4h_halo=halo)
    run_case([Group(60, BF16, B, L, 128, 128, k, 1, gate)], True, 1, W4H)


@pytest.mark.parametrize("gate", [False, True])
def test_w4c_kernel(gate, tune):
    tune(exp0=1)
    run_case([Group(70, BF16, 2, 128, 64, 256, 3, 1, gate)], True, 1, W4C)


@pytest.mark.parametrize("dtype,kind", [(F32, T128), (BF16, W4H)])
@pytest.mark.parametrize("relu", [True, False])
def test_split_k(dtype, kind, relu, tune):
    """Cin = 256, k = 3, four splits, M = 256, N = 128: the last-arriving split of a tile runs the BatchNorm epilogue."""
    if kind == W4H:
        tune(nt_w4h=1)
    run_case([Group(80, dtype, 4, 64, 256, 128, 3, 1, True)], relu, 4, kind)
