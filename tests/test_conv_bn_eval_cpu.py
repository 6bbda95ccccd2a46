"""drn_conv_bn_eval* without a GPU: the symbols, what the plan entry points refuse (DRN_ERR_UNSUPPORTED with a text, nothing launched)
and accept (a DRN_NT_KIND_*; pointers are aligned dummies that nothing dereferences), and the register budgets of the new kernel
instantiations, read from the code objects the way tests/test_kernel_resources_cpu.py reads them."""
import ctypes
import os
import re
import subprocess

import pytest

from drn_amd import _lib
from drn_amd._lib import BnApplyDesc, GemmDesc
from test_kernel_resources_cpu import kernel_table

NAMES = ("drn_conv_bn_eval", "drn_conv_bn_eval_plan", "drn_conv_bn_eval_splitk", "drn_conv_bn_eval_splitk_plan")
UNSUPPORTED = -3
P = 0x10000          # an aligned address nobody reads


def gemm(**kw):
    d = dict(A=P, B=P, C=None, M=256, N=128, Cin=64, taps=3, stride=1, pad=1, mode=0, Lout=64, Lsrc=64, lda=64, ldb=192, ldc=128)
    d.update(kw)
    return GemmDesc(**d)


def bn(**kw):
    d = dict(scale_shift=P, out=P, ld_out=128, M=256, L=64)
    d.update(kw)
    return BnApplyDesc(**d)


def plan(gs, bs, dtype=1):
    return _lib.lib().drn_conv_bn_eval_plan((GemmDesc * len(gs))(*gs), (BnApplyDesc * len(bs))(*bs), len(gs), dtype)


def test_symbols_are_declared_and_exported():
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.declared_symbols() and hasattr(lib, n), n
    assert lib.drn_abi_version() == 9


REFUSED = [("up", {}, {"up": P}), ("C2", {"C2": P}, {}), ("bias", {"bias": P}, {}), ("gate", {"gate": P}, {}), ("stats", {"stats": P}, {}),
           ("accumulate", {"accumulate": 1}, {}), ("out_f32", {"out_f32": 1}, {}), ("sumsq", {"sumsq": P}, {}),
           ("gb_act", {"gb_act": P}, {}), ("gb_dct", {"gb_dct": P}, {}), ("gb_dgate", {"gb_dgate": P}, {}), ("gb_dsum", {"gb_dsum": P}, {}),
           ("mode 1", {"mode": 1}, {}), ("misaligned out", {}, {"out": P + 4}), ("odd row stride", {}, {"ld_out": 132}),
           ("misaligned gated", {}, {"gate": P, "gated": P + 2, "ld_gated": 128, "ldg": 128})]


@pytest.mark.parametrize("what,gk,bk", REFUSED, ids=[r[0] for r in REFUSED])
def test_plan_refuses_what_the_fused_launch_does_not_serve(what, gk, bk):
    lib = _lib.lib()
    lib.drn_last_error.restype = ctypes.c_char_p
    for fn in (lambda: plan([gemm(**gk)], [bn(**bk)]),
               lambda: lib.drn_conv_bn_eval_splitk_plan((GemmDesc * 1)(gemm(Cin=256, lda=256, ldb=768, **gk)), (BnApplyDesc * 1)(bn(**bk)), 4, 1)):
        assert fn() == UNSUPPORTED, what
        assert len(lib.drn_last_error() or b"") > 10, what


def test_plan_refuses_groups_of_unequal_width():
    lib = _lib.lib()
    lib.drn_last_error.restype = ctypes.c_char_p
    assert plan([gemm(), gemm(N=256, ldc=256)], [bn(), bn(ld_out=256)]) == UNSUPPORTED
    assert b"N" in lib.drn_last_error()


def test_plan_names_a_kernel_kind_for_valid_descriptors():
    lib = _lib.lib()
    assert plan([gemm()], [bn()], 0) == 0 and plan([gemm()], [bn()], 1) == 0             # 128x128 tiles, both dtypes
    assert plan([gemm(M=120, Lout=40, Lsrc=40, N=96)], [bn(M=120, L=40, ld_out=96)], 0) == 0
    assert plan([gemm(), gemm(M=128, Lout=32, Lsrc=32)], [bn(gate=P, gated=P, ld_gated=128, ldg=128), bn(M=128, L=32)]) == 0
    one = ((GemmDesc * 1)(gemm(Cin=256, lda=256, ldb=768)), (BnApplyDesc * 1)(bn()))
    assert lib.drn_conv_bn_eval_splitk_plan(one[0], one[1], 4, 0) == 0
    assert lib.drn_conv_bn_eval_splitk_plan(one[0], one[1], 4, 1) == lib.drn_gemm_nt_splitk_plan((GemmDesc * 1)(gemm(Cin=256, lda=256, ldb=768, C=P)), 1, 4, 1)
    lib.drn_tune(b"nt_w4h", 1)
    try:
        assert plan([gemm(Cin=128, lda=128, ldb=384)], [bn()]) == 4                        # gemm_nt_w4h_kernel
        assert lib.drn_conv_bn_eval_splitk_plan(one[0], one[1], 4, 1) == 4
    finally:
        lib.drn_tune(b"nt_w4h", 160)
    lib.drn_tune(b"exp0", 1)
    try:
        assert plan([gemm(N=256, ldc=256)], [bn(ld_out=256)]) == 3                         # gemm_nt_w4c_kernel
        assert plan([gemm(N=256, ldc=256)], [bn(ld_out=256)], 0) == 1                      # 256x256 tiles
        # a large plain product would run gemm_nt_w4_kernel, which has no BatchNorm epilogue
        assert plan([gemm(N=256, ldc=256, taps=1, pad=0, Cin=128, lda=128, ldb=128)], [bn(ld_out=256)]) == UNSUPPORTED
    finally:
        lib.drn_tune(b"exp0", 0)
    assert plan([gemm()], [bn(M=128)]) == -1                                                # M differs from the convolution's


def test_new_instantiations_keep_their_register_budgets(tmp_path):
    table = kernel_table(tmp_path)
    # conv_gemm_nt_eval_kernel<T, STAGES, FAST, WM, WN, MI, NI>
    small = [k for k in table if re.search(r"conv_gemm_nt_eval_kernelI(f|DF16b)Li[24]ELb[01]ELi2ELi4ELi4ELi2EE", k)]
    big = [k for k in table if re.search(r"conv_gemm_nt_eval_kernelI(f|DF16b)Li2ELb[01]ELi2ELi4ELi8ELi4EE", k)]
    assert len(small) == 8 and len(big) == 4, (len(small), len(big))
    for k in small:      # two 8-wave workgroups per CU, as the kernels they stand in for
        r = table[k]
        assert r["vgpr"] <= 128 and r["spill"] == 0 and r["scratch"] == 0 and r["agpr"] == 0, (k, r)
    for k in big:
        r = table[k]
        assert r["vgpr"] <= 256 and r["spill"] == 0 and r["scratch"] == 0, (k, r)
    # gemm_nt_w4h_kernel<CONV, EVAL = true>, gemm_nt_w4c_kernel<SWAP = true, EVAL = true>: one wave per SIMD, the loop statement owns
    # a[0:255] and the upper VGPRs; nothing may spill around it
    w4 = [k for k in table if re.search(r"gemm_nt_w4h_kernelILb[01]ELb1EE", k) or re.search(r"gemm_nt_w4c_kernelILb1ELb1EE", k)]
    assert len(w4) == 3, w4
    for k in w4:
        r = table[k]
        assert r["agpr"] == 256 and r["vgpr"] == 512 and r["spill"] == 0 and r["scratch"] == 0, (k, r)


def test_compiler_leaves_the_accumulators_alone_in_the_new_instantiations(tmp_path):
    """AGPR use outside the asm statements, per kernel: the existing test refuses it file-wide for gemm_nt_w4.hip / gemm_nt_w4h.hip;
    here the new kernels are looked up by name in the same assembly, so the check cannot pass because they were not emitted."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "drn_amd", "csrc")
    procs = []
    for name in ("gemm_nt_w4", "gemm_nt_w4h"):
        out = os.path.join(str(tmp_path), name + ".s")
        procs.append((out, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result",
                                             "-Wno-unused-function", "--cuda-device-only", "-S", "-o", out, name + ".hip"],
                                            cwd=csrc, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
    seen = 0
    for out, p in procs:
        assert p.wait(timeout=900) == 0, out
        kernel, inasm = None, False
        for ln in open(out):
            m = re.match(r"^(_Z\S*gemm_nt_w4[ch]_kernel\S*):", ln)
            if m:
                kernel = m.group(1) if re.search(r"ILb[01]ELb1EE", m.group(1)) else None
                seen += kernel is not None
            elif "#ASMSTART" in ln:
                inasm = True
            elif "#ASMEND" in ln:
                inasm = False
            elif ".end_amdhsa_kernel" in ln or ln.startswith(".Lfunc_end"):
                kernel = None
            elif kernel and not inasm:
                assert "v_accvgpr_" not in ln, (kernel, ln.strip())
                assert not ln.lstrip().startswith(("flat_load", "flat_store", "flat_atomic")), (kernel, ln.strip())
    assert seen == 3, seen
