"""Host side of the block-scaled FP8 search index (SearchIndex.build(quantize="mxfp8")): the C-ABI boundary of drn_quantize_rows_mx8 and
drn_gate_gather_packed_q8, the refusals that need no GPU, and the format's definition -- drn_amd.index.mx8_quantize / mx8_dequantize --
on rows built for its corners and on random rows.  tests/test_search_q8_gpu.py holds the kernels to this definition byte for byte."""
import ctypes

import pytest
import torch

from test_grounding_cpu import _header_params, built_lib

NAMES = ("drn_quantize_rows_mx8", "drn_gate_gather_packed_q8")


# -- 1. the library and the refusals ------------------------------------------------------------------------------------------------------

def test_library_exports_both_entry_points_at_abi_9():
    from drn_amd import _lib, index, ops
    lib = built_lib()
    for name in NAMES:
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
    assert lib.drn_abi_version() == 9
    assert callable(ops.quantize_rows_mx8) and callable(ops.gate_gather_packed_q8)
    assert callable(index.mx8_quantize) and callable(index.mx8_dequantize) and callable(index.SearchIndex.dequantized)


@pytest.mark.parametrize("name", NAMES)
def test_header_and_ctypes_signatures_agree(name):
    from drn_amd import _lib
    params = _header_params(name)
    sig = _lib.SIGNATURES[name]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (p, t)
    assert list(getattr(built_lib(), name).argtypes) == list(sig)


def test_quantize_rows_refuses_before_anything_is_launched():
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def call(ptrs=None, ld_x=72, n=39, C=64, ld_codes=80, ld_scales=3, dtype=1):
        a = [p] * 3 if ptrs is None else ptrs              # x codes scales
        return L.drn_quantize_rows_mx8(a[0], ld_x, n, C, a[1], ld_codes, a[2], ld_scales, dtype, None)
    for i in range(3):
        assert call(ptrs=[None if j == i else p for j in range(3)]) != 0, i
        assert b"null pointer" in L.drn_last_error()
    for C in (48, 72, 1):
        assert call(C=C, ld_x=80) != 0 and b"not a multiple of the block of 32" in L.drn_last_error()
    assert call(ld_x=56) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ld_codes=48) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ld_scales=1) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ld_x=68) != 0 and b"16-byte multiples" in L.drn_last_error()               # 68 bf16 = 136 bytes
    assert call(ld_x=66, dtype=0) != 0 and b"16-byte multiples" in L.drn_last_error()      # 66 f32 = 264 bytes
    assert call(ld_codes=72) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(ptrs=[ctypes.c_void_p(0x1008), p, p]) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(ptrs=[p, ctypes.c_void_p(0x1004), p]) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(n=0) != 0 and call(C=0) != 0
    assert call(dtype=7) != 0 and b"bad dtype" in L.drn_last_error()


def test_gate_gather_q8_refuses_before_anything_is_launched():
    """tests/test_search_index_cpu.py's refusals of drn_gate_gather_packed, on the quantised entry point."""
    L = built_lib()
    p = ctypes.c_void_p(0x1000)

    def call(ptrs=None, pq_host=None, ld_codes=64, ld_scales=2, ld_pos=16, n_rows=71, pad_row=70, Nv=5, ldg=64, S=2, Vc=7, ld_out=80, Q=14,
             T=12, C=64, P=16, dtype=1):
        a = [p] * 9 if ptrs is None else ptrs              # codes scales pos prop_off gate pq pv vids out
        return L.drn_gate_gather_packed_q8(a[0], ld_codes, a[1], ld_scales, a[2], ld_pos, n_rows, pad_row, a[3], Nv, a[4], ldg, S, a[5],
                                           pq_host, a[6], a[7], Vc, a[8], ld_out, Q, T, C, P, dtype, None)
    for i in range(9):
        assert call(ptrs=[None if j == i else p for j in range(9)]) != 0, i
        assert b"null pointer" in L.drn_last_error()
    for C in (48, 72):
        assert call(C=C, ld_codes=80, ldg=80, ld_out=96) != 0 and b"not a multiple of the block of 32" in L.drn_last_error()
    assert call(P=12) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(ld_codes=72) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(ld_pos=20) != 0 and b"16-byte multiples" in L.drn_last_error()
    assert call(ld_out=72) != 0 and b"shorter than its row" in L.drn_last_error()          # ld_out < C + P
    assert call(ld_codes=48) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ld_scales=1) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ld_pos=8) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(ldg=32) != 0 and b"shorter than its row" in L.drn_last_error()
    assert call(pad_row=71) != 0 and call(pad_row=-1) != 0 and call(n_rows=0, pad_row=0) != 0
    assert call(Q=0) != 0 and call(T=0) != 0 and call(C=0) != 0 and call(P=-8) != 0 and call(S=0) != 0 and call(Vc=0) != 0 and call(Nv=0) != 0
    assert call(Q=1 << 20, T=1 << 12) != 0 and b"2^31 rows" in L.drn_last_error()
    assert call(dtype=7) != 0 and b"bad dtype" in L.drn_last_error()
    for bad, text in ((2, b"pair 3 reads sentence 2 of 2"), (-1, b"pair 3 reads sentence -1 of 2")):
        pq = (ctypes.c_int32 * 14)(*([0, 1, 1, bad] + [0] * 10))
        assert call(pq_host=ctypes.cast(pq, ctypes.c_void_p)) != 0 and text in L.drn_last_error()


def test_the_wrappers_refuse_other_code_types_and_host_tensors():
    from drn_amd import _lib, ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8)
    gate, out, pos = torch.zeros(2, 64), torch.zeros(14, 12, 80), torch.zeros(71, 16)
    args = (70, i32(6), gate, i32(14), i32(14), i32(7), out, 12, 64, 16, 0)
    with pytest.raises(_lib.DrnError, match="must be uint8"):
        ops.gate_gather_packed_q8(torch.zeros(71, 64, dtype=torch.int8), u8(71, 2), pos, *args)
    with pytest.raises(_lib.DrnError, match="must be uint8"):
        ops.gate_gather_packed_q8(torch.zeros(71, 64), u8(71, 2), pos, *args)
    with pytest.raises(_lib.DrnError, match="must be uint8"):
        ops.gate_gather_packed_q8(u8(71, 64), torch.zeros(71, 2), pos, *args)
    with pytest.raises(_lib.DrnError, match="must be uint8"):
        ops.gate_gather_packed_q8(u8(71, 64), u8(71, 1), pos, *args)                       # one scale for two blocks
    with pytest.raises(_lib.DrnError, match="pos must be"):
        ops.gate_gather_packed_q8(u8(71, 64), u8(71, 2), None, *args)
    with pytest.raises(_lib.DrnError, match="pos must be"):
        ops.gate_gather_packed_q8(u8(71, 64), u8(71, 2), pos.bfloat16(), *args)
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.gate_gather_packed_q8(u8(71, 64), u8(71, 2), pos, *args)
    with pytest.raises(_lib.DrnError, match="codes must be"):
        ops.quantize_rows_mx8(torch.zeros(5, 64), torch.zeros(5, 64, dtype=torch.int8), u8(5, 2))
    with pytest.raises(_lib.DrnError, match="scales must be"):
        ops.quantize_rows_mx8(torch.zeros(5, 64), u8(5, 64), u8(5, 1))
    with pytest.raises(_lib.DrnError, match="GPU only"):
        ops.quantize_rows_mx8(torch.zeros(5, 64), u8(5, 64), u8(5, 2))


def test_build_refuses_another_format_and_sizes_a_quantised_index_before_allocating():
    import types
    from drn_amd import FeatureStore, SearchIndex, _lib
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1))).eval()
    videos = [("v%d" % v, torch.randn(8, 64), [0, 2], [3, 7], [[0.0, 0.5], [0.25, 1.0]], 64) for v in range(3)]
    store = FeatureStore.from_tensors(videos, "cpu", torch.float32)
    for bad in ("int4", "fp8", ""):
        with pytest.raises(_lib.DrnError, match="quantize must be None or"):
            SearchIndex.build(m, store, quantize=bad)
        with pytest.raises(_lib.DrnError, match="quantize must be None or"):
            SearchIndex.bytes_of(6, 320, torch.float32, 3, quantize=bad, P=256)
    with pytest.raises(_lib.DrnError, match="store on the GPU"):
        SearchIndex.build(m, store, quantize="mxfp8")
    need = SearchIndex.bytes_of(6, 64 + 256, torch.float32, 3, quantize="mxfp8", P=256)
    assert need == 7 * (64 + 2 + 256 * 4) + 4 * 4
    # the benchmarked shape: 4736 instead of 8704 bytes a row
    assert SearchIndex.bytes_of(0, 4096 + 256, torch.bfloat16, 0, quantize="mxfp8", P=256) - 4 == 4736
    assert SearchIndex.bytes_of(0, 4096 + 256, torch.bfloat16, 0) - 4 == 8704
    with pytest.raises(_lib.DrnError, match="needs P"):
        SearchIndex.bytes_of(6, 320, torch.float32, 3, quantize="mxfp8")
    with pytest.raises(_lib.DrnError, match="multiple of 32"):
        SearchIndex.bytes_of(6, 300, torch.float32, 3, quantize="mxfp8", P=256)
    store.feats = types.SimpleNamespace(is_cuda=True, device="cuda:0")
    with pytest.raises(_lib.DrnError, match="mxfp8\\) need %d bytes on the device, max_bytes is %d" % (need, need - 1)):
        SearchIndex.build(m, store, max_bytes=need - 1, quantize="mxfp8")
    plain = SearchIndex()
    assert plain.quantize is None and plain.resident is None
    plain.rows = torch.zeros(2, 4)
    assert plain.resident is plain.rows
    with pytest.raises(_lib.DrnError, match="not quantised"):
        plain.dequantized()


# -- 2. the definition on rows built for its corners ----------------------------------------------------------------------------------

def corner_rows(C=64):
    """Rows of C >= 64 float32 columns, zero but for the planted values; every row's block 1 (columns 32..63) is zero unless said.
    -> x, and per row (block 0's e, [(column, code), ...]) where the test knows them."""
    x = torch.zeros(12, C)
    want = {}
    want[0] = (-110, [(0, 0), (31, 0)])                                # a zero row
    x[1, 40] = 3.0                                                     # a zero block (0) inside a non-zero row: block 1 = 3 = 0.75 * 2^2
    want[1] = (-110, [(0, 0), (40, 0x7c)])                             # e = -7, 3 * 2^7 = 384 = 1.5 * 2^8 -> 0x7c
    x[2, 3], x[2, 4] = 448.0 * 32, 17.0 * 32                           # amax exactly 448 * 2^5: e = 5, |code| 448 = 0x7e
    want[2] = (5, [(3, 0x7e), (4, 0x58)])                              # 17 -> 16 = 0x58
    x[3, 0], x[3, 1] = 480.0, 1.0                                      # 480 = 0.9375 * 2^9 -> e = 1; 240 = 0x77; 0.5 = 0x30
    want[3] = (1, [(0, 0x77), (1, 0x30)])
    x[4, 5] = -448.0 * 2 ** -3                                         # e = -3, the sign kept: 0xfe
    want[4] = (-3, [(5, 0xfe), (4, 0), (6, 0)])
    x[5, 0] = 3e38                                                     # 3e38 = 0.88 * 2^128 -> e = 120
    want[5] = (120, [(0, 0x76)])                                       # 3e38 / 2^120 = 225.7 -> 224 = 0x76
    x[6, 0] = 1e-38                                                    # below the clamp: e = -110, 1e-38 * 2^110 = 2^-16.2 -> 0
    want[6] = (-110, [(0, 0)])
    x[7, :5] = torch.tensor([256.0, 17.0, 19.0, 2.0 ** -10, 2.0 ** -9])  # a scale of 1 (256 = 0.5 * 2^9): the ties
    want[7] = (0, [(0, 0x78), (1, 0x58), (2, 0x5a), (3, 0), (4, 1)])   # 17 -> 16, 19 -> 20, 2^-10 -> 0; 2^-9 is the smallest code
    x[8, 0], x[8, 1], x[8, 2] = 256.0, -2.0 ** -11, -2.0 ** -10        # negatives that round to -0 keep code 0x80
    want[8] = (0, [(1, 0x80), (2, 0x80)])
    x[9, 0] = 225.0                                                    # 225 = 0.879 * 2^8 -> e = 0, rounds to 224 (scale not idempotent)
    want[9] = (0, [(0, 0x76)])
    x[10, 0] = 224.0                                                   # 224 = 0.875 * 2^8, m <= 0.875 -> e = -1, code 448
    want[10] = (-1, [(0, 0x7e)])
    x[11, 0], x[11, 33] = -1e-38, 2.0 ** -100                          # block 1 = 2^-100 -> k = -99, e = -108: a normal scale near the clamp
    want[11] = (-110, [(0, 0x80), (33, 0x78)])
    return x, want


def test_the_definition_on_the_corner_rows():
    from drn_amd.index import mx8_dequantize, mx8_quantize
    x, want = corner_rows()
    codes, scales = mx8_quantize(x)
    assert codes.dtype == scales.dtype == torch.uint8 and tuple(codes.shape) == (12, 64) and tuple(scales.shape) == (12, 2)
    for r, (e, cells) in want.items():
        assert int(scales[r, 0]) - 127 == e, (r, int(scales[r, 0]) - 127, e)
        for c, code in cells:
            assert int(codes[r, c]) == code, (r, c, hex(int(codes[r, c])), hex(code))
    assert int(scales[1, 1]) - 127 == -7 and int(scales[11, 1]) - 127 == -108
    assert scales[[0, 2, 3, 4, 5, 6, 7, 8, 9, 10], 1].tolist() == [17] * 10          # zero blocks: e = -110
    assert int(scales.max()) < 255 and int((codes & 0x7f).max()) <= 0x7e              # never the e8m0 NaN, never an e4m3 NaN
    dq = mx8_dequantize(codes, scales)
    assert dq[2, 3] == 448.0 * 32 and dq[2, 4] == 512.0 and dq[3, 0] == 480.0 and dq[4, 5] == -56.0 and dq[9, 0] == 224.0
    assert dq[7, :5].tolist() == [256.0, 16.0, 20.0, 0.0, 2.0 ** -9]
    assert dq[8, 1] == 0 and torch.signbit(dq[8, 1]) and torch.signbit(dq[11, 0]) and dq[11, 33] == 2.0 ** -100
    assert abs(float(dq[5, 0]) - 3e38) <= 3e38 / 16
    # the same rows in bf16 (the values that bf16 holds exactly), and a 3-d or ragged input is refused
    keep = [0, 1, 2, 3, 4, 7, 8, 10]
    cb, sb = mx8_quantize(x[keep].bfloat16())
    assert torch.equal(cb, codes[keep]) and torch.equal(sb, scales[keep])
    from drn_amd import _lib
    with pytest.raises(_lib.DrnError, match="multiple of 32"):
        mx8_quantize(torch.zeros(3, 48))
    with pytest.raises(_lib.DrnError, match="must be uint8"):
        mx8_dequantize(codes, scales[:, :1])


# -- 3. properties on random rows -----------------------------------------------------------------------------------------------------

def random_rows(dtype, n=64, C=96, seed=3):
    """Row r has magnitude 2^(r * 40 / (n - 1) - 20): 2^-20 .. 2^20; a few zeros are planted."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * torch.exp2(torch.linspace(-20, 20, n)).unsqueeze(1)
    x[::7, 5] = 0.0
    x[3, 32:64] = 0.0
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_properties_on_random_rows(dtype):
    from drn_amd.index import mx8_dequantize, mx8_quantize
    x = random_rows(dtype)
    n, C = x.shape
    codes, scales = mx8_quantize(x)
    e = scales.to(torch.int32) - 127
    dq = mx8_dequantize(codes, scales)
    assert dq.dtype == torch.float32
    # the error bound: half an e4m3 ulp (3 mantissa bits: 2^-4 relative) or half the smallest code (2^-9 * 2^e)
    bound = torch.maximum(x.float().abs() * 2.0 ** -4, torch.ldexp(torch.ones(()), e - 10).repeat_interleave(32, dim=1))
    assert bool(((dq - x.float()).abs() <= bound).all())
    assert not torch.equal(dq, x.float())
    # exact in the dtype: the bf16 result holds the fp32 values
    got = mx8_dequantize(codes, scales, dtype)
    assert got.dtype == dtype and torch.equal(got.float(), dq)
    assert torch.equal(mx8_dequantize(codes, scales, torch.bfloat16).float(), dq)
    # idempotent on values
    c2, s2 = mx8_quantize(got)
    assert torch.equal(mx8_dequantize(c2, s2), dq)
    # a block uses the top of the code range unless it is zero (none is clamped here): amax * 2^-e is in (224, 448] -- e is the smallest
    # scale that fits -- and the block's largest |code value| is that number rounded to e4m3, so it is in [224, 448]: 224 itself is
    # reached from (224, 232], which rounds down (the case that makes the SCALES not idempotent)
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    top = table[(codes & 0x7f).long()].reshape(n, C // 32, 32).amax(dim=2)
    amax = x.float().reshape(n, C // 32, 32).abs().amax(dim=2)
    zero = amax == 0
    assert bool(zero[3, 1]) and int(zero.sum()) == 1 and bool((e[zero] == -110).all()) and bool((top[zero] == 0).all())
    assert int(e[~zero].min()) > -110
    scaled = torch.ldexp(amax, -e)[~zero]
    assert bool(((scaled > 224) & (scaled <= 448)).all()), scaled
    assert bool(((top[~zero] >= 224) & (top[~zero] <= 448)).all()), top
    assert bool(((top[~zero] > 224) | (scaled <= 232)).all())
    assert torch.equal(top[~zero], scaled.to(torch.float8_e4m3fn).float())
