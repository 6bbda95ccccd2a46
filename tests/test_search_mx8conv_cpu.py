"""conv0 of a search on block-scaled FP8 MFMAs, the host side: drn_amd.index.mx8_conv0_reference (the oracle of drn_conv0_mx8) against
torch's own conv1d on an input assembled row by row, mx8_gate_weights against mx8_quantize of the explicit product, and the two new
kernels' resource notes.  tests/test_search_mx8conv_gpu.py holds the kernels and the search."""
import types

import torch

from test_kernel_resources_cpu import kernel_table

NPROPS, OFF, VIDS, L12 = [12, 5, 1, 0, 20], [0, 12, 17, 18, 18, 38], [4, 1, -1, 3, 0, 5, 1], 12     # test_search_index_gpu.packed_case's tables


def host_case(C, P, Cout, D=None, seed=0):
    """packed_case's videos (12, 5, 1, 0 and 20 proposals: exact fit, ragged, one row, empty, truncated at L = 12), its slots with a
    repeat, -1 and Nv, and its 2 sentences x 7 slots, as a quantised index on the host: 39 rows, the last one the pad row."""
    from drn_amd.index import mx8_gate_weights, mx8_quantize
    D = C if D is None else D
    g = torch.Generator().manual_seed(1000 * C + P + Cout + seed)
    rows = torch.randn(39, C, generator=g) * torch.exp2(torch.randint(-6, 7, (39, 1), generator=g).float())
    rows[:, D:] = 0
    codes, scales = mx8_quantize(rows)
    pos = torch.randn(39, P, generator=g).bfloat16()
    W = torch.randn(Cout, D + P, 3, generator=g) * 0.25
    gate = torch.randn(2, D, generator=g) * torch.exp2(torch.randint(-3, 4, (2, D), generator=g).float())
    wcodes, wscales = mx8_gate_weights(W, gate, D, C)
    Wpos = W[:, D:, :].permute(2, 0, 1).bfloat16().contiguous()
    index = types.SimpleNamespace(codes=codes, scales=scales, pos=pos, prop_off=torch.tensor(OFF, dtype=torch.int32), pad_row=38)
    pair = torch.arange(14, dtype=torch.int32)
    return index, W, gate, wcodes, wscales, Wpos, torch.div(pair, 7, rounding_mode="floor"), pair % 7, torch.tensor(VIDS, dtype=torch.int32)


def test_the_oracle_is_torchs_conv1d_on_the_dequantised_rows():
    """Per pair the (L, Dp + P) input is assembled row by row from the dequantised index, the weight from the dequantised gated weights
    of the pair's sentence, and conv1d(padding=1) runs in float64.  L = 12 and L = 5 (every video but the one-row and the empty one is
    then cut)."""
    from drn_amd.index import mx8_conv0_reference, mx8_dequantize
    for C, P, Cout, L in ((64, 32, 16, 12), (160, 0, 48, 12), (64, 32, 16, 5), (64, 32, 16, 1)):
        index, W, gate, wcodes, wscales, Wpos, pq, pv, vids = host_case(C, P, Cout)
        got = mx8_conv0_reference(index, wcodes, wscales, Wpos if P else None, pq, pv, vids, L)
        assert got.dtype == torch.float64 and tuple(got.shape) == (14, L, Cout)
        z = mx8_dequantize(index.codes, index.scales).double()
        w = mx8_dequantize(wcodes.reshape(-1, C), wscales.reshape(-1, C // 32)).double().view(2, 3, Cout, C)
        for p in range(14):
            v = VIDS[p % 7]
            n = NPROPS[v] if 0 <= v < 5 else 0
            x = torch.zeros(L, C + P, dtype=torch.float64)
            for t in range(L):
                src = OFF[v] + t if t < n else 38
                x[t, :C] = z[src]
                x[t, C:] = index.pos[src].double()
            weight = torch.cat([w[p // 7], Wpos.double()], dim=2).permute(1, 2, 0)            # (Cout, C + P, 3)
            want = torch.nn.functional.conv1d(x.t()[None], weight, padding=1)[0].t()
            err = (got[p] - want).abs().max()
            assert float(err) <= 1e-12 * float(want.abs().max()), (C, P, Cout, L, p, float(err))
        # the pairs of slot -1, the empty video and position Nv see nothing but the pad row; the two sentences differ
        assert torch.equal(got[2], got[3]) and torch.equal(got[2], got[5]) and not torch.equal(got[0], got[7])
        if L == 12:
            assert not torch.equal(got[1], got[2])


def test_gated_weights_are_the_quantised_explicit_product():
    from drn_amd import _lib
    from drn_amd.index import mx8_gate_weights, mx8_quantize
    import pytest
    g = torch.Generator().manual_seed(3)
    S, Cout, D, Dp, P = 3, 16, 52, 64, 32
    W = torch.randn(Cout, D + P, 3, generator=g)
    gate = torch.randn(S, D, generator=g) * torch.exp2(torch.linspace(-12, 12, S * D).view(S, D))
    wcodes, wscales = mx8_gate_weights(W, gate, D, Dp)
    assert tuple(wcodes.shape) == (S, 3, Cout, Dp) and tuple(wscales.shape) == (S, 3, Cout, Dp // 32)
    assert wcodes.dtype == wscales.dtype == torch.uint8 and wcodes.is_contiguous() and wscales.is_contiguous()
    Wg = torch.zeros(S, 3, Cout, Dp)
    for s in range(S):
        for tap in range(3):
            for n in range(Cout):
                Wg[s, tap, n, :D] = gate[s] * W[n, :D, tap]
    want_c, want_s = mx8_quantize(Wg.view(-1, Dp))
    assert torch.equal(wcodes.view(-1, Dp), want_c) and torch.equal(wscales.view(-1, Dp // 32), want_s)
    assert not wcodes[..., D:].any() and bool(wcodes[..., :D].any())
    assert int(wscales.max()) - int(wscales.min()) >= 20                     # (the gate's magnitudes reach the scales)
    for bad in (dict(D=D, Dp=48), dict(D=D + 40, Dp=Dp), dict(D=D - 1, Dp=Dp)):
        with pytest.raises(_lib.DrnError):
            mx8_gate_weights(W, gate, bad["D"], bad["Dp"])


def test_the_new_kernels_spill_nothing_and_use_no_scratch(tmp_path):
    table = kernel_table(tmp_path)
    conv = [k for k in table if "conv0_mx8_kernel" in k]
    quant = [k for k in table if "gate_quantize_weights_mx8_kernel" in k]
    assert len(conv) == 6 and len(quant) == 1, (conv, quant)                 # MI in {1, 2, 4} x {bf16, fp32} outputs
    for k in conv + quant:
        assert table[k]["spill"] == 0 and table[k]["scratch"] == 0, (k, table[k])
