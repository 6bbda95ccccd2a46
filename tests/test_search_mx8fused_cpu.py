"""drn_conv0_mx8_bn, the host side: the resource notes of conv0_mx8_tiled_kernel in the built library (registers, scratch, LDS) and the
argument checks of ops.conv0_mx8_bn, which raise before the library is reached.  tests/test_search_mx8fused_gpu.py holds the kernel and
the search."""
import os
import re
import subprocess
import types

import pytest
import torch

from test_kernel_resources_cpu import LLVM, kernel_table
from test_search_mx8conv_cpu import host_case

LDS_PER_CU = 160 * 1024


def test_the_tiled_kernel_spills_nothing_and_one_workgroup_fills_a_cu(tmp_path):
    """Both instantiations (bf16 and fp32 outputs): no spill, no scratch, at most 256 registers -- its 8 waves are two per SIMD -- and
    a static LDS of two stages of (32 KB codes + 32 KB weight codes + 2 KB scales) plus the row table: more than half a CU's 160 KB, so
    ONE workgroup per CU by design, and no more than all of it."""
    table = kernel_table(tmp_path)
    tiled = [k for k in table if "conv0_mx8_tiled_kernel" in k]
    assert len(tiled) == 2 and not [k for k in tiled if "conv0_mx8_kernel" in k], tiled
    for k in tiled:
        assert table[k]["spill"] == 0 and table[k]["scratch"] == 0 and table[k]["vgpr"] + table[k]["agpr"] <= 256, (k, table[k])
    lds = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(str(tmp_path), f)], check=True,
                               capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and name.group(1) in tiled:
                lds[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert sorted(lds) == sorted(tiled)
    for k, v in lds.items():
        assert 2 * (2 * 256 * 128 + 2 * 256 * 4) <= v <= LDS_PER_CU and 2 * v > LDS_PER_CU, (k, v)


def test_the_wrapper_refuses_bad_arguments_without_reaching_the_library(monkeypatch):
    from drn_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_library)
    index, W, gate0, wcodes, wscales, wpos, pq, pv, vids = host_case(64, 32, 16)
    out, gated, gate = torch.zeros(14, 12, 16), torch.zeros(14, 12, 16), torch.ones(14, 16)
    args = lambda **kw: dict(dict(codes=index.codes, scales=index.scales, pos=index.pos, pad_row=38, prop_off=index.prop_off, wcodes=wcodes,
                                  wscales=wscales, wpos=wpos, pq=pq, pv=pv, vids=vids, ss=None, gate=gate, out=out, gated=gated, L=12, C=64,
                                  P=32), **kw)
    for kw, what in ((dict(gate=None), "gate and gated must come together"), (dict(gated=None), "gate and gated must come together"),
                     (dict(C=48), "multiples of 32"), (dict(P=16), "multiples of 32"), (dict(codes=index.codes.float()), "must be uint8"),
                     (dict(wcodes=wcodes[:, :2]), "wcodes"), (dict(wpos=wpos.float()), "wpos must be"), (dict(pos=None), "pos must be"),
                     (dict(wcodes=wcodes[:, :, :8].contiguous(), wscales=wscales[:, :, :8].contiguous()), "multiple of 16"),
                     (dict(), "GPU only")):
        with pytest.raises(_lib.DrnError, match=what):
            ops.conv0_mx8_bn(**args(**kw))
    assert not out.any() and not gated.any()


def test_the_agreement_fixtures_first_and_second_scores_are_further_apart_than_a_bf16_rounding():
    """tests/golden/search_mx8fused_scores.json: the first two hits (one per video) of the UNFUSED conv0="mxfp8" search on the fixture of
    test_the_fused_and_the_unfused_mode_name_the_same_first_video, recorded on an MI355X; that test holds the device to the record.
    For every sentence the first score exceeds the second by more than 2^-8 of itself -- the bf16 rounding of raw that separates the
    two modes -- and the two hits name different videos: "the same first video" is a condition the reference path alone satisfies."""
    import json
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_mx8fused_scores.json")))
    assert sorted(golden["sentences"]) == ["11", "7"]
    for seed, rec in golden["sentences"].items():
        score, video = torch.tensor(rec["score"], dtype=torch.float64), rec["video"]
        assert tuple(score.shape) == (3, 2) and all(v[0] != v[1] and min(v) >= 0 for v in video), (seed, video)
        assert bool((score[:, 0] - score[:, 1] > 2.0 ** -8 * score[:, 0].abs()).all()) and bool((score > 0).all()), (seed, score.tolist())
