"""drn_conv0_mx8_bn_tile, the host side: the resource notes of every conv0_mx8_narrow_kernel instantiation against the occupancy
DESIGN.md section 3 claims for its tile, the refusal of a `tile` that is not shipped before the library is reached, the entries in the
header, the chooser's constants in the source and the shape of the recorded digests.  tests/test_search_mx8tiles_gpu.py holds the
kernels and the search."""
import json
import os
import re
import subprocess

import pytest
import torch

from test_kernel_resources_cpu import LLVM, kernel_table
from test_search_mx8conv_cpu import host_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
# tile -> (workgroups per CU claimed, registers that allows a 4-wave workgroup: 512 per SIMD lane over that many waves, in the
# allocation granule of 8).  The static LDS allowed is LDS_PER_CU over the same count.
CLAIMS = {(128, 64): (2, 256), (64, 64): (3, 168)}


def test_every_narrow_tile_fits_the_occupancy_it_claims(tmp_path):
    """Both output types of each tile: no spill, no scratch, registers and static LDS within `CLAIMS`, and at least the two stages of
    (ROWS + COLS) x (128 + 4) bytes.  The wide kernel keeps exactly its two instantiations."""
    from drn_amd import ops
    table = kernel_table(tmp_path)
    assert len([k for k in table if "conv0_mx8_tiled_kernel" in k]) == 2
    narrow = [k for k in table if "conv0_mx8_narrow_kernel" in k]
    shipped = [t for t in ops.CONV0_MX8_TILES if t != ops.CONV0_MX8_WIDE]
    assert sorted(shipped) == sorted(CLAIMS) and len(narrow) == 2 * len(shipped), narrow
    lds = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", os.path.join(str(tmp_path), f)], check=True,
                               capture_output=True, text=True).stdout
        for blk in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if name and name.group(1) in narrow:
                lds[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert sorted(lds) == sorted(narrow)
    for (rows, cols), (per_cu, regs) in CLAIMS.items():
        ks = [k for k in narrow if "Li%dELi%dEE" % (rows, cols) in k]                        # Itanium mangling of <OUT, ROWS, COLS>
        assert len(ks) == 2, (rows, cols, ks)
        for k in ks:
            r = table[k]
            assert r["spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= regs, (k, r)
            assert 2 * (rows + cols) * 132 <= lds[k] and per_cu * lds[k] <= LDS_PER_CU, (k, lds[k])


def test_the_recorded_digests_cover_the_five_geometries_in_both_modes_and_name_their_commit():
    """tests/golden/search_mx8_tile_digests.json, which test_every_tile_writes_the_recorded_bits holds the device to: one record for
    each of that file's GEOMETRIES (by the ids it gives them), each a sha256 of the operands, of the fp32 output and of the bf16 outputs,
    all different, and the commit whose wide kernel wrote them."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "search_mx8_tile_digests.json")))
    assert re.fullmatch(r"[0-9a-f]{40}", golden["commit"])
    gpu = open(os.path.join(ROOT, "tests", "test_search_mx8tiles_gpu.py")).read()
    ids = []
    for L, Cout, Dp, P, order in ((12, 16, 64, 0, "sorted"), (70, 272, 160, 32, "interleaved"), (300, 80, 384, 32, "shuffled"),
                                  (12, 80, 384, 0, "interleaved"), (70, 272, 64, 32, "shuffled")):
        assert '(%d, %d, %d, %d, %s, "%s")' % (L, Cout, Dp, P, order.upper(), order) in gpu          # (a geometry of that file)
        ids.append("L%d-Cout%d-Dp%d-P%d-%s" % (L, Cout, Dp, P, order))
    assert gpu.count(', "sorted")') + gpu.count(', "interleaved")') + gpu.count(', "shuffled")') == len(ids)
    assert sorted(golden["digests"]) == sorted(ids)
    seen = set()
    for rec in golden["digests"].values():
        assert sorted(rec) == ["bf16", "fp32", "operands"] and all(re.fullmatch(r"[0-9a-f]{64}", v) for v in rec.values()), rec
        seen.update(rec.values())
    assert len(seen) == 3 * len(ids)


def test_the_wrapper_refuses_a_tile_that_is_not_shipped_and_bad_arguments_under_auto(monkeypatch):
    from drn_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "lib", no_library)
    assert ops.CONV0_MX8_TILES[0] == ops.CONV0_MX8_WIDE == (256, 256) and len(set(ops.CONV0_MX8_TILES)) == len(ops.CONV0_MX8_TILES) <= 4
    assert any(c < 256 for _, c in ops.CONV0_MX8_TILES) and any(r < 256 for r, _ in ops.CONV0_MX8_TILES)
    index, W, gate0, wcodes, wscales, wpos, pq, pv, vids = host_case(64, 32, 16)
    out, gated, gate = torch.zeros(14, 12, 16), torch.zeros(14, 12, 16), torch.ones(14, 16)
    args = lambda **kw: dict(dict(codes=index.codes, scales=index.scales, pos=index.pos, pad_row=38, prop_off=index.prop_off, wcodes=wcodes,
                                  wscales=wscales, wpos=wpos, pq=pq, pv=pv, vids=vids, ss=None, gate=gate, out=out, gated=gated, L=12, C=64,
                                  P=32), **kw)
    not_shipped = next(t for t in ((256, 64), (128, 128), (32, 32)) if t not in ops.CONV0_MX8_TILES)
    for tile in ((100, 64), "wide", not_shipped, (64,), (64, 64, 64), (64.0, 64.0), 64, (0, 0), "AUTO", True):
        with pytest.raises(_lib.DrnError, match="tile must be"):
            ops.conv0_mx8_bn(**args(tile=tile))
    # every bad argument of tests/test_search_mx8fused_cpu.py's refusal test, under "auto" and under an explicit narrow tile
    for tile in ("auto", ops.CONV0_MX8_TILES[-1]):
        for kw, what in ((dict(gate=None), "gate and gated must come together"), (dict(gated=None), "gate and gated must come together"),
                         (dict(C=48), "multiples of 32"), (dict(P=16), "multiples of 32"), (dict(codes=index.codes.float()), "must be uint8"),
                         (dict(wcodes=wcodes[:, :2]), "wcodes"), (dict(wpos=wpos.float()), "wpos must be"), (dict(pos=None), "pos must be"),
                         (dict(wcodes=wcodes[:, :, :8].contiguous(), wscales=wscales[:, :, :8].contiguous()), "multiple of 16"),
                         (dict(), "GPU only")):
            with pytest.raises(_lib.DrnError, match=what):
                ops.conv0_mx8_bn(**args(tile=tile, **kw))
    assert not out.any() and not gated.any()


def test_the_two_entries_are_declared_exported_and_mirrored_at_abi_9():
    """Header, library and ctypes table agree on the two entries; the _tile entry is drn_conv0_mx8_bn's argument list with the two tile
    ints before the stream."""
    import ctypes
    from drn_amd import _lib
    lib = _lib.lib()
    assert lib.drn_abi_version() == 9
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "drn_hip.h")).read(), flags=re.S)
    for name in ("drn_conv0_mx8_bn_tile", "drn_conv0_mx8_bn_choose"):
        assert name in _lib.declared_symbols() and hasattr(lib, name), name
        params = [" ".join(p.split()) for p in re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr).group(1).split(",")]
        sig = _lib.SIGNATURES[name]
        assert len(params) == len(sig), (name, params)
        for p, t in zip(params, sig):
            assert t is (ctypes.c_void_p if "*" in p else ctypes.c_int), (name, p, t)
        assert list(getattr(lib, name).argtypes) == list(sig)
    wide, tile = _lib.SIGNATURES["drn_conv0_mx8_bn"], _lib.SIGNATURES["drn_conv0_mx8_bn_tile"]
    assert tile == wide[:-1] + [ctypes.c_int, ctypes.c_int] + wide[-1:]


def test_the_chooser_answers_without_a_device_and_its_constants_are_the_sources():
    """drn_conv0_mx8_bn_choose is host logic: bad shapes are refused, and on a machine without a GPU it names the wide tile.  The two
    thresholds of its rule are those ops mirrors for the GPU test of the rule."""
    from drn_amd import _lib, ops
    src = open(os.path.join(ROOT, "drn_amd", "csrc", "qconv.hip")).read()
    assert int(re.search(r"#define MXN_SMALL_UPTO_16THS\s+(\d+)", src).group(1)) == ops.CONV0_MX8_SMALL_UPTO_16THS
    assert int(re.search(r"#define MXN_MID_UPTO_16THS\s+(\d+)", src).group(1)) == ops.CONV0_MX8_MID_UPTO_16THS
    assert 0 < ops.CONV0_MX8_SMALL_UPTO_16THS < ops.CONV0_MX8_MID_UPTO_16THS <= 16
    for bad in ((0, 32, 64), (4, 0, 64), (4, 32, 0), (1 << 20, 1 << 12, 64)):
        with pytest.raises(_lib.DrnError, match="bad args"):
            ops.conv0_mx8_bn_tile(*bad)
    if not torch.cuda.is_available():
        assert ops.conv0_mx8_bn_tile(64, 32, 256) == ops.CONV0_MX8_WIDE
    # the C entry refuses a shape that is not shipped before it looks at anything else (null pointers here)
    import ctypes
    args = [None if t is ctypes.c_void_p else 0 for t in _lib.SIGNATURES["drn_conv0_mx8_bn_tile"]]
    args[-8], args[-7], args[-4], args[-3], args[-2] = 4, 32, 64, 100, 64                     # Q, L, Cout, tile_rows, tile_cols
    assert _lib.lib().drn_conv0_mx8_bn_tile(*args) != 0 and b"no 100 x 64 tile" in _lib.lib().drn_last_error()
