"""Host side of grounding without a ground truth (drn_amd.grounding): the host twin of drn_select_moments against picks recorded
from the reference evaluator (tests/golden/moments.json, made by tests/golden/gen_moments_golden.py), the loader helper, and the
C-ABI boundary of the two new entry points."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "moments.json")))


def widened(preds):
    """The fixture's decimals name float32 values: the doubles the host path sees are those float32 values widened."""
    return np.asarray(preds, dtype=np.float32).astype(np.float64).reshape(-1, 3).tolist()


def test_the_fixture_covers_what_it_was_built_for():
    cases = GOLD["cases"]
    assert len(cases) >= 200
    assert {(c["overlap"], c["k"]) for c in cases} == {(o, k) for o in (0.25, 0.45, 0.65) for k in (1, 5, 100)}
    assert any(len(c["preds"]) > 64 for c in cases) and any(len(c["preds"]) == 1 for c in cases)
    assert any(c["survivors"] < len(c["preds"]) for c in cases) and any(c["survivors"] == len(c["preds"]) > 1 for c in cases)
    assert any(len({p[2] for p in c["preds"]}) < len(c["preds"]) for c in cases)                       # exact score ties
    assert any(len({(p[0], p[1]) for p in c["preds"]}) < len(c["preds"]) for c in cases)               # duplicate segments
    assert any(sum(p[0] == p[1] for p in c["preds"]) >= 2 for c in cases)                              # 0/0 pairs
    for c in cases:
        assert len(c["picks"]) == min(c["k"], c["survivors"])


@pytest.mark.parametrize("overlap", GOLD["overlaps"])
def test_host_select_moments_equals_the_reference_picks(overlap):
    from drn_amd.metrics import select_moments
    n = 0
    for c in GOLD["cases"]:
        if c["overlap"] != overlap:
            continue
        assert select_moments(widened(c["preds"]), c["k"], c["overlap"]) == c["picks"], c["tag"]
        n += 1
    assert n >= 60


def test_host_select_moments_edges():
    from drn_amd.metrics import select_moments
    assert select_moments([], 5, 0.45) == []
    assert select_moments([[0.0, 1.0, 1.0]], 5, 0.45) == [0]
    assert select_moments([[0.1, 0.5, 0.3], [0.6, 0.9, 0.3]], 5, 0.45) == [1, 0]         # a tie goes to the later candidate
    assert select_moments([[0.1, 0.5, 0.3], [0.6, 0.9, 0.3]], 0, 0.45) == []


def test_group_by_video():
    from drn_amd import group_by_video
    unique, index = group_by_video(["b", "a", "b", "c", "a", "b"])
    assert unique == ["b", "a", "c"]
    assert index.dtype == torch.int64 and index.tolist() == [0, 1, 0, 2, 1, 0]
    unique, index = group_by_video(["x", "y"])
    assert unique == ["x", "y"] and index.tolist() == [0, 1]
    unique, index = group_by_video([])
    assert unique == [] and index.numel() == 0


def test_public_names_are_exported():
    import drn_amd
    from drn_amd import grounding
    assert drn_amd.Grounder is grounding.Grounder and drn_amd.Moments is grounding.Moments
    from drn_amd.trainer import Trainer
    assert callable(Trainer.predict)


def built_lib():
    from drn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_library_exports_the_new_entry_points_at_abi_9():
    from drn_amd import _lib
    lib = built_lib()
    for name in ("drn_select_moments", "drn_gate_gather_fwd"):
        assert name in _lib.declared_symbols(), name
        assert hasattr(lib, name), name
    assert lib.drn_abi_version() == 9


def _header_params(name):
    txt = open(os.path.join(ROOT, "include", "drn_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", ["drn_select_moments", "drn_gate_gather_fwd"])
def test_header_and_ctypes_signatures_agree(name):
    """Argument count, and argument by argument the class: pointer, double, or int."""
    import ctypes
    from drn_amd import _lib
    params = _header_params(name)
    sig = _lib.SIGNATURES[name]
    assert len(params) == len(sig), (params, sig)
    for p, t in zip(params, sig):
        want = ctypes.c_void_p if "*" in p else ctypes.c_double if p.startswith("double ") else ctypes.c_int
        assert t is want, (name, p, t)
    assert list(getattr(built_lib(), name).argtypes) == list(sig)


def test_argument_checks_answer_before_anything_is_launched():
    """Both entry points validate on the host first: a bad level table, a host index outside [0, V), rows that are not 16-byte
    multiples -- each an error return with a message, no device work (this runs without a GPU)."""
    import ctypes
    L = built_lib()
    p = ctypes.c_void_p(0x1000)
    assert L.drn_select_moments(p, p, p, 2, 3, 4 * 2048 + 1, 0.45, 5, p, p, p, p, p, None) != 0
    assert b"candidate slots per clip" in L.drn_last_error()
    assert L.drn_select_moments(p, p, p, 2, 3, 64, 0.45, 0, p, p, p, p, p, None) != 0
    assert L.drn_select_moments(p, p, p, 2, 3, 64, 0.45, 5, None, p, p, p, p, None) != 0
    vid = (ctypes.c_int32 * 3)(0, 2, 1)
    host = ctypes.cast(vid, ctypes.c_void_p)
    assert L.drn_gate_gather_fwd(p, 64, p, 64, p, 64, p, host, 2, p, 128, 3, 8, 64, 64, 0, None) != 0
    assert b"query 1 reads video 2 of 2" in L.drn_last_error()
    assert L.drn_gate_gather_fwd(p, 64, p, 64, p, 64, p, None, 2, p, 128, 3, 8, 62, 64, 0, None) != 0
    assert b"16-byte multiples" in L.drn_last_error()
    assert L.drn_gate_gather_fwd(p, 64, p, 64, None, 0, p, None, 2, p, 128, 3, 8, 64, 64, 0, None) != 0      # P > 0 without pos
    assert L.drn_gate_gather_fwd(p, 64, p, 64, p, 64, p, None, 2, p, 64, 3, 8, 64, 64, 0, None) != 0         # ld_out < C + P


def test_grounder_refuses_cpu_tensors_and_train_mode():
    from drn_amd import Grounder, _lib
    from drn_amd.model import mainModel
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, synthetic_batch
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("TINY", 64, 1)))
    batch = synthetic_batch(2, 32, 64)
    with pytest.raises(_lib.DrnError):
        Grounder(m.eval()).ground(*batch[:4])
    with pytest.raises(_lib.DrnError):
        Grounder(m.train()).ground(*batch[:4])
    assert m.fcos.box_selector_test.device_only is False
    with pytest.raises(_lib.DrnError):
        Grounder(m, top_k=0)
