"""Eval-mode inference and training-mode running statistics with REAL BatchNorm statistics, at the BASELINE.json configuration
shapes.  Every other parity test runs eval mode with running statistics of exactly 0 and 1, where eval BN reduces to
gamma * x / sqrt(1 + eps) + beta and the running mean, the conv-bias fold and the stacked towers' statistics halves do not
matter.  Here the statistics come from one momentum-1 train-mode forward of the CPU oracle on another batch (stats_state).

- eval forward (bn_eval_scale_shift + bn_apply_multi, the FPN top-down chain one bn_apply per level) vs the oracle, fp32 and bf16,
  and the device post-processor vs the oracle's on the HIP heads;
- the running statistics one train-mode forward writes at the benchmarked shape (w4h / w4c slab statistics, the one-launch
  conv -> BN) vs the oracle;
- Trainer.evaluate between hipGraph-replayed training steps: current weights, no side effect on the model or the trajectory."""
import functools

import numpy as np
import pytest
import torch

from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict, synthetic_batch
from helpers import assert_state_equal, state_snapshot
from test_configs_gpu import SHAPES, check_outputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cfg_for(D, stage):
    return default_cfg("C3D" if D == 4096 else "SYN", D, stage)


@functools.lru_cache(maxsize=3)
def stats_state(B, T, D):
    """The seed-0 oracle's state_dict after one train-mode forward (momentum 1.0, no_grad) on the seed-2 batch: every running_mean /
    running_var holds that batch's statistics (the towers' shared BNs: those of the coarsest level, the last one they saw), every
    num_batches_tracked is non-zero.  The statistics do not depend on the stage flags."""
    from oracle import drn_oracle as O
    m = O.mainModel(VOCAB_SIZE, as_namespace(cfg_for(D, 1)))
    m.load_state_dict(seeded_state_dict(m, 0))
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.momentum = 1.0
    m.train()
    with torch.no_grad():
        m(*synthetic_batch(B, T, D, seed=2))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    for k, v in sd.items():                        # (the point of the exercise)
        if k.endswith("running_mean"):
            assert float(v.abs().max()) > 1e-2, k
        elif k.endswith("running_var"):
            assert float((v - 1).abs().max()) > 1e-2, k
    return sd


def build(cls, cfg, sd, dev="cpu", **kw):
    m = cls(VOCAB_SIZE, as_namespace(cfg), **kw)
    m.load_state_dict(sd)
    return m.to(dev)


def forward(m, batch, dev, train=False):
    """One forward; returns (boxes, losses, head outputs).  In eval mode every parameter and buffer must come out bit-identical."""
    b = [x.to(dev) for x in batch]
    if dev == "cpu":
        b[1] = batch[1]
    m.train(train)
    before = None if train else state_snapshot(m)
    caught = {}
    if hasattr(m, "taps"):
        m.taps = caught
        boxes, losses = m(*b)
        m.taps = None
    else:
        h = m.fcos.head.register_forward_hook(lambda mod, i, o: caught.__setitem__("head", o))
        boxes, losses = m(*b)
        h.remove()
    if dev != "cpu":
        torch.cuda.synchronize()
    if not train:
        assert_state_equal(before, state_snapshot(m), "eval forward")
    return boxes, losses, caught["head"]


def check_detections(got, want):
    """tests/test_postproc_gpu.py's rule: per clip and level the same SET of kept location indices (exact), detections / scores
    within 2e-6."""
    assert len(got) == len(want)
    kept = 0
    for b in range(len(want)):
        lv_g = [x for l in got[b]["level"] for x in l]
        lv_w = [x for l in want[b]["level"] for x in l]
        assert lv_g == lv_w, b
        lg, lw = got[b]["locations"].cpu().numpy() * 32, want[b]["locations"].numpy() * 32
        for lvl in set(lv_g):
            sel = np.array(lv_g) == lvl
            assert sorted(lg[sel].tolist()) == sorted(lw[sel].tolist()), (b, lvl)
        kept += sum(x >= 0 for x in lv_g)

        def rows(d):
            a = np.concatenate([d["detections"].cpu().numpy(), d["scores"].cpu().numpy()[:, None], d["locations"].cpu().numpy()[:, None]], 1)
            return a[np.lexsort((a[:, 0], a[:, 3]))]
        np.testing.assert_allclose(rows(got[b]), rows(want[b]), atol=2e-6, rtol=0)
    assert kept > 0


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_fp32_eval_parity_with_running_statistics(name, B, T, D, stage):
    """Eval forward of the exact-f32 HIP path vs the fp32 oracle on the same real running statistics: losses and every head output
    within 1e-4 of the tensor scale; the HIP post-processor's detections equal the oracle's FCOSPostProcessor on the HIP heads."""
    from drn_amd.model import mainModel
    from oracle import drn_oracle as O
    cfg = cfg_for(D, stage)
    sd = stats_state(B, T, D)
    batch = synthetic_batch(B, T, D, seed=3)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        _, lo, ho = forward(build(O.mainModel, cfg, sd), batch, "cpu")
        bh, lh, hh = forward(build(mainModel, cfg, sd, DEV), batch, DEV)
    check_outputs(lh, hh, lo, ho, 1e-4)
    cls, reg, iou = ([t.detach().float().cpu() for t in hh[j]] for j in (0, 1, 3))
    locs = [O.FCOSModule.locations_for(c.shape[-1], s, "cpu") for c, s in zip(cls, cfg["fpn_stride"])]
    check_detections(bh, O.FCOSPostProcessor(cfg)(locs, cls, reg, iou))


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_bf16_eval_with_running_statistics(name, B, T, D, stage):
    """bf16 eval forward vs the fp32 HIP eval forward on the same running statistics, at test_bf16_tolerance_sweep's tolerances."""
    from drn_amd.model import mainModel
    cfg = cfg_for(D, stage)
    sd = stats_state(B, T, D)
    batch = synthetic_batch(B, T, D, seed=3)
    with torch.no_grad():
        _, l32, h32 = forward(build(mainModel, cfg, sd, DEV), batch, DEV)
        _, l16, h16 = forward(build(mainModel, cfg, sd, DEV, compute_dtype=torch.bfloat16), batch, DEV)
    for k in ("loss_cls", "loss_reg"):
        a, b = float(l16[k]), float(l32[k])
        assert abs(a - b) <= 3e-2 * max(1.0, abs(b)), (k, a, b)
    for j in (0, 1, 3):
        for l in range(3):
            x, y = h16[j][l].float(), h32[j][l].float()
            if j == 1:
                # reg = exp(scale * bbox_pred): compared as the logit it exponentiates, like the other two heads.  (As exp, eval mode
                # with real statistics reaches values of 14 at D = 500, where bf16 rounding of the logit gives 0.89 > 6e-2 * 14.)
                x, y = x.log(), y.log()
            assert float((x - y).abs().max()) <= 6e-2 * max(1.0, float(y.abs().max())), (j, l)


# the benchmarked shape in both stages, and a tiny one: there the coarsest level has 16 rows per channel, so a biased variance in the
# running-variance update (a factor (M - 1) / M) moves running_var by ~0.6 %, far beyond the gate (at M >= 2048 it hides below 1e-4)
@pytest.mark.parametrize("B,T,D,stage", [(32, 256, 4096, 1), (32, 256, 4096, 3), (2, 32, 64, 3)])
def test_train_running_statistics_at_the_benchmarked_shape(B, T, D, stage):
    """One train-mode forward (default momentum 0.1, the library's default kernel selection: w4h / w4c and the one-launch conv -> BN
    on) from the real statistics: all 13 BatchNorms' running_mean / running_var -- both halves of the stacked towers, updated
    three times in level order -- within 1e-4 * max(1, |ref|) of the oracle's, the counters equal; bf16 within 3e-2 of each
    tensor's scale of the fp32 HIP run."""
    from drn_amd import functional as DF
    from drn_amd.model import mainModel
    from oracle import drn_oracle as O
    cfg = cfg_for(D, stage)
    sd = stats_state(B, T, D)
    batch = synthetic_batch(B, T, D, seed=3)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    states = []
    with torch.no_grad():
        for cls, dev, kw in ((O.mainModel, "cpu", {}), (mainModel, DEV, {}), (mainModel, DEV, {"compute_dtype": torch.bfloat16})):
            m = build(cls, cfg, sd, dev, **kw)
            forward(m, batch, dev, train=True)
            DF.flush_bn_counters()
            states.append({k: v.detach().cpu() for k, v in m.state_dict().items()})
            del m
    ref, h32, h16 = states
    n = 0
    for k, r in ref.items():
        if k.endswith("num_batches_tracked"):
            assert int(h32[k]) == int(r) > int(sd[k]), (k, int(h32[k]), int(r), int(sd[k]))
            assert int(h16[k]) == int(r), k
        elif k.endswith(("running_mean", "running_var")):
            assert not torch.equal(r, sd[k]), k
            r64, g64 = r.double(), h32[k].double()
            err = (g64 - r64).abs() / r64.abs().clamp(min=1.0)
            assert float(err.max()) <= 1e-4, (k, float(err.max()))
            d16 = float((h16[k].double() - g64).abs().max())
            assert d16 <= 3e-2 * max(1.0, float(g64.abs().max())), (k, d16)
            n += 1
    assert n == 2 * 13


# -- Trainer.evaluate between graph-replayed training steps -----------------------------------------------------------------------

def _eval_loader(n, B, T, D):
    """n batches in drn_amd.data.collate_data's 8-tuple format (what Trainer.evaluate iterates), the last one ragged."""
    out = []
    for i in range(n):
        nb = B - 1 if i == n - 1 else B
        tok, qlen, feats, pse, gt, nprops, nframes = synthetic_batch(nb, T, D, seed=40 + i)
        out.append((["v%d_%d" % (i, b) for b in range(nb)], pse, feats, gt, tok, qlen, nprops, nframes))
    return out


def _fresh_evaluate(stage, dtype, snap, loader, with_results):
    """What Trainer.evaluate returns for a model built from scratch and loaded with `snap`."""
    from drn_amd import trainer as T
    from test_trainer_gpu import hip_model
    m = hip_model(stage)
    m.set_compute_dtype(dtype)
    m.load_state_dict(snap)
    return T.Trainer(m, stage, lr=1e-4, clip_gradient=0.5).evaluate(loader, with_results=with_results)


def _assert_same_evaluation(got, want):
    loss, topks, accs, results = got
    assert loss == want[0] and topks == want[1] and accs == want[2], (got[:3], want[:3])
    assert (results is None) == (want[3] is None)
    if results is not None:
        assert results == want[3]                          # every record: query, gt, node / edge predictions, levels


@pytest.mark.parametrize("forked", [False, True])
@pytest.mark.parametrize("dtype,stage", [(torch.bfloat16, 1), (torch.float32, 3)])
def test_evaluate_between_graph_replayed_steps(dtype, stage, forked):
    """Trainer(graph=True): steps (captured and replayed) -> evaluate(with_results=False) and evaluate() -> more steps (the captures
    re-established) -> evaluate again.  Each evaluation equals, bit for bit, that of a fresh model loaded from a state_dict snapshot
    taken at that point (the re-laid weight copies the captured optimizer keeps are current); no evaluation changes the state_dict;
    the losses and the final state_dict equal those of the same run without evaluations."""
    from drn_amd import functional as DF
    from drn_amd import trainer as T
    from test_trainer_gpu import _varying_batches, hip_model
    B, Tp, D = 4, 32, 64
    batches = _varying_batches(4, B, Tp, D)[:3]                 # query lengths 3, 5, 7: two geometries (Lq 4 and 8), four clips each
    loader = _eval_loader(2, B, Tp, D)
    # each geometry is captured and replayed before each evaluation (forked: one more eager step before its capture; after an
    # evaluation the captures are re-established)
    phases = [[0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 0], [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 0]]
    runs = []
    for with_eval in (True, False):
        m = hip_model(stage)
        m.set_compute_dtype(dtype)
        tr = T.Trainer(m, stage, lr=1e-4 if stage == 1 else 1.0, clip_gradient=0.5, graph=True, lq_bucket=4, forked=forked)
        losses = []
        for phase in phases:
            for i in phase:
                ld = tr.train_step(batches[i])
                losses.append([float(ld[k].detach().reshape(-1)[0]) for k in ("loss_cls", "loss_reg", "loss_iou")])
            torch.cuda.synchronize()
            assert sum(s.graph is not None for s in tr._slots.values()) == 2, "a geometry was never replayed"
            if not with_eval:
                continue
            snap = state_snapshot(m)
            for with_results in (False, True):
                got = tr.evaluate(loader, with_results=with_results)
                assert_state_equal(snap, state_snapshot(m), "evaluate(with_results=%s)" % with_results)
                _assert_same_evaluation(got, _fresh_evaluate(stage, dtype, snap, loader, with_results))
        torch.cuda.synchronize()
        DF.flush_bn_counters()
        runs.append((losses, state_snapshot(m)))
    (l0, s0), (l1, s1) = runs
    assert np.array_equal(np.array(l0), np.array(l1)), (l0, l1)
    assert_state_equal(s1, s0, "the run with evaluations")
