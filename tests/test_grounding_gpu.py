"""Grounding without a ground truth on the device (drn_amd.grounding): drn_select_moments against the reference evaluator's recorded
picks and against the host evaluator on real eval candidates, its agreement with drn_eval_recall, drn_gate_gather_fwd against
drn_gate_fwd, mainModel.forward_heads_shared / Grounder against the CPU oracle and the model's own eval forward at the BASELINE.json
shapes (real BatchNorm running statistics: test_eval_gpu.stats_state), shared videos, and what the new paths must leave alone."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict, synthetic_batch
from helpers import assert_state_equal, state_snapshot
from test_configs_gpu import SHAPES, check_outputs
from test_eval_gpu import build, cfg_for, check_detections, stats_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "moments.json")))
OVERLAPS = (0.25, 0.45, 0.65)


def host_picks(det, scores, n, k, overlap):
    """metrics.select_moments (pinned to the reference by tests/test_grounding_cpu.py) on one clip's device buffers copied back."""
    from drn_amd.metrics import select_moments
    preds = np.concatenate([det[:n].astype(np.float64), scores[:n, None].astype(np.float64)], axis=1).tolist()
    return select_moments(preds, k, overlap)


def level_of(counts_b, j):
    return int(np.searchsorted(np.cumsum(counts_b), j, side="right"))


def check_moments(got, det, scores, counts, k, overlap):
    """Every field of ops.select_moments' result, clip by clip, against the host twin: index / n exact, seg / score the bits of the
    candidates, level from the counts, padding 0 / -1; the fallback moment for a clip without candidates.
    -> clips in which the NMS suppressed something."""
    seg, score, level, index, n = (t.cpu().numpy() for t in got)
    assert seg.dtype == np.float32 and score.dtype == np.float32 and level.dtype == index.dtype == n.dtype == np.int32
    suppressed = 0
    for b in range(det.shape[0]):
        nb = int(counts[b].sum())
        if nb == 0:
            assert int(n[b]) == 1 and seg[b, 0].tolist() == [0.0, 1.0] and float(score[b, 0]) == 1.0, b
            assert int(level[b, 0]) == -1 and int(index[b, 0]) == -1, b
            want = [None]
        else:
            want = host_picks(det[b], scores[b], nb, k, overlap)
            assert int(n[b]) == len(want), (b, int(n[b]), len(want))
            assert index[b, :len(want)].tolist() == want, (b, index[b, :len(want)].tolist(), want)
            assert seg[b, :len(want)].tobytes() == det[b][want].tobytes(), b
            assert score[b, :len(want)].tobytes() == scores[b][want].tobytes(), b
            assert level[b, :len(want)].tolist() == [level_of(counts[b], j) for j in want], b
            suppressed += len(host_picks(det[b], scores[b], nb, nb, overlap)) < nb
        m = len(want)
        assert not seg[b, m:].any() and not score[b, m:].any() and (level[b, m:] == -1).all() and (index[b, m:] == -1).all(), b
    return suppressed


# -- 1. drn_select_moments ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", GOLD["ks"])
@pytest.mark.parametrize("overlap", GOLD["overlaps"])
def test_select_moments_equals_the_reference_picks(overlap, k):
    """The recorded cases of one (overlap, k) pair as the clips of one launch, each clip's candidates dealt onto three levels."""
    from drn_amd import ops
    cases = [c for c in GOLD["cases"] if c["overlap"] == overlap and c["k"] == k]
    assert len(cases) >= 20
    B, R = len(cases), max(len(c["preds"]) for c in cases) + 3
    det, scores = np.full((B, R, 2), 0.5, dtype=np.float32), np.full((B, R), 2.0, dtype=np.float32)      # (slots past n: never read)
    counts = np.zeros((B, 3), dtype=np.int32)
    for b, c in enumerate(cases):
        p = np.asarray(c["preds"], dtype=np.float32)
        nb = len(p)
        det[b, :nb], scores[b, :nb] = p[:, :2], p[:, 2]
        counts[b] = [nb // 3, nb // 4, nb - nb // 3 - nb // 4]
    got = ops.select_moments(torch.from_numpy(det).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(counts).to(DEV), overlap, k)
    index, n = got[3].cpu().numpy(), got[4].cpu().numpy()
    for b, c in enumerate(cases):
        assert int(n[b]) == len(c["picks"]) and index[b, :int(n[b])].tolist() == c["picks"], (c["tag"], index[b].tolist(), c["picks"])
    check_moments(got, det, scores, counts, k, overlap)


def test_select_moments_fallback_for_clips_without_candidates():
    from drn_amd import ops
    det = torch.rand(3, 40, 2).sort(dim=2)[0]
    scores = torch.rand(3, 40)
    counts = torch.tensor([[0, 0, 0], [3, 0, 2], [0, 0, 0]], dtype=torch.int32)
    got = ops.select_moments(det.to(DEV), scores.to(DEV), counts.to(DEV), 0.45, 7)
    check_moments(got, det.numpy(), scores.numpy(), counts.numpy(), 7, 0.45)
    assert got[4].tolist()[0] == 1 and got[4].tolist()[2] == 1 and got[0].shape == (3, 7, 2)
    with pytest.raises(Exception):
        ops.select_moments(det.to(DEV), scores.to(DEV), counts.to(DEV), 0.45, 0)


@functools.lru_cache(maxsize=4)
def eval_run(name, B, T, D, stage):
    """One fp32 eval forward of the HIP model on the real running statistics: the model, the device batch, the model's own records
    (host copies), its head outputs and the post-processor's device buffers."""
    from drn_amd.model import mainModel
    cfg = cfg_for(D, stage)
    m = build(mainModel, cfg, stats_state(B, T, D), DEV).eval()
    batch = [x.to(DEV) for x in synthetic_batch(B, T, D, seed=3)]
    sel = m.fcos.box_selector_test
    with torch.no_grad():
        m.taps = {}
        boxes, _ = m(*batch)
        heads = m.taps["head"]
        m.taps = None
        sel.device_only = True
        try:
            dd, _ = m(*batch)
        finally:
            sel.device_only = False
    torch.cuda.synchronize()
    boxes = [{k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()} for b in boxes]
    return m, cfg, batch, boxes, heads, dd


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_select_moments_on_eval_candidates(name, B, T, D, stage):
    """drn_postprocess's real output at the configuration shapes -> ops.select_moments == the host evaluator, exactly; in at least
    one clip the NMS has something to suppress."""
    from drn_amd import ops
    _, _, _, _, _, dd = eval_run(name, B, T, D, stage)
    det, scores, counts = dd.det.cpu().numpy(), dd.scores.cpu().numpy(), dd.counts.cpu().numpy()
    suppressed = {}
    for overlap in OVERLAPS:
        for k in (5, 100):
            got = ops.select_moments(dd.det, dd.scores, dd.counts, overlap, k)
            suppressed[overlap] = check_moments(got, det, scores, counts, k, overlap)
    print("%s: candidates per clip %d..%d, clips with a suppressed candidate %s" %
          (name, counts.sum(1).min(), counts.sum(1).max(), suppressed))
    assert all(v >= 1 for v in suppressed.values()), suppressed


# -- 2. the existing recall kernel ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_first_hit_among_the_selected_moments_is_eval_recalls(name, B, T, D, stage):
    from drn_amd import ops
    _, _, batch, _, _, dd = eval_run(name, B, T, D, stage)
    K, ious = 5, [0.3, 0.5, 0.7]
    gt = batch[4].contiguous()
    fh = ops.eval_recall(dd.det, dd.scores, dd.counts, gt, torch.tensor(ious, dtype=torch.float64, device=DEV), K).cpu().numpy()
    g = gt.double().cpu().numpy()
    for q, iou in enumerate(ious):
        seg, _, _, _, n = (t.cpu().numpy() for t in ops.select_moments(dd.det, dd.scores, dd.counts, iou - 0.05, K))
        for b in range(B):
            want = K
            for p in range(int(n[b])):
                x1, x2 = float(seg[b, p, 0]), float(seg[b, p, 1])
                if (min(g[b, 1], x2) - max(g[b, 0], x1)) / (max(g[b, 1], x2) - min(g[b, 0], x1)) >= iou:      # un-clamped
                    want = p
                    break
            assert int(fh[b, q]) == want, (b, iou, int(fh[b, q]), want)


# -- 3. drn_gate_gather_fwd ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gate_gather_with_the_identity_index_is_gate_fwd(dtype):
    from drn_amd import ops
    code = ops.F32 if dtype == torch.float32 else ops.BF16
    g = torch.Generator().manual_seed(0)
    for Q, L, C, P, ld_out in ((5, 7, 64, 0, 64), (3, 33, 128, 0, 200), (4, 16, 64, 32, 96), (2, 6, 512, 256, 776)):
        z = torch.randn(Q, L, C, generator=g).to(DEV, dtype)
        gate = torch.randn(Q, C, generator=g).to(DEV)
        pos = torch.randn(Q * L, P, generator=g).to(DEV, dtype) if P else None
        want = torch.full((Q * L, ld_out), 7.0, dtype=dtype, device=DEV)
        got = want.clone()
        ops.gate_fwd(z, C, gate, want, ld_out, Q, L, C, code)
        vid = torch.arange(Q, dtype=torch.int32, device=DEV)
        ops.gate_gather_fwd(z, C, gate, pos, P, vid, Q, got, ld_out, Q, L, C, P, code, vid_host=vid.cpu())
        assert torch.equal(got[:, :C], want[:, :C]), (Q, L, C)
        if P:
            assert torch.equal(got[:, C:C + P], pos)
        assert bool((got[:, C + P:] == 7.0).all())                       # columns past C + P are not the kernel's


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gate_gather_with_permuted_and_repeated_indices(dtype):
    from drn_amd import _lib, ops
    code = ops.F32 if dtype == torch.float32 else ops.BF16
    g = torch.Generator().manual_seed(1)
    V, L, C, P = 4, 19, 128, 64
    z = torch.randn(V, L, C, generator=g).to(DEV, dtype)
    buf = torch.randn(V * L, C + P, generator=g).to(DEV, dtype)          # the position columns live in a wider buffer, as in the model
    pos = buf[:, C:]
    for index in ([3, 1, 0, 2], [2, 2, 0, 3, 0, 2, 1, 1, 3], [1]):
        Q = len(index)
        vid = torch.tensor(index, dtype=torch.int32, device=DEV)
        gate = torch.randn(Q, C, generator=g).to(DEV)
        got = torch.empty((Q * L, C + P), dtype=dtype, device=DEV)
        ops.gate_gather_fwd(z, C, gate, pos, C + P, vid, V, got, C + P, Q, L, C, P, code)
        zz = z.index_select(0, vid.long()).contiguous()
        want = torch.empty((Q * L, C), dtype=dtype, device=DEV)
        ops.gate_fwd(zz, C, gate, want, C, Q, L, C, code)
        assert torch.equal(got[:, :C], want), index
        assert torch.equal(got[:, C:].view(Q, L, P), pos.reshape(V, L, P).index_select(0, vid.long())), index
    # an index outside [0, V): refused when the host copy is there, zeros for that query's rows when it is not
    vid = torch.tensor([0, 4, -1, 3], dtype=torch.int32, device=DEV)
    gate = torch.randn(4, C, generator=g).to(DEV)
    got = torch.full((4 * L, C + P), 3.0, dtype=dtype, device=DEV)
    with pytest.raises(_lib.DrnError):
        ops.gate_gather_fwd(z, C, gate, pos, C + P, vid, V, got, C + P, 4, L, C, P, code, vid_host=vid.cpu())
    assert bool((got == 3.0).all())
    ops.gate_gather_fwd(z, C, gate, pos, C + P, vid, V, got, C + P, 4, L, C, P, code)
    got = got.view(4, L, C + P)
    assert not bool(got[1].any()) and not bool(got[2].any()) and bool(got[0].any()) and bool(got[3].any())


# -- 4. / 5. Grounder against the oracle, the model's own eval forward, and fp32 ------------------------------------------------------

def ground_with_heads(m, batch, video_index=None, top_k=5, overlap=0.45):
    """Grounder.ground with the head outputs caught; the model's state must come out untouched."""
    from drn_amd import Grounder
    before = state_snapshot(m)
    m.taps = {}
    try:
        mom = Grounder(m, top_k=top_k, nms_overlap=overlap).ground(batch[0], batch[1], batch[2], batch[3], video_index)
        heads = m.taps["head"]
    finally:
        m.taps = None
    torch.cuda.synchronize()
    assert_state_equal(before, state_snapshot(m), "Grounder.ground")
    assert m.fcos.box_selector_test.device_only is False
    return mom, heads


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_fp32_grounder_against_the_oracle_and_the_eval_forward(name, B, T, D, stage):
    """Identity index: the head outputs of forward_heads_shared within 1e-4 of the CPU oracle's (check_outputs, the eval-parity gate);
    the post-processor's candidates on them against those of the model's own eval forward (check_detections: same kept set per level,
    values within 2e-6); the moments are the host evaluator's picks on those candidates."""
    from oracle import drn_oracle as O
    from test_eval_gpu import forward
    m, cfg, batch, boxes, _, _ = eval_run(name, B, T, D, stage)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    with torch.no_grad():
        _, lo, ho = forward(build(O.mainModel, cfg, stats_state(B, T, D)), synthetic_batch(B, T, D, seed=3), "cpu")
    mom, hh = ground_with_heads(m, batch)
    check_outputs(lo, hh, lo, ho, 1e-4)                    # (no losses on this path: the oracle's own stand in, the heads are compared)
    with torch.no_grad():
        locations, box_cls, box_reg, iou_scores = m.forward_heads_shared(*batch[:4])
        got = m.fcos.box_selector_test(locations, box_cls, box_reg, iou_scores)
    check_detections(got, boxes)
    lists = mom.tolist()
    assert len(lists) == B and mom.seg.shape == (B, 5, 2)
    for b in range(B):
        d, s = got[b]["detections"].cpu().numpy(), got[b]["scores"].cpu().numpy()
        want = host_picks(d, s, len(s), 5, 0.45)
        assert [x[:2] for x in lists[b]] == d[want].astype(np.float64).tolist(), b
        assert [x[2] for x in lists[b]] == s[want].astype(np.float64).tolist(), b


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_bf16_grounder_against_fp32(name, B, T, D, stage):
    """test_bf16_eval_with_running_statistics's rule on the heads of the two Grounders: 6e-2 of the tensor scale, reg as its log.
    D = 500 runs the shared front on the zero-padded width."""
    from drn_amd.model import mainModel
    m32, cfg, batch, _, _, _ = eval_run(name, B, T, D, stage)
    _, h32 = ground_with_heads(m32, batch)
    m16 = build(mainModel, cfg, stats_state(B, T, D), DEV, compute_dtype=torch.bfloat16).eval()
    mom, h16 = ground_with_heads(m16, batch)
    for j in (0, 1, 3):
        for l in range(3):
            x, y = h16[j][l].float(), h32[j][l].float()
            if j == 1:
                x, y = x.log(), y.log()
            assert float((x - y).abs().max()) <= 6e-2 * max(1.0, float(y.abs().max())), (j, l)
    n = mom.n.cpu().numpy()
    assert (n >= 1).all() and (n <= 5).all()


# -- 6. shared videos ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,D,dtype", [(32, 64, torch.float32), (256, 1024, torch.float32), (256, 1024, torch.bfloat16),
                                       (64, 500, torch.bfloat16)])
def test_shared_videos_equal_the_gathered_batch(T, D, dtype):
    """V = 3 videos, Q = 8 queries with a repeating, unsorted index, against the same Grounder on the videos gathered per query with
    the identity index.  The only launch whose shape differs is prop_fc (V * T rows against Q * T): where the library picks the
    same kernel kind for both, every Moments field is bit-identical; otherwise (fp32) the heads agree within 1e-4 of their scale.
    (The shapes stay below the K-loop split of few-tile products -- ops._ksplit: bf16 from K = 1536, fp32 from K = 3072 -- which
    sums in another order at another row count whatever the kernel kind.)"""
    from drn_amd import functional as DF
    from drn_amd import ops
    from drn_amd.model import mainModel
    V, Q, stage = 3, 8, 3
    cfg = default_cfg("C3D" if D == 4096 else "TINY" if D == 64 else "SYN", D, stage)
    m = mainModel(VOCAB_SIZE, as_namespace(cfg), compute_dtype=dtype)
    m.load_state_dict(stats_state(2, 32, 64) if D == 64 else seeded_state_dict(m, 0))
    m = m.to(DEV).eval()
    tok, qlen, _, _, _, _, _ = synthetic_batch(Q, T, D, seed=7)
    _, _, feats, pse, _, _, _ = synthetic_batch(V, T, D, seed=8)
    vid = torch.tensor([2, 0, 2, 1, 1, 0, 2, 0])
    tok, qlen, feats, pse = tok.to(DEV), qlen.to(DEV), feats.to(DEV), pse.to(DEV)
    shared, hs = ground_with_heads(m, (tok, qlen, feats, pse), vid)
    full, hf = ground_with_heads(m, (tok, qlen, feats.index_select(0, vid.to(DEV)), pse.index_select(0, vid.to(DEV))))
    Dp = D + m._front_pad(D)
    code = ops.F32 if dtype == torch.float32 else ops.BF16
    x = torch.empty(64, dtype=dtype, device=DEV)
    kinds = [DF._fc_kernel_kind(n, T, Dp, Dp, x, x, code, True) for n in (V, Q)]
    descs = [ops.gemm_desc(x, x, x, n * T, Dp, Dp, Lout=T) for n in (V, Q)]
    assert ops._ksplit(descs[:1], code) == ops._ksplit(descs[1:], code) == 1
    print("prop_fc kernel kinds at %d / %d rows: %s" % (V * T, Q * T, kinds))
    if (T, D) == (32, 64):
        assert kinds[0] == kinds[1] == ops.NT_KIND_TILE128, kinds
    if kinds[0] == kinds[1]:
        for f in ("seg", "score", "level", "index", "n"):
            assert torch.equal(getattr(shared, f), getattr(full, f)), f
        for j in (0, 1, 3):
            for a, b in zip(hs[j], hf[j]):
                assert torch.equal(a, b), j
    else:
        assert dtype == torch.float32, "bf16 shapes of this test are chosen so that both row counts run on the same kernel"
        for j in (0, 1, 3):
            for a, b in zip(hs[j], hf[j]):
                assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), j
    assert int(shared.n.min()) >= 1


# -- 7. hygiene ---------------------------------------------------------------------------------------------------------------------

def test_inference_only_and_no_cpu_fallback():
    from drn_amd import Grounder, _lib
    from drn_amd.model import mainModel
    m = build(mainModel, default_cfg("TINY", 64, 3), stats_state(2, 32, 64), DEV)
    sel = m.fcos.box_selector_test
    host = synthetic_batch(2, 32, 64, seed=3)
    batch = [x.to(DEV) for x in host]
    m.train()
    before = state_snapshot(m)
    with pytest.raises(_lib.DrnError):
        Grounder(m).ground(*batch[:4])
    with torch.no_grad(), pytest.raises(_lib.DrnError):
        m.forward_heads_shared(*batch[:4])
    m.eval()
    with pytest.raises(_lib.DrnError):                       # grad enabled
        m.forward_heads_shared(*batch[:4])
    with pytest.raises(_lib.DrnError):                       # CPU tensors
        Grounder(m).ground(*host[:4])
    with pytest.raises(_lib.DrnError):                       # two queries, one video, no index
        Grounder(m).ground(batch[0], batch[1], batch[2][:1], batch[3][:1])
    with pytest.raises(_lib.DrnError):                       # a host index outside [0, V): refused before the launch
        Grounder(m).ground(batch[0], batch[1], batch[2], batch[3], torch.tensor([0, 2]))
    assert sel.device_only is False
    assert_state_equal(before, state_snapshot(m), "refused calls")
    m3 = mainModel(VOCAB_SIZE, as_namespace(dict(default_cfg("TINY", 64, 3), fcos_num_class=3))).to(DEV).eval()
    with pytest.raises(_lib.DrnError, match="foreground channel"):
        Grounder(m3).ground(*batch[:4])
    assert m3.fcos.box_selector_test.device_only is False


def test_device_only_is_restored_after_an_exception(monkeypatch):
    from drn_amd import Grounder
    from drn_amd.model import mainModel
    m = build(mainModel, default_cfg("TINY", 64, 3), stats_state(2, 32, 64), DEV).eval()
    batch = [x.to(DEV) for x in synthetic_batch(2, 32, 64, seed=3)]

    def boom(*a, **k):
        assert m.fcos.box_selector_test.device_only is True
        raise ZeroDivisionError("inside the forward")
    monkeypatch.setattr(m, "forward_heads_shared", boom)
    with pytest.raises(ZeroDivisionError):
        Grounder(m).ground(*batch[:4])
    assert m.fcos.box_selector_test.device_only is False


def _mini_loader(stage):
    from torch.utils.data import DataLoader
    from drn_amd.data import CharadesSTA, collate_data
    cfg = default_cfg("TINY", 12, stage)
    cfg["feature_type"] = "C3D"
    cfg["C3D"] = {"feature_root": "./features", "feature_dim": 12, "ft_window_size": 16, "ft_overlap": 0.5}
    cfg["props_file_path"] = "./data/dataset/Charades/mini_props.txt"
    ds = CharadesSTA(cfg, "test", os.path.join(HERE, "golden", "charades_mini"), lambda s: s.split())
    return cfg, ds, list(DataLoader(ds, batch_size=4, shuffle=False, collate_fn=collate_data))


@pytest.mark.parametrize("share_videos", [True, False])
def test_trainer_predict_on_the_mini_dataset(share_videos):
    """Trainer.predict: one entry per query; its moments are metrics.select_moments applied to Trainer.evaluate(with_results=True)'s
    records (fp32: values within 2e-6, the same picks); the model comes back as it was."""
    from drn_amd import trainer as TR
    from drn_amd.metrics import select_moments
    from test_trainer_gpu import hip_model
    cfg, ds, loader = _mini_loader(3)
    m = hip_model(3, cfg=cfg)
    with torch.no_grad():                                    # (a classifier that passes most locations: the NMS has work to do)
        m.fcos.head.cls_logits.bias.fill_(0.5)
        m.fcos.head.cls_logits.weight.mul_(30.0)
    m.train()
    tr = TR.Trainer(m, 3, lr=1e-3)
    before = state_snapshot(m)
    pred = tr.predict(loader, top_k=5, nms_overlap=0.45, share_videos=share_videos)
    assert m.training
    assert_state_equal(before, state_snapshot(m), "Trainer.predict")
    _, _, _, records = tr.evaluate(loader)
    assert sum(len(v) for v in pred.values()) == len(ds) == sum(len(v) for v in records.values())
    assert set(pred) == set(records)
    suppressed = 0
    for video, items in records.items():
        assert len(pred[video]) == len(items)
        for rec, got in zip(items, pred[video]):
            assert got["query"] == rec["query"]
            preds = rec["node_predictions"]
            picks = select_moments(preds, 5, 0.45)
            suppressed += len(select_moments(preds, len(preds), 0.45)) < len(preds)
            assert len(got["moments"]) == len(picks), (video, got["moments"], picks)
            np.testing.assert_allclose(np.asarray(got["moments"]), np.asarray([preds[i] for i in picks]), atol=2e-6, rtol=0)
    assert suppressed > 0
