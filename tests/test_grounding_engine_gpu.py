"""Grounder(fused=..., graph=...) through the public interface: the one-launch eval conv blocks against the separate launches (fp32:
bit for bit), bf16 by the rule of test_bf16_grounder_against_fp32, hipGraph replay against the eager Grounder of the same setting
(bit for bit, one capture per signature, results that are copies), shared videos, weights changed after a capture, max_graphs, the
refusals, and Trainer.predict with both options."""
import numpy as np
import pytest
import torch

from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict, synthetic_batch
from test_grounding_gpu import (DEV, SHAPES, _mini_loader, assert_state_equal, build, eval_run, ground_with_heads, state_snapshot,
                                stats_state)

pytestmark = pytest.mark.gpu
FIELDS = ("seg", "score", "level", "index", "n")


def fused_with_heads(m, batch, video_index=None):
    """ground_with_heads under Grounder(fused=True): (moments, heads, conv_bn_eval launches that ran)."""
    from drn_amd import Grounder, ops
    before, n0 = state_snapshot(m), ops.conv_bn_eval_launches
    m.taps = {}
    try:
        mom = Grounder(m, fused=True).ground(batch[0], batch[1], batch[2], batch[3], video_index)
        heads = m.taps["head"]
    finally:
        m.taps = None
    torch.cuda.synchronize()
    assert_state_equal(before, state_snapshot(m), "Grounder(fused=True).ground")
    return mom, heads, ops.conv_bn_eval_launches - n0


def same_moments(a, b, what=""):
    for f in FIELDS:
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_fp32_fused_equals_the_separate_launches(name, B, T, D, stage):
    m, _, batch, _, _, _ = eval_run(name, B, T, D, stage)
    ref, h0 = ground_with_heads(m, batch)
    mom, h1, launches = fused_with_heads(m, batch)
    assert launches > 0
    for j in (0, 1, 3):
        for l, (a, b) in enumerate(zip(h1[j], h0[j])):
            assert torch.equal(a, b), (j, l)
    same_moments(mom, ref)


@pytest.mark.parametrize("name,B,T,D,stage", SHAPES)
def test_bf16_fused_against_fp32(name, B, T, D, stage):
    from drn_amd.model import mainModel
    m32, cfg, batch, _, _, _ = eval_run(name, B, T, D, stage)
    _, h32 = ground_with_heads(m32, batch)
    m16 = build(mainModel, cfg, stats_state(B, T, D), DEV, compute_dtype=torch.bfloat16).eval()
    mom, h16, launches = fused_with_heads(m16, batch)
    assert launches > 0
    for j in (0, 1, 3):
        for l in range(3):
            x, y = h16[j][l].float(), h32[j][l].float()
            if j == 1:
                x, y = x.log(), y.log()
            assert float((x - y).abs().max()) <= 6e-2 * max(1.0, float(y.abs().max())), (j, l)
    n = mom.n.cpu().numpy()
    assert (n >= 1).all() and (n <= 5).all()


def tiny_model(T, D, dtype):
    from drn_amd.model import mainModel
    cfg = default_cfg("TINY" if D == 64 else "SYN", D, 3)
    m = mainModel(VOCAB_SIZE, as_namespace(cfg), compute_dtype=dtype)
    m.load_state_dict(stats_state(2, 32, 64) if D == 64 else seeded_state_dict(m, 0))
    return m.to(DEV).eval()


def dev_batch(B, T, D, seed):
    """The first four inputs on the device, the tokens zero-padded to the longest query synthetic_batch makes (8): batches of one
    shape are batches of one signature."""
    tok, qlen, feats, pse = synthetic_batch(B, T, D, seed=seed)[:4]
    tok = torch.nn.functional.pad(tok, (0, 8 - tok.shape[1]))
    return [x.to(DEV) for x in (tok, qlen, feats, pse)]


@pytest.mark.parametrize("T,D,dtype,fused", [(32, 64, torch.float32, False), (32, 64, torch.float32, True), (32, 64, torch.bfloat16, False),
                                             (256, 1024, torch.float32, False), (256, 1024, torch.bfloat16, False)])
def test_graph_replay_equals_the_eager_grounder(T, D, dtype, fused):
    from drn_amd import Grounder
    m = tiny_model(T, D, dtype)
    eager, graphed = Grounder(m, fused=fused), Grounder(m, fused=fused, graph=True)
    before = state_snapshot(m)
    kept = []
    for seed in (3, 4, 5):
        batch = dev_batch(2, T, D, seed)
        got, want = graphed.ground(*batch), eager.ground(*batch)
        same_moments(got, want, seed)
        kept.append((got, [getattr(got, f).clone() for f in FIELDS]))
    assert graphed.captures == 1
    for got, copies in kept:                                 # results are copies: a later replay did not change an earlier one
        for f, c in zip(FIELDS, copies):
            assert torch.equal(getattr(got, f), c), f
    sig = Grounder.signature(*batch)
    static = graphed.static_inputs(sig)
    assert static is not None and static[4] is None and graphed.static_inputs(("nothing",)) is None
    for dst, src in zip(static[:4], dev_batch(2, T, D, 6)):
        dst.copy_(src)
    same_moments(graphed.ground(*static[:4]), eager.ground(*dev_batch(2, T, D, 6)), "static inputs")
    assert graphed.captures == 1
    assert_state_equal(before, state_snapshot(m), "graph replay")


def test_shared_videos_under_the_graph():
    from drn_amd import Grounder, _lib
    T, D, V, Q = 32, 64, 3, 8
    m = tiny_model(T, D, torch.float32)
    tok, qlen, _, _ = dev_batch(Q, T, D, 7)
    _, _, feats, pse = dev_batch(V, T, D, 8)
    eager, graphed = Grounder(m), Grounder(m, graph=True)
    for vid in (torch.tensor([2, 0, 2, 1, 1, 0, 2, 0]), torch.tensor([0, 1, 2, 2, 1, 0, 0, 1])):
        same_moments(graphed.ground(tok, qlen, feats, pse, vid), eager.ground(tok, qlen, feats, pse, vid), vid.tolist())
    assert graphed.captures == 1
    with pytest.raises(_lib.DrnError):
        graphed.ground(tok, qlen, feats, pse, torch.tensor([2, 0, 2, 1, 3, 0, 2, 0]))
    assert graphed.captures == 1
    same_moments(graphed.ground(tok, qlen, feats, pse, vid), eager.ground(tok, qlen, feats, pse, vid), "after the refusal")


def test_weights_changed_after_capture():
    from drn_amd import Grounder
    T, D = 32, 64
    m = tiny_model(T, D, torch.float32)
    batch = dev_batch(2, T, D, 3)
    eager, graphed = Grounder(m), Grounder(m, graph=True)
    same_moments(graphed.ground(*batch), eager.ground(*batch))
    state = seeded_state_dict(m, 5)
    m.load_state_dict(state)
    same_moments(graphed.ground(*batch), eager.ground(*batch), "new weights")
    assert graphed.captures == 2
    with torch.no_grad():                                    # running statistics changed in place: re-read at every replay
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.mul_(0.5).add_(0.01)
                mod.running_var.mul_(1.5)
    same_moments(graphed.ground(*batch), eager.ground(*batch), "new running statistics")
    assert graphed.captures == 2


def test_max_graphs_runs_further_signatures_eagerly():
    from drn_amd import Grounder
    T, D = 32, 64
    m = tiny_model(T, D, torch.float32)
    eager, graphed = Grounder(m), Grounder(m, graph=True, max_graphs=1)
    b2, b3 = dev_batch(2, T, D, 3), dev_batch(3, T, D, 4)
    same_moments(graphed.ground(*b2), eager.ground(*b2))
    same_moments(graphed.ground(*b3), eager.ground(*b3), "second signature")
    assert graphed.captures == 1 and graphed.static_inputs(Grounder.signature(*b3)) is None
    b2 = dev_batch(2, T, D, 9)
    same_moments(graphed.ground(*b2), eager.ground(*b2), "first signature again")
    assert graphed.captures == 1


def test_refusals_are_todays():
    from drn_amd import Grounder, _lib
    m = tiny_model(32, 64, torch.float32)
    host = synthetic_batch(2, 32, 64, seed=3)[:4]
    g = Grounder(m, fused=True, graph=True)
    with pytest.raises(_lib.DrnError):
        g.ground(*host)
    m.train()
    with pytest.raises(_lib.DrnError):
        g.ground(*[x.to(DEV) for x in host])
    assert g.captures == 0 and m.fcos.box_selector_test.device_only is False


def test_trainer_predict_with_both_options():
    from drn_amd import trainer as TR
    from test_trainer_gpu import hip_model
    cfg, ds, loader = _mini_loader(3)
    m = hip_model(3, cfg=cfg)
    with torch.no_grad():
        m.fcos.head.cls_logits.bias.fill_(0.5)
        m.fcos.head.cls_logits.weight.mul_(30.0)
    tr = TR.Trainer(m, 3, lr=1e-3)
    before = state_snapshot(m)
    want = tr.predict(loader, top_k=5, nms_overlap=0.45)
    got = tr.predict(loader, top_k=5, nms_overlap=0.45, fused=True, graph=True)
    assert_state_equal(before, state_snapshot(m), "Trainer.predict")
    assert set(got) == set(want)
    for video in want:
        assert len(got[video]) == len(want[video])
        for a, b in zip(got[video], want[video]):
            assert a["query"] == b["query"] and len(a["moments"]) == len(b["moments"])
            np.testing.assert_allclose(np.asarray(a["moments"]), np.asarray(b["moments"]), atol=2e-6, rtol=0)
