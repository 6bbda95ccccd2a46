"""Shared test helpers: golden loading + comparison of a model run against a golden fixture."""
import os

import numpy as np
import torch

from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict, synthetic_batch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TAPS = ["prop_fc", "backbone_net.forward_conv0", "backbone_net.forward_conv1", "backbone_net.forward_conv2",
        "fpn.fpn_layer1", "fpn.fpn_layer2", "fpn.fpn_layer3"]

# gradients that are analytically zero (pure rounding noise)
ZERO_GRADS = ("fcos.head.cls_tower.0.bias", "fcos.head.bbox_tower.0.bias", "fcos.head.mix_fc.0.bias",
              "fcos.head.iou_scores.0.bias", "query_encoder.cmd_inter2logits.bias")


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))


def case_inputs(g, device="cpu"):
    B, T, D, stage = int(g["B"]), int(g["T"]), int(g["D"]), int(g["stage"])
    cfg = default_cfg("C3D" if D == 4096 else "TINY", D, stage)
    if "num_class" in g:                                   # (the cases recorded with more than one foreground channel)
        cfg["fcos_num_class"] = int(g["num_class"])
    batch = list(synthetic_batch(B, T, D, seed=1, device=device))
    batch[4] = torch.from_numpy(g["gt"]).to(device)
    return cfg, batch


def build_model(model_cls, cfg, device="cpu", **kw):
    m = model_cls(VOCAB_SIZE, as_namespace(cfg), **kw)
    m.load_state_dict(seeded_state_dict(m, 0))
    return m.to(device)


def checksum(t):
    flat = t.detach().double().reshape(-1).cpu()
    step = max(1, flat.numel() // 64)
    return np.array([flat.sum().item(), flat.abs().sum().item()]), flat[::step][:64].float().numpy()


def load_running_stats(m, g):
    """The golden's recorded BatchNorm running statistics (rs/<key>, the *_eval_rs cases) into `m`, through load_state_dict so
    buffers that are views (the HIP head's stacked tower statistics) keep their storage.  False when the golden has none."""
    rs = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("rs/")}
    if not rs:
        return False
    sd = m.state_dict()
    assert set(rs) <= set(sd), sorted(set(rs) - set(sd))
    sd.update(rs)
    m.load_state_dict(sd)
    return True


def state_snapshot(m):
    """Every parameter and buffer of `m`, cloned to the host (pending BatchNorm counter bumps of the HIP path applied first)."""
    from drn_amd import functional as DF
    DF.flush_bn_counters()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def assert_state_equal(before, after, what="state"):
    assert set(before) == set(after)
    moved = [k for k in before if not torch.equal(before[k], after[k])]
    assert not moved, "%s changed: %s" % (what, moved[:8])


def run_and_compare(m, g, batch, atol=1e-4, grad_rtol=1e-4, taps=True, check_bn=True, tap_names=None, head_scale=False):
    """Run model `m` on the golden case and assert every recorded quantity matches.

    atol: absolute tolerance on activations / head outputs / losses (A.6: never pure relative).
    grad_rtol: relative-L2 tolerance on per-parameter gradient norms & samples.
    head_scale: losses and head outputs within atol of max(1, |tensor|) (tests/test_configs_gpu.py's check_outputs rule) instead of
    atol absolute.
    Goldens with rs/ keys are loaded into `m` first (load_running_stats).  In eval mode every parameter and buffer must come out
    of the forward bit-identical.
    """
    stage, train = int(g["stage"]), bool(int(g["train"]))
    has_rs = load_running_stats(m, g)
    if has_rs:                                  # the golden is only worth its name if the statistics move the outputs
        assert float(np.abs(g["logits0"] - g["def/logits0"]).max()) > 0.1
    before = None if train else state_snapshot(m)
    caught = {}
    hooks = []
    mods = dict(m.named_modules())
    tap_names = TAPS if tap_names is None else tap_names
    self_taps = hasattr(m, "taps")            # drn_amd.mainModel records its own (no per-module forward calls)
    if self_taps:
        m.taps = caught
    else:
        if taps:
            for t in tap_names:
                hooks.append(mods[t].register_forward_hook(lambda mod, i, o, n=t: caught.__setitem__(n, o)))
        hooks.append(m.fcos.head.register_forward_hook(lambda mod, i, o: caught.__setitem__("head", o)))
    m.train(train)
    boxes, losses = m(*batch)
    for h in hooks:
        h.remove()
    if self_taps:
        m.taps = None
    for k in ("loss_cls", "loss_reg", "loss_iou"):
        got = losses[k].detach().double().cpu().numpy().reshape(-1)
        tol = atol * max(1.0, float(np.abs(g[k]).max())) if head_scale else atol
        np.testing.assert_allclose(got, g[k], atol=tol, rtol=0, err_msg=k)
    logits, reg, _, iou = caught["head"]
    for l in range(3):
        for nm, ten in (("logits", logits), ("reg", reg), ("iou", iou)):
            got = ten[l].detach().float().cpu().numpy()
            ref = g["%s%d" % (nm, l)]
            assert got.shape == ref.shape, (nm, l, got.shape, ref.shape)
            tol = atol * max(1.0, float(np.abs(ref).max())) if head_scale else atol
            np.testing.assert_allclose(got, ref, atol=tol, rtol=0, err_msg="%s%d" % (nm, l))
    if taps:
        for t in tap_names:
            cs, smp = checksum(caught[t])
            ref = g["smp/" + t]
            np.testing.assert_allclose(smp, ref, atol=atol, rtol=0, err_msg="smp/" + t)
            n = caught[t].numel()
            np.testing.assert_allclose(cs, g["cs/" + t], atol=atol * n * 0.05 + 1e-3, rtol=1e-5, err_msg="cs/" + t)
    if train:
        loss = losses["loss_iou"] if stage == 2 else sum(l for l in losses.values())
        loss.backward()
        seen = 0
        for k, p in m.named_parameters():
            key = "gn/" + k
            if key not in g:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, "unexpected grad for " + k
                continue
            if k in ZERO_GRADS and p.grad is None:          # analytically zero: the HIP path hands out no gradient at all
                continue
            assert p.grad is not None, "missing grad for " + k
            seen += 1
            gr = p.grad.detach().double().reshape(-1).cpu()
            step = max(1, gr.numel() // 16)
            ref_n, ref_s = float(g[key][0]), g["gs/" + k].astype(np.float64)
            if k in ZERO_GRADS or ref_n < 1e-7:
                assert float(gr.abs().max()) <= 1e-5, (k, float(gr.abs().max()))
                continue
            assert abs(gr.norm().item() - ref_n) <= grad_rtol * ref_n + 1e-9, (k, gr.norm().item(), ref_n)
            got_s = gr[::step][:16].numpy()
            assert np.abs(got_s - ref_s).max() <= grad_rtol * max(ref_n / np.sqrt(gr.numel()) * 30, np.abs(ref_s).max()) + 1e-9, \
                (k, got_s, ref_s)
        assert seen > 20
        if check_bn:
            sd = m.state_dict()
            for key in g:
                if key.startswith("bn/"):
                    got = sd[key[3:]].float().cpu().numpy()
                    np.testing.assert_allclose(got, g[key], atol=atol, rtol=0, err_msg=key)
    else:
        after = state_snapshot(m)
        assert_state_equal(before, after, "eval forward")
        for key in g:
            if key.startswith("rs/"):
                assert np.array_equal(after[key[3:]].numpy(), g[key]), key
        n_det = np.array([len(b["detections"]) for b in boxes])
        np.testing.assert_array_equal(n_det, g["n_det"])
        # per-clip order inside a level is top-k(sorted=False) order: compare as sorted sets per clip
        off = 0
        for bi, b in enumerate(boxes):
            n = int(n_det[bi])
            got = np.concatenate([b["detections"].detach().float().cpu().numpy(),
                                  b["scores"].detach().float().cpu().numpy()[:, None],
                                  b["locations"].detach().float().cpu().numpy()[:, None]], 1)
            ref = np.concatenate([g["det"][off:off + n], g["score"][off:off + n, None], g["loc"][off:off + n, None]], 1)
            # (several foreground channels: one location can yield one candidate per class -- same segment, different score)
            got = got[np.lexsort((got[:, 2], got[:, 0], got[:, 3]))]
            ref = ref[np.lexsort((ref[:, 2], ref[:, 0], ref[:, 3]))]
            np.testing.assert_allclose(got, ref, atol=atol, rtol=0, err_msg="detections clip %d" % bi)
            lv = np.array([x for l in b["level"] for x in l])
            np.testing.assert_array_equal(np.sort(lv), np.sort(g["level"][off:off + n]))
            off += n
    return boxes, losses


def isolated(fn):
    """Run a GPU test in a FRESH Python process (this very test re-invoked through pytest with DRN_TEST_ISOLATED=1) and pass / fail
    with it.  Used by the bit-identity tests of the two-branch hipGraph step, which compare a whole training run.  (Introduced while
    `test_forked_graph_step_is_bit_identical` mismatched in 3 of ~10 full-suite runs and never on its own; the cause turned out not to
    be the process at all -- a ticket overtaking a write-through store in the K-split exchange of skinny_group_kernel, once in ~10^5
    launches when another branch's kernel ran beside it, fixed in qdense.hip, DESIGN.md section 3 -- the wrapper stays because a
    failure's report then names the side that moved and lands in gpurun_out/isolated_failures.log.)"""
    import functools
    import subprocess
    import sys

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        if os.environ.get("DRN_TEST_ISOLATED") == "1":
            return fn(*args, **kwargs)
        node = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        assert node, "isolated tests run under pytest"
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, DRN_TEST_ISOLATED="1")
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", node], cwd=root, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
        out = r.stdout.decode(errors="replace")
        if r.returncode and os.path.isdir(os.path.join(root, "gpurun_out")):          # (kept with the GPU box's outputs)
            with open(os.path.join(root, "gpurun_out", "isolated_failures.log"), "a") as f:
                f.write("==== %s\n%s\n" % (node, out[-6000:]))
        assert r.returncode == 0, out[-4000:]
    return wrapper
