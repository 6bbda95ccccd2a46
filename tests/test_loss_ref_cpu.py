"""tests/loss_ref.py checked without a GPU: the float64 model is the oracle's FCOSLoss (oracle/drn_oracle.py, the reference's
model/loss.py) run in float64 autograd, with the oracle's float32 decisions bit for bit; a step-by-step fp32 evaluation of the kernels'
statements sits inside the derived bound on every element of every case while twenty subtly wrong ones each leave it -- which is what
makes tests/test_loss_kernels_gpu.py worth having --; the case table reaches the paths it names; no decision of any case sits near its
threshold without sitting on it; and drn_fcos_loss_fwd / drn_fcos_loss_bwd refuse bad arguments before any launch."""
import ctypes
import os
import re
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

import loss_ref as R
from oracle import drn_oracle as O

NAMES = list(R.CASES)


# ---- the model against the oracle ---------------------------------------------------------------------------------------------------
def per_level(flat, levels, B, dtype):
    """(R, C) rows, level-first and clip-major -> the reference's list of (B, C, L) tensors."""
    flat = np.asarray(flat).reshape(flat.shape[0], -1)
    out, r = [], 0
    for L, _, _, _ in levels:
        out.append(torch.from_numpy(flat[r:r + B * L].copy()).to(dtype).reshape(B, L, -1).permute(0, 2, 1).contiguous())
        r += B * L
    return out


def flat_of(ts):
    return torch.cat([t.permute(0, 2, 1).reshape(-1, t.size(1)) for t in ts]).numpy()


def sizes_patched(monkeypatch, levels):
    """The oracle reads the sizes of interest of level l from a module table of three rows: the case's own (lo, hi), of any length."""
    monkeypatch.setattr(O, "SIZES_OF_INTEREST", tuple((l[2], l[3]) for l in levels))
    assert O.TARGET_SCALE == 32.0


def oracle_run(case, dtype, logits=None):
    """FCOSLoss on the case in `dtype`: (losses [3], labels, mask or None, dlogits, dreg, diou or None) as numpy arrays.  The ground
    truth is cast to fp32 first (main_model.py:74), whatever `dtype` is."""
    levels, B, stage = case["levels"], case["B"], case["iou_stage"]
    logits = case["logits"] if logits is None else logits
    locs = [O.FCOSModule.locations_for(L, s, "cpu").to(dtype) for L, s, _, _ in levels]
    lg = [x.requires_grad_() for x in per_level(logits[:, None], levels, B, dtype)]
    rg = [x.requires_grad_() for x in per_level(case["reg"], levels, B, dtype)]
    io = [x.requires_grad_() for x in per_level(case["iou"][:, None], levels, B, dtype)]
    gt = torch.from_numpy(np.asarray(case["gt"]).astype(np.float32)).to(dtype)
    # alpha as a one-element tensor of `dtype`: the oracle multiplies its float32 class masks by alpha and 1 - alpha first, which with a
    # Python scalar rounds 1 - alpha to fp32 even in a float64 run (exact for the default 0.25, 4e-8 off for 0.4)
    alpha = torch.tensor([R.f32(case["alpha"])], dtype=dtype)
    lc, lr, li = O.FCOSLoss({"fcos_loss_gamma": R.f32(case["gamma"]), "fcos_loss_alpha": alpha})(locs, lg, rg, gt, io, not stage)
    gc, gr, gi = (0.0 if g is None else R.f32(g) for g in case["g3"])
    tot = gc * lc + gr * lr
    if li.requires_grad:
        tot = tot + gi * li.reshape(())
    tot.backward()
    grad = lambda xs: flat_of([x.grad if x.grad is not None else torch.zeros_like(x) for x in xs])
    labels = O.fcos_targets(locs, gt)[0].numpy()
    mask = None
    if stage:                                                     # FCOSLoss.__call__'s own lines for the tIoU mask (loss.py:168-188)
        merged = torch.cat([x.detach() for x in rg], dim=-1).transpose(2, 1)
        loc = torch.cat(locs)[None, :]
        pred = torch.stack([loc - merged[:, :, 0], loc + merged[:, :, 1]], dim=-1) / O.TARGET_SCALE
        pred = torch.cat([pred[:, :1].clamp(min=0, max=1), pred[:, 1:]], dim=1)
        m = (O.segment_tiou(pred, gt[:, None, :]) > 0.9).numpy()                   # (B, sum L): clip-major over ALL levels
        mask, c0 = [], 0
        for L, _, _, _ in levels:
            mask.append(m[:, c0:c0 + L].reshape(-1))
            c0 += L
        mask = np.concatenate(mask)
    losses = np.array([float(lc.detach().reshape(-1)[0]), float(lr.detach()), float(li.detach().reshape(-1)[0])])
    return losses, labels, mask, grad(lg)[:, 0], grad(rg), (grad(io)[:, 0] if stage else None)


def close64(got, want, scale, what):
    """|got - want| <= 1e-10 x the sum of the absolute terms `want` is made of: fp64 roundoff only."""
    got, want, scale = (np.asarray(x, dtype=np.float64) for x in (got, want, scale))
    bad = np.abs(got - want) > 1e-10 * scale
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], got[bad][:5], want[bad][:5])


def check_against_oracle(case, model, diou_rows=slice(None)):
    losses, _, _, dl, dr, di = oracle_run(case, torch.float64)
    A = model["abs"]
    close64(losses, model["out6"][:3], A["out6"][:3], "losses")
    close64(dl, model["dlogits"], A["dlogits"], "dlogits")
    close64(dr, model["dreg"], A["dreg"], "dreg")
    if case["iou_stage"]:
        close64(di[diou_rows], model["diou"][diou_rows], A["diou"][diou_rows], "diou")
    assert model["out6"][5] == model["out6"][0] + model["out6"][1] + model["out6"][2]


@pytest.mark.parametrize("name", [n for n in NAMES if n != "saturated_logits"])
def test_model_values_are_the_oracle_in_float64(monkeypatch, name):
    """Losses and all three input gradients, every case (the four-level one too: the oracle's loop takes any number of levels once its
    table of sizes has as many rows)."""
    case, model, _ = R.reference(name)
    assert case["B"] >= 2 or not case["iou_stage"]                # the oracle raises for B = 1 like the reference does
    sizes_patched(monkeypatch, case["levels"])
    check_against_oracle(case, model)


@pytest.mark.parametrize("name", NAMES)
def test_model_decisions_are_the_oracle_in_float32_bit_for_bit(monkeypatch, name):
    case, model, _ = R.reference(name)
    sizes_patched(monkeypatch, case["levels"])
    _, labels, mask, _, _, _ = oracle_run(case, torch.float32, logits=np.zeros_like(case["logits"]))
    assert labels.dtype == np.float32 and np.array_equal(labels, model["labels"])
    assert model["out6"][3] == labels.sum()
    if case["iou_stage"]:
        assert np.array_equal(mask, model["mask"]) and model["out6"][4] == mask.sum()
    else:
        assert not model["mask"].any() and model["out6"][4] == 0 and model["diou"] is None


def test_four_levels_level_by_level(monkeypatch):
    """The four-level table has no three-level description (its last two levels differ in stride), so every level's labels are checked
    against a single-level call of the oracle's target assignment with that level's sizes."""
    case, model, _ = R.reference("four_levels_ragged")
    levels, B = case["levels"], case["B"]
    assert len(levels) == 4 and len(set(l[1] for l in levels[2:])) == 2
    gt = torch.from_numpy(np.asarray(case["gt"]).astype(np.float32))
    r = 0
    for L, s, lo, hi in levels:
        monkeypatch.setattr(O, "SIZES_OF_INTEREST", ((lo, hi),))
        lab = O.fcos_targets([O.FCOSModule.locations_for(L, s, "cpu")], gt)[0].numpy()
        assert np.array_equal(lab, model["labels"][r:r + B * L]) and lab.any(), (L, s)
        r += B * L


def focal_decimal(x, positive, ga, al):
    """(loss, d loss / dx) of one logit at 200 digits (1 + e^-120 needs 52 of them before its logarithm has any)."""
    getcontext().prec = 200
    x, ga, al, one = Decimal(float(x)), Decimal(ga), Decimal(al), Decimal(1)
    p = one / (one + (-x).exp())
    om = one / (one + x.exp())
    if positive:
        return float(-al * (ga * om.ln()).exp() * p.ln()), float(al * (ga * om.ln()).exp() * (ga * p * p.ln() - om))
    return float(-(one - al) * (ga * p.ln()).exp() * om.ln()), float((one - al) * (ga * p.ln()).exp() * (-ga * om * om.ln() + p))


def test_saturated_logits_against_the_oracle_and_200_digits(monkeypatch):
    """The oracle's focal formula goes through log(1 - p), which is -inf in float64 beyond |x| ~ 37, so on this case it is not finite
    and cannot be the yardstick.  Two steps instead: with the eight saturated class logits set to 0 the model equals the oracle
    everywhere as on every other case; and the model's terms of exactly those eight rows equal a 200-digit evaluation of the focal
    loss and its derivative, which is all that differs between the two inputs."""
    case, model, _ = R.reference("saturated_logits")
    sizes_patched(monkeypatch, case["levels"])
    with np.errstate(all="ignore"):
        assert not np.isfinite(oracle_run(case, torch.float64)[0][0])
    sat = np.nonzero(np.abs(case["logits"]) > 90)[0]
    pos = model["dec"]["pos"]
    assert len(sat) == 8 and pos[sat].sum() == 4
    assert sorted(case["logits"][sat][pos[sat]].tolist()) == sorted(R.SATURATED) == sorted(case["logits"][sat][~pos[sat]].tolist())
    calm = dict(case, logits=np.where(np.abs(case["logits"]) > 90, np.float32(0), case["logits"]))
    m0 = R.loss_model(*R.args_of(calm))
    mk = np.nonzero(model["mask"])[0]
    assert sorted(case["iou"][mk].tolist()) == [-120.0, 95.0]     # two masked rows with saturated IoU logits: p (1 - p) is 0 in the
    unsat = np.ones(len(case["iou"]), dtype=bool)                 # oracle's float64 beyond |x| ~ 37, 1e-42 and 1e-52 in truth
    unsat[mk] = False
    check_against_oracle(calm, m0, diou_rows=unsat)
    getcontext().prec = 200
    k_iou = R.f32(case["g3"][2]) / model["out6"][4]
    for r in mk:
        pI = Decimal(1) / (Decimal(1) + (-Decimal(float(case["iou"][r]))).exp())
        want = float(Decimal(k_iou) * (pI - Decimal(float(model["tiou"][r]))) * pI * (Decimal(1) - pI))
        assert want != 0 and abs(model["diou"][r] - want) <= 1e-12 * abs(want), r
    other = np.ones(len(pos), dtype=bool)
    other[sat] = False
    for k in ("dreg", "diou"):
        assert np.array_equal(model[k], m0[k])
    assert np.array_equal(model["dlogits"][other], m0["dlogits"][other]) and np.array_equal(model["out6"][1:5], m0["out6"][1:5])
    ga, al = R.f32(case["gamma"]), R.f32(case["alpha"])
    div = model["out6"][3] + case["B"]
    k_cls = R.f32(case["g3"][0]) / div
    diff = 0.0
    for r in sat:
        f, df = focal_decimal(case["logits"][r], pos[r], ga, al)
        f0, _ = focal_decimal(0.0, pos[r], ga, al)
        diff += f - f0
        assert np.isfinite(model["dlogits"][r]) and abs(model["dlogits"][r] - df * k_cls) <= 1e-12 * abs(df * k_cls) + 1e-300, r
    assert abs((model["out6"][0] - m0["out6"][0]) - diff / div) <= 1e-10 * model["out6"][0]
    assert all(np.isfinite(model[k]).all() for k in ("out6", "dlogits", "dreg", "diou"))


# ---- emulation and mutants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_inside_the_bound_on_every_element(name):
    case, model, bound = R.reference(name)
    r = R.ratios(R.emulate_fp32(*R.args_of(case)), model, bound)
    print("emulation, %s: |err| / bound  %s" % (name, "  ".join("%s %.3g" % (k, r[k]) for k in R.OUTPUTS)))
    assert max(r.values()) <= 1.0, r
    assert all(np.isfinite(b).all() for b in (bound["out6"], bound["dlogits"], bound["dreg"])), "a bound that allows anything"
    # teeth: the bound on loss_cls, loss_reg and the total is below 1e-5 of the loss; on loss_iou, whose terms (p - tIoU)^2 / 2 double
    # the relative error of a difference of two numbers near 1, below 3e-4 of it
    for i, rel in ((0, 1e-5), (1, 1e-5), (2, 3e-4), (5, 1e-5)):
        assert bound["out6"][i] <= rel * abs(model["out6"][i]), (i, bound["out6"][i], model["out6"][i])


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_leaves_the_bound_on_some_case(mutant):
    caught = []
    for name in NAMES:
        case, model, bound = R.reference(name)
        r = R.ratios(R.emulate_fp32(*R.args_of(case), mutant=mutant), model, bound)
        worst = max(r, key=r.get)
        if r[worst] > 1.0:
            caught.append("%s (%s %.3g x)" % (name, worst, r[worst]))
    print("%s: outside the bound on %d of %d cases: %s" % (mutant, len(caught), len(NAMES), ", ".join(caught)))
    assert caught, mutant


def test_there_are_twenty_distinct_mutants():
    assert len(R.MUTANTS) == len(set(R.MUTANTS)) == 20


@pytest.mark.parametrize("name", NAMES)
def test_the_bound_is_rounding_not_the_gap_between_its_two_float64_passes(name):
    """loss_bound adds |kernel-order float64 value - model| to every element.  That term is float64 roundoff of two formulas for the
    same number; were it ever more than a millionth of the rounding part, the V pass would have drifted from the model."""
    gap = R.reference(name)[2]["gap"]
    print("%s: largest |V pass - model| / rounding part %.3g" % (name, gap))
    assert gap <= 1e-6


# ---- the case table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_no_decision_sits_near_its_threshold(name):
    """A condition on the INPUTS: tIoU against 0.9, mn against 0, mx against lo and hi, every side test of the gradients.  Each is more
    than MARGIN_ULPS fp32 ulps from its threshold or exactly on it, and exactly on it only in the cases built for that."""
    case, model, _ = R.reference(name)
    rows, clips = R._near(case["levels"], case["B"], case["reg"], case["gt"], case["iou_stage"])
    assert len(rows) == 0 and len(clips) == 0, (rows, clips)
    seen = R.observed(case, model)
    if R.CASES[name]["kind"] != "edges":
        assert seen["reg_ties"] == seen["tiou_ties"] == seen["mn_zero"] == seen["mx_on_bound"] == 0
    D = model["dec"]
    if case["iou_stage"]:
        assert float(np.min(np.abs(D["tiou"].astype(np.float64) - float(np.float32(0.9))))) > R.MARGIN_ULPS * 2.0 ** -24


@pytest.mark.parametrize("name", NAMES)
def test_case_table_covers_what_it_says(name):
    case, model, _ = R.reference(name)
    assert R.observed(case, model) == R.CASES[name]["expect"]
    R_ = len(case["logits"])
    assert R_ == case["B"] * sum(l[0] for l in case["levels"]) and case["reg"].shape == (R_, 2) and case["iou"].shape == (R_,)
    assert case["gt"].dtype == (np.float64 if R.CASES[name]["gt64"] else np.float32)
    assert case["target_scale"] == 32.0                            # a power of two throughout


def test_case_table_as_a_whole():
    C, E = R.CASES, {n: c["expect"] for n, c in R.CASES.items()}
    rows = {n: c["B"] * sum(l[0] for l in c["levels"]) for n, c in C.items()}
    assert set(len(c["levels"]) for c in C.values()) == {1, 2, 3, 4}
    assert [l[0] for l in C["four_levels_ragged"]["levels"]] == [37, 19, 10, 5] and [l[1] for l in C["four_levels_ragged"]["levels"]] == [1, 2, 4, 8]
    assert E["four_levels_ragged"]["pos_levels"] == [0, 1, 2, 3] and rows["four_levels_ragged"] % 256 != 0 and E["four_levels_ragged"]["nblk"] == 4
    assert rows["one_level_under_a_wave"] < 64 and rows["two_levels_256_rows"] == 256 and rows["three_levels_257_rows_one_clip"] == 257
    assert rows["finalize_strides"] > 65536 and E["finalize_strides"]["nblk"] > R.THREADS
    assert set(c["stage"] for c in C.values()) == {0, 1} and set(c["gt64"] for c in C.values()) == {False, True}
    assert E["no_positive"]["n_pos"] == 0 and E["no_positive"]["n_iou"] == 0
    assert np.array_equal(R.build("no_positive")["gt"][:, 0], R.build("no_positive")["gt"][:, 1])
    e = E["positives_without_iou_positives"]
    assert e["n_pos"] > 0 and e["n_iou"] == 0
    assert any(x["iou_on_negatives"] > 0 for x in E.values())
    e = E["edges_f32"]
    assert e == E["edges_f64"] and e["mn_zero"] > 0 and e["mx_on_bound"] >= 2 and e["reg_ties"] >= 4 and e["tiou_ties"] >= 4
    assert e["clamps"][0] >= 2 and e["clamps"][3] == 2            # ps < 0 at location 0 (two of them masked rows), pe > 1 twice
    D = R.reference("edges_f32")[1]["dec"]
    lo_s, _, _, hi_e = D["clamp"]
    m = D["masked"]
    assert (lo_s & hi_e & m).sum() == 1 and (lo_s & ~hi_e & m).sum() == 1 and (~lo_s & hi_e & m).sum() == 1
    reg, pos = R.build("edges_f32")["reg"], D["pos"]
    one = ((reg[:, 0] == D["tl"]) ^ (reg[:, 1] == D["tr"])) & pos
    both = (reg[:, 0] == D["tl"]) & (reg[:, 1] == D["tr"]) & pos
    assert one.sum() >= 2 and both.sum() >= 2
    assert ((D["pe"] == D["ge"]) & (D["ps"] != D["gs"]) & m).any() and ((D["ps"] == D["gs"]) & (D["pe"] != D["ge"]) & m).any()
    assert C["gamma_alpha"]["gamma"] == 1.5 and C["gamma_alpha"]["alpha"] == 0.4
    g3s = [c["g3"] for c in C.values()]
    assert all(any(g[i] is None for g in g3s) for i in range(3)) and any(None not in g and len(set(g)) == 3 for g in g3s)
    # every case with an absent upstream gradient would notice it being read as 1: the loss it belongs to is not 0
    for n, c in C.items():
        for i in range(3):
            if c["g3"][i] is None and (i < 2 or c["stage"]):
                assert R.reference(n)[1]["out6"][i] != 0, (n, i)
    # and an absent g_iou read as 1 would move gradients: the model with g_iou = 1 differs on that case
    n = [k for k, c in C.items() if c["g3"][2] is None]
    assert n == ["gamma_alpha"] and E[n[0]]["n_iou"] > 0 and C[n[0]]["stage"] == 1
    case, model, bound = R.reference(n[0])
    as_one = R.loss_model(*R.args_of(dict(case, g3=case["g3"][:2] + (1.0,))))
    assert not model["diou"].any() and R.inside(as_one["diou"], model["diou"], bound["diou"]) > 1 and R.inside(as_one["dreg"], model["dreg"], bound["dreg"]) > 1
    assert E["positives_without_iou_positives"]["n_iou"] == 0 and C["positives_without_iou_positives"]["g3"][2] is not None


def test_fp64_ground_truth_matters():
    """The fp64 values are not fp32 numbers, and on the exact case a label differs when the cast is skipped (decisions on the fp64
    values) and when it truncates."""
    for n, c in R.CASES.items():
        if c["gt64"]:
            gt = R.build(n)["gt"]
            nz = gt != 0
            assert (gt.astype(np.float32).astype(np.float64) != gt)[nz].all(), n
    case, model, _ = R.reference("edges_f64")
    D = model["dec"]
    gs, ge = case["gt"][D["b"], 0], case["gt"][D["b"], 1]
    loc, lo, hi = (D[k].astype(np.float64) for k in ("loc", "lo", "hi"))
    tl, tr = loc - gs * 32.0, ge * 32.0 - loc
    skipped = (np.minimum(tl, tr) > 0) & (np.maximum(tl, tr) >= lo) & (np.maximum(tl, tr) <= hi)
    assert (skipped != D["pos"]).sum() >= 1
    trunc = R.emulate_fp32(*R.args_of(case), mutant="gt_truncated")
    assert (trunc["labels"] != model["labels"]).sum() >= 1
    assert np.array_equal(R.reference("edges_f32")[1]["labels"], model["labels"])


def test_bound_scales_with_the_summation_depth():
    assert R.sum_chain(1) == 17 and R.sum_chain(256) == 17 and R.sum_chain(257) == 18 and R.sum_chain(280) == 18
    assert R.POW_ULPS == 2 and (R.EXP_ULPS, R.LOG_ULPS, R.LOG1P_ULPS) == (2, 2, 2)


def test_constants_are_the_ones_in_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include/drn_hip.h")).read()
    define = lambda name: int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert define("DRN_LOSS_MAX_BUMPS") == R.MAX_BUMPS and define("DRN_MAX_GROUPS") == R.MAX_LEVELS


# ---- refusals, before any launch ------------------------------------------------------------------------------------------------------
def built_lib():
    from drn_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_fcos_loss_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call here returns DRN_ERR_ARG with a text and starts no device work (this runs without a GPU): the pointers are made up."""
    from drn_amd import _lib
    L = built_lib()
    p, cf = ctypes.c_void_p(0x1000), ctypes.c_float
    lv = lambda *Ls: (_lib.LossLevel * len(Ls))(*[_lib.LossLevel(L=n, stride=1.0, lo=-1.0, hi=6.0) for n in Ls])
    bump = (_lib.CounterBump * 33)(*[_lib.CounterBump(counter=0x1000 + 8 * i, inc=1) for i in range(33)])

    def fwd(**kw):
        a = dict(levels=lv(8, 4), nlevels=2, B=2, logits=p, reg=p, iou=p, gt=p, stage=1, out6=p, labels=None, ws=p, ticket=p, bumps=None, nbumps=0)
        a.update(kw)
        rc = L.drn_fcos_loss_fwd(a["levels"], a["nlevels"], a["B"], a["logits"], a["reg"], a["iou"], a["gt"], 0, cf(2.0), cf(0.25), cf(32.0),
                                 a["stage"], a["out6"], a["labels"], a["ws"], a["ticket"], a["bumps"], a["nbumps"], None)
        return rc, L.drn_last_error()

    def bwd(**kw):
        a = dict(levels=lv(8, 4), nlevels=2, B=2, logits=p, reg=p, iou=p, gt=p, stage=1, out=p, dlogits=p, dreg=p, diou=p)
        a.update(kw)
        rc = L.drn_fcos_loss_bwd(a["levels"], a["nlevels"], a["B"], a["logits"], a["reg"], a["iou"], a["gt"], 0, cf(2.0), cf(0.25), cf(32.0),
                                 a["stage"], a["out"], p, p, p, a["dlogits"], a["dreg"], a["diou"], None)
        return rc, L.drn_last_error()

    def refused(res, text):
        assert res[0] == -1 and text in res[1], res

    for call, who in ((fwd, b"drn_fcos_loss_fwd"), (bwd, b"drn_fcos_loss_bwd")):
        refused(call(nlevels=0), who + b": bad level table")
        refused(call(levels=lv(8, 4, 2, 1, 1), nlevels=5), who + b": bad level table")
        refused(call(levels=None), who + b": bad level table")
        refused(call(B=0), who + b": bad level table")
        refused(call(B=-1), who + b": bad level table")
        refused(call(levels=lv(8, 0)), who + b": level 1 has no locations")
        for name in ("logits", "reg", "gt"):
            refused(call(**{name: None}), who + b": null pointer")
        refused(call(iou=None), who + b": null pointer")
    refused(fwd(out6=None), b"drn_fcos_loss_fwd: null pointer")
    refused(fwd(ws=None), b"drn_fcos_loss_fwd: workspace")
    refused(fwd(bumps=bump, nbumps=33), b"drn_fcos_loss_fwd: at most 32 counter bumps")
    refused(fwd(bumps=bump, nbumps=-1), b"drn_fcos_loss_fwd: at most 32 counter bumps")
    refused(fwd(bumps=None, nbumps=1), b"drn_fcos_loss_fwd: at most 32 counter bumps")
    for name in ("out", "dlogits", "dreg", "diou"):
        refused(bwd(**{name: None}), b"drn_fcos_loss_bwd: null pointer")
