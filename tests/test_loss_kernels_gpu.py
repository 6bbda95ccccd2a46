"""drn_fcos_loss_fwd / drn_fcos_loss_bwd (drn_amd/csrc/loss.hip) against the float64 model of tests/loss_ref.py on every case of its
table: labels and counts exactly, every loss and gradient element within loss_bound -- no tolerance is fixed by hand in this file --,
through the raw entry points, through DF.fcos_loss's autograd, on the one-launch (ticket) and the two-launch path, back to back on
one workspace, and with the counter bumps.  tests/test_loss_ref_cpu.py shows that twenty subtly wrong kernels each miss these bounds.

Largest |kernel - model| / bound observed on an MI355X, per output, and the case it came from (the bound assumes 2 ulps each for
expf, logf, log1pf and powf, none of them measured on gfx950; the figures say how much of that room the kernels use):
    loss_cls 0.056 (gamma_alpha)            loss_reg 0.039 (two_levels_256_rows)    loss_iou 0.023 (saturated_logits)
    total    0.044 (gamma_alpha)            dlogits  0.27  (finalize_strides, through autograd's `total`)
    dreg     0.22  (two_levels_256_rows)    diou     0.094 (edges_f32)
The losses sit far inside because their bound is the worst case of a sum (gamma over 17 or 18 additions, every term off the same way).
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref as R

pytestmark = pytest.mark.gpu

NAMES = list(R.CASES)
MULTI_BLOCK = [n for n in NAMES if R.CASES[n]["expect"]["nblk"] > 1]
GUARD = 96                 # elements behind every output that no launch may write
SENTINEL = -7.5


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


_on_device = {}


def device_case(name, dev):
    """The case's inputs on the device, uploaded once and never written."""
    if name not in _on_device:
        c = R.build(name)
        t = lambda a: torch.from_numpy(np.array(a)).to(dev)
        _on_device[name] = dict(logits=t(c["logits"]), reg=t(c["reg"]), iou=t(c["iou"]), gt=t(c["gt"]))
    return _on_device[name]


def guarded(n, dev, cols=None):
    shape = (n + GUARD,) if cols is None else (n + GUARD, cols)
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)


def untouched(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def g3_tensors(g3, dev):
    return [None if g is None else torch.tensor([g], dtype=torch.float32, device=dev) for g in g3]


def run_raw(name, dev, g3=None):
    """ops.fcos_loss_fwd (with labels=) and ops.fcos_loss_bwd on guarded buffers -> dict of numpy arrays and the buffers' guards."""
    from drn_amd import ops
    c, d = R.build(name), device_case(name, dev)
    n = len(c["logits"])
    stage = c["iou_stage"]
    levels = ops.loss_levels(c["levels"])
    out6, labels = guarded(6, dev), guarded(n, dev)
    dlogits, dreg, diou = guarded(n, dev), guarded(n, dev, 2), guarded(n, dev)
    iou = d["iou"] if stage else None
    ops.fcos_loss_fwd(levels, c["B"], d["logits"], d["reg"], iou, d["gt"], c["gamma"], c["alpha"], c["target_scale"], stage, out6, labels=labels)
    ops.fcos_loss_bwd(levels, c["B"], d["logits"], d["reg"], iou, d["gt"], c["gamma"], c["alpha"], c["target_scale"], stage, out6,
                      g3_tensors(c["g3"] if g3 is None else g3, dev), dlogits, dreg, diou)
    torch.cuda.synchronize()
    guards = all(untouched(b, k) for b, k in ((out6, 6), (labels, n), (dlogits, n), (dreg, n))) and untouched(diou, n if stage else 0)
    got = dict(out6=out6[:6].cpu().numpy(), labels=labels[:n].cpu().numpy(), dlogits=dlogits[:n].cpu().numpy(), dreg=dreg[:n].cpu().numpy(),
               diou=diou[:n].cpu().numpy() if stage else None)
    return got, guards


def check(name, got, model, bound, what):
    """Labels and counts exact, everything else inside the bound and finite; prints the ratios before it asserts."""
    r = R.ratios(got, model, bound)
    print("LOSS-RATIO %s %s: %s" % (what, name, "  ".join("%s %.3g" % (k, r[k]) for k in R.OUTPUTS)))
    assert got["labels"] is None or np.array_equal(got["labels"], model["labels"])
    assert np.array_equal(got["out6"][3:5].astype(np.float64), model["out6"][3:5])
    for k in ("out6", "dlogits", "dreg", "diou"):
        assert got[k] is None or np.isfinite(got[k]).all(), k
    assert max(r.values()) <= 1.0, r
    return r


@pytest.mark.parametrize("name", NAMES)
def test_values_against_the_model(dev, name):
    """Every case through ops.fcos_loss_fwd / ops.fcos_loss_bwd.  Nothing behind the last row of any output is written, nor diou at all
    when iou_stage = 0; with saturated logits everything is finite (check() asserts it for every case)."""
    case, model, bound = R.reference(name)
    got, guards = run_raw(name, dev)
    assert guards, "a launch wrote behind the rows it owns"
    check(name, got, model, bound, "raw")
    if not case["iou_stage"]:
        assert got["out6"][2] == 0.0 and got["out6"][4] == 0.0
    if model["out6"][3] == 0:
        assert got["out6"][1] == 0.0 and not got["dreg"].any()


@pytest.mark.parametrize("name", NAMES)
def test_autograd_against_the_model(dev, name):
    """DF.fcos_loss: backward of sum g_i loss_i with the absent g_i left out (their gradients arrive as None), then backward of the
    `total` output alone, which is the same gradient for all three losses.  The second pass of the 264-row two-block case feeds
    non-contiguous views of logits and reg."""
    from drn_amd import functional as DF
    case, model, bound = R.reference(name)
    d = device_case(name, dev)
    stage = case["iou_stage"]
    for which in ("weights", "total"):
        if which == "total" and name == "gamma_alpha":
            wide_l = torch.stack([d["logits"], d["logits"] + 1.0], 1)
            wide_r = torch.stack([d["reg"][:, 0], d["reg"][:, 0] * 3.0, d["reg"][:, 1], d["reg"][:, 1] * 5.0], 1)
            leaf_l, leaf_r = wide_l.requires_grad_(), wide_r.requires_grad_()
            L_, R_ = leaf_l[:, :1], leaf_r[:, ::2]
            assert not L_.is_contiguous() and not R_.is_contiguous()
        else:
            leaf_l, leaf_r = d["logits"][:, None].clone().requires_grad_(), d["reg"].clone().requires_grad_()
            L_, R_ = leaf_l, leaf_r
        I_ = d["iou"][:, None].clone().requires_grad_()
        l_cls, l_reg, l_iou, counts, total = DF.fcos_loss(L_, R_, I_, d["gt"], case["levels"], case["B"], case["gamma"], case["alpha"],
                                                          case["target_scale"], stage)
        assert l_cls.shape == l_reg.shape == l_iou.shape == total.shape == (1,) and counts.shape == (2,) and not counts.requires_grad
        out6 = torch.cat([l_cls, l_reg, l_iou, counts, total]).detach().cpu().numpy()
        if which == "weights":
            g3 = case["g3"]
            m, b = model, bound
            sum(g * l for g, l in zip(g3, (l_cls, l_reg, l_iou)) if g is not None).sum().backward()
        else:
            g3 = (2.5, 2.5, 2.5)
            m = R.loss_model(*R.args_of(dict(case, g3=g3)))
            b = R.loss_bound(*R.args_of(dict(case, g3=g3)), model=m)
            (2.5 * total).sum().backward()
        dl, dr = leaf_l.grad.cpu().numpy(), leaf_r.grad.cpu().numpy()
        if dl.shape[1] == 2:                                       # the views' gradients, and nothing in the columns beside them
            assert not dl[:, 1].any() and not dr[:, 1::2].any()
            dl, dr = dl[:, :1], dr[:, ::2]
        if stage:
            di = I_.grad.cpu().numpy()[:, 0]
        else:
            assert I_.grad is None
            di = None
        check(name, dict(out6=out6, labels=None, dlogits=dl[:, 0], dreg=dr, diou=di), m, b, "autograd-" + which)


def fwd_ctypes(name, dev, out6, labels, ws, ticket, bumps=()):
    """drn_fcos_loss_fwd itself: ticket = None takes the two-launch path."""
    from drn_amd import _lib, ops
    c, d = R.build(name), device_case(name, dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    nb = len(bumps)
    arr = (_lib.CounterBump * nb)(*[_lib.CounterBump(counter=p(t), inc=int(n)) for t, n in bumps]) if nb else None
    _lib.check(_lib.lib().drn_fcos_loss_fwd(ops.loss_levels(c["levels"]), len(c["levels"]), c["B"], p(d["logits"]), p(d["reg"]),
                                            p(d["iou"]) if c["iou_stage"] else None, p(d["gt"]), int(d["gt"].dtype == torch.float64),
                                            ctypes.c_float(c["gamma"]), ctypes.c_float(c["alpha"]), ctypes.c_float(c["target_scale"]),
                                            int(c["iou_stage"]), p(out6), p(labels), p(ws), p(ticket), arr, nb, ops._stream()), "drn_fcos_loss_fwd")


def fwd_ops(name, dev, out6, labels=None, bumps=None):
    from drn_amd import ops
    c, d = R.build(name), device_case(name, dev)
    ops.fcos_loss_fwd(ops.loss_levels(c["levels"]), c["B"], d["logits"], d["reg"], d["iou"] if c["iou_stage"] else None, d["gt"], c["gamma"],
                      c["alpha"], c["target_scale"], c["iou_stage"], out6, labels=labels, bumps=bumps)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", MULTI_BLOCK)
def test_two_launches_give_the_bits_of_one(dev, name):
    """A null ticket: fcos_loss_fwd_partial_kernel's `!ticket` branch and fcos_loss_fwd_final_kernel, which the source promises to be
    the same bits as the last-arriver path.  The workspace starts as NaN: a partial the final kernel read without its block having
    written it would show."""
    case, model, bound = R.reference(name)
    n, nblk = len(case["logits"]), R.CASES[name]["expect"]["nblk"]
    one6, one_lab = guarded(6, dev), guarded(n, dev)
    fwd_ops(name, dev, one6, labels=one_lab)
    two6, two_lab = guarded(6, dev), guarded(n, dev)
    ws = torch.full((5 * nblk + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    fwd_ctypes(name, dev, two6, two_lab, ws, None)
    torch.cuda.synchronize()
    assert np.array_equal(bits(one6), bits(two6)) and np.array_equal(bits(one_lab), bits(two_lab))
    assert untouched(two6, 6) and untouched(two_lab, n) and bool(torch.isnan(ws[5 * nblk:]).all()) and bool(torch.isfinite(ws[:5 * nblk]).all())
    r = R.ratios(dict(out6=two6[:6].cpu().numpy(), labels=two_lab[:n].cpu().numpy(), dlogits=None, dreg=None, diou=None),
                 dict(model, dlogits=None, dreg=None, diou=None), bound)
    assert max(r.values()) <= 1.0, r


def test_back_to_back_launches_rearm_the_ticket(dev):
    """Eight ticket launches on the shared workspace, alternating a 4-block and a 2-block input (then the 280-block one between two of
    them): every result is the bits of its first, so no launch read a partial an earlier one left, and the ticket word is 0 at the end."""
    from drn_amd import ops
    order = ["four_levels_ragged", "three_levels_257_rows_one_clip"] * 4 + ["finalize_strides", "saturated_logits", "finalize_strides"]
    assert R.CASES[order[0]]["expect"]["nblk"] != R.CASES[order[1]]["expect"]["nblk"]
    outs = [guarded(6, dev) for _ in order]
    for name, o in zip(order, outs):
        fwd_ops(name, dev, o)
    torch.cuda.synchronize()
    first = {}
    for name, o in zip(order, outs):
        assert untouched(o, 6)
        assert np.array_equal(bits(o), first.setdefault(name, bits(o))), name
        _, model, bound = R.reference(name)
        got = dict(out6=o[:6].cpu().numpy(), labels=None, dlogits=None, dreg=None, diou=None)
        assert max(R.ratios(got, dict(model, dlogits=None, dreg=None, diou=None), bound).values()) <= 1.0, name
    assert int(ops._counters(dev)[-1].item()) == 0


@pytest.mark.parametrize("path", ["ticket", "two_launches"])
@pytest.mark.parametrize("nbumps", [0, 1, R.MAX_BUMPS])
def test_counter_bumps_are_applied_once_per_launch(dev, path, nbumps):
    """nbumps distinct int64 counters at every other element of one tensor, increments 1..3: after k launches each has moved by k x its
    increment and no other element has changed; the losses are the same bits as without bumps."""
    from drn_amd import _lib, ops
    assert R.MAX_BUMPS == _lib.LOSS_MAX_BUMPS
    name, k = "four_levels_ragged", 3
    nblk = R.CASES[name]["expect"]["nblk"]
    start = torch.arange(2 * R.MAX_BUMPS + 3, dtype=torch.int64, device=dev) * 1000 - 5
    counters = start.clone()
    inc = [1 + i % 3 for i in range(nbumps)]
    bumps = [(counters[2 * i + 1:2 * i + 2], inc[i]) for i in range(nbumps)]
    plain, out6 = guarded(6, dev), guarded(6, dev)
    fwd_ops(name, dev, plain)
    ws = torch.zeros(5 * nblk, dtype=torch.float32, device=dev)
    for _ in range(k):
        if path == "ticket":
            fwd_ops(name, dev, out6, bumps=bumps)
        else:
            fwd_ctypes(name, dev, out6, None, ws, None, bumps)
    torch.cuda.synchronize()
    want = start.clone()
    for i in range(nbumps):
        want[2 * i + 1] += k * inc[i]
    assert torch.equal(counters, want)
    assert np.array_equal(bits(out6), bits(plain))
    assert int(ops._counters(dev)[-1].item()) == 0
