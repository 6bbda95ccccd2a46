"""A float64 model of the fused FCOS loss kernels of drn_amd/csrc/loss.hip (drn_fcos_loss_fwd / drn_fcos_loss_bwd), a forward error
bound for them, an fp32 evaluation in the kernels' order with named wrong variants, and the cases the CPU and GPU tests share
(tests/test_loss_ref_cpu.py, tests/test_loss_kernels_gpu.py).  numpy only: nothing here touches a device.

Rows are level-first and clip-major: row = row_start[level] + b * L[level] + t.  Per row, with loc = t * stride + stride / 2, (gs, ge)
the clip's ground truth ROUNDED TO fp32 (main_model.py:74), S = target_scale:

    tl = loc - gs S, tr = ge S - loc;   positive  <=>  min(tl, tr) > 0 and lo <= max(tl, tr) <= hi            (loss.py:98-110)
    focal   = alpha (1 - p)^gamma (-log p) on positives, (1 - alpha) p^gamma (-log(1 - p)) on the others, p = sigmoid(logit)
    iou     = -log((inter + 1e-8) / (union + 1e-8)),  inter = min(pr, tr) + min(pl, tl), union = (tl + tr) + (pl + pr) - inter
    tIoU    = max(min(pe, ge) - max(ps, gs), 0) / (max(max(pe, ge) - min(ps, gs), 0) + 1e-6),  ps = (loc - pl) / S, pe = (loc + pr) / S,
              both clamped to [0, 1] at location 0 of level 0 of every clip (loss.py:180-181); masked <=> tIoU > 0.9
    sl1     = SmoothL1(sigmoid(iou logit) - tIoU) on masked rows, the target keeping its gradient into reg
    loss_cls = sum focal / (n_pos + B);  loss_reg = sum iou / n_pos (0 without positives);  loss_iou = sum sl1 / n_iou (0 without)

`loss_model`: DECISIONS in fp32, in the reference's operation order (the reference runs in fp32, so its decisions are the definition);
VALUES in float64 from the same fp32 inputs.  `loss_bound`: how far a correct fp32 evaluation in the kernels' order may sit from the
model, per output element.  `emulate_fp32`: such an evaluation (and, with `mutant=`, a subtly wrong one)."""
import numpy as np

from optim_ref import DIV_ULPS, POW_ULPS, U, f32, gamma as higham, inside

F = np.float32
# expf, logf, log1pf: like powf (optim_ref.POW_ULPS), no error table of the device math library ships with the toolchain this project
# builds with, and nobody has measured them on gfx950, so the values are ASSUMED: 2 ulps each, twice what the HIP programming guide's
# table of device functions gives (expf 1, logf 1, log1pf 1); OpenCL's limits are 3, 3 and 2.
EXP_ULPS = 2
LOG_ULPS = 2
LOG1P_ULPS = 2
TINY = 2.0 ** -126          # results below the normal range may be flushed or lose bits: every rounded operation may also be off by this
EPS8, EPS6 = 1e-8, 1e-6     # iou_loss.py:12, loss.py:256
THREADS = 256               # rows per workgroup of the partial kernel; threads of the finalize loop
MAX_LEVELS = 4              # DRN_MAX_GROUPS
MAX_BUMPS = 32              # DRN_LOSS_MAX_BUMPS


# ----------------------------------------------------------------------------------------------------------------------------------
# rows and decisions
# ----------------------------------------------------------------------------------------------------------------------------------
def nblocks(levels, B):
    return (B * sum(l[0] for l in levels) + THREADS - 1) // THREADS


def rows_of(levels, B):
    """(level, b, t) of every row."""
    lvl = np.concatenate([np.full(B * l[0], i, dtype=np.int64) for i, l in enumerate(levels)])
    b = np.concatenate([np.repeat(np.arange(B, dtype=np.int64), l[0]) for l in levels])
    t = np.concatenate([np.tile(np.arange(l[0], dtype=np.int64), B) for l in levels])
    return lvl, b, t


def half(lt, eq):
    """1 where lt, 1/2 where eq, else 0: torch's rule for the gradient of an elementwise min / max at a tie."""
    return np.where(lt, 1.0, np.where(eq, 0.5, 0.0))


def decide(levels, B, reg, gt, target_scale, iou_stage):
    """Every decision of the loss in np.float32 elementwise operations, in the reference's order, and the fp32 quantities they are
    taken on.  gt: (B, 2) fp32 or fp64, rounded to fp32 first."""
    assert 1 <= len(levels) <= MAX_LEVELS and B >= 1
    lvl, b, t = rows_of(levels, B)
    st = np.array([l[1] for l in levels], dtype=F)[lvl]
    lo = np.array([l[2] for l in levels], dtype=F)[lvl]
    hi = np.array([l[3] for l in levels], dtype=F)[lvl]
    ts = F(target_scale)
    g = np.asarray(gt).astype(F)                       # round to nearest even: torch's .float()
    gs, ge = g[b, 0], g[b, 1]
    reg = np.asarray(reg, dtype=F)
    pl, pr = reg[:, 0], reg[:, 1]
    with np.errstate(all="ignore"):
        loc = t.astype(F) * st + st * F(0.5)
        tl, tr = loc - gs * ts, ge * ts - loc
        mn, mx = np.minimum(tl, tr), np.maximum(tl, tr)
        pos = (mn > 0) & (mx >= lo) & (mx <= hi)
        ps, pe = (loc - pl) / ts, (loc + pr) / ts
        head = (lvl == 0) & (t == 0)
        ms = np.where(head & ~((ps >= 0) & (ps <= 1)), 0.0, 1.0)      # inclusive: clamp's gradient is 1 on the boundary
        me = np.where(head & ~((pe >= 0) & (pe <= 1)), 0.0, 1.0)
        lo_s, hi_s, lo_e, hi_e = head & (ps < 0), head & (ps > 1), head & (pe < 0), head & (pe > 1)
        ps = np.where(head, np.clip(ps, F(0), F(1)), ps)
        pe = np.where(head, np.clip(pe, F(0), F(1)), pe)
        imax, imin = np.minimum(pe, ge), np.maximum(ps, gs)
        umax, umin = np.maximum(pe, ge), np.minimum(ps, gs)
        inter, uni = np.maximum(imax - imin, F(0)), np.maximum(umax - umin, F(0))
        tiou = inter / (uni + F(EPS6))
        masked = (tiou > F(0.9)) & bool(iou_stage)
    assert loc.dtype == tl.dtype == ps.dtype == tiou.dtype == F
    return dict(level=lvl, b=b, t=t, loc=loc, lo=lo, hi=hi, gs=gs, ge=ge, tl=tl, tr=tr, mn=mn, mx=mx, pos=pos, head=head, ps=ps, pe=pe,
                ms=ms, me=me, clamp=(lo_s, hi_s, lo_e, hi_e), tiou=tiou, masked=masked,
                dil=half(pl < tl, pl == tl), dir=half(pr < tr, pr == tr),            # d min(pl, tl) / d pl, d min(pr, tr) / d pr
                e_lt=half(pe < ge, pe == ge), e_gt=half(pe > ge, pe == ge),          # d min(pe, ge) / d pe, d max(pe, ge) / d pe
                s_gt=half(ps > gs, ps == gs), s_lt=half(ps < gs, ps == gs))          # d max(ps, gs) / d ps, d min(ps, gs) / d ps


def _softplus(z):
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def _g3(g3):
    return [0.0 if g is None else f32(g) for g in g3]


# ----------------------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------------------
def loss_model(levels, B, logits, reg, iou, gt, gamma, alpha, target_scale, iou_stage, g3=(1.0, 1.0, 1.0)):
    """dict(out6, labels, mask, dlogits, dreg, diou, abs, dec).  out6 = loss_cls, loss_reg, loss_iou, n_pos, n_iou, their sum (float64);
    labels: fp32 0 / 1 per row; mask: tIoU > 0.9 per row (all False when iou_stage = 0); dlogits (R,), dreg (R, 2), diou (R,; None when
    iou_stage = 0): the gradients of g3[0] loss_cls + g3[1] loss_reg + g3[2] loss_iou, None reading as 0; tiou: the float64 tIoU of the
    masked rows (0 elsewhere; None when iou_stage = 0); abs: for every one of these,
    the sum of the absolute values of the terms it is made of (what fp64 roundoff and the bound scale with); dec: decide()'s result."""
    D = decide(levels, B, reg, gt, target_scale, iou_stage)
    x = np.asarray(logits, dtype=F).astype(np.float64).reshape(-1)
    reg = np.asarray(reg, dtype=F).astype(np.float64)
    pl, pr = reg[:, 0], reg[:, 1]
    loc, gs, ge = (D[k].astype(np.float64) for k in ("loc", "gs", "ge"))
    ga, al, ts = f32(gamma), f32(alpha), f32(target_scale)
    gc, gr, gi = _g3(g3)
    pos, masked = D["pos"], D["masked"]
    R = x.shape[0]
    assert R == D["level"].shape[0] and reg.shape == (R, 2)
    with np.errstate(all="ignore"):
        # focal: -log p = softplus(-x), -log(1 - p) = softplus(x), (1 - p)^g = exp(-g softplus(x)), p^g = exp(-g softplus(-x))
        spp, spn = _softplus(x), _softplus(-x)
        p, om = np.exp(-spn), np.exp(-spp)
        focal = np.where(pos, al * np.exp(-ga * spp) * spn, (1.0 - al) * np.exp(-ga * spn) * spp)
        dfocal = np.where(pos, al * np.exp(-ga * spp) * (-ga * p * spn - om), (1.0 - al) * np.exp(-ga * spn) * (ga * om * spp + p))
        # IoU loss on positives; the side of each min is the fp32 decision
        tl, tr = loc - gs * ts, ge * ts - loc
        dil, dir_ = D["dil"], D["dir"]
        i_reg = np.where(dir_ > 0, pr, tr) + np.where(dil > 0, pl, tl)
        u_reg = (tl + tr) + (pl + pr) - i_reg
        ioul = np.where(pos, -np.log((i_reg + EPS8) / (u_reg + EPS8)), 0.0)
        n_pos, n_iou = float(pos.sum()), float(masked.sum())
        S_f, S_l = float(focal.sum()), float(ioul.sum())
        out = np.zeros(6)
        out[0] = S_f / (n_pos + B)
        out[1] = S_l / n_pos if n_pos > 0 else 0.0
        out[3], out[4] = n_pos, n_iou
        k_cls = gc / (n_pos + B)
        k_reg = gr / n_pos if n_pos > 0 else 0.0
        k_iou = gi / n_iou if (iou_stage and n_iou > 0) else 0.0
        dlogits = dfocal * k_cls
        ie, ue = i_reg + EPS8, u_reg + EPS8
        a0, b0, a1, b1 = -dil / ie, (1.0 - dil) / ue, -dir_ / ie, (1.0 - dir_) / ue
        dreg = np.where(pos[:, None], k_reg * np.stack([a0 + b0, a1 + b1], 1), 0.0)
        adreg = np.where(pos[:, None], abs(k_reg) * np.stack([np.abs(a0) + np.abs(b0), np.abs(a1) + np.abs(b1)], 1), 0.0)
        diou = tiou64 = None
        a_sl1 = 0.0
        if iou_stage:
            xi = np.asarray(iou, dtype=F).astype(np.float64).reshape(-1)
            assert xi.shape[0] == R
            lo_s, hi_s, lo_e, hi_e = D["clamp"]
            ps = np.where(lo_s, 0.0, np.where(hi_s, 1.0, (loc - pl) / ts))
            pe = np.where(lo_e, 0.0, np.where(hi_e, 1.0, (loc + pr) / ts))
            # sides by the fp32 decisions; at a tie both sides hold the same value
            imax, imin = np.where(D["e_lt"] > 0, pe, ge), np.where(D["s_gt"] > 0, ps, gs)
            umax, umin = np.where(D["e_gt"] > 0, pe, ge), np.where(D["s_lt"] > 0, ps, gs)
            inter, den = imax - imin, (umax - umin) + EPS6           # both differences are positive where tIoU > 0.9
            tiou = inter / den
            tiou64 = np.where(masked, tiou, 0.0)
            pI = np.exp(-_softplus(-xi))
            d = pI - tiou
            ad = np.abs(d)
            sl1 = np.where(masked, np.where(ad < 1, 0.5 * d * d, ad - 0.5), 0.0)
            S_s = float(sl1.sum())
            a_sl1 = S_s
            out[2] = S_s / n_iou if n_iou > 0 else 0.0
            sl = np.where(ad < 1, d, np.sign(d))
            diou = np.where(masked, k_iou * sl * pI * np.exp(-_softplus(xi)), 0.0)
            dt = -k_iou * sl
            t_e = (D["me"] * D["e_lt"] * den, D["me"] * inter * D["e_gt"])
            t_s = (-D["ms"] * D["s_gt"] * den, -D["ms"] * inter * D["s_lt"])
            dt_de, dt_ds = (t_e[0] - t_e[1]) / (den * den), (t_s[0] - t_s[1]) / (den * den)
            dreg = dreg + np.where(masked[:, None], np.stack([dt * dt_ds * (-1.0 / ts), dt * dt_de * (1.0 / ts)], 1), 0.0)
            a_s = (np.abs(t_s[0]) + np.abs(t_s[1])) / (den * den)
            a_e = (np.abs(t_e[0]) + np.abs(t_e[1])) / (den * den)
            adreg = adreg + np.where(masked[:, None], np.abs(dt)[:, None] * np.stack([a_s, a_e], 1) / ts, 0.0)
        out[5] = out[0] + out[1] + out[2]
    aout = np.array([out[0], float(np.abs(ioul).sum()) / max(n_pos, 1.0), a_sl1 / max(n_iou, 1.0), 0.0, 0.0, 0.0])
    aout[5] = aout[0] + aout[1] + aout[2]
    return dict(out6=out, labels=pos.astype(F), mask=masked.copy(), dlogits=dlogits, dreg=dreg, diou=diou, dec=D, tiou=tiou64,
                abs=dict(out6=aout, dlogits=np.abs(dlogits), dreg=adreg, diou=None if diou is None else np.abs(diou)))


# ----------------------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------------------
class V(object):
    """A float64 value v and a bound e on |what a correct fp32 evaluation holds - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.asarray(e, dtype=np.float64)


def _r(v, e, k=1.0):
    """One rounded operation (k: its error in units of U) on a result known to e before rounding: the computed value c has |c - v| <= e,
    so rounding adds at most k U |c| <= k U (|v| + e), or TINY below the normal range."""
    return V(v, e + k * U * (np.abs(v) + e) + TINY)


def vadd(a, b):
    return _r(a.v + b.v, a.e + b.e)


def vsub(a, b):
    return _r(a.v - b.v, a.e + b.e)


def vmul(a, b):
    return _r(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e + a.e * b.e)


def vdiv(a, b):
    """|a'/b' - a/b| = |(a' - a) b - a (b' - b)| / (|b| |b'|) <= (ea + |a/b| eb) / (|b| - eb)."""
    room = np.abs(b.v) - b.e
    q = a.v / b.v
    return _r(q, np.where(room > 0, (a.e + np.abs(q) * b.e) / np.where(room > 0, room, 1.0), np.inf), 2.0 * DIV_ULPS)


def vmin(a, b):
    return V(np.minimum(a.v, b.v), np.maximum(a.e, b.e))       # min and max are 1-Lipschitz in the max norm and round nothing


def vmax(a, b):
    return V(np.maximum(a.v, b.v), np.maximum(a.e, b.e))


def vneg(a):
    return V(-a.v, a.e)


def vexp(a):
    v = np.exp(a.v)
    return _r(v, v * np.expm1(a.e), 2.0 * EXP_ULPS)             # convex and increasing: the upper side is the larger one


def vlog1p(a):
    return _r(np.log1p(a.v), np.log1p(a.v) - np.log1p(np.maximum(a.v - a.e, -1.0)), 2.0 * LOG1P_ULPS)     # concave: the lower side


def vlog(a):
    room = a.v - a.e
    return _r(np.log(a.v), np.where(room > 0, -np.log1p(-a.e / a.v), np.inf), 2.0 * LOG_ULPS)


def vpow(a, g):
    """a >= 0, g >= 1 (convex and increasing there: the upper side is the larger one)."""
    assert g >= 1.0
    v = a.v ** g
    return _r(v, (a.v + a.e) ** g - v, 2.0 * POW_ULPS)


def vsoftplus(z):
    """The kernel's softplus(): z > 0 ? z + log1pf(expf(-z)) : log1pf(expf(z)).  z: exact float64 array."""
    t = vlog1p(vexp(V(-np.abs(z))))
    s = vadd(V(z), t)
    return V(np.where(z > 0, s.v, t.v), np.where(z > 0, s.e, t.e))


def vwhere(c, a, b):
    return V(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def sum_chain(nblk):
    """The longest chain of rounded additions a term of a loss sum goes through.  block_sum5: the wave tree over 64 lanes (6), then the
    tree over the 256 / 64 = 4 per-wave sums (2: the other 60 lanes add zeros, which rounds nothing).  loss_finalize: a thread adds
    ceil(nblk / 256) partials in a row, then the same two trees."""
    return 6 + 2 + -(-nblk // THREADS) + 6 + 2


def vsum(terms, keep, chain):
    """The kernels' sum of the per-row terms where `keep`: every term passes through at most `chain` rounded additions, so the computed
    sum is sum t'_i (1 + theta_i), |theta_i| <= gamma(chain)."""
    v = np.where(keep, terms.v, 0.0)
    e = np.where(keep, terms.e, 0.0)
    gk = higham(chain)
    return V(float(v.sum()), float(e.sum()) * (1.0 + gk) + gk * float(np.abs(v).sum()))


def loss_bound(levels, B, logits, reg, iou, gt, gamma, alpha, target_scale, iou_stage, g3=(1.0, 1.0, 1.0), model=None):
    """dict(out6, dlogits, dreg, diou, gap): per-element bounds on |kernel - loss_model| for a correct fp32 evaluation in the kernels'
    operation order.  Every statement of the kernels is redone on V pairs (float64 value, bound on the fp32 result's distance from it):
    a rounded +, -, * adds U of the result, a division 2 DIV_ULPS U, expf / logf / log1pf / powf their named ulps; errors of the
    operands are carried through exactly (products of two errors included: no first-order cut), through exp / log / pow by the
    function's own monotonicity and convexity; min, max and the clamp carry the larger operand error.  A fused multiply-add rounds
    once where two operations round twice, so contraction only lowers a count.  The three sums use Higham's gamma over sum_chain().
    The reference's 1e-8 / 1e-6: in fp32 `inter + 1e-8f` is inter for inter > 0.17, in fp64 it is not; that is the rounding of that
    addition, U (inter + 1e-8) >= 1e-8 there, which _r charges; the constants themselves differ (1e-8f - 1e-8 = 6e-17,
    1e-6f - 1e-6 = -2.5e-14) and enter as the operand error of EPS8 / EPS6.  The V pass follows the KERNEL's formulas (1 - p by
    subtraction), the model the stable ones: what the two float64 values differ by is added to the bound, and `gap` is the largest
    share that addition has of the rounding part on any element (the CPU test keeps it negligible: a V pass that drifted from the
    model, or copied a kernel mistake, must fail there, not widen the bound).
    Counts (out6[3:5]) and labels are exact: their bound is 0."""
    M = model if model is not None else loss_model(levels, B, logits, reg, iou, gt, gamma, alpha, target_scale, iou_stage, g3)
    D = M["dec"]
    x = np.asarray(logits, dtype=F).astype(np.float64).reshape(-1)
    reg = np.asarray(reg, dtype=F).astype(np.float64)
    pl, pr = V(reg[:, 0]), V(reg[:, 1])
    loc, gs, ge = (V(D[k].astype(np.float64)) for k in ("loc", "gs", "ge"))     # loc: t * stride + stride / 2 is exact for the strides used
    ga, al, ts = f32(gamma), V(f32(alpha)), V(f32(target_scale))
    gc, gr, gi = _g3(g3)
    pos, masked = D["pos"], D["masked"]
    chain = sum_chain(nblocks(levels, B))
    one = V(1.0)
    e8, e6 = V(EPS8, abs(float(F(EPS8)) - EPS8)), V(EPS6, abs(float(F(EPS6)) - EPS6))
    n_pos, n_iou = M["out6"][3], M["out6"][4]
    with np.errstate(all="ignore"):
        # ---- forward ----
        p = vdiv(one, vadd(one, vexp(V(-x))))
        om = vsub(one, p)
        spp, spn = vsoftplus(x), vsoftplus(-x)
        oma = vsub(one, al)
        w_pos, w_neg = vmul(al, vpow(om, ga)), vmul(oma, vpow(p, ga))
        focal = vwhere(pos, vmul(w_pos, spn), vmul(w_neg, spp))
        tl, tr = vsub(loc, vmul(gs, ts)), vsub(vmul(ge, ts), loc)
        i_reg = vadd(vmin(pr, tr), vmin(pl, tl))
        u_reg = vsub(vadd(vadd(tl, tr), vadd(pl, pr)), i_reg)
        ie, ue = vadd(i_reg, e8), vadd(u_reg, e8)
        ioul = vneg(vlog(vdiv(ie, ue)))
        S_f, S_l = vsum(focal, np.ones_like(pos), chain), vsum(ioul, pos, chain)
        o0 = vdiv(S_f, V(n_pos + B))
        o1 = vdiv(S_l, V(n_pos)) if n_pos > 0 else V(0.0)
        o2 = V(0.0)
        if iou_stage:
            xi = np.asarray(iou, dtype=F).astype(np.float64).reshape(-1)
            ps, pe = vdiv(vsub(loc, pl), ts), vdiv(vadd(loc, pr), ts)
            head = D["head"]
            ps, pe = V(np.where(head, np.clip(ps.v, 0, 1), ps.v), ps.e), V(np.where(head, np.clip(pe.v, 0, 1), pe.v), pe.e)
            zero = V(0.0)
            inter = vmax(vsub(vmin(pe, ge), vmax(ps, gs)), zero)
            uni = vmax(vsub(vmax(pe, ge), vmin(ps, gs)), zero)
            den = vadd(uni, e6)
            tiou = vdiv(inter, den)
            pI = vdiv(one, vadd(one, vexp(V(-xi))))
            d = vsub(pI, tiou)
            assert not masked.any() or float(np.max((np.abs(d.v) + d.e)[masked])) < 1.0     # the quadratic branch of SmoothL1, for sure
            sl1 = vmul(vmul(V(0.5), d), d)
            o2 = vdiv(vsum(sl1, masked, chain), V(n_iou)) if n_iou > 0 else V(0.0)
        o5 = vadd(vadd(o0, o1), o2)
        # ---- backward ----
        k_cls = vdiv(V(gc), V(n_pos + B))
        k_reg = vdiv(V(gr), V(n_pos)) if n_pos > 0 else V(0.0)
        k_iou = vdiv(V(gi), V(n_iou)) if (iou_stage and n_iou > 0) else V(0.0)
        dx_pos = vmul(w_pos, vsub(vmul(vmul(V(-ga), p), spn), om))
        dx_neg = vmul(w_neg, vadd(vmul(vmul(V(ga), vsub(one, p)), spp), p))
        dlog = vmul(vwhere(pos, dx_pos, dx_neg), k_cls)
        reg_on = pos & (k_reg.v != 0)
        d0 = vmul(k_reg, vadd(vdiv(V(-D["dil"]), ie), vdiv(V(1.0 - D["dil"]), ue)))
        d1 = vmul(k_reg, vadd(vdiv(V(-D["dir"]), ie), vdiv(V(1.0 - D["dir"]), ue)))
        d0, d1 = vwhere(reg_on, d0, V(np.zeros_like(x))), vwhere(reg_on, d1, V(np.zeros_like(x)))
        di = None
        if iou_stage:
            on = masked & (k_iou.v != 0)
            den2 = vmul(den, den)
            dt_de = vmul(V(D["me"]), vdiv(vsub(vmul(V(D["e_lt"]), den), vmul(inter, V(D["e_gt"]))), den2))
            dt_ds = vmul(V(D["ms"]), vdiv(vsub(vmul(V(-D["s_gt"]), den), vmul(inter, V(-D["s_lt"]))), den2))
            ks = vmul(k_iou, d)
            di = vmul(vmul(ks, pI), vsub(one, pI))
            di = vwhere(on, di, V(np.zeros_like(x)))
            dt = vneg(ks)
            its = vdiv(one, ts)
            add0, add1 = vmul(vmul(dt, dt_ds), vneg(its)), vmul(vmul(dt, dt_de), its)
            d0, d1 = vwhere(on, vadd(d0, add0), d0), vwhere(on, vadd(d1, add1), d1)

    gaps = []

    def total(val, want):
        want = np.asarray(want, dtype=np.float64)
        diff = np.abs(val.v - want)
        with np.errstate(all="ignore"):
            gaps.append(float(np.max(np.nan_to_num(np.where(diff == 0, 0.0, diff / val.e), nan=np.inf), initial=0.0)))
        return np.nan_to_num(val.e + diff, nan=np.inf)

    b6 = np.array([float(total(o, M["out6"][i])) for i, o in ((0, o0), (1, o1), (2, o2))] + [0.0, 0.0, float(total(o5, M["out6"][5]))])
    return dict(out6=b6, dlogits=total(dlog, M["dlogits"]), dreg=np.stack([total(d0, M["dreg"][:, 0]), total(d1, M["dreg"][:, 1])], 1),
                diou=None if di is None else total(di, M["diou"]), gap=max(gaps))


# ----------------------------------------------------------------------------------------------------------------------------------
# an fp32 evaluation in the kernels' order, and wrong ones
# ----------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("div_n_pos", "n_iou_divisor_dropped", "reg_tie_one_sided", "tiou_tie_one_sided", "clamp_clip0_only", "clamp_every_level",
           "clamp_no_grad_mask", "upper_clamp_mask_missing", "sl1_target_detached", "mx_lt_hi", "mn_ge_0", "alpha_on_negatives",
           "level_gt_row_start", "loc_no_half_stride", "gt_next_clip", "last_block_dropped", "tiou_no_eps", "sl1_no_half",
           "gt_truncated", "focal_log_p")


def _butterfly(v):
    """wave_sum(): v += shfl_xor(v, o) for o = 32 .. 1, as lane 0 sees it.  v: (..., 64) fp32."""
    n = v.shape[-1]
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def _block_sum(v):
    """block_sum5() of a 256-thread workgroup.  v: (nblk, 256) fp32 -> (nblk,)."""
    w = _butterfly(v.reshape(v.shape[0], THREADS // 64, 64))
    pad = np.zeros((v.shape[0], 64), dtype=F)
    pad[:, :w.shape[1]] = w
    return _butterfly(pad)


def _kernel_sum(terms, drop_last=False):
    """fcos_loss_fwd_partial_kernel's partial sums and loss_finalize's sum of them."""
    R = terms.shape[0]
    nblk = (R + THREADS - 1) // THREADS
    pad = np.zeros(nblk * THREADS, dtype=F)
    pad[:R] = terms
    part = _block_sum(pad.reshape(nblk, THREADS))
    if drop_last:
        part = part[:-1]
    k = (part.shape[0] + THREADS - 1) // THREADS
    pp = np.zeros(max(k, 1) * THREADS, dtype=F)
    pp[:part.shape[0]] = part
    lanes = np.zeros(THREADS, dtype=F)
    for row in pp.reshape(-1, THREADS):
        lanes = lanes + row
    return _block_sum(lanes[None])[0]


def _sp32(z):
    t = np.log1p(np.exp(-np.abs(z)))
    return np.where(z > 0, z + t, t).astype(F)


def emulate_fp32(levels, B, logits, reg, iou, gt, gamma, alpha, target_scale, iou_stage, g3=(1.0, 1.0, 1.0), mutant=None):
    """The kernels' statements one by one in numpy.float32 (no contraction), sums in the kernels' order; `mutant`: one of MUTANTS, a
    subtly wrong kernel.  dict(out6, labels, dlogits, dreg, diou), all fp32."""
    assert mutant is None or mutant in MUTANTS
    m = mutant
    lvl, b, t = rows_of(levels, B)
    R = lvl.shape[0]
    if m == "level_gt_row_start":         # `r > row_start[i]`: the first row of every later level falls to the level before it, as
        starts = np.cumsum([0] + [B * l[0] for l in levels])[:-1]       # its row B * L (the clip index is kept inside the batch)
        for i in range(1, len(levels)):
            r = starts[i]
            lvl[r], t[r], b[r] = i - 1, 0, B - 1
    st = np.array([l[1] for l in levels], dtype=F)[lvl]
    lo = np.array([l[2] for l in levels], dtype=F)[lvl]
    hi = np.array([l[3] for l in levels], dtype=F)[lvl]
    ga, al, ts = F(gamma), F(alpha), F(target_scale)
    one, zero = F(1), F(0)
    gt = np.asarray(gt)
    if m == "gt_truncated" and gt.dtype == np.float64:
        g = gt.astype(F)
        over = np.abs(g.astype(np.float64)) > np.abs(gt)
        g = np.where(over, np.nextafter(g, F(0)), g).astype(F)
    else:
        g = gt.astype(F)
    bb = (b + 1) % B if m == "gt_next_clip" else b
    gs, ge = g[bb, 0], g[bb, 1]
    x = np.asarray(logits, dtype=F).reshape(-1)
    reg = np.asarray(reg, dtype=F)
    pl, pr = reg[:, 0], reg[:, 1]
    gc, gr, gi = (F(v) for v in _g3(g3))
    with np.errstate(all="ignore"):
        loc = t.astype(F) * st + (zero if m == "loc_no_half_stride" else st * F(0.5))
        tl, tr = loc - gs * ts, ge * ts - loc
        mn, mx = np.minimum(tl, tr), np.maximum(tl, tr)
        pos = (mn >= 0 if m == "mn_ge_0" else mn > 0) & (mx >= lo) & (mx < hi if m == "mx_lt_hi" else mx <= hi)
        p = one / (one + np.exp(-x))
        om = one - p
        if m == "focal_log_p":
            f_pos, f_neg = -al * np.power(om, ga) * np.log(p), -(one - al) * np.power(p, ga) * np.log(one - p)
        else:
            f_pos, f_neg = al * np.power(om, ga) * _sp32(-x), (one - al) * np.power(p, ga) * _sp32(x)
        if m == "alpha_on_negatives":
            f_neg = al * np.power(p, ga) * _sp32(x)
        focal = np.where(pos, f_pos, f_neg).astype(F)
        i_reg = np.minimum(pr, tr) + np.minimum(pl, tl)
        u_reg = (tl + tr) + (pl + pr) - i_reg
        ioul = np.where(pos, -np.log((i_reg + F(EPS8)) / (u_reg + F(EPS8))), zero).astype(F)
        sl1 = np.zeros(R, dtype=F)
        masked = np.zeros(R, dtype=bool)
        if iou_stage:
            xi = np.asarray(iou, dtype=F).reshape(-1)
            ps, pe = (loc - pl) / ts, (loc + pr) / ts
            head = (t == 0) if m == "clamp_every_level" else (lvl == 0) & (t == 0)
            if m == "clamp_clip0_only":
                head = head & (b == 0)
            ms = np.where(head & ~((ps >= 0) & (ps <= 1)), zero, one)
            me = np.where(head & ~((pe >= 0) & ((pe <= 1) | (m == "upper_clamp_mask_missing"))), zero, one)
            if m == "upper_clamp_mask_missing":
                ms = np.where(head & ~(ps >= 0), zero, one)
            if m == "clamp_no_grad_mask":
                ms, me = np.ones(R, dtype=F), np.ones(R, dtype=F)
            ps = np.where(head, np.clip(ps, zero, one), ps)
            pe = np.where(head, np.clip(pe, zero, one), pe)
            imax, imin = np.minimum(pe, ge), np.maximum(ps, gs)
            umax, umin = np.maximum(pe, ge), np.minimum(ps, gs)
            inter, uni = np.maximum(imax - imin, zero), np.maximum(umax - umin, zero)
            den = uni if m == "tiou_no_eps" else uni + F(EPS6)
            tiou = inter / den
            masked = tiou > F(0.9)
            pI = one / (one + np.exp(-xi))
            d = pI - tiou
            ad = np.abs(d)
            sl1 = np.where(masked, np.where(ad < 1, (one if m == "sl1_no_half" else F(0.5)) * d * d, ad - F(0.5)), zero).astype(F)
        drop = m == "last_block_dropped"
        v = [_kernel_sum(a, drop) for a in (focal, ioul, sl1, pos.astype(F), masked.astype(F))]
        out = np.zeros(6, dtype=F)
        cls_div = v[3] if m == "div_n_pos" else v[3] + F(B)
        out[0] = v[0] / cls_div
        out[1] = v[1] / v[3] if v[3] > 0 else zero
        iou_div = one if m == "n_iou_divisor_dropped" else v[4]
        out[2] = (v[2] / iou_div if v[4] > 0 else zero)
        out[3], out[4] = v[3], v[4]
        out[5] = out[0] + out[1] + out[2]
        # backward
        n_pos, n_iou = out[3], out[4]
        k_cls = gc / cls_div
        k_reg = gr / n_pos if n_pos > 0 else zero
        k_iou = gi / iou_div if (iou_stage and n_iou > 0) else zero
        sp_n, sp_p = _sp32(-x), _sp32(x)
        if m == "focal_log_p":
            sp_n, sp_p = -np.log(p), -np.log(one - p)
        dx_pos = al * np.power(om, ga) * (-ga * p * sp_n - om)
        dx_neg = (al if m == "alpha_on_negatives" else one - al) * np.power(p, ga) * (ga * (one - p) * sp_p + p)
        dlogits = (np.where(pos, dx_pos, dx_neg) * k_cls).astype(F)
        if m == "reg_tie_one_sided":
            dil, dir_ = np.where(pl <= tl, one, zero), np.where(pr <= tr, one, zero)
        else:
            dil, dir_ = half(pl < tl, pl == tl).astype(F), half(pr < tr, pr == tr).astype(F)
        on = pos & (k_reg != 0)
        d0 = np.where(on, k_reg * (-dil / (i_reg + F(EPS8)) + (one - dil) / (u_reg + F(EPS8))), zero).astype(F)
        d1 = np.where(on, k_reg * (-dir_ / (i_reg + F(EPS8)) + (one - dir_) / (u_reg + F(EPS8))), zero).astype(F)
        diou = None
        if iou_stage:
            tie = zero if m == "tiou_tie_one_sided" else F(0.5)
            tie_lo = one if m == "tiou_tie_one_sided" else F(0.5)
            h = lambda lt, eq, tv: np.where(lt, one, np.where(eq, tv, zero)).astype(F)
            ok_i, ok_u = imax - imin >= 0, umax - umin >= 0
            di_de = np.where(ok_i, h(pe < ge, pe == ge, tie_lo), zero)
            di_ds = np.where(ok_i, -h(ps > gs, ps == gs, tie_lo), zero)
            du_de = np.where(ok_u, h(pe > ge, pe == ge, tie), zero)
            du_ds = np.where(ok_u, -h(ps < gs, ps == gs, tie), zero)
            dn = uni + F(EPS6)
            dt_de = me * (di_de * dn - inter * du_de) / (dn * dn)
            dt_ds = ms * (di_ds * dn - inter * du_ds) / (dn * dn)
            on = masked & (k_iou != 0)
            sl = np.where(ad < 1, (F(2) if m == "sl1_no_half" else one) * d, np.sign(d)).astype(F)
            diou = np.where(on, k_iou * sl * pI * (one - pI), zero).astype(F)
            if m != "sl1_target_detached":
                dt = -k_iou * sl
                d0 = np.where(on, d0 + dt * dt_ds * (-one / ts), d0).astype(F)
                d1 = np.where(on, d1 + dt * dt_de * (one / ts), d1).astype(F)
    assert out.dtype == dlogits.dtype == d0.dtype == F
    return dict(out6=out, labels=pos.astype(F), dlogits=dlogits, dreg=np.stack([d0, d1], 1), diou=diou)


def ratios(got, model, bound):
    """|got - model| / bound per output: dict(loss_cls, loss_reg, loss_iou, total, dlogits, dreg, diou), the largest of each; a count or
    label that differs gives inf under `exact`."""
    r = {}
    g6 = np.asarray(got["out6"], dtype=np.float64)
    for i, k in ((0, "loss_cls"), (1, "loss_reg"), (2, "loss_iou"), (5, "total")):
        r[k] = inside(g6[i], model["out6"][i], bound["out6"][i])
    for k in ("dlogits", "dreg", "diou"):
        r[k] = 0.0 if model[k] is None else inside(got[k], model[k], bound[k])
    same = np.array_equal(g6[3:5], model["out6"][3:5]) and (got.get("labels") is None or np.array_equal(got["labels"], model["labels"]))
    r["exact"] = 0.0 if same else np.inf
    return r


OUTPUTS = ("loss_cls", "loss_reg", "loss_iou", "total", "dlogits", "dreg", "diou")


# ----------------------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------------------
INF = 1e8
S3 = ((-1.0, 6.0), (5.6, 11.0), (11.0, INF))                      # the reference's sizes of interest
S4 = ((-1.0, 6.0), (5.6, 11.0), (11.0, 20.0), (20.0, INF))


def table(Ls, strides, sizes):
    return [(int(L), float(s), float(lo), float(hi)) for L, s, (lo, hi) in zip(Ls, strides, sizes)]


W3 = (0.7, 1.3, 2.1)
# name: dict(levels, B, stage, gt64, kind, g3, gamma, alpha, seed, paths: what the row is there for,
#            expect: dict(nblk, n_pos, n_iou, pos_levels, reg_ties, tiou_ties, clamps (ps < 0, ps > 1, pe < 0, pe > 1 at location 0)))
CASES = {
    "one_level_under_a_wave": dict(
        levels=table((23,), (1,), ((-1.0, INF),)), B=2, stage=1, gt64=False, kind="matched", g3=(None, 1.3, 2.1), seed=1,
        paths="nlevels = 1; total_rows < 64; g_cls absent; n_iou > 0 on positives",
        expect=dict(nblk=1, n_pos=12, n_iou=1, pos_levels=[0], reg_ties=0, tiou_ties=0, clamps=(2, 0, 0, 0), iou_on_negatives=0, mn_zero=0, mx_on_bound=0)),
    "two_levels_256_rows": dict(
        levels=table((43, 21), (1, 2), ((-1.0, 7.0), (7.0, INF))), B=4, stage=0, gt64=True, kind="random", g3=(0.7, None, 2.1), seed=2,
        paths="nlevels = 2; exactly 256 rows; stage 0 (diou not written); fp64 ground truth; g_reg absent; L no power of two",
        expect=dict(nblk=1, n_pos=18, n_iou=0, pos_levels=[0, 1], reg_ties=0, tiou_ties=0, clamps=(3, 0, 0, 0), iou_on_negatives=0, mn_zero=0, mx_on_bound=0)),
    "three_levels_257_rows_one_clip": dict(
        levels=table((147, 73, 37), (1, 2, 4), S3), B=1, stage=0, gt64=False, kind="random", g3=W3, seed=3,
        paths="nlevels = 3; 257 rows: a second block of one row; B = 1 (divisor n_pos + 1)",
        expect=dict(nblk=2, n_pos=5, n_iou=0, pos_levels=[1, 2], reg_ties=0, tiou_ties=0, clamps=(1, 0, 0, 0), iou_on_negatives=0, mn_zero=0, mx_on_bound=0)),
    "four_levels_ragged": dict(
        levels=table((37, 19, 10, 5), (1, 2, 4, 8), S4), B=13, stage=1, gt64=True, kind="matched", g3=W3, seed=4,
        paths="nlevels = 4; L (37, 19, 10, 5): level and clip boundaries inside waves; 923 rows: 4 blocks, ragged last; fp64 ground truth; "
              "n_iou > 0 on rows that are no positives",
        expect=dict(nblk=4, n_pos=49, n_iou=9, pos_levels=[0, 1, 2, 3], reg_ties=0, tiou_ties=0, clamps=(11, 0, 0, 0), iou_on_negatives=2, mn_zero=0, mx_on_bound=0)),
    "finalize_strides": dict(
        levels=table((1024, 512, 256), (1, 2, 4), S3), B=40, stage=1, gt64=False, kind="matched", g3=W3, seed=5,
        paths="71680 rows, 280 blocks: loss_finalize's loop takes a second turn",
        expect=dict(nblk=280, n_pos=173, n_iou=23, pos_levels=[0, 1, 2], reg_ties=0, tiou_ties=0, clamps=(35, 0, 0, 0), iou_on_negatives=4, mn_zero=0, mx_on_bound=0)),
    "no_positive": dict(
        levels=table((16, 8, 4), (1, 2, 4), S3), B=3, stage=1, gt64=False, kind="empty_gt", g3=W3, seed=6,
        paths="zero-length ground truth: n_pos = 0 and n_iou = 0 (loss_reg = loss_iou = 0, k_reg = k_iou = 0)",
        expect=dict(nblk=1, n_pos=0, n_iou=0, pos_levels=[], reg_ties=0, tiou_ties=0, clamps=(2, 0, 0, 0), iou_on_negatives=0, mn_zero=0, mx_on_bound=0)),
    "positives_without_iou_positives": dict(
        levels=table((37, 19, 10), (1, 2, 4), S3), B=3, stage=1, gt64=False, kind="random", g3=(2.1, 0.7, 1.3), seed=7,
        paths="n_iou = 0 with n_pos > 0 and a g_iou that is present; 198 rows",
        expect=dict(nblk=1, n_pos=16, n_iou=0, pos_levels=[0, 2], reg_ties=0, tiou_ties=0, clamps=(3, 0, 0, 0), iou_on_negatives=0, mn_zero=0, mx_on_bound=0)),
    "edges_f32": dict(
        levels=table((16, 8, 4), (1, 2, 4), S3), B=6, stage=1, gt64=False, kind="edges", g3=W3, seed=8,
        paths="exact by construction: ground truth on location centres (mn = 0) and on size bounds (mx = hi of level 0, mx = lo of "
              "level 2); reg = target on one side and on both; tIoU with pe = ge and with ps = gs; location 0 with ps < 0 alone, pe > 1 "
              "alone and both (gt = [0, 1], reg = (5, 40))",
        expect=dict(nblk=1, n_pos=29, n_iou=8, pos_levels=[0, 1, 2], reg_ties=6, tiou_ties=10, clamps=(5, 0, 0, 2), iou_on_negatives=3, mn_zero=6, mx_on_bound=2)),
    "edges_f64": dict(
        levels=table((16, 8, 4), (1, 2, 4), S3), B=6, stage=1, gt64=True, kind="edges", g3=W3, seed=8,
        paths="edges_f32 with fp64 ground truth a few 1e-10 off the fp32 values it rounds to: labels differ if the cast is skipped or "
              "truncates",
        expect=dict(nblk=1, n_pos=29, n_iou=8, pos_levels=[0, 1, 2], reg_ties=6, tiou_ties=10, clamps=(5, 0, 0, 2), iou_on_negatives=3, mn_zero=6, mx_on_bound=2)),
    "saturated_logits": dict(
        levels=table((37, 19, 10), (1, 2, 4), S3), B=4, stage=1, gt64=False, kind="saturated", g3=W3, seed=9,
        paths="logits of +-95 and +-120 on positives and on negatives (class and IoU logits)",
        expect=dict(nblk=2, n_pos=19, n_iou=2, pos_levels=[0, 1, 2], reg_ties=0, tiou_ties=0, clamps=(4, 0, 0, 0), iou_on_negatives=1, mn_zero=0, mx_on_bound=0)),
    "gamma_alpha": dict(
        levels=table((37, 19, 10), (1, 2, 4), S3), B=4, stage=1, gt64=True, kind="matched", g3=(0.7, 1.3, None), seed=10, gamma=1.5, alpha=0.4,
        paths="gamma = 1.5, alpha = 0.4; 264 rows: two blocks; g_iou absent with n_iou > 0 (read as 1 it would show in diou and dreg)",
        expect=dict(nblk=2, n_pos=17, n_iou=2, pos_levels=[0, 1, 2], reg_ties=0, tiou_ties=0, clamps=(4, 0, 0, 0), iou_on_negatives=0, mn_zero=0, mx_on_bound=0)),
}
SATURATED = (95.0, -95.0, 120.0, -120.0)
MARGIN_ULPS = 16            # no decision of a case sits within this many fp32 ulps of its threshold unless it sits ON it by construction


def _edges(levels, B, gt64):
    """Six clips on the (16, 8, 4) table; every quantity a multiple of 1/64 below 64, so every fp32 operation on the decision paths is
    exact.  Ground truth in units of 1/32 (gs S and ge S are integers or halves)."""
    assert [l[0] for l in levels] == [16, 8, 4] and B == 6
    S = 32.0
    gt = np.array([[0.0, 32.0],      # 0: location 0 clamped on both sides
                   [0.0, 8.0],       # 1: ps < 0 alone
                   [0.25, 32.0],     # 2: pe > 1 alone
                   [2.0, 8.5],       # 3: level 0, loc 2.5: tr = 6 = hi (positive, inclusive); ties with reg below
                   [2.5, 6.5],       # 4: level 0, loc 2.5: tl = 0 (mn = 0: no positive); loc 6.5: tr = 0
                   [1.0, 13.0]]) / S  # 5: level 2, loc 2: tr = 11 = lo (positive, inclusive); level 1, loc 1: tl = 0
    rng = np.random.default_rng(8)
    R = B * 28
    logits = rng.standard_normal(R).astype(F)
    iou = rng.standard_normal(R).astype(F)
    reg = (np.round(np.exp(0.5 * rng.standard_normal((R, 2))) * 128) / 64 + 0.015625).astype(F)     # multiples of 1/64: fp32-exact paths
    row = lambda lvl, b, t: [0, 6 * 16, 6 * 16 + 6 * 8][lvl] + b * [16, 8, 4][lvl] + t
    reg[row(0, 0, 0)] = (5.0, 40.0)           # ps = -4.5 / 32 -> 0 = gs, pe = 40.5 / 32 -> 1 = ge: both masks 0, both tIoU ties
    reg[row(0, 1, 0)] = (3.0, 7.25)           # ps < 0 -> 0 = gs (tie), pe = 7.75 / 32 < ge: tIoU 0.97
    reg[row(0, 2, 0)] = (0.125, 40.0)         # ps = 0.375 / 32 > gs, pe > 1 -> 1 = ge (tie): tIoU 0.996
    reg[row(0, 3, 3)] = (1.5, 4.75)           # loc 3.5: tl = 1.5 = pl (one side), pr < tr = 5;  ps = gs (tie), pe = 8.25 / 32 < ge
    reg[row(0, 3, 4)] = (2.5, 4.0)            # loc 4.5: tl = 2.5, tr = 4: both sides; ps = gs and pe = ge
    reg[row(0, 3, 5)] = (3.25, 3.0)           # loc 5.5: tr = 3 = pr (the other side), pl < tl = 3.5; pe = ge
    reg[row(2, 5, 0)] = (1.0, 11.0)           # level 2, loc 2: both sides on a positive with mx = lo
    reg[row(1, 1, 0)] = (1.5, 6.75)           # level 1, t = 0: ps = -0.5 / 32 < 0 and NOT clamped (tIoU 0.91): only level 0 is
    gt = gt.astype(np.float64)
    if gt64:
        # off the fp32 value by less than half an fp32 ulp, TOWARDS zero for starts (the start moves down: a row with tl = 0 in fp32
        # has tl > 0 without the cast) and AWAY for ends; truncation of an end that lies above lands on it, of a start below it one
        # ulp lower: the labels of the tl = 0 rows turn
        gt = gt * (1.0 + np.array([-3e-10, 3e-10]))[None, :]
        assert np.array_equal(gt.astype(F).astype(np.float64) * S, np.round(gt * S * 64) / 64)
    else:
        gt = gt.astype(F)
    return logits, reg, iou, gt


def _random(levels, B, seed, kind, gt64):
    rng = np.random.default_rng(seed)
    Ls = [l[0] for l in levels]
    R = B * sum(Ls)
    lvl, b, t = rows_of(levels, B)
    logits = rng.standard_normal(R).astype(F)
    iou = rng.standard_normal(R).astype(F)
    reg = (np.exp(rng.standard_normal((R, 2))) * (1.5 + lvl)[:, None]).astype(F)
    length = np.exp(rng.uniform(np.log(0.06), np.log(0.95), B))
    start = rng.uniform(0, 1, B) * (1 - length)
    gt = np.stack([start, start + length], 1)
    if kind == "empty_gt":
        gt[:, 1] = gt[:, 0]
    if len(levels) == 4:                           # one long ground truth, so that the last level owns positives too
        gt[1] = (0.05, 0.95)
    if kind in ("matched", "saturated"):           # one prediction of every other clip, on level 0, within 1.5 % a side of the ground
        span = sum(l[0] * l[1] for l in levels[:1])        # truth: tIoU ~ 0.97; the other clips keep their (longer) random ground truth
        for c in range(0, B, 2):
            tt = (3 + 5 * c) % Ls[0]
            r = c * Ls[0] + tt
            loc = (tt + 0.5) * levels[0][1]
            s, e = (loc - float(reg[r, 0])) / 32.0, min((loc + float(reg[r, 1])) / 32.0, span / 32.0)
            if s < 0:
                reg[r, 0] = F(loc * 0.5)
                s = (loc - float(reg[r, 0])) / 32.0
            gt[c] = (s + 0.015 * (e - s), e - 0.015 * (e - s))
    gt = gt * (1.0 + 1e-9 * rng.standard_normal(gt.shape)) if gt64 else gt.astype(F)
    if kind == "empty_gt":
        gt[:, 1] = gt[:, 0]
    return logits, reg, iou, gt


def _near(levels, B, reg, gt, stage):
    """(rows whose reg decides a decision within MARGIN_ULPS of its threshold without sitting on it, clips whose gt does)."""
    D = decide(levels, B, reg, gt, 32.0, stage)
    reg = np.asarray(reg, dtype=F)
    sp = lambda *a: MARGIN_ULPS * np.spacing(np.maximum.reduce([np.abs(v).astype(F) for v in a]).astype(F))
    close = lambda a, b, *scale: (a != b) & (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= sp(a, b, *scale))
    zero = np.zeros_like(D["mn"])
    by_gt = close(D["mn"], zero, D["loc"], D["gs"] * F(32), D["ge"] * F(32)) | close(D["mx"], D["lo"]) | close(D["mx"], D["hi"])
    by_reg = close(reg[:, 0], D["tl"]) | close(reg[:, 1], D["tr"])
    if stage:
        by_reg |= close(D["tiou"], np.full_like(D["tiou"], F(0.9)), np.ones_like(D["tiou"]))
        by_reg |= close(D["ps"], D["gs"], np.ones_like(D["ps"])) | close(D["pe"], D["ge"], np.ones_like(D["pe"]))
        one = np.ones_like(D["loc"])                        # the clamp at location 0: the unclamped ps and pe against 0 and 1
        raw_s, raw_e = (D["loc"] - reg[:, 0]) / F(32), (D["loc"] + reg[:, 1]) / F(32)
        by_reg |= D["head"] & (close(raw_s, zero, one) | close(raw_s, one) | close(raw_e, zero, one) | close(raw_e, one))
    return np.nonzero(by_reg)[0], np.unique(D["b"][by_gt])


_built = {}


def build(name):
    """dict(name, levels, B, logits (R,), reg (R, 2), iou (R,), gt (B, 2), gamma, alpha, target_scale, iou_stage, g3) of a row of CASES,
    built once.  Rows and clips that _near() finds are nudged (reg by 1 / 32 of itself, gt by 2^-10) until none is left; the exact
    cases are built clear of that and nothing of theirs is moved."""
    if name in _built:
        return _built[name]
    c = CASES[name]
    levels, B = c["levels"], c["B"]
    if c["kind"] == "edges":
        logits, reg, iou, gt = _edges(levels, B, c["gt64"])
    else:
        logits, reg, iou, gt = _random(levels, B, c["seed"], c["kind"], c["gt64"])
        for _ in range(20):
            rows, clips = _near(levels, B, reg, gt, c["stage"])
            if not len(rows) and not len(clips):
                break
            reg[rows] = reg[rows] * F(1.03125)
            gt[clips] = gt[clips] + gt.dtype.type(2.0 ** -10)
        if c["kind"] == "saturated":
            D = decide(levels, B, reg, gt, 32.0, c["stage"])
            posr, negr = np.nonzero(D["pos"])[0], np.nonzero(~D["pos"])[0]
            assert len(posr) >= 4 and len(negr) >= 4
            for i, v in enumerate(SATURATED):
                logits[posr[i]], logits[negr[3 * i]] = v, v
                iou[posr[i]], iou[negr[3 * i]] = -v, v
            mk = np.nonzero(D["masked"])[0]
            iou[mk[0]], iou[mk[1]] = 95.0, -120.0
    out = dict(name=name, levels=levels, B=B, logits=logits, reg=reg, iou=iou, gt=gt, gamma=c.get("gamma", 2.0), alpha=c.get("alpha", 0.25),
               target_scale=32.0, iou_stage=c["stage"], g3=c["g3"])
    for k in ("logits", "reg", "iou", "gt"):
        out[k].setflags(write=False)
    _built[name] = out
    return out


def args_of(case):
    """The positional arguments of loss_model / loss_bound / emulate_fp32."""
    return (case["levels"], case["B"], case["logits"], case["reg"], case["iou"], case["gt"], case["gamma"], case["alpha"],
            case["target_scale"], case["iou_stage"], case["g3"])


_reference = {}


def reference(name):
    """(case, model, bound), computed once per process and shared by the tests; the arrays are read-only."""
    if name not in _reference:
        case = build(name)
        model = loss_model(*args_of(case))
        _reference[name] = (case, model, loss_bound(*args_of(case), model=model))
    return _reference[name]


def observed(case, model):
    """What test_case_table_covers_what_it_says compares with CASES[...]['expect']."""
    D = model["dec"]
    pos, masked = D["pos"], D["masked"]
    reg = np.asarray(case["reg"])
    lo_s, hi_s, lo_e, hi_e = D["clamp"]
    return dict(nblk=nblocks(case["levels"], case["B"]), n_pos=int(pos.sum()), n_iou=int(masked.sum()),
                pos_levels=sorted(set(D["level"][pos].tolist())),
                reg_ties=int(((reg[:, 0] == D["tl"]) & pos).sum() + ((reg[:, 1] == D["tr"]) & pos).sum()),
                tiou_ties=int(((D["ps"] == D["gs"]) & masked).sum() + ((D["pe"] == D["ge"]) & masked).sum()),
                clamps=tuple(int(v.sum()) for v in (lo_s, hi_s, lo_e, hi_e)),
                iou_on_negatives=int((masked & ~pos).sum()), mn_zero=int((D["mn"] == 0).sum()),
                mx_on_bound=int((((D["mx"] == D["hi"]) | (D["mx"] == D["lo"])) & (D["mn"] > 0)).sum()))
