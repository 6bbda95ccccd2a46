"""fp64 model, exact data and error bounds for the 1-2 channel output heads (csrc/heads.hip: cls_logits, exp(scale_l * bbox_pred), the
last iou_scores conv), shared by tests/test_heads_ref_cpu.py (which checks this file without a GPU) and tests/test_heads_gpu.py.

Layout.  A head reads `nl` pyramid levels, level l a channels-last (B, L_l, C) tensor.  Its outputs live in the level-concatenated row
space: level-first, clip-major, row = start_l + b * L_l + t, R = B * sum(L_l) rows.  out / z / dout are (R, N); W is the nn.Conv1d
weight (N, C, taps), taps in {1, 3}, zero padding (taps - 1) / 2 per clip.

The model.  tap_pairs lists, tap by tap, the (output row, input row) pairs of the convolution: a loop over level, clip and position that
keeps a tap exactly when its source position lies inside the clip.  forward_ref, backward_ref are sums over those pairs in float64:

    z[r, n]   = bias[n] + sum_tap sum_c X[src(r, tap), c] W[n, c, tap]          out = z            (linear)
                                                                                 out = exp(s_l z)  (exp mode, s_l the level's scale)
    dz        = dout (linear)  |  s_l out dout (exp mode: `out` is an ARGUMENT, so a test can hand in the device's own)
    dX[src]  += dz[r, n] W[n, :, tap]      dW[n, :, tap] += dz[r, n] X[src]      dbias[n] = sum_r dz[r, n]
    dscale_l  = sum over the level's rows and n of z out dout

and next to every sum the sum of the absolute values of its terms (`*_abs`), which the bounds below are made of.
`fault=` switches ONE deliberate error on (FAULTS); tests/test_heads_ref_cpu.py uses them to show on which geometry the data can tell
right from wrong.

The data (exact_case).  X = k / 8 in [-2, 2] (exact in bf16), bias = k / 4, dout = integers in [-3, 3], the old values of the accumulate
modes = k / 4, W = k / 4 in [-1, 1] (linear) or k / 64 in [-1/16, 1/16] (exp mode; per-level scales are distinct values out of
{0.75, 1, 1.25, 1.5}).  Every term of z is then a multiple of q = 1/32 (1/512 in exp mode), every term of the linear-mode dX of 1/4, of
dW of 1/8, of dbias of 1/4, and exact_case asserts  sum |terms| < 2^24 q  for every output: every partial sum, in ANY order, is an integer
multiple of q below 2^24 q, so it is a float32 number and no fp32 addition or fma rounds.

The bounds.  u = 2^-24, gamma_k = k u / (1 - k u) (k roundings compound to at most gamma_k).

  linear mode: 0.  out, dW, dbias and the fp32 dX equal the float64 value bit for bit, with and without accumulation (the old values are
      further exact terms).  A bf16 dX is that exact fp32 value stored with one (bf16_t) conversion: the float64 value rounded to
      nearest-even.
  exp mode, z: 0, as above.
  exp mode, out = expf(fl(s z)):  |out - exp(s z)| <= (|s z| + E + 1) u exp(s z).                                            (out_bound)
      fl(s z) = s z (1 + d), |d| <= u, moves the ARGUMENT by at most |s z| u, i.e. the result by the factor exp(|s z| u) ~ 1 + |s z| u;
      expf itself is off by at most E u relative (E = EXPF_E); the product of the two factors is 1 + (|s z| + E) u + second-order terms,
      which with |s z| <= 30 are below 1e-12 u and far inside the `+ 1`.
  exp mode, gradients: compared with backward_ref fed the DEVICE's out (already checked), so only the backward arithmetic is in them.
      dz = fl(fl(s out) dout) or fl(s fl(out dout)): two roundings.
      dX: N taps terms dz w, each entering through one fma: <= N taps + 2 roundings per term (accumulate: the old value is one more
          term of the same chain)                       |dX~ - dX| <= gamma_{N taps + 3} sum |dz w|   (+ half a bf16 ulp in bf16)
      dW: one term per row and tap, an fma each, then additions in some tree: a term passes at most R roundings on top of dz's two; any
          summation order                               |dW~ - dW| <= gamma_{R + 2} sum |dz x|
      dbias: R terms dz, R - 1 additions                |db~ - db| <= gamma_{R + 1} sum |dz|
      dscale_l: N M_l terms fl(fl(z out) dout)          |ds~ - ds| <= gamma_{N M_l + 2} sum |z out dout|
      accumulate_dw adds the old value as one more term and one more addition: k + 1 in the last three (sum_bound(acc=1)).
"""
import zlib

import torch

U = 2.0 ** -24
# expf's error in units of u.  Assumed: 1 ulp (the ROCm packages carry no copy of the HIP math documentation to take the figure from;
# DESIGN.md section 4); one fp32 ulp is at most 2 u relative.
EXPF_E = 2.0
ROWS_PER_WAVE, ROWS_PER_FWD_WG, ROWS_PER_W_WG = 8, 32, 64        # heads.hip: HEAD_RPW, 4 waves, x HEAD_WRUNS
MAX_GROUPS = 4

GEOMETRIES = {
    "one_run": (1, (8,)),                    # one window run that is a whole sequence; r0 + 8 == total_rows
    "short_tail": (1, (11,)),                # a window run, then 3 rows on the general path with rows past the end
    "wrap": (8, (3,)),                       # window runs across 3-4 clips: t wraps up to three times
    "unit": (3, (1, 1, 1)),                  # L = 1: only the centre tap is live; a run over three levels
    "ragged3": (3, (50, 25, 13)),            # level boundaries at rows 150 and 225, straddling runs, L % 8 != 0
    "four": (2, (16, 8, 4, 2)),              # four levels, 60 rows; a window run with L = 4; a last run of 4 live rows
    "many_blocks": (10, (255, 127, 65)),     # 4470 rows = 70 weight-gradient row blocks, the last one ragged
}

# fault -> the geometries on which it must show (tests/test_heads_ref_cpu.py); "chan64" needs C > 64 vectors, "scale0" exp mode,
# "dx0" accumulate_dx, "swap" N = 2
_ALL = ("one_run", "short_tail", "wrap", "unit", "ragged3", "four", "many_blocks")
FAULTS = {
    "noclip": ("wrap", "unit", "ragged3", "four", "many_blocks"),          # no mask at clip boundaries
    "nolevel": ("unit", "ragged3", "four", "many_blocks"),                # no mask at level boundaries
    "lastrow": _ALL,                                         # last row dropped
    "chan64": ("ragged3", "four"),                                        # channels from 64 * VN upward dropped
    "blk64": ("many_blocks",),                                            # row blocks >= 64 dropped from the dW / dbias / dscale sums
    "scale0": ("unit", "ragged3", "four", "many_blocks"),                 # level 0's scale used for every level
    "dx0": _ALL,                                             # old dX ignored under accumulate
    "swap": _ALL,                                            # the two outputs of an N = 2 head swapped
}


def geometry(name):
    """-> (B, Ls)"""
    return GEOMETRIES[name]


def gamma_n(n):
    return n * U / (1.0 - n * U)


def vn_of(dtype):
    """channels per 16-byte vector"""
    return 8 if dtype == torch.bfloat16 else 4


def half_ulp(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else U


def total_rows(B, Ls):
    return B * sum(Ls)


def level_starts(B, Ls):
    out, r = [], 0
    for L in Ls:
        out.append(r)
        r += B * L
    return out


def row_levels(B, Ls):
    """(R,) long: the level of every row"""
    return torch.cat([torch.full((B * L,), l, dtype=torch.long) for l, L in enumerate(Ls)])


def flat(xs):
    """per-level (B, L, C) -> (R, C)"""
    return torch.cat([x.reshape(-1, x.shape[-1]) for x in xs])


def split(rows, B, Ls):
    """(R, C) -> per-level (B, L, C)"""
    out, r = [], 0
    for L in Ls:
        out.append(rows[r:r + B * L].reshape(B, L, -1))
        r += B * L
    return out


def tap_pairs(B, Ls, taps, fault=None):
    """-> per tap (dst, src): output row dst reads input row src = dst + tap - pad through that tap.  A tap is kept when its source
    position t + tap - pad lies inside the clip [0, L).  fault "noclip" keeps it whenever the source row lies in the same level,
    "nolevel" whenever it lies in ANOTHER level (still dropped between the clips of one level and outside the row space)."""
    pad = (taps - 1) // 2
    R = total_rows(B, Ls)
    out = []
    for tap in range(taps):
        off = tap - pad
        dst = []
        for start, L in zip(level_starts(B, Ls), Ls):
            for b in range(B):
                for t in range(L):
                    r = start + b * L + t
                    ok = 0 <= t + off < L
                    if not ok and fault in ("noclip", "nolevel"):
                        in_level = 0 <= b * L + t + off < B * L
                        ok = in_level if fault == "noclip" else (not in_level and 0 <= r + off < R)
                    if ok:
                        dst.append(r)
        dst = torch.tensor(dst, dtype=torch.long)
        out.append((dst, dst + off))
    return out


def _row_scale(scales, B, Ls, fault):
    s = scales.double()
    if fault == "scale0":
        s = s[:1].expand(len(Ls))
    return s[row_levels(B, Ls)][:, None]


def _cut(C, vn, fault):
    return min(C, 64 * vn) if fault == "chan64" else C


def forward_ref(xs, W, bias, scales=None, fault=None, vn=4):
    """xs: per-level (B, L, C); W (N, C, taps); bias (N,); scales (nl,) switches exp mode on.
    -> dict(z, z_abs, out [, sz]) in float64, (R, N); z_abs = |bias| + sum |x| |w|."""
    B, Ls = xs[0].shape[0], tuple(x.shape[1] for x in xs)
    X, W, bias = flat(xs).double(), W.double(), bias.double()
    R, (N, C, taps) = X.shape[0], W.shape
    cut = _cut(C, vn, fault)
    z = bias[None, :].repeat(R, 1)
    za = bias.abs()[None, :].repeat(R, 1)
    for tap, (dst, src) in enumerate(tap_pairs(B, Ls, taps, fault)):
        z.index_add_(0, dst, X[src, :cut] @ W[:, :cut, tap].t())
        za.index_add_(0, dst, X[src, :cut].abs() @ W[:, :cut, tap].abs().t())
    r = dict(z=z, z_abs=za)
    if scales is not None:
        r["sz"] = _row_scale(scales, B, Ls, fault) * z
        r["out"] = torch.exp(r["sz"])
    else:
        r["out"] = z.clone()
    if fault == "lastrow":
        r["z"][R - 1] = 0.0
        r["out"][R - 1] = 0.0
    if fault == "swap":
        r["z"], r["out"] = r["z"].flip(1), r["out"].flip(1)
    return r


def backward_ref(xs, W, dout, out=None, z=None, scales=None, dx0=None, dW0=None, db0=None, ds0=None, fault=None, vn=4):
    """dout (R, N); exp mode (scales given) needs out and z.  dx0 (per level) / dW0, db0, ds0: the old values of accumulate_dx /
    accumulate_dw.  -> dict(dz, dX, dX_abs (per level), dW, dW_abs (N, C, taps), dbias, dbias_abs (N,), dscale, dscale_abs (nl,))."""
    B, Ls = xs[0].shape[0], tuple(x.shape[1] for x in xs)
    X, W, dout = flat(xs).double(), W.double(), dout.double()
    R, (N, C, taps) = X.shape[0], W.shape
    cut = _cut(C, vn, fault)
    if fault == "swap":
        dout = dout.flip(1)
    dz = dout if scales is None else _row_scale(scales, B, Ls, fault) * out.double() * dout
    keep = torch.ones(R, 1, dtype=torch.float64)    # the rows the weight / bias / scale sums see
    if fault == "lastrow":
        keep[R - 1] = 0.0
    if fault == "blk64":
        keep[64 * ROWS_PER_W_WG:] = 0.0
    dzw = dz * keep
    dX, dXa = torch.zeros(R, C, dtype=torch.float64), torch.zeros(R, C, dtype=torch.float64)
    dW, dWa = torch.zeros_like(W), torch.zeros_like(W)
    for tap, (dst, src) in enumerate(tap_pairs(B, Ls, taps, fault)):
        dX[:, :cut].index_add_(0, src, dz[dst] @ W[:, :cut, tap])
        dXa[:, :cut].index_add_(0, src, dz[dst].abs() @ W[:, :cut, tap].abs())
        dW[:, :cut, tap] = dzw[dst].t() @ X[src, :cut]
        dWa[:, :cut, tap] = dzw[dst].abs().t() @ X[src, :cut].abs()
    if fault == "lastrow":
        dX[R - 1], dXa[R - 1] = 0.0, 0.0
    if dx0 is not None and fault != "dx0":
        dX, dXa = dX + flat(dx0).double(), dXa + flat(dx0).double().abs()
    db, dba = dzw.sum(0), dzw.abs().sum(0)
    r = dict(dz=dz)
    if scales is not None:
        term = z.double() * out.double() * dout * keep
        lv = row_levels(B, Ls)
        ds = torch.zeros(len(Ls), dtype=torch.float64).index_add_(0, lv, term.sum(1))
        dsa = torch.zeros(len(Ls), dtype=torch.float64).index_add_(0, lv, term.abs().sum(1))
        if ds0 is not None:
            ds, dsa = ds + ds0.double(), dsa + ds0.double().abs()
        r.update(dscale=ds, dscale_abs=dsa)
    if dW0 is not None:
        dW, dWa = dW + dW0.double(), dWa + dW0.double().abs()
    if db0 is not None:
        db, dba = db + db0.double(), dba + db0.double().abs()
    r.update(dX=split(dX, B, Ls), dX_abs=split(dXa, B, Ls), dW=dW, dW_abs=dWa, dbias=db, dbias_abs=dba)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid(g, shape, lo, hi, step):
    """multiples of `step` in [lo, hi], float64"""
    return torch.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape, generator=g).double() * step


def exact_case(geometry_name, C, N, taps, exp, dtype, seed=0):
    """-> dict(name, B, Ls, R, C, N, taps, exp, dtype, xs, W, bias, scales|None, dout, dx0, dW0, db0, ds0|None), all float64 on the CPU.
    Asserts what the module docstring promises: operands exact in `dtype`, every sum's absolute terms below 2^24 quanta (z always;
    dX, dW, dbias in linear mode, with the old values of the accumulate modes as further terms) and max |s z| <= 30 in exp mode."""
    B, Ls = geometry(geometry_name)
    assert len(Ls) <= MAX_GROUPS and N in (1, 2) and taps in (1, 3) and C % vn_of(dtype) == 0
    g = torch.Generator().manual_seed(1000003 * seed + zlib.crc32(("%s/%d/%d/%d/%d" % (geometry_name, C, N, taps, exp)).encode()) % 999983)
    R = total_rows(B, Ls)
    xs = [_grid(g, (B, L, C), -2.0, 2.0, 0.125) for L in Ls]
    bias = _grid(g, (N,), -1.0, 1.0, 0.25)
    dout = _grid(g, (R, N), -3.0, 3.0, 1.0)
    dx0 = [_grid(g, (B, L, C), -2.0, 2.0, 0.25) for L in Ls]
    dW0 = _grid(g, (N, C, taps), -2.0, 2.0, 0.25)
    db0 = _grid(g, (N,), -2.0, 2.0, 0.25)
    if exp:
        W = _grid(g, (N, C, taps), -1.0 / 16, 1.0 / 16, 1.0 / 64)
        scales = torch.tensor([0.75, 1.0, 1.25, 1.5], dtype=torch.float64)[torch.randperm(4, generator=g)][:len(Ls)].clone()
        ds0 = _grid(g, (len(Ls),), -2.0, 2.0, 0.25)
    else:
        W = _grid(g, (N, C, taps), -1.0, 1.0, 0.25)
        scales, ds0 = None, None
    for t in xs + dx0:
        assert torch.equal(t.to(dtype).double(), t), "activations and old gradients must be exact in the compute type"
    limit = 2.0 ** 24
    f = forward_ref(xs, W, bias, scales)
    assert float(f["z_abs"].max()) < limit * (1.0 / 512 if exp else 1.0 / 32), "a partial sum of z may need more than 24 bits"
    if exp:
        assert float(f["sz"].abs().max()) <= 30.0, "exp would overflow or flush"
    else:
        b = backward_ref(xs, W, dout, dx0=dx0, dW0=dW0, db0=db0)
        assert max(float(a.max()) for a in b["dX_abs"]) < limit / 4, "a partial sum of dX may need more than 24 bits"
        assert float(b["dW_abs"].max()) < limit / 8, "a partial sum of dW may need more than 24 bits"
        assert float(b["dbias_abs"].max()) < limit / 4, "a partial sum of dbias may need more than 24 bits"
    return dict(name=geometry_name, B=B, Ls=Ls, R=R, C=C, N=N, taps=taps, exp=bool(exp), dtype=dtype, xs=xs, W=W, bias=bias,
                scales=scales, dout=dout, dx0=dx0, dW0=dW0, db0=db0, ds0=ds0)


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds (module docstring)
# ---------------------------------------------------------------------------------------------------------------------------------
def out_bound(sz):
    """exp mode: |out - exp(s z)| <= (|s z| + E + 1) u exp(s z)"""
    return (sz.abs() + EXPF_E + 1.0) * U * torch.exp(sz)


def dx_bound(dX_abs, dX, N, taps, dtype):
    """exp mode: gamma_{N taps + 3} sum |dz w|, plus half a bf16 ulp of the result in bf16"""
    b = gamma_n(N * taps + 3) * dX_abs
    return b + half_ulp(dtype) * (dX.abs() + b) if dtype == torch.bfloat16 else b


def sum_bound(abs_sum, k, acc=0):
    """exp mode: gamma_k sum |terms| with k = R + 2 (dW), R + 1 (dbias), N M_l + 2 (dscale); acc = 1 under accumulate_dw"""
    return gamma_n(k + acc) * abs_sum


def fp32_sum_any_order(terms, seed):
    """float32 sum of `terms` (T, ...) over dim 0 in a random order, one addition at a time"""
    perm = torch.randperm(terms.shape[0], generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(terms.shape[1:], dtype=torch.float32)
    for i in perm.tolist():
        acc = acc + terms[i].float()
    return acc


def differs(a, b, bound=0.0):
    """does any element of a leave b by more than its bound?  (how a GPU test would see a fault)"""
    return bool(((a.double() - b.double()).abs() > bound).any())


def rne(x, dtype):
    """float64 (exact in fp32) -> `dtype`, one rounding to nearest-even, back in float64"""
    return x.float().to(dtype).double()

