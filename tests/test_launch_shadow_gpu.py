"""The shadow step: every GEMM launch of a real training step checked on its own inputs against the float64 launch model
(tests/launch_ref.py), at the configured shapes, with default tuning (no drn_tune calls) on the kernels the library picks.

The eager step (red.zero(), forward, backward, red.finish(), opt.step()) runs with these drn_amd.ops functions wrapped:
gemm_desc / wgrad_desc (remember which tensors and arguments a descriptor was made from), gemm_nt, gemm_wgrad,
gemm_wgrad_multi, skinny_group, outer_wgrad (synchronise, clone the inputs, fill the written region with NaN, launch,
synchronise, compare every output), wgrad_reduce_pending (compare the weight gradients whose reduce was deferred into that
launch) and conv_bn_train (off by default: must not launch unchecked).  Descriptor fields are raw pointers; they are read
back as tensors through the storages of the tensors the step handed to the library (ops._p).  Two steps run: the second one
reads the weight copies the optimizer kernels and repack_all refreshed, and every cached copy a launch reads is compared with
a fresh permute + cast of its parameters.  After step 1 the optimizer is compared with torch's clip_grad_norm_ + Adam fed the
same gradients.  One line per launch is printed (run with -s): tag, kernel kind, M/N/K, max err/bound, rel-L2."""
import collections

import pytest
import torch

import launch_ref as LR

pytestmark = pytest.mark.gpu

KIND_NAMES = {0: "TILE128", 1: "TILE256", 2: "W4", 3: "W4C", 4: "W4H"}
NAN = float("nan")


class Memory(object):
    """Device pointers -> tensor views, through the storages of every tensor whose pointer went to the library this step."""

    def __init__(self):
        self.st = {}

    def add(self, t):
        if t is not None and torch.is_tensor(t) and t.is_cuda:
            s = t.untyped_storage()
            self.st[s.data_ptr()] = (s, t.device)

    def view(self, ptr, dtype, shape, strides):
        ptr = int(ptr)
        es = torch.empty((), dtype=dtype).element_size()
        ext = (1 + sum((n - 1) * st for n, st in zip(shape, strides))) * es if all(n > 0 for n in shape) else 0
        for base, (s, dev) in self.st.items():
            if base <= ptr and ptr + ext <= base + s.nbytes():
                assert (ptr - base) % es == 0
                raw = torch.empty(0, dtype=torch.uint8, device=dev)
                raw.set_(s, 0, (s.nbytes(),), (1,))
                off = (ptr - base) // es
                flat = raw[:(s.nbytes() // es) * es].view(dtype)
                return flat.as_strided(shape, strides, off)
        raise AssertionError("pointer 0x%x (+%d bytes) is not inside any tensor the step handed to the library" % (ptr, ext))

    def clear(self):
        self.st.clear()


def cached_copies(store):
    """Every cached re-laid weight copy of a model's WeightCopies: [(buffer, function giving its fresh value, name)]."""
    out = []
    for key, (ver, buf, ref) in store.pack.items():
        w = ref()
        if w is not None:
            w3 = w.detach().unsqueeze(-1) if w.dim() == 2 else w.detach()
            out.append((buf, lambda w3=w3, perm=key[2], dt=buf.dtype: w3.permute(*perm).to(dt), "packed perm=%s" % (key[2],)))
    for key, (ver, buf, refs) in store.pstack.items():
        ps = [r() for r in refs]
        if all(p is not None for p in ps):
            perm = key[1]
            out.append((buf, lambda ps=ps, perm=perm, dt=buf.dtype: torch.cat([p.detach().permute(*perm) for p in ps],
                                                                               0 if perm[0] == 0 else 2).to(dt), "pstack perm=%s" % (perm,)))
    for key, (ver, buf, refs) in store.stack.items():
        ps = [r() for r in refs]
        if any(p is None for p in ps):
            continue
        if key[0] == "t":
            out.append((buf, lambda ps=ps: torch.cat([p.detach().t() for p in ps], 1), "stacked_t"))
        else:
            out.append((buf, lambda ps=ps, tail=tuple(buf.shape[1:]): torch.cat(
                [p.detach().reshape(p.shape[0], *tail) if p.dim() > 1 else p.detach() for p in ps], 0), "stacked"))
    return out


class Shadow(object):
    def __init__(self, monkeypatch, model, dtype, verbose=True):
        import drn_amd.ops as ops
        from drn_amd import _lib
        self.ops, self.lib, self.model, self.dtype = ops, _lib.lib(), model, dtype
        self.mem = Memory()
        self.made = {}                 # id(descriptor) -> (descriptor, the tensors / arguments it was made from)
        self.kinds = collections.Counter()
        self.lines = []
        self.checked_timed = 0         # launches checked that ops._timed records (gemm_nt / gemm_wgrad / gemm_wgrad_multi)
        self.checked_other = 0         # skinny_group / outer_wgrad launches checked
        self.pending = []              # (tag, dW, Expect) of weight gradients whose reduce was deferred
        self.dw_final = []             # (tag, gradient, Expect) re-checked at the end of finish()
        self.copies_checked = 0
        self.step_no = 0
        self.verbose = verbose
        real = dict((n, getattr(ops, n)) for n in ("_p", "gemm_desc", "wgrad_desc", "gemm_nt", "gemm_wgrad", "gemm_wgrad_multi",
                                                      "wgrad_reduce_pending", "skinny_group", "outer_wgrad", "conv_bn_train"))
        self.real = real
        mem = self.mem

        def _p(t):
            mem.add(t)
            return real["_p"](t)

        def gemm_desc(*a, **kw):
            d = real["gemm_desc"](*a, **kw)
            self.made[id(d)] = (d, a, kw)
            return d

        def wgrad_desc(*a, **kw):
            d = real["wgrad_desc"](*a, **kw)
            self.made[id(d)] = (d, a, kw)
            return d

        def conv_bn_train(descs, levels, dtype, relu=True, up_group=None):
            ran = real["conv_bn_train"](descs, levels, dtype, relu=relu, up_group=up_group)
            assert not ran, "the one-launch conv->BN kernel ran: its GEMM is not checked by this test (DRN_BN_FUSE is off by default)"
            return ran

        monkeypatch.setattr(ops, "_p", _p)
        monkeypatch.setattr(ops, "gemm_desc", gemm_desc)
        monkeypatch.setattr(ops, "wgrad_desc", wgrad_desc)
        monkeypatch.setattr(ops, "gemm_nt", self.gemm_nt)
        monkeypatch.setattr(ops, "gemm_wgrad", self.gemm_wgrad)
        monkeypatch.setattr(ops, "gemm_wgrad_multi", self.gemm_wgrad_multi)
        monkeypatch.setattr(ops, "wgrad_reduce_pending", self.wgrad_reduce_pending)
        monkeypatch.setattr(ops, "skinny_group", self.skinny_group)
        monkeypatch.setattr(ops, "outer_wgrad", self.outer_wgrad)
        monkeypatch.setattr(ops, "conv_bn_train", conv_bn_train)

    # -- bookkeeping ---------------------------------------------------------------------------------------------------
    def log(self, tag, kind, mnk, mx, rel):
        line = "%-60s %-22s %-22s err/bound %.3f  rel-L2 %.2e" % (tag, kind, mnk, mx, rel)
        self.lines.append((kind, mx, rel, line))
        if self.verbose:
            print(line)

    def tdt(self, code):
        return torch.bfloat16 if code == self.ops.BF16 else torch.float32

    def check_copies(self, ptrs):
        """Every cached weight copy a launch reads equals a fresh permute + cast of its parameters."""
        for buf, fresh_of, name in cached_copies(self.model.weight_copies):
            lo = buf.data_ptr()
            hi = lo + buf.numel() * buf.element_size()
            if any(p is not None and lo <= int(p) < hi for p in ptrs):
                fresh = fresh_of()
                assert torch.equal(buf.reshape(fresh.shape), fresh), "stale %s copy (step %d): max diff %g" % (
                    name, self.step_no, float((buf.reshape(fresh.shape).float() - fresh.float()).abs().max()))
                self.copies_checked += 1

    def _made(self, d):
        ent = self.made.get(id(d))
        assert ent is not None and ent[0] is d, "a launch descriptor that did not come from ops.gemm_desc / wgrad_desc"
        return ent

    # -- gemm_nt ---------------------------------------------------------------------------------------------------------
    def _nt_kind(self, descs, code):
        ops = self.ops
        arr = (type(descs[0]) * len(descs))(*descs)
        ks = ops._ksplit_w4h(descs, code)
        if ks > 1:
            return "%s/splitK%d" % (KIND_NAMES[self.lib.drn_gemm_nt_splitk_plan(arr, 1, ks, code)], ks)
        ks = ops._ksplit256(descs, code)
        if ks > 1:
            return "W4/splitK256x%d" % ks
        ks = ops._ksplit(descs, code)
        if ks > 1:
            return "%s/splitK%d" % (KIND_NAMES[self.lib.drn_gemm_nt_splitk_plan(arr, len(descs), ks, code)], ks)
        return KIND_NAMES[ops.gemm_nt_plan(descs, code)]

    def gemm_nt(self, descs, dtype):
        torch.cuda.synchronize()
        mem, cdt = self.mem, self.tdt(dtype)
        kind = self._nt_kind(descs, dtype)
        jobs = []
        for d in descs:
            self._made(d)
            M, N, Cin, taps, Lout, Lsrc = d.M, d.N, d.Cin, d.taps, d.Lout, d.Lsrc
            nseq = M // Lout
            K = taps * Cin
            odt = torch.float32 if d.out_f32 else cdt
            src_rows = nseq * Lsrc
            inp = dict(A=mem.view(d.A, cdt, (src_rows, Cin), (d.lda, 1)).clone(), B=mem.view(d.B, cdt, (N, K), (d.ldb, 1)).clone())
            if d.bias:
                inp["bias"] = mem.view(d.bias, torch.float32, (N,), (1,)).clone()
            if d.gate:
                inp["gate"] = mem.view(d.gate, torch.float32, (nseq, N), (d.ldg, 1)).clone()
            outs = {}
            gb = bool(d.gb_act)
            if gb:
                inp["gb_act"] = mem.view(d.gb_act, cdt, (M, N), (d.gb_ld_act, 1)).clone()
                outs["gb_dct"] = mem.view(d.gb_dct, cdt, (N, M), (d.gb_ldt, 1))
                outs["gb_dgate"] = mem.view(d.gb_dgate, torch.float32, (nseq, N), (N, 1))
                outs["gb_dsum"] = mem.view(d.gb_dsum, torch.float32, (nseq, N), (N, 1))
            else:
                outs["C"] = mem.view(d.C, odt, (M, N), (d.ldc, 1))
                if d.accumulate:
                    inp["C_old"] = outs["C"].clone()
            if d.C2:
                outs["C2"] = mem.view(d.C2, cdt, (M, N), (d.ldc2, 1))
            if d.stats:
                outs["stats"] = mem.view(d.stats, torch.float32, ((M + 127) // 128, 2, N), (2 * N, N, 1))
            if d.sumsq:
                outs["sumsq"] = mem.view(d.sumsq, torch.float32, ((M // 256) * (N // 256),), (1,))
            for name, t in outs.items():
                if not (name == "C" and d.accumulate):
                    t.fill_(NAN)
            self.check_copies([d.B])
            jobs.append((d, inp, outs, odt))
        torch.cuda.synchronize()
        self.real["gemm_nt"](descs, dtype)
        torch.cuda.synchronize()
        self.checked_timed += 1
        feats = []
        for i, (d, inp, outs, odt) in enumerate(jobs):
            exp = LR.gemm_nt_ref(inp["A"], inp["B"], d.M, d.N, d.Cin, taps=d.taps, stride=d.stride, pad=d.pad, mode=d.mode, Lout=d.Lout,
                                 Lsrc=d.Lsrc, bias=inp.get("bias"), gate=inp.get("gate"), C_old=inp.get("C_old"), out_dtype=odt,
                                 C2=bool(d.C2), stats=bool(d.stats), sumsq=bool(d.sumsq), gb_act=inp.get("gb_act"))
            tag = "gemm_nt[%s] g%d/%d mode=%d k=%d s=%d" % ("bf16" if dtype == self.ops.BF16 else "f32", i, len(descs), d.mode, d.taps, d.stride)
            mx, rel = LR.compare_all(tag, exp, outs)
            f = [n for n in ("C2", "stats", "sumsq", "gb_dct") if n in outs] + (["gate"] if d.gate else []) + \
                (["bias"] if d.bias else []) + (["f32out"] if d.out_f32 else []) + (["acc"] if d.accumulate else [])
            feats += f
            self.log(tag, kind + ("+" + "+".join(f) if f else ""), "%dx%dx%d" % (d.M, d.N, d.taps * d.Cin), mx, rel)
            if d.out_f32:
                self.dw_final.append((tag, outs["C"], exp["C"]))
            del exp
        self.kinds[kind.split("/")[0] + ("/split" if "/" in kind else "")] += 1
        if "/" in kind:
            self.kinds[kind] += 1
        for f in set(feats):
            self.kinds[kind.split("/")[0] + "+" + f] += 1
        del jobs

    # -- weight gradients ---------------------------------------------------------------------------------------------------
    def _wgrad_probs(self, d, N, Cin, code):
        self._made(d)
        cdt = self.tdt(code)
        nseq = d.M // d.Lout
        return dict(dY=self.mem.view(d.dY, cdt, (d.M, N), (d.ldy, 1)).clone(),
                    X=self.mem.view(d.X, cdt, (nseq * d.Lsrc, Cin), (d.ldx, 1)).clone(), M=d.M, Lout=d.Lout, Lsrc=d.Lsrc)

    def _fused_tap(self, descs, taps, stride, pad, code):
        # include/drn_hip.h (DrnWgradDesc): bf16, taps 3, stride 1, pad 1, Lsrc == Lout and >= 4096 rows -> the fused-tap kernel
        return code == self.ops.BF16 and taps == 3 and stride == 1 and pad == 1 and all(d.Lsrc == d.Lout for d in descs) and \
            sum(d.M for d in descs) >= 4096

    def _run_wgrad(self, tag, kind, groups, dWs, launch, accumulate):
        """groups[i]: (problems, N, Cin, taps, stride, pad, w_layout) of dWs[i]."""
        olds = [dW.clone() if accumulate else None for dW in dWs]
        pend = self.ops.pending_for(dWs)
        n0 = len(pend) if pend is not None else 0
        for dW in dWs:
            if not accumulate:
                dW.fill_(NAN)
        torch.cuda.synchronize()
        launch()
        torch.cuda.synchronize()
        self.checked_timed += 1
        deferred = pend is not None and len(pend) > n0
        self.kinds[kind] += 1
        for i, (g, dW) in enumerate(zip(groups, dWs)):
            probs, N, Cin, taps, stride, pad, wl = g
            exp = LR.wgrad_ref(probs, N, Cin, taps=taps, stride=stride, pad=pad, w_layout=wl, dW_old=olds[i])
            t = "%s p%d" % (tag, i)
            if deferred:
                self.pending.append((t, kind, "%dx%dx%d" % (N, taps * Cin, sum(p["M"] for p in probs)), dW, exp))
            else:
                mx, rel = LR.compare(t, exp, dW)
                self.log(t, kind, "%dx%dx%d" % (N, taps * Cin, sum(p["M"] for p in probs)), mx, rel)
            self.dw_final.append((t, dW, exp))

    def gemm_wgrad(self, descs, dW, N, Cin, taps=1, stride=1, pad=0, w_layout=0, accumulate=False, dtype=0):
        torch.cuda.synchronize()
        probs = [self._wgrad_probs(d, N, Cin, dtype) for d in descs]
        kind = "wgrad-fused3" if self._fused_tap(descs, taps, stride, pad, dtype) else "wgrad-pertap"
        tag = "gemm_wgrad[%s] g=%d k=%d s=%d" % ("bf16" if dtype == self.ops.BF16 else "f32", len(descs), taps, stride)
        self._run_wgrad(tag, kind, [(probs, N, Cin, taps, stride, pad, w_layout)], [dW],
                        lambda: self.real["gemm_wgrad"](descs, dW, N, Cin, taps=taps, stride=stride, pad=pad, w_layout=w_layout,
                                                        accumulate=accumulate, dtype=dtype), accumulate)

    def gemm_wgrad_multi(self, descs, dWs, N, Cin, taps=1, stride=1, pad=0, w_layout=0, accumulate=False, dtype=0):
        torch.cuda.synchronize()
        cins = [Cin] * len(descs) if isinstance(Cin, int) else [int(c) for c in Cin]
        groups = [([self._wgrad_probs(d, N, c, dtype)], N, c, taps, stride, pad, w_layout) for d, c in zip(descs, cins)]
        kind = "wgrad-multi-" + ("fused3" if self._fused_tap(descs, taps, stride, pad, dtype) else "pertap")
        tag = "gemm_wgrad_multi[%s] n=%d k=%d s=%d" % ("bf16" if dtype == self.ops.BF16 else "f32", len(descs), taps, stride)
        self._run_wgrad(tag, kind, groups, list(dWs),
                        lambda: self.real["gemm_wgrad_multi"](descs, dWs, N, Cin, taps=taps, stride=stride, pad=pad, w_layout=w_layout,
                                                              accumulate=accumulate, dtype=dtype), accumulate)

    def wgrad_reduce_pending(self, pend, sumsq=False):
        n = len(pend)
        res = self.real["wgrad_reduce_pending"](pend, sumsq=sumsq)
        torch.cuda.synchronize()
        assert len(self.pending) == n, "%d weight gradients recorded as deferred, the list holds %d" % (len(self.pending), n)
        if n:
            self.kinds["deferred-reduce"] += 1
        for tag, kind, mnk, dW, exp in self.pending:
            mx, rel = LR.compare(tag + " (deferred reduce)", exp, dW)
            self.log(tag, kind + "+deferred", mnk, mx, rel)
        if res is not None:
            # the flush's squared-sum partials are exactly the gradients it wrote
            ranges, part = res
            tot = sum(float(e.ref.pow(2).sum()) for _, _, _, _, e in self.pending)
            assert abs(float(part.double().sum()) - tot) <= 1e-5 * tot, (float(part.double().sum()), tot)
        del self.pending[:]
        return res

    # -- the query side ---------------------------------------------------------------------------------------------------
    def skinny_group(self, probs):
        torch.cuda.synchronize()
        jobs, probs2 = [], []
        for q in probs:
            X, W = q["X"], q["W"]
            Y = q.get("Y")
            if Y is None:
                Y = torch.empty((X.shape[0], W.shape[0]), dtype=torch.float32, device=X.device)
            Y.fill_(NAN)
            q = dict(q, Y=Y)
            probs2.append(q)
            m = q.get("mask")
            jobs.append((LR.skinny_ref(X.clone(), W.clone(), bias=q.get("bias"), mask=m.clone() if m is not None else None,
                                       relu=bool(q.get("relu"))), Y, X, W))
            self.check_copies([W.data_ptr()])
        torch.cuda.synchronize()
        outs = self.real["skinny_group"](probs2)
        torch.cuda.synchronize()
        self.checked_other += (len(probs2) + 15) // 16
        self.kinds["skinny_group"] += 1
        for i, (exp, Y, X, W) in enumerate(jobs):
            tag = "skinny_group p%d/%d%s" % (i, len(jobs), " bf16-rows" if X.dtype == torch.bfloat16 else "")
            mx, rel = LR.compare(tag, exp, Y)
            self.log(tag, "skinny", "%dx%dx%d" % (X.shape[0], W.shape[0], X.shape[1]), mx, rel)
        return outs

    def outer_wgrad(self, probs, lowp=False):
        torch.cuda.synchronize()
        jobs = []
        for q in probs:
            dY, X = q["dY"], q.get("X")
            exp = LR.outer_ref(dY.clone(), X.clone() if (X is not None and q.get("dW") is not None) else None, lowp=lowp)
            outs = {}
            if q.get("dW") is not None:
                outs["dW"] = q["dW"]
            for k in ("db", "db2"):
                if q.get(k) is not None:
                    outs[k] = q[k]
            for t in outs.values():
                t.fill_(NAN)
            jobs.append((exp, outs, dY, X))
        torch.cuda.synchronize()
        self.real["outer_wgrad"](probs, lowp=lowp)
        torch.cuda.synchronize()
        self.checked_other += (len(probs) + 15) // 16
        self.kinds["outer_wgrad"] += 1
        for i, (exp, outs, dY, X) in enumerate(jobs):
            tag = "outer_wgrad p%d/%d%s" % (i, len(jobs), " lowp" if lowp else "")
            mx = rel = 0.0
            for k, t in outs.items():
                a, b = LR.compare(tag + " " + k, exp["dW" if k == "dW" else "db"], t)
                mx, rel = max(mx, a), max(rel, b)
            self.log(tag, "outer", "%dx%dx%d" % (dY.shape[1], X.shape[1] if "dW" in outs else 0, dY.shape[0]), mx, rel)

    # -- the step --------------------------------------------------------------------------------------------------------
    def begin_step(self):
        self.step_no += 1
        self.ops.kernel_timer = []
        self.checked_timed = 0
        self.dw_final = []
        if self.verbose:
            print("\n---- step %d ----" % self.step_no)

    def end_backward(self):
        """After red.finish(): nothing deferred is left, every weight gradient still holds what its launch (and reduce) wrote,
        and every GEMM launch of the step was checked."""
        assert not self.pending, "deferred weight-gradient reduces that never ran: %s" % [p[0] for p in self.pending]
        for tag, dW, exp in self.dw_final:
            LR.compare(tag + " (end of finish)", exp, dW)
        timed = len(self.ops.kernel_timer)
        self.ops.kernel_timer = None
        assert timed == self.checked_timed, "%d GEMM launches in the step, %d checked" % (timed, self.checked_timed)
        self.dw_final = []
        self.mem.clear()
        self.made.clear()


def build_case(dtype, B, T, D, stage, seed_model=0):
    from drn_amd.dist import GradReducer
    from drn_amd.model import mainModel
    from drn_amd.optim import FusedAdam
    from drn_amd.utils.synthetic import VOCAB_SIZE, as_namespace, default_cfg, seeded_state_dict, synthetic_batch
    dev = torch.device("cuda", 0)
    # as bench.py builds its one-GPU step: stage-1 freezing, one bucket, stacked head gradients adjacent
    m = mainModel(VOCAB_SIZE, as_namespace(default_cfg("C3D" if D == 4096 else "SYN", D, stage)), compute_dtype=dtype)
    m.load_state_dict(seeded_state_dict(m, seed_model))
    m = m.to(dev).train()
    for n, p in m.named_parameters():
        if stage == 1 and ("iou_scores" in n or "mix_fc" in n):
            p.requires_grad_(False)
    params = m.learned_parameters()
    red = GradReducer(params, world_size=1, bucket_bytes=1 << 30, adjacent=m.grad_stack_groups())
    opt = FusedAdam(red, lr=1e-3, max_norm=0.5)
    batch = [b.to(dev) for b in synthetic_batch(B, T, D, seed=1)]
    return m, red, opt, batch, stage


def loss_of(losses, stage):
    import drn_amd.functional as DF
    return losses["loss_iou"] if stage == 2 else DF.loss_total(losses)


def optimizer_against_torch(red, opt):
    """After backward of step 1: FusedAdam against clip_grad_norm_ + torch.optim.Adam on fp32 twins fed the same gradients.
    (Step 1 from zero state: m_hat / sqrt(v_hat) = sign(g), so the clip coefficient, grad_scale, the norm and both betas cancel out of
    the parameters compared here -- this pins the tables and the launch, not the arithmetic; tests/test_optim_kernels_gpu.py does that.)"""
    params = [p for b in red.buckets for p in b.params]
    p0 = [p.detach().clone() for p in params]
    g = [p.grad.detach().clone() for p in params]
    norm64 = float(sum(x.double().pow(2).sum() for x in g).sqrt())
    opt.max_norm = 0.5 * norm64                  # clipping active (coefficient 1/2)
    opt.step()
    torch.cuda.synchronize()
    tn = float(opt.total_norm())
    assert abs(tn - norm64) <= 1e-5 * norm64, ("FusedAdam.total_norm", tn, norm64)
    twins = [x.clone().requires_grad_(True) for x in p0]
    for t, gg in zip(twins, g):
        t.grad = gg.clone()
    torch.nn.utils.clip_grad_norm_(twins, opt.max_norm)
    torch.optim.Adam(twins, lr=opt.lr, betas=opt.betas, eps=opt.eps).step()
    for p, t in zip(params, twins):
        torch.testing.assert_close(p.detach(), t.detach(), atol=2e-6, rtol=1e-5, msg=lambda m: "parameter %s: %s" % (tuple(p.shape), m))
    print("optimizer: total norm %.6g (fp64 %.6g), %d parameters agree with clip_grad_norm_ + torch.optim.Adam" % (tn, norm64, len(params)))


# the kinds the benchmarked step must run (each asserted; see REQUIRED_NOTES for any the default step does not use)
REQUIRED_BENCH = {
    "W4+gate": "prop_fc forward (gate + pre-gate copy)",
    "W4+f32out": "prop_fc weight gradient as an fp32 NT product",
    "W4C+gb_dct": "conv0 data gradient with the gate backward in its epilogue",
    "W4H+stats": "a pyramid conv with slab statistics",
    "W4H/split": "conv0 forward with in-launch split-K",
    "general": "a launch on the general tile kernel",
    "wgrad-fused3": "fused-tap weight gradient",
    "wgrad-pertap": "per-tap weight gradient",
    "deferred-reduce": "a non-empty deferred weight-gradient reduce",
    "skinny_group": "the query side's skinny products",
    "outer_wgrad": "the query side's weight gradients",
}


def kinds_seen(kinds):
    seen = set(kinds)
    if any(k.startswith("TILE") for k in kinds):
        seen.add("general")
    if any(k.startswith("wgrad-multi-fused3") for k in kinds):
        seen.add("wgrad-fused3")
    if any(k.startswith("wgrad-multi-pertap") for k in kinds):
        seen.add("wgrad-pertap")
    return seen


CASES = [
    pytest.param(torch.bfloat16, 32, 256, 4096, 1, False, True, id="bf16-B32-T256-D4096-s1"),
    pytest.param(torch.bfloat16, 32, 256, 4096, 3, False, True, id="bf16-B32-T256-D4096-s3"),
    pytest.param(torch.bfloat16, 64, 512, 1024, 1, False, False, id="bf16-B64-T512-D1024-s1"),
    pytest.param(torch.bfloat16, 16, 1024, 500, 1, False, False, id="bf16-B16-T1024-D500-s1"),
    pytest.param(torch.float32, 32, 256, 4096, 3, False, False, id="fp32-B32-T256-D4096-s3"),
    pytest.param(torch.bfloat16, 32, 256, 4096, 1, True, False, id="bf16-B32-T256-D4096-s1-splitk256-extsumsq"),
    pytest.param(torch.bfloat16, 2, 32, 64, 3, False, False, id="bf16-B2-T32-D64-s3"),
]


@pytest.mark.parametrize("dtype,B,T,D,stage,opt_in,bench_shape", CASES)
def test_every_gemm_launch_of_the_step(monkeypatch, dtype, B, T, D, stage, opt_in, bench_shape):
    import drn_amd.ops as ops
    import drn_amd.optim as optim
    if opt_in:
        # shipped but off by default: conv0's forward on full-width tiles with split planes (ops.SPLITK256), and the producers'
        # squared-sum partials for the norm pass (optim.EXT_SUMSQ: DrnGemmDesc::sumsq of prop_fc's weight gradient, the flush's sumsq)
        # (the in-launch W4H split is tried first and takes conv0's forward whenever it applies: off here, so SPLITK256 runs)
        monkeypatch.setattr(ops, "SPLITK256", True)
        monkeypatch.setattr(ops, "KSPLIT_W4H", False)
        monkeypatch.setattr(optim, "EXT_SUMSQ", True)
    m, red, opt, batch, stage = build_case(dtype, B, T, D, stage)
    sh = Shadow(monkeypatch, m, dtype)
    for step in range(2):
        sh.begin_step()
        red.zero()
        _, losses = m(*batch)
        loss_of(losses, stage).backward()
        red.finish()
        sh.end_backward()
        if step == 0:
            optimizer_against_torch(red, opt)
        else:
            opt.step()
        torch.cuda.synchronize()
    assert sh.copies_checked > 0
    seen = kinds_seen(sh.kinds)
    print("kinds: %s" % dict(sh.kinds))
    print("per kind (max err/bound, max rel-L2):")
    agg = {}
    for kind, mx, rel, _ in sh.lines:
        a = agg.setdefault(kind, [0, 0.0, 0.0])
        a[0] += 1
        a[1], a[2] = max(a[1], mx), max(a[2], rel)
    for kind, (n, mx, rel) in sorted(agg.items()):
        print("  %-40s %4d launches/outputs  err/bound %.3f  rel-L2 %.2e" % (kind, n, mx, rel))
    print("checked: %d GEMM outputs, %d weight copies fresh" % (len(sh.lines), sh.copies_checked))
    if bench_shape:
        missing = [("%s (%s)" % (k, v)) for k, v in REQUIRED_BENCH.items() if k not in seen]
        assert not missing, "kernel kinds the benchmarked step did not run: %s" % missing
    if opt_in:
        assert any(k.startswith("W4/splitK256") for k in sh.kinds), sh.kinds
        assert "W4+sumsq" in seen, sh.kinds
