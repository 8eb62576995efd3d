"""Parity cases of the DMAE stage-3 head kernels (csrc/tpmcl.hip) on LONG token rows -- more than 128 tokens per item, more than 1024 columns, selector
rows of more than 64 tokens -- shared by the emulator and the GPU suites.  Every reference is the plain torch fp32 expression on the CPU, as in
kernel_cases.case_tpmcl_ops, and every `tpmcl.*` call runs under `no_torch_path()`: the wrappers may not reach torch's softmax / einsum / argsort /
cumsum for any shape.

Tolerances are kernel_cases.case_tpmcl_ops's (forward 1e-5 / 1e-6, dfeat 1e-4 / 1e-6, dw 1e-4 / 1e-5, pair ops 1e-5 / 1e-5: rtol / atol as a fraction
of the reference's largest element).  Where a sum is long enough for fp32 summation order to matter, the absolute term is the larger of that figure and
4 x the error of the fp32 torch reference against an fp64 torch evaluation of the same inputs (`_atol`): the kernel adds in another order than torch, so
it is allowed the reference's own distance from the exact value four times over.  Measured on the CPU (reference fp32 vs fp64, fraction of the
largest element; forward / dfeat / dw): token_weights (5, 129, 96) 2.0e-7 / 3.7e-7 / 3.9e-7, (3, 257, 1028) 7.9e-7 / 2.3e-6 / 1.2e-6, (3, 130, 1030) 2.6e-7 / 9.0e-7 /
7.4e-7, (2, 4096, 64) 5.6e-7 / 6.0e-7 / 1.3e-6 -- so the absolute term rises above the base figure for the forward at (3, 257, 1028) and (2, 4096, 64) (3.2e-6,
2.2e-6) and for dfeat at the three larger shapes (9.2e-6, 3.6e-6, 2.4e-6); dw keeps 1e-5 everywhere.  The pair operators stay at 1e-5: their references are
within 1.5e-6 of fp64 at (3, 300, 1028)."""
import contextlib

import torch

from kernel_cases import check, rnd

GUARDED = ("softmax", "einsum", "argsort", "cumsum")
EINVAL = -22


@contextlib.contextmanager
def no_torch_path():
    """torch.softmax / einsum / argsort / cumsum raise inside the block: what the wrappers fell back to beyond the kernels' old row budget."""
    saved = {n: getattr(torch, n) for n in GUARDED}

    def trap(n):
        def f(*a, **k):
            raise AssertionError(f"torch.{n} was called on the TPM-CL kernel path")
        return f

    for n in GUARDED:
        setattr(torch, n, trap(n))
    try:
        yield
    finally:
        for n, f in saved.items():
            setattr(torch, n, f)


@contextlib.contextmanager
def tpmcl_calls_guarded():
    """Model-level form: every public `antmmf.hip.tpmcl` row operator runs under no_torch_path() (the model around them is free to use torch)."""
    from antmmf.hip import tpmcl

    names = ("token_weights", "pair_dots", "pair_wsum", "tis_keep")
    saved = {n: getattr(tpmcl, n) for n in names}
    calls = dict.fromkeys(names, 0)

    def wrap(n):
        def f(*a, **k):
            calls[n] += 1
            with no_torch_path():
                return saved[n](*a, **k)
        return f

    for n in names:
        setattr(tpmcl, n, wrap(n))
    try:
        yield calls
    finally:
        for n, f in saved.items():
            setattr(tpmcl, n, f)


def _atol(base, ref32, ref64):
    """max(base, 4 x the fp32 reference's own error against fp64), as a fraction of the reference's largest element; also returns the measured error"""
    scale = max(float(ref64.abs().max()), 1e-30)
    e = float((ref32.detach().double() - ref64.detach()).abs().max()) / scale
    return max(base, 4.0 * e), e


def _token_weights_ref(feat, w, b, mask, dout):
    fr, wr, br = (x.clone().requires_grad_(True) for x in (feat, w, b))
    ref = torch.softmax((fr @ wr.t()).squeeze(-1).add(br).masked_fill(mask < 0.5, float("-inf")), dim=-1)
    (ref * dout).sum().backward()
    return ref.detach(), fr.grad, wr.grad, br.grad


def case_token_weights(dev, N, T, D):
    """tpmcl.token_weights forward and backward at [N, T, D]: masked softmax weights, dfeat, dw, and the analytically vanishing bias gradient."""
    from antmmf.hip import tpmcl

    feat = rnd((N, T, D), 801, 1.0)
    w, b = rnd((1, D), 802, 0.3), rnd((1,), 803, 0.1)
    mask = (rnd((N, T), 804, 1.0) > -0.5).float()
    mask[:, 0] = 1.0
    dout = rnd((N, T), 805, 1.0)
    ref, dfeat, dw, db = _token_weights_ref(feat, w, b, mask, dout)
    ref64, dfeat64, dw64, _ = _token_weights_ref(feat.double(), w.double(), b.double(), mask, dout.double())
    fd, wd, bd = (x.clone().to(dev).requires_grad_(True) for x in (feat, w, b))
    with no_torch_path():
        got = tpmcl.token_weights(fd, wd, bd, mask.to(dev))
        (got * dout.to(dev)).sum().backward()
    figures = {}
    for name, g, r, r64, rtol, base in (("fwd", got, ref, ref64, 1e-5, 1e-6), ("dfeat", fd.grad, dfeat, dfeat64, 1e-4, 1e-6), ("dw", wd.grad, dw, dw64, 1e-4, 1e-5)):
        atol, e = _atol(base, r, r64)
        figures[name] = (e, atol)
        print(f"tpm_long.token_weights[{N},{T},{D}].{name}: fp32 reference vs fp64 {e:.3g}, atol {atol:.3g}, kernel max err "
              f"{float((g.detach().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-30):.3g} (fractions of the largest element)")
        check(f"tpm_long.token_weights.{name}", g, r, rtol, atol)
    # the bias gradient vanishes analytically (a softmax does not see a shift of its logits): both sides hold rounding noise; the kernel is allowed the
    # base figure of case_tpmcl_ops or 4 x the noise the fp32 reference itself shows
    lim = max(1e-5 * float(dw.abs().max()), 4.0 * float(db.abs().max()))
    assert float(bd.grad.abs().max()) <= lim, (float(bd.grad), float(db), lim)
    masked = mask.to(dev) < 0.5
    assert bool(masked.any())
    assert float(got.detach()[masked].abs().max()) == 0.0, "a masked token has a non-zero weight"
    assert float(fd.grad[masked].abs().max()) == 0.0, "a masked token has a non-zero gradient"
    return figures


def case_pair_ops(dev, C, V, D):
    """tpmcl.pair_dots / pair_wsum at [C, V, D] through their autograd wrappers (whose backward runs pair_wsum / pair_outer / pair_dots): both outputs and all of dx, dy, dw."""
    from antmmf.hip import tpmcl

    x, y, ww = rnd((C, D), 806, 1.0), rnd((C, V, D), 807, 1.0), rnd((C, V), 808, 1.0)
    g1, g2 = rnd((C, V), 809, 1.0), rnd((C, D), 810, 1.0)

    def ref_of(dt):
        xr, yr, wwr = (t.to(dt).clone().requires_grad_(True) for t in (x, y, ww))
        d = torch.einsum("cd,cvd->cv", xr, yr)
        s = torch.einsum("cv,cvd->cd", wwr, yr)
        ((d * g1.to(dt)).sum() + (s * g2.to(dt)).sum()).backward()
        return d.detach(), s.detach(), xr.grad, yr.grad, wwr.grad

    r32, r64 = ref_of(torch.float32), ref_of(torch.float64)
    xd, yd, wwd = (t.clone().to(dev).requires_grad_(True) for t in (x, y, ww))
    with no_torch_path():
        dgot, sgot = tpmcl.pair_dots(xd, yd), tpmcl.pair_wsum(wwd, yd)
        ((dgot * g1.to(dev)).sum() + (sgot * g2.to(dev)).sum()).backward()
    figures = {}
    for name, g, r, r6 in zip(("pair_dots", "pair_wsum", "dx", "dy", "dw"), (dgot, sgot, xd.grad, yd.grad, wwd.grad), r32, r64):
        atol, e = _atol(1e-5, r, r6)
        figures[name] = (e, atol)
        print(f"tpm_long.pair[{C},{V},{D}].{name}: fp32 reference vs fp64 {e:.3g}, atol {atol:.3g}")
        check(f"tpm_long.{name}", g, r, 1e-5, atol)
    return figures


TIS_THRESHOLDS = (0.3, 0.6, 0.95)
TIS_MARGIN = 1e-4
# seeds for which, for every row and every threshold, no fp64 descending cumulative sum comes within TIS_MARGIN of the threshold (found on the CPU from the
# reference alone; tis_rows asserts it): (R, T) -> seed
TIS_SEEDS = {(9, 65): 901, (9, 130): 900, (6, 1024): 903, (3, 65): 900, (3, 130): 900, (2, 65): 900}


def tis_rows(R, T, seed):
    """[R, T] softmax weights with masked tokens (exact zeros, so many ties at 0); row 0 carries groups of EQUAL non-zero weights at distinct indices
    (equal logits give bit-equal softmax values).  Asserts the margin condition on the fp64 descending cumulative sums."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(R, T, generator=g) * 3.0
    logits[0, 1::3] = logits[0, 1]        # a third of row 0 shares one logit,
    logits[0, 2::7] = logits[0, 2]        # another group a second one
    mask = torch.rand(R, T, generator=g) > 0.2
    mask[:, 0] = True
    mask[0, 1] = mask[0, 2] = True
    w = torch.softmax(logits.masked_fill(~mask, float("-inf")), dim=-1)
    assert int((w[0] == w[0, 1]).sum()) >= 2 and float(w[0, 1]) > 0.0 and int((w == 0).sum()) > 0
    cum = torch.sort(w.double(), dim=1, descending=True, stable=True).values.cumsum(dim=1)
    for th in TIS_THRESHOLDS:
        gap = float((cum - th).abs().min())
        assert gap >= TIS_MARGIN, f"seed {seed}: a descending cumulative sum lies {gap:.3g} from threshold {th} (choose another seed, keep the rows)"
    return w


def tis_reference(w, thresh):
    ws, order = torch.sort(w, dim=1, descending=True, stable=True)
    return 1.0 - torch.zeros_like(w).scatter(1, order, (ws.cumsum(dim=1) < thresh).float())


def case_tis_keep(dev, R, T):
    """tpmcl.tis_keep on rows of T tokens against a STABLE descending sort, cumsum and scatter on the CPU: bit-equal masks at the three thresholds."""
    from antmmf.hip import tpmcl

    w = tis_rows(R, T, TIS_SEEDS[(R, T)])
    dropped = {}
    for th in TIS_THRESHOLDS:
        ref = tis_reference(w, th)
        with no_torch_path():
            keep = tpmcl.tis_keep(w.to(dev), th)
        assert torch.equal(keep.cpu(), ref), (T, th, int((keep.cpu() != ref).sum()))
        dropped[th] = int((ref == 0).sum())
    assert 0 < dropped[0.95] < w.numel() and dropped[0.3] <= dropped[0.6] <= dropped[0.95], dropped   # (a row whose first weight passes a threshold drops nothing there)
    return dropped


def case_out_of_range(ops, dev):
    """One past every limit: the wrappers raise ValueError naming the limit, the C entry points return ANTMMF_EINVAL and launch nothing (outputs keep their fill)."""
    from antmmf.hip import _lib, tpmcl

    max_t, max_d, max_keep = ops.tpmcl_limits()
    assert (max_t, max_d, max_keep) == (4096, 4096, 1024)
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
    p, st = ops._p, ops._stream()
    for T, D in ((max_t + 1, 8), (2, max_d + 1)):
        feat, w, mask, xx, ww = z(1, T, D), z(1, D), torch.ones(1, T, device=dev), z(1, D), z(1, T)
        with no_torch_path():
            for fn, args in ((tpmcl.token_weights, (feat, w, None, mask)), (tpmcl.pair_dots, (xx, feat)), (tpmcl.pair_wsum, (ww, feat))):
                try:
                    fn(*args)
                except ValueError as e:
                    assert str(max_t if T > max_t else max_d) in str(e), str(e)
                else:
                    raise AssertionError(f"{fn.__name__} accepted T = {T}, D = {D}")
        out, dfeat, dw, scratch = torch.full((1, T), 7.0, device=dev), torch.full((1, T, D), 7.0, device=dev), torch.full((D,), 7.0, device=dev), z(512 * (D + 1))
        outd, outs = torch.full((1, D), 7.0, device=dev), torch.full((1, T), 7.0, device=dev)
        assert lib.antmmf_token_weight_fwd(p(feat), p(w), 0, p(mask), p(out), 1, T, D, st) == EINVAL
        assert lib.antmmf_token_weight_bwd(p(feat), p(w), p(ww), p(ww), p(dfeat), p(dw), 0, p(scratch), scratch.numel(), 1, T, D, st) == EINVAL
        assert lib.antmmf_pair_dots(p(xx), p(feat), p(outs), 1, T, D, st) == EINVAL
        assert lib.antmmf_pair_wsum(p(ww), p(feat), p(outd), 1, T, D, st) == EINVAL
        assert lib.antmmf_pair_outer(p(ww), p(xx), p(dfeat), 1, T, D, st) == EINVAL
        for t in (out, dfeat, dw, outd, outs):
            assert bool((t == 7.0).all()), "an out-of-range call wrote its output"
    wt = torch.full((2, max_keep + 1), 1.0 / (max_keep + 1), device=dev)
    with no_torch_path():
        try:
            tpmcl.tis_keep(wt, 0.3)
        except ValueError as e:
            assert str(max_keep) in str(e), str(e)
        else:
            raise AssertionError("tis_keep accepted a row past the limit")
    keep = torch.full_like(wt, 7.0)
    assert lib.antmmf_tis_keep(p(wt), 0.3, p(keep), 2, max_keep + 1, st) == EINVAL
    assert bool((keep == 7.0).all())


def case_direct_ops(ops, dev):
    """The C entry points one past the OLD row budget (129 tokens, selector rows of 65), called without the autograd wrappers: served, not refused."""
    T, D = 129, 32
    feat, w, mask = rnd((2, T, D), 821).to(dev), rnd((D,), 822, 0.3).to(dev), torch.ones(2, T, device=dev)
    p = ops.token_weight_fwd(feat, w, None, mask)
    check("tpm_long.direct.token_weight_fwd", p, torch.softmax(feat.cpu() @ w.cpu(), dim=-1), 1e-5, 1e-6)
    ww, x = rnd((2, T), 823).to(dev), rnd((2, D), 824).to(dev)
    check("tpm_long.direct.pair_wsum", ops.pair_wsum(ww, feat), torch.einsum("cv,cvd->cd", ww.cpu(), feat.cpu()), 1e-5, 1e-5)
    check("tpm_long.direct.pair_outer", ops.pair_outer(ww, x), ww.cpu()[:, :, None] * x.cpu()[:, None, :], 1e-6, 1e-6)
    w65 = tis_rows(2, 65, TIS_SEEDS[(2, 65)])
    assert torch.equal(ops.tis_keep(w65.to(dev), 0.6).cpu(), tis_reference(w65, 0.6))


def case_scratch_grows(ops, dev):
    """ops.token_weight_bwd sizes its cached workspace from D: a wide D after a narrow one gets 512 * (D + 1) floats, not a fixed 512 * 1025."""
    for D in (8, 1100):
        feat, w = rnd((1, 2, D), 831).to(dev), rnd((D,), 832, 0.3).to(dev)
        p = ops.token_weight_fwd(feat, w, None, None)
        dw = torch.zeros(D, device=dev)
        ops.token_weight_bwd(feat, w, p, torch.ones_like(p), dw)
        assert ops._TW_SCRATCH[feat.device].numel() >= 512 * (D + 1)


def case_dmae_long_rows(dev, ptypes=(2, 3, 4)):
    """A DmaeUtils head at hidden_size 128 with 70 words and 69 + 1 frame tokens (tis_keep rows and both weight predictors past 64 tokens): the TPM-CL margin loss
    of partial types 2 / 3 / 4 and its gradients against oracle.losses.dmae_tpmcl_margin_loss on the same parameters; gates of model_cases.case_dmae_tpmcl
    (loss 1e-3, gradient norms 5e-3).  The tpmcl row operators run under the no-torch guard."""
    import model_cases as mc
    from antmmf.common.configuration import Configuration
    from oracle import losses as olosses

    mod = mc.load_dmae_utils()
    B, Nw, V, D = 16, 70, 69, 128
    norm = lambda x: x / x.norm(dim=-1, keepdim=True)  # noqa: E731
    # a common component with opposite signs in the text and the video tokens makes the pair scores negative: the importance-masked scores then lie ABOVE the
    # full ones and every margin term of every partial type is active (on uncorrelated features type 3 is 0 with zero gradients on both sides)
    text, word, video = norm(rnd((B, 1, D), 841) + 1.0), norm(rnd((B, Nw, D), 842) + 1.0), norm(rnd((B, V + 1, D), 843) - 1.0)
    wm = torch.ones(B, Nw)
    wm[3, 40:] = 0
    wm[10, 66:] = 0
    vm = torch.ones(B, V + 1)
    res = {}
    for ptype in ptypes:
        du = mod.DmaeUtils(Configuration(dict(mc.DMAE_CFG, l3_interaction="wti", l3_with_nfc=True, l3_sim_header="meanP", l3_partial_type=ptype,
                                              l3_max_frames=V, l3_max_words=Nw)))
        mc.W.fill_module_(du)
        du.tis_selector.thresh.fill_(0.6)
        P = {n: p.detach().clone().requires_grad_(True) for n, p in du.named_parameters()}
        tr, wr, vr = (x.clone().requires_grad_(True) for x in (text, word, video))
        ref = olosses.dmae_tpmcl_margin_loss(P, tr, wr, vr, wm, vm, ptype, cis_thresh=0.6)
        ref.backward()
        du = du.to(dev).train()
        t, w_, v = (x.clone().to(dev).requires_grad_(True) for x in (text, word, video))
        with tpmcl_calls_guarded() as calls:
            loss = du.get_partial_similarity((t, w_), v, wm.to(dev), vm.to(dev), ptype)
            loss.backward()
        assert calls["tis_keep"] >= 2 and calls["token_weights"] >= 2 and calls["pair_dots"] >= 1 and calls["pair_wsum"] >= 2, calls
        assert float(ref.detach()) > 0.0 and abs(float(loss.detach()) - float(ref.detach())) <= 1e-3 * abs(float(ref.detach())), (ptype, float(loss.detach()), float(ref.detach()))
        for nm, x, xr in (("dtext", t, tr), ("dword", w_, wr), ("dvideo", v, vr)):
            gn = float(x.grad.norm()) if x.grad is not None else 0.0
            rn = float(xr.grad.norm()) if xr.grad is not None else 0.0
            assert abs(gn - rn) <= 5e-3 * max(rn, 1e-6), (ptype, nm, gn, rn)
        for n, p in du.named_parameters():
            gn = float(p.grad.norm()) if p.grad is not None else 0.0
            rn = float(P[n].grad.norm()) if P[n].grad is not None else 0.0
            if n.endswith("_weight_fc.bias"):
                # analytically zero (a softmax does not see a shift of its logits): both sides hold rounding noise, which has no norm to compare.  The
                # bound is case_tpmcl_ops's for the same quantity, 1e-5 of the weight gradient of the same Linear, or 4 x the fp32 reference's own
                # distance from the exact 0 (the sums run over 256 pairs x 70 tokens here, and the weight gradient nearly cancels)
                wn = float(P[n[:-4] + "weight"].grad.norm())
                assert gn <= max(1e-5 * wn, 4.0 * rn), (ptype, n, gn, rn, wn)
                continue
            assert abs(gn - rn) <= 5e-3 * max(rn, 1e-5), (ptype, n, gn, rn)
        res[ptype] = (float(loss.detach()), float(ref.detach()))
    return res
