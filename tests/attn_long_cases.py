"""Attention for token rows longer than the whole-row kernels' 288 (csrc/attention.hip: attn_fwd_stream_kernel, attn_bwd_dq_stream_kernel,
attn_bwd_dkv_stream_kernel), shared by the CPU-emulator tests and the hardware tests.  Tolerances are kernel_cases.case_attention's: o 2e-2 / 2e-2, lse 1e-2 / 1e-2,
gradients 3e-2 / 3e-2 (kernel_cases.check, median-relative-error criterion included); that helper is called directly wherever its signature covers the case.

QB is the streamed kernels' token block per workgroup, KB[head size] the block of the opposite side staged in LDS per trip (ATTN_STREAM_QB / ATTN_STREAM_KEYS in
attention.hip): the shapes below are written in terms of them, so that another block size moves the edge cases with it."""
import ctypes

import numpy as np
import torch

import kernel_cases as kc
from kernel_cases import BF, check, q, rnd
from oracle import ops as oops

QB = 128
KB = {64: 256, 128: 128}
WALL = 288          # the whole-row kernels' limit
LIMIT = 4096        # the streamed kernels' limit
EINVAL = -22

FIRST_PAST_THE_WALL = [(dh, bias, packed) for dh in (64, 128) for bias in ("none", "bert", "inf") for packed in (True, False)]


def block_edge_shapes(dh):
    """(Nq, Nk): the last key tile / query tile holds one token, a block is exactly full, one block more"""
    return [(WALL + 1, KB[dh] + 1), (WALL + 1, 2 * KB[dh]), (WALL + 1, 2 * KB[dh] + 1), (3 * QB, WALL + 1), (3 * QB + 1, WALL + 1)]


def cross_length_shapes(dh, gpu):
    """(Nq, Nk).  (37, 2 KB + 1) is 37 x 257 at head size 128 -- a whole-row plan -- so the hardware list also holds the short-query shape one key block further"""
    return [(16, WALL + 1), (300, 40)] + ([(37, 2 * KB[dh] + 1), (37, 3 * KB[dh] + 1)] if gpu else [])


def run(ops, dev, B, heads, Nq, Nk, dh, key_bias=None, seed=900, dropout_p=0.0, dropout_seed=0, mask=None):
    """Product forward + backward and the fp32 oracle on the same bf16-rounded tensors.  mask: explicit [B, heads, Nq, Nk] dropout factors for the oracle.
    -> dict(o, lse, dq, dk, dv) and dict(o, lse, dq, dk, dv) (oracle; lse of the undropped scores)."""
    D = heads * dh
    scale = dh ** -0.5
    qt, kt, vt, d_o = q(rnd((B, Nq, D), seed)), q(rnd((B, Nk, D), seed + 1)), q(rnd((B, Nk, D), seed + 2)), q(rnd((B, Nq, D), seed + 3))
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (qt, kt, vt))
    s = torch.matmul(oops.split_heads(qr, heads), oops.split_heads(kr, heads).transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + key_bias[:, None, None, :]
    p = torch.softmax(s, -1)
    p = torch.nan_to_num(p, nan=0.0)   # fully masked rows: the kernels' rule (zeros), not the softmax's NaN
    if mask is not None:
        p = p * mask
    ref_o = oops.merge_heads(torch.matmul(p, oops.split_heads(vr, heads)))
    ref_o.backward(d_o)
    ref = dict(o=ref_o.detach(), lse=torch.logsumexp(s.detach(), -1), dq=qr.grad, dk=kr.grad, dv=vr.grad)
    qd, kd, vd = qt.to(dev, BF), kt.to(dev, BF), vt.to(dev, BF)
    kb = None if key_bias is None else key_bias.to(dev)
    o, lse = ops.attention_fwd(qd, kd, vd, heads, scale, kb, dropout_p=dropout_p, dropout_seed=dropout_seed)
    dq, dk, dv = ops.attention_bwd(qd, kd, vd, o, lse, d_o.to(dev, BF), heads, scale, kb, dropout_p=dropout_p, dropout_seed=dropout_seed)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, inputs=(qd, kd, vd, d_o.to(dev, BF), scale)), ref


def compare(tag, got, ref, lse=True):
    check(tag + ".o", got["o"], ref["o"], 2e-2, 2e-2)
    if lse:
        check(tag + ".lse", got["lse"], ref["lse"], 1e-2, 1e-2)
    for g in ("dq", "dk", "dv"):
        check(f"{tag}.{g}", got[g], ref[g], 3e-2, 3e-2)


def assert_finite(tag, got):
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n].float()).all()), f"{tag}.{n} holds a non-finite value"


def case_leading_masked_block(ops, dev, dh, B=2, heads=2):
    """key_bias = -inf on the keys [0, KB) of the LAST batch item -- its first LDS block is masked entirely before any valid key is seen (running maximum -inf) --
    and valid keys behind it: output, lse and gradients against the oracle, every value finite."""
    Nq, Nk = 40, max(KB[dh] + 33, WALL + 1)   # beyond the whole-row limit at both head sizes: the streamed kernels serve it
    assert Nk > WALL and Nk > KB[dh]
    kb = torch.zeros(B, Nk)
    kb[B - 1, :KB[dh]] = float("-inf")
    got, ref = run(ops, dev, B, heads, Nq, Nk, dh, kb, seed=910)
    assert_finite("attn_long.leading_masked", got)
    compare(f"attn_long.leading_masked[{dh}]", got, ref)
    assert bool((got["dk"][B - 1, :KB[dh]] == 0).all()) and bool((got["dv"][B - 1, :KB[dh]] == 0).all())


def case_fully_masked_row(ops, dev, dh, B=2, heads=2):
    """One batch item with every key at -inf: lse and o equal what the whole-row kernel returns for the same item truncated to 288 keys (lse = -inf, o = 0), its dq,
    dk and dv are zero, and nothing is NaN in the other item (which is compared with the oracle)."""
    Nq, Nk = 33, WALL + 1
    kb = torch.zeros(B, Nk)
    kb[0] = float("-inf")
    got, ref = run(ops, dev, B, heads, Nq, Nk, dh, kb, seed=920)
    qd, kd, vd, d_o, scale = got["inputs"]
    o_w, lse_w = ops.attention_fwd(qd, kd[:, :WALL].contiguous(), vd[:, :WALL].contiguous(), heads, scale, kb[:, :WALL].contiguous().to(dev))
    assert torch.equal(got["o"][0], o_w[0]) and torch.equal(got["lse"][0], lse_w[0]), "fully masked item: streamed and whole-row forward disagree"
    assert bool((got["lse"][0] == float("-inf")).all()) and bool((got["o"][0] == 0).all())
    for g in ("dq", "dk", "dv"):
        assert bool((got[g][0] == 0).all()), f"fully masked item: {g} is not zero"
    other = {k: v[1:] for k, v in got.items() if k != "inputs"}
    assert_finite("attn_long.fully_masked.other_item", other)
    compare(f"attn_long.fully_masked.other_item[{dh}]", other, {k: v[1:] for k, v in ref.items()})


def case_consistency_with_whole_row(ops, dev, dh, B=2, heads=2, bias_kind="bert"):
    """289 keys whose key 288 carries -inf (streamed kernels) against the call on keys [0, 288) (whole-row kernels), no oracle: o, lse, dq, dk[:, :288], dv[:, :288]
    agree within the project's bf16 attention tolerances, dk and dv of the masked key are zero."""
    N = WALL + 1
    D = heads * dh
    scale = dh ** -0.5
    qd, kd, vd, d_o = (q(rnd((B, N, D), 930 + i)).to(dev, BF) for i in range(4))
    kb = torch.zeros(B, N)
    if bias_kind == "bert":
        kb[1, 200:] = -10000.0
    kb[:, WALL] = float("-inf")
    kb = kb.to(dev)
    o, lse = ops.attention_fwd(qd, kd, vd, heads, scale, kb)
    dq, dk, dv = ops.attention_bwd(qd, kd, vd, o, lse, d_o, heads, scale, kb)
    k2, v2, kb2 = kd[:, :WALL].contiguous(), vd[:, :WALL].contiguous(), kb[:, :WALL].contiguous()
    o2, lse2 = ops.attention_fwd(qd, k2, v2, heads, scale, kb2)
    dq2, dk2, dv2 = ops.attention_bwd(qd, k2, v2, o2, lse2, d_o, heads, scale, kb2)
    tag = f"attn_long.vs_whole_row[{dh}]"
    check(tag + ".o", o, o2, 2e-2, 2e-2)
    check(tag + ".lse", lse, lse2, 1e-2, 1e-2)
    check(tag + ".dq", dq, dq2, 3e-2, 3e-2)
    check(tag + ".dk", dk[:, :WALL], dk2, 3e-2, 3e-2)
    check(tag + ".dv", dv[:, :WALL], dv2, 3e-2, 3e-2)
    assert bool((dk[:, WALL] == 0).all()) and bool((dv[:, WALL] == 0).all()), tag + ": gradient at the masked key"


def case_dropout(ops, dev, dh, B=2, heads=2):
    """p = 0.2 with a 64-bit seed at 289 x 289: forward and all three gradients against the oracle attention with the explicit mask rebuilt by the numpy twin of the
    counter hash (kernel_cases.dropout_keep_np); keep rate within 4 sigma of 0.8."""
    N, p, seed = WALL + 1, 0.2, (0x5EED << 32) | 0x1234567
    n = B * heads * N * N
    keep = kc.dropout_keep_np(np.arange(n).reshape(B, heads, N, N), seed, p).float()
    rate, sigma = float(keep.mean()), (p * (1 - p) / n) ** 0.5
    assert abs(rate - (1 - p)) <= 4 * sigma, (rate, sigma)
    kb = torch.zeros(B, N)
    kb[B - 1, N // 3:] = -10000.0
    got, ref = run(ops, dev, B, heads, N, N, dh, kb, seed=940, dropout_p=p, dropout_seed=seed, mask=keep / (1 - p))
    compare(f"attn_long.dropout[{dh}]", got, ref)


def case_reproducible(ops, dev, B=2, heads=2, N=321, dh=64):
    D = heads * dh
    qd, kd, vd, d_o = (q(rnd((B, N, D), 950 + i)).to(dev, BF) for i in range(4))
    o, lse = ops.attention_fwd(qd, kd, vd, heads, dh ** -0.5)
    a = ops.attention_bwd(qd, kd, vd, o, lse, d_o, heads, dh ** -0.5)
    b = ops.attention_bwd(qd, kd, vd, o, lse, d_o, heads, dh ** -0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the streamed backward is not bit-reproducible"
    o2, lse2 = ops.attention_fwd(qd, kd, vd, heads, dh ** -0.5)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def case_refusals(ops, dev):
    """The limits query, the raw entry points' ANTMMF_EINVAL beyond 4096 (outputs keep their fill), ValueError from ops, and what keeps the 288 limit."""
    from antmmf.hip import _lib

    assert ops.attention_limits() == (WALL, LIMIT)
    assert ops.ATTN_MAX_TOKENS == WALL
    lib = _lib.load()
    heads, dh = 1, 64
    for Nq, Nk in ((LIMIT + 1, 16), (16, LIMIT + 1)):
        qd = torch.zeros(1, Nq, dh, dtype=BF, device=dev)
        kd = torch.zeros(1, Nk, dh, dtype=BF, device=dev)
        o = torch.full((1, Nq, dh), 3.0, dtype=BF, device=dev)
        lse = torch.full((1, heads, Nq), 5.0, device=dev)
        rc = lib.antmmf_attention_fwd_hd(_ptr(qd), _ptr(kd), _ptr(kd), None, _ptr(o), _ptr(lse), 1, heads, dh, Nq, Nk, dh, dh, dh, dh, 0.125, 0.0, 0, None)
        assert rc == EINVAL and bool((o == 3.0).all()) and bool((lse == 5.0).all()), (Nq, Nk, rc)
        dq, dk = torch.full_like(qd, 3.0), torch.full_like(kd, 3.0)
        dv = torch.full_like(kd, 3.0)
        rc = lib.antmmf_attention_bwd_hd(_ptr(qd), _ptr(kd), _ptr(kd), None, _ptr(o), _ptr(lse), _ptr(qd), _ptr(dq), _ptr(dk), _ptr(dv), 1, heads, dh, Nq, Nk,
                                         dh, dh, dh, dh, dh, dh, dh, dh, 0.125, 0.0, 0, None)
        assert rc == EINVAL and all(bool((t == 3.0).all()) for t in (dq, dk, dv)), (Nq, Nk, rc)
        for call in (lambda: ops.attention_fwd(qd, kd, kd, heads, 0.125), lambda: ops.attention_bwd(qd, kd, kd, o, lse, qd, heads, 0.125)):
            try:
                call()
            except ValueError as e:
                assert str(LIMIT) in str(e), e
            else:
                raise AssertionError(f"{Nq} x {Nk}: no ValueError")
    assert not ops.attention_packed_ok(64, WALL + 1) and not ops.attention_bwd_sums_ok(64, WALL + 1, WALL + 1)
    assert ops.attention_packed_ok(64, 128) and ops.attention_bwd_sums_ok(64, 257, 257)
    # the probability maps and the key importance keep the whole-row limit
    N = WALL + 1
    qd = torch.zeros(1, N, dh, dtype=BF, device=dev)
    lse = torch.zeros(1, heads, N, device=dev)
    probs = torch.full((1, heads, N, N), 2.0, device=dev)
    imp = torch.full((1, N), 2.0, device=dev)
    rc = lib.antmmf_attention_probs(_ptr(qd), _ptr(qd), None, _ptr(lse), _ptr(probs), None, 1, heads, dh, N, N, dh, dh, 0.125, 0.0, 0, 1.0, None)
    assert rc == EINVAL and bool((probs == 2.0).all())
    rc = lib.antmmf_attention_key_importance(_ptr(qd), _ptr(qd), None, _ptr(lse), _ptr(imp), 1, heads, N, N, dh, dh, 0.125, 0.0, 0, 1.0, None)
    assert rc == EINVAL and bool((imp == 2.0).all())


def case_key_importance_both_head_sizes(ops, dev, N=77, B=2, heads=2):
    """attention_key_importance_ (head size 64: now the probability-map kernel without the maps) against the oracle's column sums, with and without dropout."""
    for dh in (64, 128):
        D = heads * dh
        scale, p, seed = dh ** -0.5, 0.2, (9 << 32) | 77
        qt, kt, vt = (q(rnd((B, N, D), 960 + i)) for i in range(3))
        kb = torch.zeros(B, N)
        kb[B - 1, 30:] = -10000.0
        s = torch.matmul(oops.split_heads(qt, heads), oops.split_heads(kt, heads).transpose(-1, -2)) * scale + kb[:, None, None, :]
        mask = kc.dropout_keep_np(np.arange(B * heads * N * N).reshape(B, heads, N, N), seed, p).float() / (1 - p)
        qd, kd, vd = qt.to(dev, BF), kt.to(dev, BF), vt.to(dev, BF)
        for pp, m in ((0.0, 1.0), (p, mask)):
            _, lse = ops.attention_fwd(qd, kd, vd, heads, scale, kb.to(dev), dropout_p=pp, dropout_seed=seed)
            imp = torch.full((B, N), 0.5, device=dev)
            ops.attention_key_importance_(imp, qd, kd, lse, heads, scale, kb.to(dev), dropout_p=pp, dropout_seed=seed, weight=1.0 / heads)
            check(f"attn_long.importance[{dh},{pp}]", imp, 0.5 + (torch.softmax(s, -1) * m).mean(1).sum(1), 2e-2, 2e-2)


# ------------------------------------------------------------------------------ layer and model level (hardware)
def case_visual_transformer(dev, resolution=144, patch=8):
    """CLIP-arch VisionTransformer at a resolution with more than 288 tokens (18 x 18 + 1 = 325): forward and backward run and give finite values."""
    from antmmf.modules.vision.backbone.clip.model import VisionTransformer
    import weightgen as W

    m = VisionTransformer(input_resolution=resolution, patch_size=patch, width=128, layers=2, heads=2, output_dim=64)
    W.fill_module_(m)
    m = m.to(dev).train()
    assert (resolution // patch) ** 2 + 1 > WALL
    x = (W.data_tensor("attn_long.vit.image", (2, 3, resolution, resolution)) * 0.25 + 0.5).to(dev)
    y = m(x)
    y.float().square().sum().backward()
    assert bool(torch.isfinite(y.float()).all())
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), n
    return tuple(y.shape)


def case_m2_long_image_rows(dev, image_size=144):
    """A tiny M2 (model_cases.TINY_M2) at image_size 144 -- 18 x 18 + 1 = 325 image tokens -- against the CPU oracle's ITC step on the same weights: loss and
    gradients the way model_cases.case_m2_itc_vs_oracle compares them, with that case's tolerances (loss 1e-3 relative, gradient norms 5 %, directions)."""
    import model_cases as mc
    import weightgen as W
    import tiny_models
    from oracle import step as ostep
    from vlmo.config import default_config
    from vlmo.modules.vlmo_module import VLMo

    cfg = default_config()
    cfg.update(dict(mc.TINY_M2, image_size=image_size))
    model = VLMo(cfg)
    W.fill_module_(model)
    model = model.to(dev).train()
    shapes = tiny_models.m2_shapes()
    P = {n: p.detach().float().cpu().clone().requires_grad_(True) for n, p in model.named_parameters() if n in shapes}
    assert len(P) > 50
    lengths = torch.tensor([12, 5, 8, 3])
    mask = (torch.arange(12)[None, :] < lengths[:, None]).long()
    img = (W.data_tensor("attn_long.m2.image", (4, 3, image_size, image_size)) * 0.25 + 0.5).clamp(0, 1)
    ids = W.data_ints("m2s.ids", (4, 12), 1, 300) * mask
    out = model({"image": [img.to(dev)], "text_ids": ids.to(dev), "text_masks": mask.to(dev)})
    loss = out["losses"]["itc_loss"] + out["losses"]["itc_vl_loss"]
    ref = ostep.m2_itc(P, img, ids, mask, heads=2, patch=8)
    rel = (float(loss) - float(ref["loss"])) / abs(float(ref["loss"]))
    print(f"m2 long rows: loss {float(loss):.6f} oracle {float(ref['loss']):.6f} rel {rel:+.3e}")
    assert abs(rel) <= 1e-3, rel
    loss.backward()
    ref["loss"].backward()
    named = dict(model.named_parameters())
    rels = []
    gold = {f"gfull.{n}": p.grad for n, p in P.items() if p.grad is not None}
    for n, p in P.items():
        if p.grad is None or named[n].grad is None or float(p.grad.norm()) < 1e-6:
            continue
        rn = float(p.grad.norm())
        rels.append((abs(float(named[n].grad.float().norm()) - rn) / rn, n))
    rels.sort(reverse=True)
    print("m2 long rows: worst gradient norms", rels[:3])
    assert len(rels) > 50 and rels[0][0] < 0.05, rels[:5]
    mc.assert_grad_directions(named.items(), gold, "", min_checked=50)
