"""Cases of the attention probability maps on request (csrc/attention.hip::attn_probs_kernel behind antmmf_attention_probs, ops.attention_probs,
functional.attention(return_probs=True), BertEncoder(output_attentions="maps"), BertBiAttention(visualization=True)), shared by the emulator and the GPU suites.

Expected values are plain fp64 torch on the SAME bf16-rounded q / k: softmax(q k^T scale + key_bias), times dropout_keep_np(idx, seed, p) / (1 - p) -- with the
kernel's stated rule for a query row whose keys are all at -inf (zeros, where the softmax gives NaN).

Tolerance of the maps (fp32 output, so not the bf16 kernels' 2e-2): the largest absolute error against that expectation over the whole of case 1 (`MAP_SHAPES_*`, both
head sizes, packed and separate operands) is MEASURED_MAP_ERR below; the gate is 4 x the larger of the emulator's and the MI355X's figure (room for the hardware's
v_exp_f32 / v_log_f32, the MFMA summation order and the forward kernel's own lse), and may never exceed 1e-3.  The row sums of valid query rows get the same treatment
(MEASURED_ROWSUM_ERR: |sum - 1|).  Every case prints its figures before it asserts.
    emulator (28 cases of tests/test_attn_probs_emu.py): map 3.31e-07 (dh 128, 17 x 15), row sum 6.65e-07 (dh 64, 65 x 97)
    MI355X (32 cases of tests/test_attn_probs_gpu.py, profiles/attn_probs_pytest_gpu.log): map 2.00e-07 (dh 128, 17 x 15), row sum 8.64e-07 (dh 128, 77 x 77 packed)
    gates: map 4 x 3.31e-07 = 1.32e-06, row sum 4 x 8.64e-07 = 3.46e-06 -- a few fp32 roundings of a probability <= 1 and of the lse it is normalised by
"""
import math

import numpy as np
import torch

from kernel_cases import BF, check, dropout_keep_np, q as bfq, rnd

EINVAL = -22
MEASURED_MAP_ERR = {"emulator": 3.31e-07, "mi355x": 2.00e-07}
MEASURED_ROWSUM_ERR = {"emulator": 6.65e-07, "mi355x": 8.64e-07}
MAP_ATOL = 4.0 * max(MEASURED_MAP_ERR.values())
ROWSUM_ATOL = 4.0 * max(MEASURED_ROWSUM_ERR.values())
assert MAP_ATOL <= 1e-3 and ROWSUM_ATOL <= 1e-3

# (Nq, Nk): Nk % 4 in {0, 1, 3}, a last key tile with a single key (33, 65, 257), more query tiles than waves (257, 288), the cross-length ViLBERT shape (37, 21)
MAP_SHAPES = [(1, 1), (16, 16), (17, 15), (21, 33), (77, 77), (37, 21)]
MAP_SHAPES_EMU = MAP_SHAPES + [(65, 97)]            # the multi-chunk case the emulator affords
MAP_SHAPES_GPU = MAP_SHAPES + [(257, 257), (288, 288)]


def split_heads(t, heads):
    b, n, d = t.shape
    return t.view(b, n, heads, d // heads).permute(0, 2, 1, 3)


def expected_maps(qt, kt, heads, scale, key_bias=None, p=0.0, seed=0):
    """fp64 [B, heads, Nq, Nk] from the bf16-rounded q / k (any float dtype, any device)"""
    qh, kh = split_heads(qt.detach().cpu().double(), heads), split_heads(kt.detach().cpu().double(), heads)
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if key_bias is not None:
        s = s + key_bias.detach().cpu().double()[:, None, None, :]
    dead = torch.isinf(s).all(-1, keepdim=True)        # every key at -inf: the kernel's rule is a row of zeros
    pr = torch.softmax(s.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0)
    if p > 0:
        pr = pr * dropout_keep_np(np.arange(pr.numel()).reshape(pr.shape), seed, p).double() / (1.0 - p)
    return pr


def _operands(B, heads, dh, Nq, Nk, dev, packed, seed):
    """bf16 q, k, v on `dev`: three views of one packed [B, N, 3 d] buffer (a self-attention projection) or three separate tensors"""
    d = heads * dh
    if packed:
        assert Nq == Nk
        buf = bfq(rnd((B, Nq, 3 * d), seed)).to(dev, BF)
        return buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
    return tuple(bfq(rnd((B, n, d), seed + i)).to(dev, BF) for i, n in enumerate((Nq, Nk, Nk)))


def _map_errors(got, want):
    g = got.detach().cpu().double()
    return float((g - want).abs().max()), float((g.sum(-1) - want.sum(-1)).abs().max())


def case_maps(ops, dev, dh, Nq, Nk, B=1, heads=2, packed=False):
    """Maps without dropout against the fp64 expectation; every query row sums to 1.  -> (largest absolute error, largest row-sum error)"""
    qd, kd, vd = _operands(B, heads, dh, Nq, Nk, dev, packed, 600 + Nq + Nk)
    scale = dh ** -0.5
    _, lse = ops.attention_fwd(qd, kd, vd, heads, scale)
    got = ops.attention_probs(qd, kd, lse, heads, scale)
    assert got.shape == (B, heads, Nq, Nk) and got.dtype == torch.float32
    want = expected_maps(qd, kd, heads, scale)
    err, rerr = _map_errors(got, want)
    print(f"attn_probs.maps[dh {dh}, {Nq} x {Nk}, B {B}, heads {heads}, {'packed' if packed else 'separate'}]: max abs err {err:.3g} (gate {MAP_ATOL:.3g}), "
          f"row sum err {rerr:.3g} (gate {ROWSUM_ATOL:.3g})")
    assert torch.isfinite(got).all()
    assert err <= MAP_ATOL, (err, MAP_ATOL)
    assert rerr <= ROWSUM_ATOL, (rerr, ROWSUM_ATOL)
    return err, rerr


def case_masks(ops, dev, dh, N=21):
    """One batch: no mask | a -10000 tail | a -inf tail | every key at -inf.  Masked keys are exactly 0 under -inf; the fully masked item is zeros, no NaN."""
    B, heads = 4, 1
    qd, kd, vd = _operands(B, heads, dh, N, N, dev, False, 640)
    kb = torch.zeros(B, N)
    kb[1, 9:] = -10000.0
    kb[2, 9:] = float("-inf")
    kb[3, :] = float("-inf")
    scale = dh ** -0.5
    _, lse = ops.attention_fwd(qd, kd, vd, heads, scale, kb.to(dev))
    got = ops.attention_probs(qd, kd, lse, heads, scale, kb.to(dev))
    assert torch.isfinite(got).all(), "NaN / inf in the maps"
    g = got.cpu()
    assert float(g[2, :, :, 9:].abs().max()) == 0.0, "a key masked with -inf has a non-zero probability"
    assert float(g[3].abs().max()) == 0.0, "the item with every key at -inf is not a map of zeros"
    want = expected_maps(qd, kd, heads, scale, kb)
    err, rerr = _map_errors(got[:3], want[:3])
    print(f"attn_probs.masks[dh {dh}]: max abs err {err:.3g}, row sum err {rerr:.3g}")
    assert err <= MAP_ATOL and rerr <= ROWSUM_ATOL, (err, rerr)
    assert float((g[:3].sum(-1) - 1.0).abs().max()) <= ROWSUM_ATOL


def case_dropout(ops, dev, dh, N=21):
    """p = 0.2 with a 64-bit seed: zeros exactly where the host twin of the mask drops, values as expected, and probs @ v equals the o of the forward with the
    same p and seed (kernel_cases.case_dropout's 2e-2 / 2e-2): the mask is the forward's, not merely a mask."""
    B, heads, p, seed = 2, 2, 0.2, (77 << 32) | 4242
    qd, kd, vd = _operands(B, heads, dh, N, N, dev, True, 650)
    kb = torch.zeros(B, N).masked_fill(~(torch.arange(N)[None, :] < torch.tensor([N, 9])[:, None]), -10000.0)
    scale = dh ** -0.5
    o, lse = ops.attention_fwd(qd, kd, vd, heads, scale, kb.to(dev), dropout_p=p, dropout_seed=seed)
    got = ops.attention_probs(qd, kd, lse, heads, scale, kb.to(dev), dropout_p=p, dropout_seed=seed)
    keep = dropout_keep_np(np.arange(got.numel()).reshape(got.shape), seed, p)
    g = got.cpu()
    assert 0 < int((~keep).sum()) < keep.numel()
    assert float(g[~keep].abs().max()) == 0.0, "a dropped element is not exactly 0"
    want = expected_maps(qd, kd, heads, scale, kb, p, seed)
    err = float((g.double() - want).abs().max())
    print(f"attn_probs.dropout[dh {dh}]: max abs err {err:.3g} (gate {MAP_ATOL / (1 - p):.3g})")
    assert err <= MAP_ATOL / (1 - p), err      # kept elements are scaled by 1 / (1 - p), and so is their error
    ctx = torch.matmul(g, split_heads(vd.float().cpu(), heads)).permute(0, 2, 1, 3).reshape(B, N, heads * dh)
    check("attn_probs.dropout.pv_vs_forward_o", o, ctx, 2e-2, 2e-2)


def case_importance(ops, dev, N=21):
    """attention_key_importance_ at head size 128 (the new kernel's importance output), accumulated into a buffer pre-filled with 0.5, with and without dropout;
    head size 64 (its own, older kernel family, unchanged) against the head mean / query sum of the maps; and one call with both outputs."""
    B, heads, p, seed = 2, 2, 0.2, (77 << 32) | 4242
    kb = torch.zeros(B, N).masked_fill(~(torch.arange(N)[None, :] < torch.tensor([N, 9])[:, None]), -10000.0)
    for dh in (128, 64):
        qd, kd, vd = _operands(B, heads, dh, N, N, dev, True, 660)
        scale = dh ** -0.5
        for pp, ss in ((p, seed), (0.0, 0)):
            _, lse = ops.attention_fwd(qd, kd, vd, heads, scale, kb.to(dev), dropout_p=pp, dropout_seed=ss)
            imp = torch.full((B, N), 0.5, device=dev)
            ops.attention_key_importance_(imp, qd, kd, lse, heads, scale, kb.to(dev), dropout_p=pp, dropout_seed=ss, weight=1.0 / heads)
            want = expected_maps(qd, kd, heads, scale, kb, pp, ss)
            check(f"attn_probs.importance[dh {dh}, p {pp}]", imp, 0.5 + want.mean(1).sum(1).float(), 2e-2, 2e-2)
            maps = ops.attention_probs(qd, kd, lse, heads, scale, kb.to(dev), dropout_p=pp, dropout_seed=ss)
            # NOT bit-identical, at either head size: the importance leaves both kernels through fp32 atomics (waves into the LDS strip, heads into the buffer) whose
            # order is not fixed, and torch's mean / sum add in yet another order.  Compared as kernel_cases.case_dropout compares the importance: 2e-2 / 2e-2
            print(f"attn_probs.importance[dh {dh}, p {pp}]: max |importance - maps.mean(1).sum(1)| = {float((imp - 0.5 - maps.mean(1).sum(1)).abs().max()):.3g}")
            check(f"attn_probs.importance_vs_maps[dh {dh}, p {pp}]", imp - 0.5, maps.mean(1).sum(1), 2e-2, 2e-2)
            # both outputs from ONE launch against the separate calls: the same arithmetic per element (bit-equal maps); the sums differ by the order of at most
            # heads * N fp32 additions of terms <= 1 / (1 - p) (2 * 21 * 2^-24 = 2.5e-6 of the result: 1e-5)
            both_p, both_i = torch.full_like(maps, 7.0), torch.full((B, N), 0.5, device=dev)
            ops.attention_probs_into(qd, kd, lse, heads, scale, kb.to(dev), pp, ss, probs=both_p, importance=both_i, weight=1.0 / heads)
            assert torch.equal(both_p, maps)
            only_i = torch.full((B, N), 0.5, device=dev)
            ops.attention_probs_into(qd, kd, lse, heads, scale, kb.to(dev), pp, ss, importance=only_i, weight=1.0 / heads)
            check(f"attn_probs.both_outputs[dh {dh}, p {pp}]", both_i, only_i, 1e-5, 1e-5)


def case_refusals(ops, dev):
    """289 queries, 289 keys, head size 96, no output: ANTMMF_EINVAL from the entry point (nothing launched: the outputs keep their fill), ValueError from ops."""
    from antmmf.hip import _lib

    lib = _lib.load()
    p, st = ops._p, ops._stream()
    for what, dh, Nq, Nk, outs in (("Nq", 64, 289, 16, 3), ("Nk", 64, 16, 289, 3), ("head size", 96, 16, 16, 3), ("outputs", 64, 16, 16, 0)):
        heads = 2
        d = heads * dh
        qd, kd = torch.zeros(1, Nq, d, dtype=BF, device=dev), torch.zeros(1, Nk, d, dtype=BF, device=dev)
        lse = torch.zeros(1, heads, Nq, device=dev)
        probs, imp = torch.full((1, heads, Nq, Nk), 7.0, device=dev), torch.full((1, Nk), 7.0, device=dev)
        rc = lib.antmmf_attention_probs(p(qd), p(kd), 0, p(lse), p(probs) if outs else 0, p(imp) if outs else 0, 1, heads, dh, Nq, Nk, d, d, 0.125, 0.0, 0, 1.0, st)
        assert rc == EINVAL, (what, rc)
        assert bool((probs == 7.0).all()) and bool((imp == 7.0).all()), f"{what}: a refused call wrote an output"
        try:
            if outs:
                ops.attention_probs(qd, kd, lse, heads, 0.125)
            else:
                ops.attention_probs_into(qd, kd, lse, heads, 0.125)
        except ValueError:
            pass
        else:
            raise AssertionError(f"ops accepted a bad {what}")
    # the limit itself is served
    qd, kd, vd = _operands(1, 1, 64, 288, 288, dev, True, 670)
    _, lse = ops.attention_fwd(qd, kd, vd, 1, 0.125)
    assert ops.attention_probs(qd, kd, lse, 1, 0.125).shape == (1, 1, 288, 288)


def _tiny_bert_encoder(dev, output_attentions=False, p=0.0):
    import weightgen as W
    from antmmf.modules.vision.backbone.clip.configuration_bert import BertConfig
    from antmmf.modules.vision.backbone.clip.modeling_bert import BertEncoder

    cfg = BertConfig(vocab_size_or_config_json_file=50, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256, hidden_act="gelu",
                     hidden_dropout_prob=p, attention_probs_dropout_prob=p, layer_norm_eps=1e-12, output_attentions=output_attentions)
    return W.fill_module_(BertEncoder(cfg)).to(dev)      # (name-keyed fill: every encoder built here has the same weights)


def case_bert_encoder(dev, B=2, N=12):
    """BertEncoder(output_attentions="maps"), call argument and constructor flag: 2 maps of [B, heads, N, N] whose rows sum to 1 and whose head mean / query sum over
    the layers is the KeyImportance of an output_attentions=True run (2e-2, kernel_cases' figure for that reduction); hidden states bit-identical to a run
    without the flag; in training mode with dropout the maps hold exact zeros and the hidden states equal the no-flag run with the same seeds."""
    import weightgen as W
    from antmmf.modules.vision.backbone.clip.modeling_bert import KeyImportance

    heads = 2
    x = W.data_tensor("attn_probs.bert.x", (B, N, 128)).to(dev, BF)
    kb = ((1.0 - (torch.arange(N)[None, :] < torch.tensor([N, 7])[:, None]).float()) * -10000.0).to(dev)
    enc = _tiny_bert_encoder(dev).eval()
    plain = enc(x, kb)
    assert len(plain) == 1
    out = enc(x, kb, output_attentions="maps")
    maps = out[-1]
    assert isinstance(maps, tuple) and len(maps) == 2 and all(m.shape == (B, heads, N, N) and m.dtype == torch.float32 and not m.requires_grad for m in maps)
    assert torch.equal(out[0], plain[0]), "asking for the maps changed the hidden states"
    for m in maps:
        assert float((m.sum(-1) - 1.0).abs().max()) <= ROWSUM_ATOL
        assert float(m[1, :, :, 7:].abs().max()) == 0.0      # exp(-10000) is 0 in fp32 too
    imp = enc(x, kb, output_attentions=True)[-1]
    assert isinstance(imp, KeyImportance)
    check("attn_probs.bert.maps_vs_key_importance", sum(m.mean(1).sum(1) for m in maps), imp.value, 2e-2, 2e-2)
    flagged = _tiny_bert_encoder(dev, output_attentions="maps").eval()(x, kb)      # the constructor flag, through BertConfig
    assert len(flagged) == 2 and all(torch.equal(a, b) for a, b in zip(flagged[-1], maps))
    try:
        enc(x, kb, output_attentions="probabilities")
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown output_attentions string was accepted")
    # training mode, dropout 0.1 on the probabilities and the dense outputs, the layers' seeds drawn from torch's CPU generator
    tr = _tiny_bert_encoder(dev, p=0.1).train()
    with torch.no_grad():
        torch.manual_seed(1234)
        h0 = tr(x, kb)[0]
        torch.manual_seed(1234)
        h1, tmaps = tr(x, kb, output_attentions="maps")
    assert torch.equal(h0, h1)
    for m in tmaps:
        live = m[0]                                    # item 0 has no masked key: its zeros are dropped elements
        zeros = float((live == 0).float().mean())
        assert 0.03 <= zeros <= 0.25, zeros           # p = 0.1 over heads * N * N = 288 elements (sigma 0.018)
        assert float(live.max()) > 0.0 and torch.isfinite(m).all()


def case_vilbert_visualization(dev, head_size, B=2, Nv=37, Nt=21):
    """BertBiAttention(visualization=True): the reference's six keys; attn1 [B, h, Nt, Nv] / attn2 [B, h, Nv, Nt] match the fp64 expectation from the dict's own
    queries / keys; ctx1 / ctx2 bit-identical to the visualization=False module with the same weights."""
    import weightgen as W
    from antmmf.common.configuration import Configuration
    from antmmf.models.vilbert import BertBiAttention

    heads = 2
    cfg = dict(bi_hidden_size=heads * head_size, bi_num_attention_heads=heads, v_hidden_size=96, hidden_size=128, v_attention_probs_dropout_prob=0.1,
               attention_probs_dropout_prob=0.1)
    vis = W.fill_module_(BertBiAttention(Configuration(dict(cfg, visualization=True)))).to(dev).eval()
    ref = W.fill_module_(BertBiAttention(Configuration(dict(cfg, visualization=False)))).to(dev).eval()
    x1 = W.data_tensor("attn_probs.bi.x1", (B, Nv, 96)).to(dev, BF)
    x2 = W.data_tensor("attn_probs.bi.x2", (B, Nt, 128)).to(dev, BF)
    m1 = ((1.0 - (torch.arange(Nv)[None, :] < torch.tensor([Nv, 30])[:, None]).float()) * -10000.0).view(B, 1, 1, Nv).to(dev)
    m2 = ((1.0 - (torch.arange(Nt)[None, :] < torch.tensor([13, Nt])[:, None]).float()) * -10000.0).view(B, 1, 1, Nt).to(dev)
    with torch.no_grad():
        c1, c2, data = vis(x1, m1, x2, m2)
        r1, r2, none = ref(x1, m1, x2, m2)
    assert none is None and torch.equal(c1, r1) and torch.equal(c2, r2)
    assert set(data) == {"attn1", "queries1", "keys1", "attn2", "querues2", "keys2"}
    assert data["attn1"].shape == (B, heads, Nt, Nv) and data["attn2"].shape == (B, heads, Nv, Nt)
    assert data["queries1"].shape == (B, heads, Nt, head_size) and data["keys1"].shape == (B, heads, Nv, head_size)
    assert data["querues2"].shape == (B, heads, Nv, head_size) and data["keys2"].shape == (B, heads, Nt, head_size)
    merge = lambda t: t.permute(0, 2, 1, 3).reshape(t.shape[0], t.shape[2], -1)   # noqa: E731
    for a, qn, kn, mask in (("attn1", "queries1", "keys1", m1), ("attn2", "querues2", "keys2", m2)):
        want = expected_maps(merge(data[qn]), merge(data[kn]), heads, 1.0 / math.sqrt(head_size), mask.reshape(B, -1))
        err, rerr = _map_errors(data[a], want)
        print(f"attn_probs.vilbert[{head_size}].{a}: max abs err {err:.3g}, row sum err {rerr:.3g}")
        assert err <= MAP_ATOL and rerr <= ROWSUM_ATOL, (a, err, rerr)


def case_packed_with_map_collector(dev):
    """A token-packed layer input while a map collector is set: the ValueError the key-importance collector gets."""
    import pytest
    import weightgen as W
    from antmmf.hip import functional as HF

    layer = _tiny_bert_encoder(dev).eval().layer[0]
    items = torch.tensor([[0, 5], [5, 40]], dtype=torch.int32, device=dev)
    text = HF.PackedText(items, 77, 45, 64)
    x = W.data_tensor("attn_probs.packed.x", (64, 128)).to(dev, BF)
    HF.ATTENTION_MAPS = []
    try:
        with pytest.raises(ValueError, match="collector"):
            HF.transformer_layer(x, layer._spec, layer._params(), packed=text)
        assert HF.ATTENTION_MAPS == []
    finally:
        HF.ATTENTION_MAPS = None
