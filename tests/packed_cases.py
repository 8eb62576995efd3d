"""Parity cases of the token-packed text path (packed attention / embedding entry points against the strided ones), shared by the emulator and the GPU suites.
`ops` is antmmf.hip.ops bound to whichever library is loaded; every case returns the figures it checked."""
import torch

BF = torch.bfloat16
LENGTHS = (1, 8, 32, 33, 64, 77)
SENTINEL = 7.0   # exactly representable in bf16: rows the packed kernels must not write keep it bit for bit


def item_table(lengths, device):
    ln = torch.tensor(lengths, dtype=torch.int32)
    off = torch.cumsum(ln, 0, dtype=torch.int32) - ln
    return torch.stack([off, ln], dim=1).contiguous().to(device)


def pack_rows(x, lengths, T, fill=0.0):
    """[B, N, D] -> [T, D]: the first lengths[b] rows of every item, item after item; the other rows hold `fill`"""
    out = torch.full((T, x.shape[-1]), fill, dtype=x.dtype, device=x.device)
    r = 0
    for b, n in enumerate(lengths):
        out[r:r + n] = x[b, :n]
        r += n
    return out


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == BF else t.contiguous().view(torch.int32)


def assert_rows_identical(packed, padded, lengths, what):
    r = 0
    for b, n in enumerate(lengths):
        assert torch.equal(_bits(packed[r:r + n]), _bits(padded[b, :n])), f"{what}: item {b} (length {n}) differs from the strided entry point"
        r += n
    return r


def case_attention_packed(ops, dev, lengths=LENGTHS, heads=2, n_max=77, slack=77, seed=0):
    """Forward, backward and token sums over one packed batch against the strided entry points under a -inf prefix key_bias: item rows bit-identical in o, lse, dq, dk, dv;
    token sums equal up to fp32 summation order; every row of no item (the slack behind the last item) untouched."""
    g = torch.Generator().manual_seed(seed)
    B, D = len(lengths), 64 * heads
    scale = 0.125
    qkv = (torch.randn(B, n_max, 3 * D, generator=g) * 0.7).to(BF).to(dev)
    d_o = (torch.randn(B, n_max, D, generator=g) * 0.5).to(BF).to(dev)
    ln = torch.tensor(lengths, device=dev)
    valid = torch.arange(n_max, device=dev)[None, :] < ln[:, None]
    d_o = d_o * valid[..., None].to(BF)            # padded rows carry no gradient (their outputs are never read)
    key_bias = torch.zeros(B, n_max, dtype=torch.float32, device=dev).masked_fill_(~valid, float("-inf"))
    q, k, v = qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:]
    o_ref, lse_ref = ops.attention_fwd(q, k, v, heads, scale, key_bias)
    dqkv_ref = torch.empty_like(qkv)
    sums_ref = torch.empty(B, 3 * D, dtype=torch.float32, device=dev)
    assert ops.attention_bwd_sums_ok(64, n_max, n_max)
    ops.attention_bwd(q, k, v, o_ref, lse_ref, d_o, heads, scale, key_bias, dq=dqkv_ref[..., :D], dk=dqkv_ref[..., D:2 * D], dv=dqkv_ref[..., 2 * D:], sums=sums_ref)
    dqkv_ref2 = torch.empty_like(qkv)
    ops.attention_bwd(q, k, v, o_ref, lse_ref, d_o, heads, scale, key_bias, dq=dqkv_ref2[..., :D], dk=dqkv_ref2[..., D:2 * D], dv=dqkv_ref2[..., 2 * D:])

    assert ops.attention_packed_ok(64, n_max) and not ops.attention_packed_ok(64, 32) and not ops.attention_packed_ok(128, n_max) and not ops.attention_packed_ok(64, 129)
    total = sum(lengths)
    T = total + slack
    items = item_table(lengths, dev)
    qkv_p = pack_rows(qkv, lengths, T, fill=SENTINEL)   # (finite garbage in the rows of no item: nothing may depend on it)
    do_p = pack_rows(d_o, lengths, T, fill=SENTINEL)
    qp, kp, vp = qkv_p[:, :D], qkv_p[:, D:2 * D], qkv_p[:, 2 * D:]
    o_p = torch.full((T, D), SENTINEL, dtype=BF, device=dev)
    o_p, lse_p = ops.attention_fwd_packed(qp, kp, vp, items, heads, scale, n_max, o=o_p)
    assert assert_rows_identical(o_p, o_ref, lengths, "o") == total
    assert torch.equal(_bits(o_p[total:]), _bits(torch.full((slack, D), SENTINEL, dtype=BF, device=dev))), "o: rows of no item were written"
    for b, n in enumerate(lengths):
        assert torch.equal(_bits(lse_p[b, :, :n]), _bits(lse_ref[b, :, :n])), f"lse: item {b}"
    out = {}
    for with_sums in (True, False):
        dqkv_p = torch.full((T, 3 * D), SENTINEL, dtype=BF, device=dev)
        sums_p = torch.empty(B, 3 * D, dtype=torch.float32, device=dev) if with_sums else None
        ops.attention_bwd_packed(qp, kp, vp, items, o_p, lse_p, do_p, heads, scale, n_max, dqkv_p[:, :D], dqkv_p[:, D:2 * D], dqkv_p[:, 2 * D:], sums=sums_p)
        ref = dqkv_ref if with_sums else dqkv_ref2
        for i, nm in enumerate(("dq", "dk", "dv")):
            assert_rows_identical(dqkv_p[:, i * D:(i + 1) * D], ref[..., i * D:(i + 1) * D], lengths, nm)
        assert torch.equal(_bits(dqkv_p[total:]), _bits(torch.full((slack, 3 * D), SENTINEL, dtype=BF, device=dev))), "dq | dk | dv: rows of no item were written"
        if with_sums:
            # the same fp32 terms in another order (here: the zero terms of the padded rows are absent): a few ulp of the largest partial sum
            err = (sums_p - sums_ref).abs().max().item()
            tol = 1e-5 * max(1.0, sums_ref.abs().max().item())
            out["sums_max_abs_diff"] = err
            assert err <= tol, (err, tol)
    return out


def case_embed_packed(ops, dev, lengths=LENGTHS, seq=77, d=64, vocab=50, seed=1, big=False):
    """Packed embedding gather against the padded kernel with zeroed padded rows, and both gradient scatters (word table: sorted form with packed source rows when `big`
    makes the row count reach the sorted path; position table) against the padded kernels fed the unpacked gradient."""
    g = torch.Generator().manual_seed(seed)
    if big:
        reps = ops.SCATTER_SORT_MIN_ROWS // (seq * len(lengths)) + 1
        lengths = tuple(lengths) * reps
    B = len(lengths)
    ids = torch.randint(1, vocab, (B, seq), generator=g).to(dev)
    ln = torch.tensor(lengths, device=dev)
    valid = torch.arange(seq, device=dev)[None, :] < ln[:, None]
    ids = ids * valid
    word = torch.randn(vocab, d, generator=g).to(dev)
    pos = torch.randn(seq + 2, d, generator=g).to(dev)
    zero_rows = (~valid).to(torch.uint8).contiguous()
    ref = ops.embed_gather(ids, word, pos, None, None, zero_rows, 2)
    total = sum(lengths)
    T = total + 5
    items = item_table(lengths, dev)
    out = torch.full((T, d), SENTINEL, dtype=BF, device=dev)
    ops.embed_gather_packed(ids, word, pos, items, out, 2)
    assert assert_rows_identical(out, ref, lengths, "embedding") == total
    assert torch.equal(_bits(out[total:]), _bits(torch.full((5, d), SENTINEL, dtype=BF, device=dev)))
    # gradients
    dx = (torch.randn(B, seq, d, generator=g)).to(BF).to(dev) * valid[..., None].to(BF)
    dx_p = pack_rows(dx, lengths, T, fill=SENTINEL)
    dpos_ref = ops.embed_scatter_add_(torch.zeros_like(pos), dx, None, zero_rows, seq=seq, offset=2)
    dpos = ops.embed_scatter_add_pos_packed_(torch.zeros_like(pos), dx_p, items, seq, offset=2)
    assert torch.allclose(dpos, dpos_ref, rtol=1e-5, atol=1e-5 * max(1.0, dpos_ref.abs().max().item())), (dpos - dpos_ref).abs().max()
    dword_ref = ops.embed_scatter_add_(torch.zeros_like(word), dx, ids.contiguous(), zero_rows)
    keys = torch.where(valid.reshape(-1), ids.reshape(-1), torch.full_like(ids.reshape(-1), vocab))
    sorted_idx, src = torch.sort(keys, stable=True)
    packed_row = (items[:, :1].long() + torch.arange(seq, device=dev)[None, :]).reshape(-1)
    dword = ops.embed_scatter_add_sorted_(torch.zeros_like(word), dx_p, sorted_idx, packed_row[src].contiguous())
    if big:   # (both through the sorted kernel, same order within a run: identical)
        assert torch.equal(dword, dword_ref)
    else:
        assert torch.allclose(dword, dword_ref, rtol=1e-5, atol=1e-5 * max(1.0, dword_ref.abs().max().item()))
    return {"rows": total}


# ------------------------------------------------------------------------------------------------ model level (tiny M2 dual tower, captions wide enough to be packed)
def ragged_text_batch(dev, B, seq, seed=0, must_have=(1, 8), vocab=300):
    """lengths: `must_have`, the full width, random ones in between"""
    g = torch.Generator().manual_seed(seed)
    lengths = list(must_have) + [seq] + torch.randint(2, seq + 1, (B - len(must_have) - 1,), generator=g).tolist()
    ln = torch.tensor(lengths)
    mask = (torch.arange(seq)[None, :] < ln[:, None]).long()
    ids = torch.randint(1, vocab, (B, seq), generator=g) * mask
    img = torch.rand(B, 3, 32, 32, generator=g)
    return {"image": [img.to(dev)], "text_ids": ids.to(dev), "text_masks": mask.to(dev)}, lengths


class pack_text:
    """with pack_text(False): the padded path of the same build"""

    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        from antmmf.hip import functional as HF

        self.HF, self.old = HF, HF.PACK_TEXT
        HF.PACK_TEXT = self.flag

    def __exit__(self, *exc):
        self.HF.PACK_TEXT = self.old


def case_infer_text_packed(dev, model, seq=77, B=12):
    """infer_text packed against the same build's padded path: cls_feats / cls_vlffn_feats bit-identical, text_feats (lazy unpack) identical on the real tokens"""
    from antmmf.hip import functional as HF

    batch, lengths = ragged_text_batch(dev, B, seq, seed=11)
    with torch.no_grad():
        assert HF.packed_text_finish(HF.packed_text_begin(batch["text_masks"])) is not None, "this batch must take the packed path"
        with pack_text(True):
            got = model.infer_text(batch)
        with pack_text(False):
            ref = model.infer_text(batch)
    assert type(got) is not dict and type(ref) is dict
    for k in ("cls_feats", "cls_vlffn_feats"):
        assert torch.equal(_bits(got[k]), _bits(ref[k])), f"{k}: packed differs from padded (max abs {float((got[k].float() - ref[k].float()).abs().max())})"
    tf = got["text_feats"]
    assert tf.shape == ref["text_feats"].shape
    for b, n in enumerate(lengths):
        assert torch.equal(_bits(tf[b, :n]), _bits(ref["text_feats"][b, :n])) and float(tf[b, n:].abs().sum()) == 0.0
    return {"lengths": lengths}


def case_non_prefix_mask_takes_padded_path(dev, model, seq=77, B=6):
    from antmmf.hip import functional as HF

    batch, _ = ragged_text_batch(dev, B, seq, seed=12)
    m = batch["text_masks"].clone()
    m[2, 1] = 0          # a hole in item 2 (its length is the full width): real tokens are no longer a prefix
    batch["text_masks"] = m
    batch["text_ids"] = batch["text_ids"] * m
    with torch.no_grad():
        assert HF.packed_text_finish(HF.packed_text_begin(m)) is None
        with pack_text(True):
            got = model.infer_text(batch)
        with pack_text(False):
            ref = model.infer_text(batch)
    assert type(got) is dict
    for k in ("cls_feats", "cls_vlffn_feats", "text_feats"):
        assert torch.equal(_bits(got[k]), _bits(ref[k])), k


def _itc_grads(model, batch):
    for p in model.parameters():
        p.grad = None
    out = model(batch)
    loss = out["losses"]["itc_loss"] + out["losses"]["itc_vl_loss"]
    loss.backward()
    return loss.detach().clone(), {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}


def case_itc_grad_parity(dev, model, seq=77, B=12):
    """One compute_itc + backward, packed against padded: loss bit-identical; per-parameter relative gradient difference (L2) at most 4 x the MEASURED noise floor of the
    padded path itself -- the same step with the batch items permuted (same mathematics, another summation order).  -> rows for the parity record."""
    batch, lengths = ragged_text_batch(dev, B, seq, seed=13)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(14)).to(dev)
    batch_perm = {"image": [batch["image"][0][perm]], "text_ids": batch["text_ids"][perm], "text_masks": batch["text_masks"][perm]}
    with pack_text(False):
        loss_a, g_a = _itc_grads(model, batch)
        _, g_b = _itc_grads(model, batch_perm)
    with pack_text(True):
        loss_p, g_p = _itc_grads(model, batch)
    rows, bad = [], []
    for n, ga in g_a.items():
        na = float(ga.norm())
        floor = float((g_b[n] - ga).norm()) / na if na > 0 else 0.0
        diff = float((g_p[n] - ga).norm()) / na if na > 0 else float(g_p[n].norm())
        rows.append({"param": n, "grad_norm": na, "floor_rel": floor, "packed_rel": diff, "ratio": (diff / floor) if floor > 0 else (0.0 if diff == 0 else float("inf"))})
        print(f"grad parity {n}: |g| {na:.4e} floor {floor:.3e} packed-vs-padded {diff:.3e}")
        if diff > 4 * floor:
            bad.append((n, floor, diff))
    print(f"loss padded {float(loss_a)!r} packed {float(loss_p)!r}")
    assert set(g_p) == set(g_a)
    return {"loss_padded": float(loss_a), "loss_packed": float(loss_p), "loss_identical": bool(torch.equal(loss_a, loss_p)), "rows": rows, "bad": bad, "lengths": lengths}
