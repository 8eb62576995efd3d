#!/usr/bin/env python
"""M2-Encoder 10B (Encoder_10B.json: beit huge, d = 4096, 32 heads of 128, FFN 16384, 21 + 3 layers) on one MI355X.

    python tools/m2_huge_bench.py [--batch 64] [--train-batch 8] [--iters 20] [--skip-train]      -> JSON lines, one per measurement

  ln       the wide LayerNorm kernels alone (ln_wide_fwd_kernel / ln_wide_bwd_kernel) on the 10B model's ffn_layernorm rows: cols 16384,
           rows = B * 197 (image tower) and B * 52 (text tower), fused GELU, statistics written, backward with dxsum through the partials slab
           (what the layer launches); ms per launch (HIP events over `iters` launches after a warm-up), algorithmic GB/s (fwd 2 * cols * 2 B + 8 B
           per row, bwd 3 * cols * 2 B per row) and its fraction of 8 TB/s
  attn     the head-128 attention kernels at the same rows (forward, backward): ms per launch
  embed    full-depth towers with random weights built ON the device (no 40 GB of fp32 weights in host RAM), no_grad, eval mode,
           at --batch (one eval_retrieval.extract_feats pass first, then infer_image / infer_text timed: the calls it makes); images/s and texts/s
  train    one ITC training step (forward + backward + HipAdamW) at --train-batch with its peak device memory; an out-of-memory is reported as such
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ant-multi-modal-framework_amd")
sys.path[:0] = [PKG, os.path.join(PKG, "prj", "M2_Encoder"), ROOT]
CONFIG_10B = os.path.join(ROOT, "tests", "golden", "Encoder_10B.json")
DEV = torch.device("cuda:0")
HBM = 8.0e12


def emit(**kw):
    print(json.dumps(kw), flush=True)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def bench_ln(batch, iters):
    from antmmf.hip import ops

    cols = 16384
    g = (1 + 0.1 * torch.randn(cols, device=DEV))
    b = 0.1 * torch.randn(cols, device=DEV)
    for tower, tokens in (("image", 197), ("text", 52)):
        rows = batch * tokens
        x = torch.randn(rows, cols, device=DEV).to(torch.bfloat16)
        dy = torch.randn(rows, cols, device=DEV).to(torch.bfloat16)
        _, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-5, act="gelu")
        dg, db, dxs = (torch.zeros(cols, device=DEV) for _ in range(3))
        ms_f = timed(lambda: ops.layernorm_fwd(x, g, b, 1e-5, act="gelu"), iters)
        ms_b = timed(lambda: ops.layernorm_bwd(dy, x, mean, rstd, g, dg, db, act="gelu", dxsum=dxs), iters)
        for kind, ms, nbytes in (("fwd", ms_f, rows * (2 * cols * 2 + 8)), ("bwd", ms_b, rows * 3 * cols * 2)):
            emit(part="ln", tower=tower, kernel=kind, act="gelu", rows=rows, cols=cols, ms=round(ms, 4), gbps=round(nbytes / ms / 1e6, 1),
                 frac_8tbps=round(nbytes / ms / 1e-3 / HBM, 3))
        del x, dy


def bench_attn(batch, iters):
    from antmmf.hip import ops

    heads, d = 32, 4096
    for tower, N in (("image", 197), ("text", 52)):
        qkv = (0.5 * torch.randn(batch, N, 3 * d, device=DEV)).to(torch.bfloat16)
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        kb = None
        if tower == "text":   # key-padding bias of ragged captions
            kb = torch.zeros(batch, N, device=DEV)
            kb[:, N // 2:] = -1e4
        scale = (d // heads) ** -0.5
        o, lse = ops.attention_fwd(q, k, v, heads, scale, kb)
        do = torch.randn_like(o)
        ms_f = timed(lambda: ops.attention_fwd(q, k, v, heads, scale, kb), iters)
        ms_b = timed(lambda: ops.attention_bwd(q, k, v, o, lse, do, heads, scale, kb), iters)
        fl = 4.0 * batch * heads * N * N * (d // heads)
        emit(part="attn", tower=tower, head_dim=128, batch=batch, tokens=N, fwd_ms=round(ms_f, 4), bwd_ms=round(ms_b, 4),
             fwd_tflops=round(fl / ms_f / 1e9, 1), bwd_tflops=round(2.5 * fl / ms_b / 1e9, 1))


def build_model(**overrides):
    from vlmo.config import load_json_config
    from vlmo.modules.vlmo_module import VLMo

    cfg = load_json_config(CONFIG_10B, tokenizer=None, **overrides)
    torch.manual_seed(0)
    t0 = time.time()
    with torch.device(DEV):
        model = VLMo(cfg)
    torch.cuda.synchronize()
    return model, cfg, time.time() - t0


def inputs(B, cfg, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    seq = cfg["max_text_len"]
    img = torch.rand(B, 3, cfg["image_size"], cfg["image_size"], generator=g, device=DEV)
    ids = torch.randint(1, cfg["vocab_size"], (B, seq), generator=g, device=DEV)
    mask = (torch.arange(seq, device=DEV)[None] < torch.randint(8, seq + 1, (B, 1), generator=g, device=DEV)).long()
    return img, ids * mask, mask


def bench_embed(batch, reps):
    from eval_retrieval import extract_feats

    model, cfg, t_build = build_model()
    nparam = sum(p.numel() for p in model.parameters())
    img, ids, mask = inputs(batch, cfg, 1)
    tb = [{"text_ids": ids, "text_masks": mask}]
    with torch.no_grad():
        tf, imf = extract_feats(model, tb, [img])   # the retrieval evaluation's embedding pass; also the warm-up (workspaces, bf16 copies of the weights)
        model.eval()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(reps):
            model.infer_image({"image": [img]})   # what extract_feats runs per image batch
        torch.cuda.synchronize()
        ti = (time.time() - t0) / reps
        t0 = time.time()
        for _ in range(reps):
            model.infer_text(tb[0])
        torch.cuda.synchronize()
        tt = (time.time() - t0) / reps
    emit(part="embed", params_billion=round(nparam / 1e9, 3), layers=[cfg["encoder_layers"], cfg["beit3_vl_layers"]], batch=batch, build_s=round(t_build, 1),
         image_ms=round(ti * 1e3, 1), images_per_s=round(batch / ti, 1), text_ms=round(tt * 1e3, 1), texts_per_s=round(batch / tt, 1),
         feat_dim=int(tf.shape[1]), finite=bool(torch.isfinite(tf).all() and torch.isfinite(imf).all()), peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
    del model
    torch.cuda.empty_cache()


def bench_train(batch):
    from antmmf.hip.arena import HipAdamW

    torch.cuda.reset_peak_memory_stats()
    try:
        model, cfg, t_build = build_model()
        model.train()
        opt = HipAdamW([{"params": list(model.parameters())}], lr=1e-5)
        img, ids, mask = inputs(batch, cfg, 2)
        times, losses = [], []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.time()
            out = model({"image": [img], "text_ids": ids, "text_masks": mask})
            loss = out["losses"]["itc_loss"] + out["losses"]["itc_vl_loss"]
            loss.backward()
            opt.step()
            opt.zero_grad()
            torch.cuda.synchronize()
            times.append(time.time() - t0)
            losses.append(float(loss.detach()))
        emit(part="train", batch=batch, step_s=[round(t, 3) for t in times], pairs_per_s=round(batch / min(times[1:]), 2), losses=[round(l, 4) for l in losses],
             ln_batch=round(math.log(batch), 4), peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))
    except torch.cuda.OutOfMemoryError as e:
        emit(part="train", batch=batch, error="out of memory", detail=str(e).splitlines()[0], peak_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--train-batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    from antmmf.hip import _lib

    assert _lib.backend() == 1 and torch.cuda.is_available(), "needs the gfx950 library and a GPU"
    emit(part="device", name=torch.cuda.get_device_name(0), hbm_gib=round(torch.cuda.get_device_properties(0).total_memory / 2 ** 30, 1))
    bench_ln(a.batch, a.iters)
    bench_attn(a.batch, a.iters)
    bench_embed(a.batch, a.reps)
    if not a.skip_train:
        bench_train(a.train_batch)


if __name__ == "__main__":
    main()
