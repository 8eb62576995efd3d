"""Attention for rows longer than 288 tokens (csrc/attention.hip: attn_fwd_stream_kernel, attn_bwd_dq_stream_kernel, attn_bwd_dkv_stream_kernel): HIP events
around `iters` calls after a warm-up of each shape, median and minimum over the rounds, one process.

Shapes [B, heads, tokens, head size]: 64 x 16 x 577 x 64 (ViT-L/14 at 336 px), 64 x 12 x 577 x 64 (ViT-B/16 at 384 px), 16 x 16 x 1025 x 64 (ViT-L/14 at 448 px),
8 x 32 x 577 x 128.  Beside each:
  * floor_fwd_ms: the algorithmic HBM bytes of the forward -- four tensor passes (q, k, v, o: 2 B * B * N * heads * dh each) + lse (4 B * B * heads * N) -- at the
    6.29 TB/s a float4 copy reaches on this part; the streamed forward re-reads K and V once per 128-query block, which the floor does not count;
  * sdpa_*: torch.nn.functional.scaled_dot_product_attention forward and forward + backward on the same tensors in the same process;
  * per-score throughput (B * heads * Nq * Nk scores per microsecond) of forward and backward next to the whole-row kernels' at 64 x 16 x 288 x 64, and the ratio.
Also words_importance's kernel (ops.attention_key_importance_, head size 64: 64 x 12 x 77 x 77 and 64 x 16 x 257 x 257) -- since it moved to the probability-map
kernel; run the tool on both commits for the ratio.  Nothing here is gated anywhere.

    python tools/attn_long_bench.py [--rounds 7] [--iters 50] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ant-multi-modal-framework_amd"))
from antmmf.hip import ops  # noqa: E402

HBM_MEASURED_TBS = 6.29
SHAPES = ((64, 16, 577, 64), (64, 12, 577, 64), (16, 16, 1025, 64), (8, 32, 577, 128))
WHOLE_ROW = (64, 16, 288, 64)
IMPORTANCE_SHAPES = ((64, 12, 77), (64, 16, 257))


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def med_min(fn, rounds, iters):
    for _ in range(3):   # warm-up: code objects, the caching allocator
        fn()
    torch.cuda.synchronize()
    t = [time_ms(fn, iters) for _ in range(rounds)]
    return round(statistics.median(t), 4), round(min(t), 4)


def attention_row(B, heads, N, dh, args, dev, g, sdpa=True):
    d = heads * dh
    qkv = torch.randn(B, N, 3 * d, generator=g, device=dev).to(torch.bfloat16)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    d_o = torch.randn(B, N, d, generator=g, device=dev).to(torch.bfloat16)
    scale = dh ** -0.5
    o, lse = ops.attention_fwd(q, k, v, heads, scale)
    dq, dk, dv = (torch.empty(B, N, d, dtype=torch.bfloat16, device=dev) for _ in range(3))
    fwd_ms, fwd_min = med_min(lambda: ops.attention_fwd(q, k, v, heads, scale), args.rounds, args.iters)
    bwd_ms, bwd_min = med_min(lambda: ops.attention_bwd(q, k, v, o, lse, d_o, heads, scale, dq=dq, dk=dk, dv=dv), args.rounds, args.iters)
    scores = B * heads * N * N
    fwd_bytes = 4 * 2 * B * N * d + 4 * B * heads * N
    floor = fwd_bytes / (HBM_MEASURED_TBS * 1e12) * 1e3
    row = {"op": "attention", "shape": [B, heads, N, dh], "fwd_ms": fwd_ms, "fwd_ms_min": fwd_min, "bwd_ms": bwd_ms, "bwd_ms_min": bwd_min,
           "floor_fwd_ms": round(floor, 4), "fwd_x_floor": round(fwd_ms / floor, 2), "fwd_scores_per_us": round(scores / fwd_ms / 1e3, 1),
           "bwd_scores_per_us": round(scores / bwd_ms / 1e3, 1), "rounds": args.rounds, "iters": args.iters}
    if sdpa:
        qs, ks, vs = (t.reshape(B, N, heads, dh).transpose(1, 2).contiguous().requires_grad_(True) for t in (q, k, v))
        gs = d_o.reshape(B, N, heads, dh).transpose(1, 2).contiguous()
        F = torch.nn.functional

        def sdpa_step():
            for t in (qs, ks, vs):
                t.grad = None
            F.scaled_dot_product_attention(qs, ks, vs).backward(gs)

        def sdpa_fwd():
            with torch.no_grad():
                F.scaled_dot_product_attention(qs, ks, vs)

        row["sdpa_fwd_ms"], _ = med_min(sdpa_fwd, args.rounds, args.iters)
        row["sdpa_fwd_bwd_ms"], _ = med_min(sdpa_step, args.rounds, args.iters)
        row["fwd_bwd_over_sdpa"] = round((fwd_ms + bwd_ms) / row["sdpa_fwd_bwd_ms"], 3)
    del qkv, d_o, o, lse, dq, dk, dv
    torch.cuda.empty_cache()
    return row


def importance_row(B, heads, N, args, dev, g):
    d = heads * 64
    qkv = torch.randn(B, N, 3 * d, generator=g, device=dev).to(torch.bfloat16)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    _, lse = ops.attention_fwd(q, k, v, heads, 0.125)
    imp = torch.zeros(B, N, device=dev)
    ms, mn = med_min(lambda: ops.attention_key_importance_(imp, q, k, lse, heads, 0.125, weight=1.0 / heads), args.rounds, args.iters)
    return {"op": "attention_key_importance", "shape": [B, heads, N, N], "head_dim": 64, "ms": ms, "ms_min": mn, "rounds": args.rounds, "iters": args.iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--importance-only", action="store_true", help="only the key-importance rows (what also runs on a commit without the streamed kernels)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_long_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    if not args.importance_only:
        base = attention_row(*WHOLE_ROW, args, dev, g, sdpa=False)
        base["op"] = "attention_whole_row"
        print(json.dumps(base), flush=True)
        rows.append(base)
        for shape in SHAPES:
            row = attention_row(*shape, args, dev, g)
            row["fwd_per_score_vs_whole_row_288"] = round(row["fwd_scores_per_us"] / base["fwd_scores_per_us"], 3)
            row["bwd_per_score_vs_whole_row_288"] = round(row["bwd_scores_per_us"] / base["bwd_scores_per_us"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    for shape in IMPORTANCE_SHAPES:
        row = importance_row(*shape, args, dev, g)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
