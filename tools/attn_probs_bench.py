"""The attention probability maps on request (csrc/attention.hip::attn_probs_kernel, ops.attention_probs) against the floor of writing them: HIP events around
`iters` calls after a warm-up of each shape, median and minimum over the rounds.

Shapes [B, heads, Nq, Nk]: 64 x 16 x 257 x 257 at head size 64 (a ViT-L/14 image tower layer at 64 images) and 64 x 32 x 197 x 197 at head size 128 (the M2 10B
image tower).  Algorithmic bytes = the map itself, B * heads * Nq * Nk * 4 (q, k and lse are under 3 % of that and not counted); floor_ms = those bytes at the 6.29 TB/s
a float4 copy reaches on this part, floor_ms_spec at the 8 TB/s of the data sheet.  x_floor = kernel ms / floor_ms.  The importance output alone (no map written:
what the kernel costs without its stores) is timed next to it.  Not gated anywhere: the kernel runs only when a caller asks for the maps.

    python tools/attn_probs_bench.py [--rounds 7] [--iters 10] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ant-multi-modal-framework_amd"))
from antmmf.hip import ops  # noqa: E402

HBM_MEASURED_TBS, HBM_SPEC_TBS = 6.29, 8.0


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_probs_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for B, heads, N, dh in ((64, 16, 257, 64), (64, 32, 197, 128)):
        d = heads * dh
        qkv = torch.randn(B, N, 3 * d, generator=g, device=dev).to(torch.bfloat16)
        q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
        scale = dh ** -0.5
        _, lse = ops.attention_fwd(q, k, v, heads, scale)
        probs = torch.empty(B, heads, N, N, dtype=torch.float32, device=dev)
        imp = torch.zeros(B, N, device=dev)
        maps = lambda: ops.attention_probs_into(q, k, lse, heads, scale, probs=probs)            # noqa: E731
        sums = lambda: ops.attention_probs_into(q, k, lse, heads, scale, importance=imp)         # noqa: E731
        fwd = lambda: ops.attention_fwd(q, k, v, heads, scale)                                   # noqa: E731
        for fn in (maps, sums, fwd):   # warm-up: code objects, the caching allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        assert abs(float(probs[0, 0].sum(-1).mean()) - 1.0) < 1e-4   # (it ran, and on these operands)
        tm, ts, tf = [], [], []
        for _ in range(args.rounds):
            tm.append(time_ms(maps, args.iters))
            ts.append(time_ms(sums, args.iters))
            tf.append(time_ms(fwd, args.iters))
        nbytes = probs.numel() * 4
        ms = statistics.median(tm)
        floor = nbytes / (HBM_MEASURED_TBS * 1e12) * 1e3
        row = {"op": "attention_probs", "shape": [B, heads, N, N], "head_dim": dh, "maps_ms": round(ms, 4), "maps_ms_min": round(min(tm), 4),
               "importance_only_ms": round(statistics.median(ts), 4), "attention_fwd_ms": round(statistics.median(tf), 4), "map_mb": round(nbytes / 1e6, 1),
               "maps_gbs": round(nbytes / ms / 1e6, 1), "floor_ms": round(floor, 4), "floor_ms_spec": round(nbytes / (HBM_SPEC_TBS * 1e12) * 1e3, 4),
               "x_floor": round(ms / floor, 2), "rounds": args.rounds, "iters": args.iters}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del qkv, probs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
