"""The DMAE stage-3 head kernels (csrc/tpmcl.hip) on long token rows against the torch expressions that antmmf/hip/tpmcl.py used for such rows before the kernels
served them (softmax of a broadcast product with torch autograd, einsum, argsort / cumsum / scatter_): both arms in ONE process, interleaved round by round, HIP
events around `iters` calls after a warm-up of every shape, median and minimum over the rounds.

Shapes: (128, 2364, 768) = 12 frames x 197 patch tokens per video, (2048, 77, 768) = CLIP's context length at the dmae12 pair count; tis_keep rows (2048, 77) and
(2048, 1024).  Algorithmic bytes (one slab = items x tokens x D x 4 B): token_weights forward 1 slab read, forward + backward 2 reads + 1 write (dfeat);
pair_dots / pair_wsum forward 1 read each; the pair operators forward + backward (both operators, all of dx, dy, dw) 4 reads + 1 write; tis_keep one read and one
write of the [rows, tokens] weights.  ratio = torch ms / kernel ms (> 1: the kernel path is faster).

    python tools/tpmcl_long_bench.py [--rounds 7] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ant-multi-modal-framework_amd"))
from antmmf.hip import tpmcl  # noqa: E402


# ---- the torch arm: the expressions of the former shape guards of antmmf/hip/tpmcl.py
def torch_token_weights(feat, weight, bias, mask):
    logits = (feat.float() * weight.float().reshape(-1)).sum(-1)
    logits = logits + bias.float().reshape(())
    logits = logits.masked_fill(mask < 0.5, float("-inf"))
    return torch.softmax(logits, dim=-1)


def torch_pair_dots(x, y):
    return torch.einsum("cd,cvd->cv", x.float(), y.float())


def torch_pair_wsum(w, y):
    return torch.einsum("cv,cvd->cd", w.float(), y.float())


def torch_tis_keep(w, thresh):
    order = torch.argsort(w, dim=-1, descending=True)
    drop_sorted = torch.cumsum(torch.gather(w, -1, order), dim=-1) < thresh
    return 1.0 - torch.zeros_like(w).scatter_(-1, order, drop_sorted.float())


def time_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def compare(name, shape, kernel_fn, torch_fn, nbytes, rounds, iters):
    for fn in (kernel_fn, torch_fn):   # warm-up: code objects, rocBLAS / sort algorithm choice, the caching allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    k, t = [], []
    for _ in range(rounds):
        k.append(time_ms(kernel_fn, iters))
        t.append(time_ms(torch_fn, iters))
    km, tm = statistics.median(k), statistics.median(t)
    return {"op": name, "shape": list(shape), "kernel_ms": round(km, 4), "kernel_ms_min": round(min(k), 4), "torch_ms": round(tm, 4), "torch_ms_min": round(min(t), 4),
            "algorithmic_mb": round(nbytes / 1e6, 2), "kernel_gbs": round(nbytes / km / 1e6, 1), "torch_gbs": round(nbytes / tm / 1e6, 1),
            "ratio_torch_over_kernel": round(tm / km, 3), "rounds": rounds, "iters": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tpmcl_long_bench.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []

    def emit(d):
        print(json.dumps(d), flush=True)
        rows.append(d)

    for N, T, D in ((128, 2364, 768), (2048, 77, 768)):
        slab = N * T * D * 4
        iters = 10
        feat = torch.randn(N, T, D, generator=g, device=dev)
        weight, bias = torch.randn(1, D, generator=g, device=dev) * 0.05, torch.zeros(1, device=dev)
        mask = (torch.rand(N, T, generator=g, device=dev) > 0.2).float()
        mask[:, 0] = 1.0
        dout = torch.randn(N, T, generator=g, device=dev)
        x, ww = torch.randn(N, D, generator=g, device=dev), torch.randn(N, T, generator=g, device=dev)
        g1, g2 = torch.randn(N, T, generator=g, device=dev), torch.randn(N, D, generator=g, device=dev)
        with torch.no_grad():
            emit(compare("token_weights.fwd", (N, T, D), lambda: tpmcl.token_weights(feat, weight, bias, mask), lambda: torch_token_weights(feat, weight, bias, mask),
                         slab, args.rounds, iters))
            emit(compare("pair_dots.fwd", (N, T, D), lambda: tpmcl.pair_dots(x, feat), lambda: torch_pair_dots(x, feat), slab, args.rounds, iters))
            emit(compare("pair_wsum.fwd", (N, T, D), lambda: tpmcl.pair_wsum(ww, feat), lambda: torch_pair_wsum(ww, feat), slab, args.rounds, iters))
        fg, wg, bg = feat.clone().requires_grad_(True), weight.clone().requires_grad_(True), bias.clone().requires_grad_(True)
        xg, wwg = x.clone().requires_grad_(True), ww.clone().requires_grad_(True)

        def tw_step(fn):
            fg.grad = wg.grad = bg.grad = None
            (fn(fg, wg, bg, mask) * dout).sum().backward()

        def pair_step(dots, wsum):
            fg.grad = xg.grad = wwg.grad = None
            ((dots(xg, fg) * g1).sum() + (wsum(wwg, fg) * g2).sum()).backward()

        emit(compare("token_weights.fwd_bwd", (N, T, D), lambda: tw_step(tpmcl.token_weights), lambda: tw_step(torch_token_weights), 3 * slab, args.rounds, iters))
        emit(compare("pair_dots+pair_wsum.fwd_bwd", (N, T, D), lambda: pair_step(tpmcl.pair_dots, tpmcl.pair_wsum), lambda: pair_step(torch_pair_dots, torch_pair_wsum),
                     5 * slab, args.rounds, iters))
        del feat, fg, xg, wwg
        torch.cuda.empty_cache()
    for R, T in ((2048, 77), (2048, 1024)):
        w = torch.softmax(torch.randn(R, T, generator=g, device=dev) * 2.0, dim=-1)
        emit(compare("tis_keep", (R, T), lambda: tpmcl.tis_keep(w, 0.6), lambda: torch_tis_keep(w, 0.6), 2 * R * T * 4, args.rounds, 20))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for d in rows:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
