"""Token-packed text path on the CPU lane emulation of the HIP kernels: the packed attention / embedding entry points against the strided ones (tests/packed_cases.py),
and the packed transformer layer / embedding autograd functions against the padded ones."""
import os
import subprocess
import sys

import pytest
import torch

import packed_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_LIB = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
CSRC = os.path.join(ROOT, "ant-multi-modal-framework_amd", "csrc")
DEV = torch.device("cpu")


def _stale():
    if not os.path.isfile(EMU_LIB):
        return True
    t = os.path.getmtime(EMU_LIB)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(ROOT, "tests", "emu", "hip_emu.h")]
    return any(os.path.getmtime(s) > t for s in srcs)


@pytest.fixture(scope="module")
def ops():
    if not os.path.isfile("/opt/rocm/lib/llvm/bin/clang++") and not os.environ.get("EMU_CXX"):
        pytest.skip("no clang++ to build the emulator")
    if _stale():
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    from antmmf.hip import _lib

    old = os.environ.get("ANTMMF_HIP_LIB")
    os.environ["ANTMMF_HIP_LIB"] = EMU_LIB
    _lib.reset_for_tests()
    from antmmf.hip import ops as hops

    assert _lib.backend() == 0
    yield hops
    if old is None:
        os.environ.pop("ANTMMF_HIP_LIB", None)
    else:
        os.environ["ANTMMF_HIP_LIB"] = old
    _lib.reset_for_tests()


def test_attention_packed(ops):
    """lengths {1, 8, 32, 33, 64, 77} in one batch, one item per workgroup"""
    pc.case_attention_packed(ops, DEV)


def test_attention_packed_persistent_walk():
    """... and on a grid of two workgroups (lab knob of the emulator build), so that every workgroup walks six items of different lengths: the next item's Q / dO / K
    pieces are fetched by row-clipped LDS-DMA while the current one computes."""
    code = ("import os, sys, torch; sys.path[:0] = [%r, %r, %r]; os.environ['ANTMMF_HIP_LIB'] = %r; os.environ['ANTMMF_ATTN_PERSIST_WGS'] = '2';"
            "import packed_cases as pc; from antmmf.hip import ops;"
            "pc.case_attention_packed(ops, torch.device('cpu'), lengths=(77, 1, 33, 8, 64, 32), seed=3); print('okwalk')"
            % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "ant-multi-modal-framework_amd"), ROOT, EMU_LIB))
    if _stale():
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=2400)
    assert "okwalk" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_attention_packed_rejects_unserved_shapes(ops):
    items = pc.item_table((4, 4), DEV)
    x = torch.zeros(8, 3 * 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="code -22"):
        ops.attention_fwd_packed(x[:, :64], x[:, 64:128], x[:, 128:], items, 1, 0.125, 16)   # (n_max <= 32: the two-kernel backward has no packed form)


def test_embed_packed(ops):
    pc.case_embed_packed(ops, DEV)
    pc.case_embed_packed(ops, DEV, big=True)


def test_layer_and_embedding_packed_autograd(ops):
    """functional.transformer_layer(kind="m2") on a packed [T, d] input + item table against the padded call with a -inf prefix key_bias: outputs of the item rows
    bit-identical, parameter gradients equal up to summation order; functional.embed packed against padded."""
    from antmmf.hip import functional as HF

    g = torch.Generator().manual_seed(5)
    lengths, n_max, d, heads = (40, 1, 77, 33), 77, 64, 1
    B = len(lengths)
    spec = HF.LayerSpec(kind="m2", heads=heads, eps=1e-5, act="gelu", packed_qkv=False)

    def mk(*shape, s=0.2):
        return torch.nn.Parameter(torch.randn(*shape, generator=g) * s)

    P = dict(ln1_w=mk(d, s=0.1), ln1_b=mk(d), wq=mk(d, d), bq=mk(d), wk=mk(d, d), bk=mk(d), wv=mk(d, d), bv=mk(d), inner_w=mk(d), inner_b=mk(d), wo=mk(d, d), bo=mk(d),
             ln2_w=mk(d), ln2_b=mk(d), w1=mk(4 * d, d), b1=mk(4 * d), ffn_w=mk(4 * d), ffn_b=mk(4 * d), w2=mk(d, 4 * d), b2=mk(d))
    for nm in ("ln1_w", "inner_w", "ln2_w", "ffn_w"):
        P[nm].data.add_(1.0)
    ln = torch.tensor(lengths)
    valid = torch.arange(n_max)[None, :] < ln[:, None]
    x = (torch.randn(B, n_max, d, generator=g)).to(torch.bfloat16) * valid[..., None].to(torch.bfloat16)
    key_bias = torch.zeros(B, n_max).masked_fill_(~valid, float("-inf"))
    dy = torch.randn(B, n_max, d, generator=g).to(torch.bfloat16) * valid[..., None].to(torch.bfloat16)

    xr = x.clone().requires_grad_(True)
    y_ref = HF.transformer_layer(xr, spec, P, key_bias)
    y_ref.backward(dy)
    g_ref = {k: v.grad.clone() for k, v in P.items()}
    dx_ref = xr.grad.clone()
    for v in P.values():
        v.grad = None

    total = sum(lengths)
    T = total + 11
    items = pc.item_table(lengths, DEV)
    text = HF.PackedText(items, n_max, total, T)
    xp = pc.pack_rows(x, lengths, T).requires_grad_(True)
    y = HF.transformer_layer(xp, spec, P, packed=text)
    assert y.shape == (T, d)
    pc.assert_rows_identical(y.detach(), y_ref.detach(), lengths, "layer output")
    y.backward(pc.pack_rows(dy, lengths, T))
    pc.assert_rows_identical(xp.grad, dx_ref, lengths, "layer input gradient")
    assert float(xp.grad[total:].abs().max()) == 0.0
    for k, v in P.items():
        ref = g_ref[k]
        assert torch.isfinite(v.grad).all(), k
        err = float((v.grad - ref).abs().max()) / max(1e-6, float(ref.abs().max()))
        assert err <= 2e-3, (k, err)   # fp32 sums of the same bf16 products in another order; the emulator's wgrad partial sums are fp32 (< 1e-5), LayerNorm-parameter sums as well


def test_m2_text_tower_packed_vs_padded(ops):
    """The tiny M2 dual tower with 40-token captions: infer_text packed == padded bit for bit, a non-prefix mask takes the padded path, and a full ITC step's
    loss is bit-identical with parameter gradients inside 4 x the padded path's own reorder noise (the hardware-sized version is tests/test_packed_text_gpu.py)."""
    import model_cases as mc

    model = mc.build_tiny_m2(DEV)
    pc.case_infer_text_packed(DEV, model, seq=40, B=5)
    pc.case_non_prefix_mask_takes_padded_path(DEV, model, seq=40, B=5)
    r = pc.case_itc_grad_parity(DEV, model, seq=40, B=5)
    assert r["loss_identical"], (r["loss_padded"], r["loss_packed"])
    assert not r["bad"], r["bad"]
