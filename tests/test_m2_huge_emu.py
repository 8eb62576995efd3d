"""M2-Encoder 10B (`Encoder_10B.json`: beit huge, d = 4096, 32 heads of 128, FFN 16384) on the CPU lane emulator and on the meta device:
the LayerNorm kernels over rows wider than 4096 columns (ln_wide_fwd_kernel / ln_wide_bwd_kernel), the fused layer at head size 128, and the
model's construction.  Hardware parity at the real widths is tests/test_m2_huge_gpu.py."""
import os
import sys
import subprocess

import pytest
import torch

import kernel_cases as kc
import model_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M2 = os.path.join(ROOT, "ant-multi-modal-framework_amd", "prj", "M2_Encoder")
if M2 not in sys.path:
    sys.path.insert(0, M2)
EMU_LIB = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
CONFIG_10B = os.path.join(ROOT, "tests", "golden", "Encoder_10B.json")   # the reference's prj/M2_Encoder/configs/Encoder_10B.json, unchanged
DEV = torch.device("cpu")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not os.path.isfile("/opt/rocm/lib/llvm/bin/clang++") and not os.environ.get("EMU_CXX"):
        pytest.skip("no clang++ to build the emulator")
    from test_kernels_emu import _stale

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


def huge_config(**overrides):
    """Encoder_10B.json through the VLMo config loader.  The json names a SentencePiece tokenizer file that is not part of this repository:
    tokenizer=None builds the model without the host-side tokenizer (the training step takes ids)."""
    from vlmo.config import load_json_config

    return load_json_config(CONFIG_10B, tokenizer=None, **overrides)


def test_wide_layernorm(ops):
    # plain LayerNorm (forward, backward with dres + dxsum through the partials slab, the renorm backward through atomics): 16384 and a
    # width that is not a power of two (1025 vectors: thread 0 owns a second vector, the rest one)
    kc.case_layernorm(ops, DEV, BF, rows=3, cols=16384)
    kc.case_layernorm(ops, DEV, BF, rows=5, cols=8200)


def test_wide_act_layernorm(ops):
    kc.case_act_layernorm(ops, DEV, BF, rows=3, cols=16384, act="gelu")
    kc.case_act_layernorm(ops, DEV, BF, rows=4, cols=12288, act="quick_gelu")


def test_wide_layernorm_limits(ops):
    """fp32 rows wider than 4096 and rows wider than 16384 are refused (EINVAL), not computed wrong."""
    with pytest.raises(RuntimeError, match="code -22"):
        ops.layernorm_fwd(torch.randn(2, 8192), torch.ones(8192), torch.zeros(8192), 1e-5)
    x = torch.randn(2, 8192)
    with pytest.raises(RuntimeError, match="code -22"):
        ops.layernorm_bwd(x, x, torch.zeros(2), torch.ones(2), torch.ones(8192), act="gelu")
    with pytest.raises(RuntimeError, match="code -22"):
        ops.layernorm_fwd(torch.randn(2, 16392, dtype=BF), torch.ones(16392), torch.zeros(16392), 1e-5)


@pytest.mark.parametrize("heads", [2, 4])
def test_m2_layer_head_size(ops, heads):
    """The fused M2 layer at d = 256: 2 heads of 128 (the 10B model's head size) and 4 heads of 64 (control) against the fp32 oracle layer:
    the softmax scale follows the head size."""
    print(mc.case_layer_real_width(DEV, "m2", d=256, heads=heads, N=19, B=2, pad_tail=5))


def test_multihead_attention_head_sizes():
    from vlmo.modules.modeling_utils import get_config
    from vlmo.torchscale.component.multihead_attention import MultiheadAttention

    args = get_config("huge")
    with torch.device("meta"):
        m = MultiheadAttention(args, 4096, 32, self_attention=True, subln=True)
        assert m.head_dim == 128 and m.scaling == 128 ** -0.5
        assert MultiheadAttention(args, 1024, 16, self_attention=True, subln=True).head_dim == 64
        with pytest.raises(ValueError, match="64.*128"):
            MultiheadAttention(args, 768, 8, self_attention=True, subln=True)   # head size 96


def test_encoder_10b_parameter_shapes():
    """VLMo from Encoder_10B.json at reduced depth (2 + 1 layers, small vocabulary), built on the meta device: 32 heads of 128, the 16384-wide
    ffn_layernorm of every multiway branch, the towers' parameter count per layer."""
    from vlmo.modules.vlmo_module import VLMo

    cfg = huge_config(encoder_layers=2, beit3_vl_layers=1, vocab_size=1000)
    assert (cfg["beit_version"], cfg["encoder_embed_dim"], cfg["out_embed_dim"], cfg["patch_size"]) == ("huge", 4096, 1024, 16)
    with torch.device("meta"):
        model = VLMo(cfg)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    attn = model.backbone.encoder.layers[0].self_attn
    assert (attn.num_heads, attn.head_dim) == (32, 128)
    for pre in ("backbone.encoder.layers.0.", "backbone.encoder.layers.1.", "backbone_vl.layers.0."):
        for br in ("A", "B"):
            assert shapes[f"{pre}ffn.{br}.ffn_layernorm.weight"] == (16384,)
            assert shapes[f"{pre}ffn.{br}.fc1.weight"] == (16384, 4096)
            assert shapes[f"{pre}ffn.{br}.fc2.weight"] == (4096, 16384)
            assert shapes[f"{pre}self_attn.q_proj.{br}.weight"] == (4096, 4096)
    assert "backbone.encoder.layers.2.ffn.A.fc1.weight" not in shapes
    assert shapes["backbone.vision_embed.proj.weight"] == (4096, 3, 16, 16)
    per_layer = sum(p.numel() for n, p in model.named_parameters() if n.startswith("backbone.encoder.layers.0."))
    assert per_layer == 2 * (4 * (4096 * 4096 + 4096) + 2 * 4096 * 16384 + 16384 + 4096 + 2 * 16384 + 3 * 2 * 4096), per_layer
