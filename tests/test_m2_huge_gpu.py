"""M2-Encoder 10B on a real MI355X (-m gpu): the LayerNorm kernels over rows wider than 4096 columns at the 10B model's 16384-wide ffn_layernorm,
the fused layer at d = 4096 / 32 heads of 128, and a reduced-depth VLMo built from Encoder_10B.json against the CPU oracle."""
import math
import os
import sys

import pytest
import torch

import kernel_cases as kc
import model_cases as mc
import real_width_case as rwc
import weightgen as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M2 = os.path.join(ROOT, "ant-multi-modal-framework_amd", "prj", "M2_Encoder")
if M2 not in sys.path:
    sys.path.insert(0, M2)
CONFIG_10B = os.path.join(ROOT, "tests", "golden", "Encoder_10B.json")   # the reference's prj/M2_Encoder/configs/Encoder_10B.json, unchanged
DEV = torch.device("cuda:0")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from antmmf.hip import _lib

    os.environ.pop("ANTMMF_HIP_LIB", None)
    _lib.reset_for_tests()
    from antmmf.hip import ops as hops

    assert _lib.backend() == 1, "the GPU tests must run against the gfx950 library, not the emulator"
    assert torch.cuda.is_available()
    return hops


def huge_config(**overrides):
    """Encoder_10B.json through the VLMo config loader (tokenizer=None: the json's SentencePiece file is not part of this repository; the step takes ids)."""
    from vlmo.config import load_json_config

    return load_json_config(CONFIG_10B, tokenizer=None, **overrides)


@pytest.mark.parametrize("rows", [1, 31, 4 * 52, 64 * 197])
def test_wide_layernorm(ops, rows):
    """cols 16384, bf16: forward; backward with dres and dxsum through the partials slab; the renorm backward (y re-emitted, bit-identical) through atomics."""
    kc.case_layernorm(ops, DEV, BF, rows=rows, cols=16384)
    kc.case_act_layernorm(ops, DEV, BF, rows=rows, cols=16384, act="gelu")


def test_wide_act_layernorm_quick_gelu_and_atomics(ops):
    kc.case_act_layernorm(ops, DEV, BF, rows=77, cols=16384, act="quick_gelu")
    kc.case_act_layernorm(ops, DEV, BF, rows=6, cols=8200, act="gelu")
    # the fused-GELU backward with its column sums through atomics (no partials slab) == through the slab
    from antmmf.hip import _lib
    from antmmf.hip.ops import _p, _stream

    rows, cols = 300, 16384
    x, dy = kc.q(kc.rnd((rows, cols), 7, 1.5)).to(DEV, BF), kc.q(kc.rnd((rows, cols), 8)).to(DEV, BF)
    g, b = (1 + 0.1 * kc.rnd((cols,), 9)).to(DEV), (0.1 * kc.rnd((cols,), 10)).to(DEV)
    _, mean, rstd = ops.layernorm_fwd(x, g, b, 1e-5, act="gelu")
    sums = [torch.zeros(cols, device=DEV) for _ in range(3)]
    dx = ops.layernorm_bwd(dy, x, mean, rstd, g, sums[0], sums[1], act="gelu", dxsum=sums[2])
    at = [torch.zeros(cols, device=DEV) for _ in range(3)]
    dx2 = torch.empty_like(dx)
    rc = _lib.load().antmmf_act_layernorm_bwd(_p(dy), _p(x), _p(mean), _p(rstd), _p(g), None, _p(dx2), _p(at[0]), _p(at[1]), _p(at[2]), rows, cols,
                                              _lib.ACT_IDS["gelu"], _lib.BF16, None, 0, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    for name, s, a in zip(("dgamma", "dbeta", "dxsum"), sums, at):
        kc.check(f"atomics.{name}", a, s, 1e-4, 1e-4)


@pytest.mark.parametrize("N,pad", [(197, 0), (52, 20)])
def test_m2_layer_huge_real_width(N, pad):
    """transformer_layer at the 10B widths (d = 4096, 32 heads of 128, FFN 16384) against the fp32 oracle layer: output element-wise, input and every
    parameter gradient by cosine >= 0.999 and norm within 2 % (the existing real-width contract)."""
    print(mc.case_layer_real_width(DEV, "m2", d=4096, heads=32, N=N, B=2, pad_tail=pad))


@pytest.fixture(scope="module")
def huge_pair():
    """VLMo from Encoder_10B.json at 2 + 1 layers (vocabulary 1000) on the device, and the oracle's fp32 parameters: the same bf16-rounded values."""
    from oracle.shapes import m2_shapes
    from vlmo.modules.vlmo_module import VLMo

    cfg = huge_config(encoder_layers=2, beit3_vl_layers=1, vocab_size=1000)
    d = cfg["encoder_embed_dim"]
    P = W.fill_dict(m2_shapes(d=d, layers=2, vl_layers=1, patch=cfg["patch_size"], res=cfg["image_size"], vocab=cfg["vocab_size"], out=cfg["out_embed_dim"]))
    P = {k: v.to(BF).float() for k, v in P.items()}
    with torch.device(DEV):
        model = VLMo(cfg)
    missing = rwc.copy_weights(model, P)
    assert all(n.startswith(("norm.", "pooler.")) for n in missing), missing[:8]
    return model.train(), P, cfg


def _batch(k, B, cfg, mask):
    im = (W.data_tensor(f"m2h.image.{k}", (B, 3, cfg["image_size"], cfg["image_size"])) * 0.25 + 0.5).clamp(0, 1)
    return im, W.data_ints(f"m2h.ids.{k}", (B, cfg["max_text_len"]), 1, cfg["vocab_size"]) * mask


def test_m2_huge_towers_and_itc_vs_oracle(huge_pair):
    """infer_image / infer_text features, the ITC loss (the contract of case_m2_itc_vs_oracle: mean over seeded batches within 1e-3, any batch within
    5e-3) and every parameter gradient's direction (assert_grad_directions) against oracle.step.m2_itc with 32 heads of 128."""
    from oracle import step as ostep
    from oracle import towers as otowers

    model, P, cfg = huge_pair
    heads, patch, seq, B = 32, cfg["patch_size"], cfg["max_text_len"], 4
    mask = rwc.ragged_mask([seq, 30, 9, 41], seq)
    img, ids = _batch(0, B, cfg, mask)
    with torch.no_grad():
        oi = model.infer_image({"image": [img.to(DEV)]})
        ot = model.infer_text({"text_ids": ids.to(DEV), "text_masks": mask.to(DEV)})
        ri = otowers.m2_infer_image(P, img, heads, patch)
        rt = otowers.m2_infer_text(P, ids, mask, heads)
    from eval_retrieval import extract_feats   # the retrieval evaluation's embedding pass: the same features

    with torch.no_grad():
        tf, imf = extract_feats(model, [{"text_ids": ids.to(DEV), "text_masks": mask.to(DEV)}], [img.to(DEV)])
    assert model.training
    kc.check("m2h.extract.txt", tf, ot["cls_vlffn_feats"], 1e-3, 1e-3)
    kc.check("m2h.extract.img", imf, oi["cls_vlffn_feats"], 1e-3, 1e-3)
    for k in ("cls_feats", "cls_vlffn_feats"):
        kc.check(f"m2h.img.{k}", oi[k], ri[k], 5e-2, 4e-2)
        kc.check(f"m2h.txt.{k}", ot[k], rt[k], 5e-2, 4e-2)
        for got, want in ((oi[k], ri[k]), (ot[k], rt[k])):
            cos = torch.nn.functional.cosine_similarity(got.float().cpu(), want, dim=-1)
            assert float(cos.min()) >= 0.999, (k, cos)
    for v in P.values():
        v.requires_grad_(True)
    out = model({"image": [img.to(DEV)], "text_ids": ids.to(DEV), "text_masks": mask.to(DEV)})
    loss = out["losses"]["itc_loss"] + out["losses"]["itc_vl_loss"]
    ref = ostep.m2_itc(P, img, ids, mask, heads=heads, patch=patch)
    rel = [(float(loss.detach()) - float(ref["loss"].detach())) / abs(float(ref["loss"].detach()))]
    with torch.no_grad():
        for k in range(1, 4):
            im_k, ids_k = _batch(k, B, cfg, mask)
            o_k = model({"image": [im_k.to(DEV)], "text_ids": ids_k.to(DEV), "text_masks": mask.to(DEV)})
            r_k = float(ostep.m2_itc({n: v.detach() for n, v in P.items()}, im_k, ids_k, mask, heads=heads, patch=patch)["loss"])
            rel.append((float(o_k["losses"]["itc_loss"] + o_k["losses"]["itc_vl_loss"]) - r_k) / abs(r_k))
    print("loss rel", rel)
    assert abs(sum(rel) / len(rel)) <= 1e-3 and max(abs(r) for r in rel) <= 5e-3, rel
    model.zero_grad(set_to_none=True)
    loss.backward()
    ref["loss"].backward()
    named = dict(model.named_parameters())
    gold = {f"gfull.{n}": p.grad for n, p in P.items() if p.grad is not None and n in named}
    print(mc.assert_grad_directions(named.items(), gold, "", min_checked=50))
    for v in P.values():
        v.grad = None
        v.requires_grad_(False)
    model.zero_grad(set_to_none=True)


def test_m2_huge_step_properties(huge_pair):
    """The properties test_m2_full_width_step_properties checks at the large width, here at the 10B width (224 x 224 frames, 52-token captions):
    loss at init ~ ln(B), finite, deterministic forward, lower after one AdamW step."""
    from antmmf.hip.arena import HipAdamW
    from vlmo.modules.vlmo_module import VLMo

    _, _, cfg = huge_pair
    torch.manual_seed(0)
    with torch.device(DEV):
        model = VLMo(cfg).train()
    opt = HipAdamW([{"params": list(model.parameters())}], lr=1e-3)
    B, seq = 16, cfg["max_text_len"]
    g = torch.Generator(device=DEV).manual_seed(1)
    img = torch.rand(B, 3, 224, 224, generator=g, device=DEV)
    ids = torch.randint(1, cfg["vocab_size"], (B, seq), generator=g, device=DEV)
    mask = (torch.arange(seq, device=DEV)[None] < torch.randint(8, seq + 1, (B, 1), generator=g, device=DEV)).long()
    batch = {"image": [img], "text_ids": ids * mask, "text_masks": mask}

    def run():
        out = model(batch)
        return out["losses"]["itc_loss"] + out["losses"]["itc_vl_loss"]

    l0 = run()
    l0b = run()
    assert float(l0) == float(l0b), "forward must be deterministic"
    assert abs(float(l0) - math.log(B)) < 0.5, float(l0)
    l0.backward()
    gn = float(opt.arena.grad_norm())
    assert math.isfinite(gn) and gn > 0
    opt.step()
    opt.zero_grad()
    l1 = run()
    assert float(l1) < float(l0), (float(l0), float(l1))
