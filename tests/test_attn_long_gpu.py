"""Attention for rows longer than 288 tokens on hardware: the streamed forward, dQ and dK / dV kernels of csrc/attention.hip at B = heads = 2, every block edge,
cross-length calls, masks, dropout, reproducibility, the refusals, and the layers and models that reach them (tests/attn_long_cases.py)."""
import pytest
import torch

import attn_long_cases as al
import kernel_cases as kc
import model_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import os

    from antmmf.hip import _lib

    os.environ.pop("ANTMMF_HIP_LIB", None)
    _lib.reset_for_tests()
    from antmmf.hip import ops as hops

    assert _lib.backend() == 1, "the GPU tests must run against the gfx950 library, not the emulator"
    assert torch.cuda.is_available()
    return hops


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("dh,bias,packed", al.FIRST_PAST_THE_WALL)
def test_first_row_past_the_wall(ops, dev, dh, bias, packed):
    kc.case_attention(ops, dev, Nq=al.WALL + 1, Nk=al.WALL + 1, bias_kind=bias, packed=packed, seed=880, head_dim=dh)


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("i", range(5))
def test_block_edges(ops, dev, dh, i):
    Nq, Nk = al.block_edge_shapes(dh)[i]
    kc.case_attention(ops, dev, Nq=Nq, Nk=Nk, bias_kind="inf" if i % 2 else "none", packed=False, seed=882 + i, head_dim=dh)


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("i", range(4))
def test_cross_length(ops, dev, dh, i):
    Nq, Nk = al.cross_length_shapes(dh, gpu=True)[i]
    kc.case_attention(ops, dev, Nq=Nq, Nk=Nk, bias_kind="bert" if i == 1 else "inf", packed=False, seed=890 + i, head_dim=dh)


@pytest.mark.parametrize("dh", [64, 128])
def test_leading_masked_block(ops, dev, dh):
    al.case_leading_masked_block(ops, dev, dh)


@pytest.mark.parametrize("dh", [64, 128])
def test_fully_masked_row(ops, dev, dh):
    al.case_fully_masked_row(ops, dev, dh)


@pytest.mark.parametrize("dh", [64, 128])
def test_consistency_with_the_whole_row_kernels(ops, dev, dh):
    al.case_consistency_with_whole_row(ops, dev, dh)


@pytest.mark.parametrize("dh", [64, 128])
def test_dropout(ops, dev, dh):
    al.case_dropout(ops, dev, dh)


def test_backward_is_bit_reproducible(ops, dev):
    al.case_reproducible(ops, dev)


def test_refusals_and_limits(ops, dev):
    al.case_refusals(ops, dev)


def test_key_importance_both_head_sizes(ops, dev):
    al.case_key_importance_both_head_sizes(ops, dev)


def test_clip_layer_321_tokens(dev):
    mc.case_layer_real_width(dev, kind="clip", d=128, heads=2, N=321, B=2)


def test_m2_layer_300_tokens_padded_tail(dev):
    mc.case_layer_real_width(dev, kind="m2", d=128, heads=2, N=300, pad_tail=40)


def test_m2_itc_step_with_325_image_tokens(dev):
    al.case_m2_long_image_rows(dev)


def test_vision_transformer_beyond_288_tokens(dev):
    al.case_visual_transformer(dev)
