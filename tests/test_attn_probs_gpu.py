"""Attention probability maps on request (csrc/attention.hip::attn_probs_kernel) on a real MI355X (-m gpu): the cases of tests/attn_probs_cases.py, with the
257- and 288-token maps (more query tiles than waves, the whole-row limit) at B = 2, heads = 2."""
import os

import pytest
import torch

import attn_probs_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from antmmf.hip import _lib

    os.environ.pop("ANTMMF_HIP_LIB", None)
    _lib.reset_for_tests()
    from antmmf.hip import ops as hops

    assert _lib.backend() == 1, "the GPU tests must run against the gfx950 library, not the emulator"
    assert torch.cuda.is_available()
    return hops


DEV = torch.device("cuda:0")


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("shape", ac.MAP_SHAPES_GPU, ids=lambda s: "x".join(map(str, s)))
def test_maps(ops, dh, shape):
    ac.case_maps(ops, DEV, dh, *shape, B=2, packed=False)


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("n", [16, 77, 257])
def test_maps_of_a_packed_projection(ops, dh, n):
    ac.case_maps(ops, DEV, dh, n, n, B=2, packed=True)


@pytest.mark.parametrize("dh", [64, 128])
def test_masks(ops, dh):
    ac.case_masks(ops, DEV, dh)


@pytest.mark.parametrize("dh", [64, 128])
def test_dropout_mask_is_the_forwards(ops, dh):
    ac.case_dropout(ops, DEV, dh)


def test_importance(ops):
    ac.case_importance(ops, DEV)


def test_refusals(ops):
    ac.case_refusals(ops, DEV)
    torch.cuda.synchronize()


def test_bert_encoder_maps(ops):
    ac.case_bert_encoder(DEV)


@pytest.mark.parametrize("head_size", [64, 128])
def test_vilbert_visualization(ops, head_size):
    ac.case_vilbert_visualization(DEV, head_size)


def test_packed_text_with_map_collector_is_refused(ops):
    ac.case_packed_with_map_collector(DEV)
