"""Attention probability maps on request (csrc/attention.hip::attn_probs_kernel) on the CPU lane emulator: the cases of tests/attn_probs_cases.py with
B * heads <= 4 workgroups per launch (the emulator pays per emulated workgroup); the 257- and 288-token maps run on hardware only
(tests/test_attn_probs_gpu.py), the multi-chunk case here is 65 x 97."""
import os
import subprocess

import pytest
import torch

import attn_probs_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_LIB = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
CSRC = os.path.join(ROOT, "ant-multi-modal-framework_amd", "csrc")


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


DEV = torch.device("cpu")


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("shape", ac.MAP_SHAPES_EMU, ids=lambda s: "x".join(map(str, s)))
def test_maps(ops, dh, shape):
    ac.case_maps(ops, DEV, dh, *shape, packed=False)


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("n", [16, 77])
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


def test_bert_encoder_maps(ops):
    ac.case_bert_encoder(DEV)


@pytest.mark.parametrize("head_size", [64, 128])
def test_vilbert_visualization(ops, head_size):
    ac.case_vilbert_visualization(DEV, head_size)


def test_packed_text_with_map_collector_is_refused(ops):
    ac.case_packed_with_map_collector(DEV)
