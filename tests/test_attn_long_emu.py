"""Attention for rows longer than 288 tokens (the streamed kernels of csrc/attention.hip) on the CPU lane emulator: B = heads = 1 -- the emulator pays per emulated
workgroup -- and only the smallest shapes that take the streamed path; block edges, the layers and the models run on hardware (tests/test_attn_long_gpu.py)."""
import os
import subprocess

import pytest
import torch

import attn_long_cases as al
import kernel_cases as kc

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


@pytest.mark.parametrize("dh,bias,packed", al.FIRST_PAST_THE_WALL)
def test_first_row_past_the_wall(ops, dh, bias, packed):
    kc.case_attention(ops, DEV, B=1, heads=1, Nq=al.WALL + 1, Nk=al.WALL + 1, bias_kind=bias, packed=packed, seed=880, head_dim=dh)


@pytest.mark.parametrize("dh", [64, 128])
def test_cross_length(ops, dh):
    Nq, Nk = al.cross_length_shapes(dh, gpu=False)[0]
    kc.case_attention(ops, DEV, B=1, heads=1, Nq=Nq, Nk=Nk, bias_kind="inf", packed=False, seed=881, head_dim=dh)


def test_leading_masked_block(ops):
    al.case_leading_masked_block(ops, DEV, 128, B=1, heads=1)   # (head size 128: the smaller key block)


@pytest.mark.parametrize("dh", [64, 128])
def test_dropout(ops, dh):
    al.case_dropout(ops, DEV, dh, B=1, heads=1)


@pytest.mark.parametrize("dh", [64, 128])
def test_fully_masked_row(ops, dh):
    al.case_fully_masked_row(ops, DEV, dh, B=2, heads=1)


def test_refusals_and_limits(ops):
    al.case_refusals(ops, DEV)


def test_key_importance_head_size_64_runs_the_probs_kernel(ops):
    al.case_key_importance_both_head_sizes(ops, DEV, N=40, B=1, heads=2)
