"""The long-row forms of the DMAE stage-3 head kernels (csrc/tpmcl.hip) on the CPU lane emulator: the cases of tests/tpmcl_long_cases.py at reduced counts (the
emulator pays ~15 ms per emulated workgroup and more per long row; the limit cases shrink to T = 300 and selector rows of 130).  Hardware parity at the full
shapes is tests/test_tpmcl_long_gpu.py."""
import os
import subprocess

import pytest
import torch

import tpmcl_long_cases as tc

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


@pytest.mark.parametrize("shape", [(3, 129, 96), (2, 257, 1028), (2, 130, 1030), (2, 300, 64)], ids=lambda s: "x".join(map(str, s)))
def test_token_weights_long(ops, shape):
    print(tc.case_token_weights(DEV, *shape))


@pytest.mark.parametrize("shape", [(3, 129, 96), (2, 300, 1028)], ids=lambda s: "x".join(map(str, s)))
def test_pair_ops_long(ops, shape):
    print(tc.case_pair_ops(DEV, *shape))


@pytest.mark.parametrize("T", [65, 130])
def test_tis_keep_long(ops, T):
    print(tc.case_tis_keep(DEV, 3, T))


def test_out_of_range_is_refused(ops):
    tc.case_out_of_range(ops, DEV)


def test_direct_entry_points_past_the_old_budget(ops):
    tc.case_direct_ops(ops, DEV)


def test_token_weight_bwd_workspace_grows_with_d(ops):
    tc.case_scratch_grows(ops, DEV)
