"""Hardware parity of the long-row forms of the DMAE stage-3 head kernels (csrc/tpmcl.hip) on a real MI355X (-m gpu): the cases of tests/tpmcl_long_cases.py at the
smallest shapes that cross each boundary (129 tokens, a fifth column accumulator, the scalar-D path, the 4096-token limit, selector rows of 65 / 130 / 1024), the
refusals one past every limit, and a DmaeUtils head whose token sets pass 64."""
import os

import pytest
import torch

import tpmcl_long_cases as tc

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


@pytest.mark.parametrize("shape", [(5, 129, 96), (3, 257, 1028), (3, 130, 1030), (2, 4096, 64)], ids=lambda s: "x".join(map(str, s)))
def test_token_weights_long(ops, shape):
    print(tc.case_token_weights(DEV, *shape))


@pytest.mark.parametrize("shape", [(5, 129, 96), (3, 300, 1028)], ids=lambda s: "x".join(map(str, s)))
def test_pair_ops_long(ops, shape):
    print(tc.case_pair_ops(DEV, *shape))


@pytest.mark.parametrize("R,T", [(9, 65), (9, 130), (6, 1024)])
def test_tis_keep_long(ops, R, T):
    print(tc.case_tis_keep(DEV, R, T))


def test_out_of_range_is_refused(ops):
    tc.case_out_of_range(ops, DEV)
    torch.cuda.synchronize()


def test_direct_entry_points_past_the_old_budget(ops):
    tc.case_direct_ops(ops, DEV)


def test_token_weight_bwd_workspace_grows_with_d(ops):
    tc.case_scratch_grows(ops, DEV)


def test_dmae_head_with_long_token_rows(ops):
    print(tc.case_dmae_long_rows(DEV))
