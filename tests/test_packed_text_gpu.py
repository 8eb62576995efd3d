"""Token-packed M2 text tower on the MI355X (-m gpu): the packed kernels against the strided ones, infer_text / compute_itc packed against the same build's padded path.

Gradient parity is judged against a MEASURED noise floor: the padded step run twice, the second time with the batch items permuted (same mathematics, another
summation order); packed-vs-padded may be at most 4 x that per-parameter relative difference.  Floor and measured values go to profiles/packed_text_grad_parity.jsonl."""
import json
import os

import pytest
import torch

import model_cases as mc
import packed_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def real_lib():
    from antmmf.hip import _lib

    os.environ.pop("ANTMMF_HIP_LIB", None)
    _lib.reset_for_tests()
    assert _lib.backend() == 1


@pytest.fixture(scope="module")
def ops():
    from antmmf.hip import ops as hops

    return hops


def test_attention_packed(ops):
    print(pc.case_attention_packed(ops, DEV))
    # every workgroup of the persistent backward walks several items: 300 items x 16 heads over 256 workgroups
    g = torch.Generator().manual_seed(2)
    lengths = tuple(pc.LENGTHS) + tuple(torch.randint(1, 78, (294,), generator=g).tolist())
    print(pc.case_attention_packed(ops, DEV, lengths=lengths, heads=16, seed=4))


def test_embed_packed(ops):
    pc.case_embed_packed(ops, DEV)
    pc.case_embed_packed(ops, DEV, big=True)


def test_infer_text_packed_vs_padded():
    print(pc.case_infer_text_packed(DEV, mc.build_tiny_m2(DEV), seq=77, B=12))


def test_non_prefix_mask_takes_padded_path():
    pc.case_non_prefix_mask_takes_padded_path(DEV, mc.build_tiny_m2(DEV), seq=77, B=6)


def test_itc_step_packed_vs_padded():
    # 256 items: enough rows that the fp32 column sums of bf16 values are no longer exact (with a dozen items many of them are, and the permuted run then
    # measures a floor of exactly 0 for parameters whose atomically accumulated sums still differ from run to run by an ulp)
    r = pc.case_itc_grad_parity(DEV, mc.build_tiny_m2(DEV), seq=77, B=256)
    out = os.path.join(ROOT, "profiles", "packed_text_grad_parity.jsonl")
    try:
        with open(out, "w") as f:
            f.write(json.dumps({"loss_padded": r["loss_padded"], "loss_packed": r["loss_packed"], "loss_identical": r["loss_identical"], "lengths": r["lengths"],
                                "bound": "packed_rel <= 4 * floor_rel"}) + "\n")
            for row in r["rows"]:
                f.write(json.dumps(row) + "\n")
    except OSError:
        pass   # (a read-only checkout: the figures are in the test's output)
    assert r["loss_identical"], (r["loss_padded"], r["loss_packed"])
    assert not r["bad"], r["bad"]
