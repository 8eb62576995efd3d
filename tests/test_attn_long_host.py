"""The streamed attention kernels' register budget, read from the built product library (tools/kernel_inventory.py; no GPU): all six instantiations exist, none
uses scratch or spills, and the head-size-64 forms stay at or below 128 VGPRs -- two 8-wave workgroups per CU, which their 66 KiB of LDS is sized for.  (They
hold that budget because the per-block staging addresses are kept from being hoisted out of the block loop: see ATTN_PER_BLOCK in csrc/attention.hip.)"""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ant-multi-modal-framework_amd", "lib", "libantmmf_hip.so")
VGPR_MAX = {64: 128, 128: 256}   # waves per SIMD: 4 (two workgroups per CU) / 2 (one)


def test_stream_kernel_resources():
    assert os.path.isfile(LIB), "the product library is not built (__graft_entry__.build())"
    spec = importlib.util.spec_from_file_location("kernel_inventory", os.path.join(ROOT, "tools", "kernel_inventory.py"))
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    ks = inv.kernels(LIB)
    dm = inv.demangle(list(ks))
    by = {re.sub(r"^void ", "", dm[n]).split("(")[0]: v for n, v in ks.items()}
    for kern in ("attn_fwd_stream_kernel", "attn_bwd_dq_stream_kernel", "attn_bwd_dkv_stream_kernel"):
        for dh in (64, 128):
            name = f"{kern}<{dh}>"
            assert name in by, f"{name} is not in the product library"
            k = by[name]
            assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["vgpr"] + k["agpr"] <= VGPR_MAX[dh], (name, k)
    assert not any(n.startswith("attn_key_importance_kernel") for n in by)   # (its entry point launches attn_probs_kernel)
