"""CPU tests of the host-side mirror of the reference's plugin surface: registries, Configuration, the C-ABI library
(loads + exports every symbol include/antmmf_hip.h declares; no compute), trainer plumbing, and the multi-process
(gloo, world 2) communication helpers."""
import ctypes
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ant-multi-modal-framework_amd")


def test_registry_and_module_registry():
    from antmmf.common.registry import registry
    from antmmf.modules.encoders import TextEncoder, VisualEncoder
    from antmmf.modules.module_registry import ModuleRegistry

    @registry.register_model("dummy_model_for_test")
    class M:
        pass

    assert registry.get_model_class("dummy_model_for_test") is M
    assert registry.get_model_class("nope") is None
    registry.register("a.b.c", 5)
    assert registry.get("a.b.c") == 5 and registry.get("a.b") == {"c": 5} and registry.get("zz", 7) == 7

    @VisualEncoder.register()
    class TinyVis(torch.nn.Module):
        def __init__(self, width=3):
            super().__init__()
            self.out_dim = width

    from antmmf.common.configuration import Configuration

    enc = VisualEncoder(Configuration({"type": "TinyVis", "params": {"width": 9}}))
    assert enc.module.out_dim == 9
    with pytest.raises(ValueError):
        TextEncoder.get("TinyVis")  # families keep separate tables
    with pytest.raises(ValueError):
        ModuleRegistry.register(3)


def test_configuration_includes_overrides_freeze(tmp_path):
    from antmmf.common.configuration import Configuration

    (tmp_path / "base.yml").write_text("training_parameters:\n  batch_size: 4\n  lr: 0.1\nmodel_attributes:\n  univl:\n    hidden_size: 768\n")
    (tmp_path / "child.yml").write_text("includes:\n- ./base.yml\ntraining_parameters:\n  batch_size: 8\n  dir: ${HOME}\n")
    cfg = Configuration.from_file(str(tmp_path / "child.yml"))
    assert cfg.training_parameters.batch_size == 8 and cfg.training_parameters.lr == 0.1
    assert cfg.training_parameters.dir == os.environ["HOME"]
    assert "includes" not in cfg
    cfg.override_with_cmd_opts(["model_attributes.univl.hidden_size", "1024", "training_parameters.betas", "[0.9, 0.98]", "x.y", "abc"])
    assert cfg.model_attributes.univl.hidden_size == 1024 and cfg.training_parameters.betas == [0.9, 0.98] and cfg.x.y == "abc"
    cfg.freeze()
    with pytest.raises(AttributeError):
        cfg.training_parameters.batch_size = 1
    cfg.defrost()
    cfg.training_parameters.batch_size = 1
    assert cfg.to_dict()["training_parameters"]["batch_size"] == 1
    with pytest.raises(FileNotFoundError):
        Configuration.from_file(str(tmp_path / "missing.yml"))


def test_reference_style_yaml_with_defaults(tmp_path):
    from antmmf.common.build import build_config
    from antmmf.common.registry import registry

    y = tmp_path / "c.yml"
    y.write_text("model_attributes:\n  univl:\n    training_head_type: video_text_retrieval\n    arch_type: clip\n"
                 "optimizer_attributes:\n  type: AdamW\n  params:\n    lr: 1e-5\n    betas: [0.9, 0.98]\n    weight_decay: 1e-4\n")
    cfg = build_config(str(y), opts_override=["training_parameters.batch_size", "2"])
    assert cfg.training_parameters.trainer == "base_trainer" and cfg.training_parameters.batch_size == 2
    assert registry.get("config") is cfg


def test_c_abi_library_exports_every_declared_symbol():
    lib_path = os.path.join(PKG, "lib", "libantmmf_hip.so")
    assert os.path.isfile(lib_path), "run __graft_entry__.build() first"
    lib = ctypes.CDLL(lib_path)
    header = open(os.path.join(ROOT, "include", "antmmf_hip.h")).read()
    names = re.findall(r"\bint\s+(antmmf_\w+)\s*\(", header)
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/antmmf_hip.h but not exported"
    lib.antmmf_backend.restype = ctypes.c_int
    assert lib.antmmf_backend() == 1 and lib.antmmf_abi_version() == 2
    from antmmf.hip import _lib

    assert set(names) == set(_lib._SIGNATURES), set(names) ^ set(_lib._SIGNATURES)
    # the product library is a product: nothing but the declared entry points and two read-only probes, no environment variable is read (no "ANTMMF_*" string in it)
    import subprocess

    exported = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True).stdout.splitlines() if " T antmmf_" in ln}
    assert exported == set(names) | {"antmmf_debug_gemm_clock", "antmmf_debug_gemm_k64_launches"}, exported ^ set(names)
    assert b"ANTMMF_" not in open(lib_path, "rb").read()
    # the lab library (tests / tools only): everything above plus include/antmmf_hip_lab.h
    lab_path = os.path.join(PKG, "lib", "libantmmf_hip_lab.so")
    assert os.path.isfile(lab_path), "run __graft_entry__.build() first (make -C csrc lab)"
    lab = ctypes.CDLL(lab_path)
    lab_names = re.findall(r"\bint\s+(antmmf_\w+)\s*\(", open(os.path.join(ROOT, "include", "antmmf_hip_lab.h")).read())
    assert set(lab_names) == set(_lib._LAB_SIGNATURES), set(lab_names) ^ set(_lib._LAB_SIGNATURES)
    for n in names + lab_names:
        assert hasattr(lab, n), f"{n} not exported by the lab library"


def test_product_kernel_resources():
    """The built product library's own kernel metadata (tools/kernel_inventory.py: AMDGPU notes of the embedded gfx950 code objects): the kernels the flagship step
    launches keep the register budget their occupancy depends on and use no scratch -- a register-allocation regression (the round-3 incident: an edit in a shared
    device function cost the wgrad kernel 528 B of spills and 17 % without any warning) fails HERE, without a GPU -- and the library holds only product kernels."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_inventory", os.path.join(ROOT, "tools", "kernel_inventory.py"))
    inv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(inv)
    lib_path = os.path.join(PKG, "lib", "libantmmf_hip.so")
    ks = inv.kernels(lib_path)
    dm = inv.demangle(list(ks))
    by = {re.sub(r"^void ", "", dm[n]).split("(")[0]: v for n, v in ks.items()}
    assert 150 <= len(by) <= 275, len(by)    # 234 in round 5 (292 before the lab split); round 6: + 14 forms of the attention backward with token sums
    # (name, max VGPRs): 512-thread GEMM workgroups run 2 waves per SIMD -> <= 256; the 8-wave attention workgroups 2 per CU -> <= 128 (the one-kernel backward: 1 per CU -> <= 256)
    must = [("gemm_nt_k64r_kernel<0, 0>", 240), ("gemm_nt_k64r_kernel<1, 0>", 240), ("gemm_nt_k64r_kernel<2, 0>", 240), ("gemm_nt_k64r_kernel<3, 0>", 240),
            ("gemm_nt_k64r_kernel<5, 0>", 256), ("gemm_nt_k64r_kernel<37, 0>", 240), ("gemm_nt_k64r_kernel<69, 0>", 240), ("gemm_nt_k64r_kernel<8, 0>", 248), ("gemm_nt_k64r_kernel<10, 0>", 256), ("gemm_tn_k64_kernel<1>", 256), ("gemm_nt_k64p_kernel<8, 37>", 256), ("gemm_nt_k64p_kernel<9, 37>", 256),
            ("attn_fwd_kernel<9, false, 64, 0>", 128), ("attn_fwd_kernel<3, false, 64, 0>", 128), ("attn_bwd_dq_kernel<9, false, 64>", 128), ("attn_bwd_dq_kernel<3, false, 64>", 128),
            ("attn_bwd_dkv_kernel<false, 64>", 128),
            ("attn_bwd_fused64_kernel<8, true, true, 9, true, 0, false, 0>", 256), ("attn_bwd_fused64_kernel<7, false, false, 0, true, 0, false, 0>", 256),
            ("attn_bwd_fused64_kernel<3, false, false, 0, true, 0, true, 0>", 256),   # one 8-wave workgroup per CU (151 KB of LDS)
            # ... and with the token sums of dQ | dK (| dV) for the q / k / v bias gradients (round 6: 252 VGPRs; as a block behind the register prefetch it spilled 144 B)
            ("attn_bwd_fused64_kernel<8, true, true, 9, true, 0, false, 2>", 256), ("attn_bwd_fused64_kernel<7, false, false, 0, true, 0, false, 1>", 256)]
    for name, vmax in must:
        assert name in by, f"{name} is not in the product library"
        k = by[name]
        assert k["scratch"] == 0 and k["spill_vgpr"] == 0 and k["vgpr"] + k["agpr"] <= vmax, (name, k)
    scratch = sorted(n for n, v in by.items() if v["scratch"])
    assert scratch == [], scratch   # (round 6: the one kernel that had 20 B per lane, the burst kernel's run-time epilogue form gemm_nt_k64p_kernel<4, 33>, is gone from the product)
    # experiment kernels stay in the lab library
    for n in by:
        assert not n.startswith(("attn_fwd32_kernel", "ffn_")) and "gemm_nt_k64r_kernel<0, 8>" not in n, n
    lab = {re.sub(r"^void ", "", d).split("(")[0] for d in inv.demangle(list(inv.kernels(os.path.join(PKG, "lib", "libantmmf_hip_lab.so")))).values()}
    assert set(by) <= lab and any(n.startswith("attn_fwd32_kernel") for n in lab)


def test_k64r_isa_audit(tmp_path):
    """tools/k64r_audit.py over the ISA hipcc emits for csrc/gemm.hip TODAY (device-only -S, ~1 min): the rolling-epilogue kernel's residual vectors are loaded by inline
    asm into registers hipcc believes already written -- any instruction that touches one of them between its load and the counted `s_waitcnt vmcnt(N)` that retires it is
    silent data corruption on hardware that neither the emulator nor a lucky GPU run shows.  Also: no scratch, no v_accvgpr moves in the five product instantiations (plain, bias, residual, bias + residual, gate)."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "gemm_dev.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-S", "--cuda-device-only",
                           os.path.join(PKG, "csrc", "gemm.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "k64r_audit.py"), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("k64r<")]
    assert len(lines) == 6 and all("problems 0" in ln or "no residual loads" in ln for ln in lines), p.stdout   # plain, bias, residual, bias + residual, gate, gate + column sums
    assert sum("loads 28 problems 0" in ln for ln in lines) == 2 and sum("loads 16 problems 0" in ln for ln in lines) == 2, p.stdout    # the two residual kernels and the two gate kernels were really audited


def test_attention_m0_audit(tmp_path):
    """tools/m0_audit.py over the ISA hipcc emits for csrc/attention.hip (device-only -S, ~40 s): the one-kernel attention backward sets M0 and issues its LDS-DMA pieces
    from inline asm (attn_dma_piece, "m0" clobbered) -- every such piece has its own `s_mov_b32 m0` and the compiler never reads M0 behind one of them without writing it
    first."""
    import shutil
    import subprocess

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.isfile(hipcc):
        pytest.skip("hipcc not available")
    assert '"memory", "m0")' in open(os.path.join(PKG, "csrc", "attention.hip")).read()
    out = tmp_path / "attn_dev.s"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", "-S", "--cuda-device-only",
                           os.path.join(PKG, "csrc", "attention.hip"), "-o", str(out)], stderr=subprocess.DEVNULL)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "m0_audit.py"), str(out)], capture_output=True, text=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("m0 audit ")]
    assert p.returncode == 0 and len(lines) >= 10 and all(ln.endswith("problems 0") for ln in lines), p.stdout[-3000:]


def test_hip_ops_refuse_cpu_tensors_and_missing_library(monkeypatch):
    from antmmf.hip import _lib, ops

    monkeypatch.delenv("ANTMMF_HIP_LIB", raising=False)
    _lib.reset_for_tests()
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.act_fwd(torch.zeros(8), "gelu")  # host tensor into the device library: loud failure, no fallback
    monkeypatch.setenv("ANTMMF_HIP_LIB", "/nonexistent/libantmmf_hip.so")
    _lib.reset_for_tests()
    with pytest.raises(_lib.HipLibraryError):
        _lib.load()
    # the emulator build is refused outside pytest (it is test infrastructure, never a product backend)
    emu_lib = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
    if os.path.isfile(emu_lib):
        import subprocess

        code = ("import os, sys; sys.path.insert(0, %r); os.environ['ANTMMF_HIP_LIB'] = %r; os.environ.pop('PYTEST_CURRENT_TEST', None);"
                "from antmmf.hip import _lib\n"
                "try:\n    _lib.load(); print('loaded')\nexcept _lib.HipLibraryError as e:\n    print('refused' if 'EMULATOR' in str(e) else 'other')" % (PKG, emu_lib))
        env = {k: v for k, v in os.environ.items() if k not in ("PYTEST_CURRENT_TEST", "ANTMMF_ALLOW_EMULATOR")}
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert "refused" in out.stdout, out.stdout + out.stderr
    monkeypatch.delenv("ANTMMF_HIP_LIB")
    _lib.reset_for_tests()


# ------------------------------------------------------------------------------ multi-process (gloo, world 2)
def _install_gloo_reduce_scatter():
    """TEST SHIM: gloo has no reduce_scatter_tensor; the product code calls it unconditionally (RCCL has it), so the CPU multi-process tests
    provide it as all_reduce + slice."""
    if getattr(dist, "_antmmf_rs_shim", False):
        return
    real = dist.reduce_scatter_tensor

    def shim(output, input, op=dist.ReduceOp.SUM, group=None, async_op=False):
        if dist.get_backend(group) != "gloo":
            return real(output, input, op=op, group=group, async_op=async_op)
        full = input.clone()
        dist.all_reduce(full, op=op, group=group)
        r, n = dist.get_rank(group), output.shape[0]
        output.copy_(full[r * n:(r + 1) * n])
        return None

    dist.reduce_scatter_tensor = shim
    dist._antmmf_rs_shim = True


def _worker(rank, world, port, fn, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    for p in (ROOT, PKG, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _install_gloo_reduce_scatter()
    try:
        ret[rank] = fn(rank, world)
    finally:
        dist.destroy_process_group()


def _spawn(fn, port, world=2):
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, fn, ret), nprocs=world, join=True)
    return dict(ret)


def _gather_case(rank, world):
    import weightgen as W
    from antmmf.utils import distributed_utils as du
    from oracle import losses

    t = W.data_tensor("gather.t", (world * 3, 8))[rank * 3:(rank + 1) * 3].clone().requires_grad_(True)
    v = W.data_tensor("gather.v", (world * 3, 8))[rank * 3:(rank + 1) * 3].clone().requires_grad_(True)
    gt = du.gather_tensor(t, method="cat", back_gradient=True, pad_tensors=True)
    gv = du.gather_tensor(v, method="cat", back_gradient=True, pad_tensors=True)
    loss = losses.mil_nce(gt @ gv.t(), world * 3, 1)
    loss.backward()
    ragged = du.gather_tensor(torch.full((rank + 1, 2), float(rank)), method="cat", pad_tensors=True)
    stacked = du.gather_tensor(torch.tensor(float(rank)))
    objs = du.all_gather({"rank": rank})
    red = du.reduce_dict({"a": torch.tensor(float(rank + 1))})
    return dict(loss=loss.detach(), dt=t.grad, dv=v.grad, ragged=ragged, stacked=stacked, objs=objs, red=float(red["a"]),
                world=du.get_world_size(), main=du.is_main_process())


def test_gather_tensor_matches_reference_two_ranks(golden):
    """gather_tensor(back_gradient=True) over 2 gloo ranks == the fixture produced by the reference's GradientAllGather
    (loss identical on both ranks, local grad = W x single-process grad slice)."""
    g = golden("gather_w2.pt")
    out = _spawn(_gather_case, 29641)
    for r in range(2):
        torch.testing.assert_close(out[r]["loss"], g[f"rank{r}.loss"], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out[r]["dt"], g[f"rank{r}.dt"], rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(out[r]["dv"], g[f"rank{r}.dv"], rtol=1e-4, atol=1e-6)
        assert out[r]["ragged"].shape == (3, 2) and out[r]["ragged"][0, 0] == 0 and out[r]["ragged"][2, 0] == 1
        assert out[r]["stacked"].tolist() == [0.0, 1.0]
        assert out[r]["objs"] == [{"rank": 0}, {"rank": 1}]
        assert out[r]["world"] == 2 and out[r]["main"] == (r == 0)
    assert out[0]["red"] == 1.5


def _sharded_loss_case(rank, world):
    """Row-sharded MIL-NCE / ITC through the emulated kernels on 2 ranks."""
    os.environ["ANTMMF_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
    import weightgen as W
    from antmmf.hip import _lib, contrastive

    _lib.reset_for_tests()
    B, n, D = 3, 2, 16
    T = torch.nn.functional.normalize(W.data_tensor("shard.t", (world * B, D)), dim=-1)
    V = torch.nn.functional.normalize(W.data_tensor("shard.v", (world * B * n, D)), dim=-1)
    t = T[rank * B:(rank + 1) * B].clone().requires_grad_(True)
    v = V[rank * B * n:(rank + 1) * B * n].clone().requires_grad_(True)
    loss = contrastive.mil_nce_sharded(t, v, n_clips=n)
    loss.backward()
    ls = torch.tensor(2.0, requires_grad=True)
    i2 = T[rank * B:(rank + 1) * B].clone().requires_grad_(True)
    t2 = V[::n][rank * B:(rank + 1) * B].clone().requires_grad_(True)
    l2 = contrastive.clip_itc_sharded(i2, t2, ls)
    l2.backward()
    return dict(loss=loss.detach(), dt=t.grad, dv=v.grad, itc=l2.detach(), di=i2.grad, dt2=t2.grad, dls=ls.grad)


def test_sharded_losses_two_ranks_match_oracle():
    import weightgen as W
    from oracle import losses
    from test_kernels_emu import _stale

    if _stale():
        import subprocess

        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    world, B, n, D = 2, 3, 2, 16
    out = _spawn(_sharded_loss_case, 29643)
    T = torch.nn.functional.normalize(W.data_tensor("shard.t", (world * B, D)), dim=-1).requires_grad_(True)
    V = torch.nn.functional.normalize(W.data_tensor("shard.v", (world * B * n, D)), dim=-1).requires_grad_(True)
    simi = torch.matmul(V.view(world * B, n, D), T.t()).permute(2, 0, 1)
    mil = simi.unsqueeze(1).expand(world * B, n, world * B, n).reshape(world * B * n, world * B * n)
    ref = losses.mil_nce(mil, world * B, n)
    ref.backward()
    I2 = T.detach().clone().requires_grad_(True)
    T2 = V.detach()[::n].clone().requires_grad_(True)
    ls = torch.tensor(2.0, requires_grad=True)
    ref2, _ = losses.clip_itc(I2, T2, ls)
    ref2.backward()
    for r in range(world):
        torch.testing.assert_close(out[r]["loss"], ref.detach(), rtol=1e-5, atol=1e-6)
        # W x the single-process gradient, as the reference's gradient all-gather yields before DDP's 1/W
        torch.testing.assert_close(out[r]["dt"], world * T.grad[r * B:(r + 1) * B], rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(out[r]["dv"], world * V.grad[r * B * n:(r + 1) * B * n], rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(out[r]["itc"], ref2.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out[r]["di"], world * I2.grad[r * B:(r + 1) * B], rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(out[r]["dt2"], world * T2.grad[r * B:(r + 1) * B], rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(out[0]["dls"] + out[1]["dls"], world * ls.grad, rtol=1e-3, atol=1e-6)


def _ragged_loss_case(rank, world):
    """Row-sharded MIL-NCE / ITC on 2 ranks with UNEQUAL batches (3 and 2 pairs; max_rows = 3): pad + mask instead of the equal-batch assert."""
    os.environ["ANTMMF_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
    import weightgen as W
    from antmmf.hip import _lib, contrastive

    _lib.reset_for_tests()
    counts, n, D = [3, 2], 2, 16
    lo = sum(counts[:rank])
    B = counts[rank]
    Bg = sum(counts)
    T = torch.nn.functional.normalize(W.data_tensor("ragged.t", (Bg, D)), dim=-1)
    V = torch.nn.functional.normalize(W.data_tensor("ragged.v", (Bg * n, D)), dim=-1)
    wgt = W.data_tensor("ragged.w", (Bg,)).abs() + 0.5
    t = T[lo:lo + B].clone().requires_grad_(True)
    v = V[lo * n:(lo + B) * n].clone().requires_grad_(True)
    loss = contrastive.mil_nce_sharded(t, v, n_clips=n, weight=wgt[lo:lo + B], max_rows=3)
    loss.backward()
    ls1, ls2 = torch.tensor(2.0, requires_grad=True), torch.tensor(1.5, requires_grad=True)
    i1 = T[lo:lo + B].clone().requires_grad_(True)
    t1 = V[::n][lo:lo + B].clone().requires_grad_(True)
    i2 = V[1::n][lo:lo + B].clone().requires_grad_(True)
    t2 = T[lo:lo + B].clone().requires_grad_(True)
    contrastive.set_max_rows_per_rank(3)       # the trainer's way of switching the ragged path on
    try:
        l1, l2 = contrastive.clip_itc_pair_sharded(i1, t1, ls1, i2, t2, ls2)
    finally:
        contrastive.set_max_rows_per_rank(None)
    (l1 + 2.0 * l2).backward()
    return dict(loss=loss.detach(), dt=t.grad, dv=v.grad, l1=l1.detach(), l2=l2.detach(), di1=i1.grad, dt1=t1.grad, di2=i2.grad, dt2=t2.grad,
                dls1=ls1.grad, dls2=ls2.grad)


def test_sharded_losses_ragged_batches_match_oracle():
    """the last, partial batch of an epoch (reference: pad + trim on every gather, antmmf/utils/distributed_utils.py:131-160).
    2 gloo ranks with 3 and 2 pairs == the oracle on the 5-pair global batch: loss on both ranks, W x the single-process gradient slices, the
    logit-scale gradients summed over ranks."""
    import weightgen as W
    from oracle import losses
    from test_kernels_emu import _stale

    if _stale():
        import subprocess

        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    world, counts, n, D = 2, [3, 2], 2, 16
    Bg = sum(counts)
    out = _spawn(_ragged_loss_case, 29647)
    T = torch.nn.functional.normalize(W.data_tensor("ragged.t", (Bg, D)), dim=-1).requires_grad_(True)
    V = torch.nn.functional.normalize(W.data_tensor("ragged.v", (Bg * n, D)), dim=-1).requires_grad_(True)
    wgt = W.data_tensor("ragged.w", (Bg,)).abs() + 0.5
    simi = torch.matmul(V.view(Bg, n, D), T.t()).permute(2, 0, 1)
    mil = simi.unsqueeze(1).expand(Bg, n, Bg, n).reshape(Bg * n, Bg * n)
    ref = losses.mil_nce(mil, Bg, n, weight=wgt)
    ref.backward()
    I1, T1 = T.detach().clone().requires_grad_(True), V.detach()[::n].clone().requires_grad_(True)
    I2, T2 = V.detach()[1::n].clone().requires_grad_(True), T.detach().clone().requires_grad_(True)
    ls1, ls2 = torch.tensor(2.0, requires_grad=True), torch.tensor(1.5, requires_grad=True)
    r1, _ = losses.clip_itc(I1, T1, ls1)
    r2, _ = losses.clip_itc(I2, T2, ls2)
    (r1 + 2.0 * r2).backward()
    lo = 0
    for r in range(world):
        B = counts[r]
        torch.testing.assert_close(out[r]["loss"], ref.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out[r]["dt"], world * T.grad[lo:lo + B], rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(out[r]["dv"], world * V.grad[lo * n:(lo + B) * n], rtol=1e-3, atol=1e-6)
        torch.testing.assert_close(out[r]["l1"], r1.detach(), rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(out[r]["l2"], r2.detach(), rtol=1e-5, atol=1e-6)
        for got, want in (("di1", I1), ("dt1", T1), ("di2", I2), ("dt2", T2)):
            assert out[r][got].shape[0] == B
            torch.testing.assert_close(out[r][got], world * want.grad[lo:lo + B], rtol=1e-3, atol=1e-6)
        lo += B
    torch.testing.assert_close(out[0]["dls1"] + out[1]["dls1"], world * ls1.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(out[0]["dls2"] + out[1]["dls2"], world * ls2.grad, rtol=1e-3, atol=1e-6)


def _trainer_case(rank, world):
    from antmmf.common.configuration import Configuration
    from antmmf.common.registry import registry
    from antmmf.models.base_model import BaseModel
    from antmmf.structures.sample import SampleList
    from antmmf.trainers.build import build_trainer

    @registry.register_model("toy_contrastive")
    class Toy(BaseModel):
        def build(self):
            self.lin = torch.nn.Linear(4, 4)

        def forward(self, sample_list):
            y = self.lin(sample_list["image_data"])
            return {"losses": {"toy_loss": ((y - sample_list["caption_target"]) ** 2).mean()}}

    cfg = Configuration({
        "training_parameters": {"trainer": "base_trainer", "device": "cpu", "max_iterations": 6, "log_interval": 100, "seed": 3,
                                "clip_gradients": True, "max_grad_l2_norm": 10.0},
        "optimizer_attributes": {"type": "SGD", "params": {"lr": 0.1}},
        "model_attributes": {"toy_contrastive": {}},
    })
    g = torch.Generator().manual_seed(100 + rank)
    batches = [SampleList(image_data=torch.randn(5, 4, generator=g), caption_target=torch.randn(5, 4, generator=g)) for _ in range(8)]
    tr = build_trainer(cfg, batches)
    tr.load()
    meters = tr.train()
    w = torch.cat([p.detach().flatten() for p in tr.model.parameters()])
    return dict(iters=tr.current_iteration, w=w, loss=meters["toy_loss"])


def _too_many_rows_case(rank, world):
    """rank 1 holds 4 rows against max_rows = 3: BOTH ranks must fail in the same loss call (the offending rank used to raise before the count exchange and the
    other one blocked in it)"""
    os.environ["ANTMMF_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
    from antmmf.hip import contrastive

    B = 4 if rank == 1 else 2
    t = torch.nn.functional.normalize(torch.randn(B, 8), dim=-1)
    try:
        contrastive.clip_itc_sharded(t, t.clone(), torch.tensor(1.0), max_rows=3)
    except (ValueError, RuntimeError, AssertionError) as e:
        return type(e).__name__ + ": " + str(e)
    return "no error"


def test_ragged_batch_over_the_maximum_fails_on_every_rank():
    if not os.path.exists(os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")):
        pytest.skip("emulated kernel library not built")
    out = _spawn(_too_many_rows_case, 29649)
    # the SAME host-side ValueError on both ranks, raised from the gathered counts (not a device-side assert: stock ROCm wheels compile those out)
    assert all(out[r].startswith("ValueError: a rank holds 4 rows, more than max_rows = 3") for r in (0, 1)), out


def test_base_trainer_data_parallel_two_ranks():
    out = _spawn(_trainer_case, 29645)
    assert out[0]["iters"] == 6 and out[1]["iters"] == 6  # one increment per batch
    torch.testing.assert_close(out[0]["w"], out[1]["w"])  # replicas stay in sync (broadcast init + averaged grads)


def _moco_queue_case(rank, world):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "ant-multi-modal-framework_amd", "prj", "base_vtp"))
    from antmmf.common.configuration import Configuration
    from roi_univl.univl.model.moco_utils import MocoUtils

    mu = MocoUtils(Configuration(dict(hidden_size=8, K=12)), img_encoder=torch.nn.Linear(2, 2), txt_encoder=torch.nn.Linear(2, 2))
    mu.txt_queue.zero_()
    out = []
    for step in range(3):  # 3 pushes of 2 x 3 keys into K = 12: the third wraps (write pointer back to 0, tail overwritten)
        keys = torch.full((3, 8), float(10 * step + rank + 1))
        vkeys = keys.clone()
        if step == 1 and rank == 1:
            vkeys[0, 0] = float("nan")  # a NaN anywhere in the gathered keys skips the whole update on every rank
        mu.dequeue_and_enqueue(vkeys, keys)
        out.append((mu.txt_queue[0].clone(), int(mu.txt_queue_ptr), torch.isfinite(mu.img_queue).all().item()))
    return out


def test_moco_enqueue_two_ranks():
    """dequeue_and_enqueue over 2 gloo ranks: every rank's queue receives [rank0 keys ; rank1 keys] at the shared write pointer,
    the pointer wraps at K, replicas stay identical, and a NaN key leaves the (image) queue untouched on every rank."""
    out = _spawn(_moco_queue_case, 29655)
    for step in range(3):
        torch.testing.assert_close(out[0][step][0], out[1][step][0])
        assert out[0][step][1] == out[1][step][1] == (6 * (step + 1)) % 12
        assert out[0][step][2] and out[1][step][2]
    q1 = out[0][0][0]
    assert q1[:6].tolist() == [1.0, 1.0, 1.0, 2.0, 2.0, 2.0] and q1[6:].abs().sum() == 0
    q3 = out[0][2][0]
    assert q3[:6].tolist() == [21.0, 21.0, 21.0, 22.0, 22.0, 22.0] and q3[6:].tolist() == [11.0, 11.0, 11.0, 12.0, 12.0, 12.0]


def _dmae_wti_case(rank, world):
    """DMAE wti_interaction on 2 ranks (emulated kernels): each rank holds half of the batch, scores the gathered global batch."""
    os.environ["ANTMMF_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
    import model_cases as mc
    import weightgen as W
    from antmmf.common.configuration import Configuration

    g = torch.load(os.path.join(ROOT, "tests", "golden", "ops_dmae_wti.pt"))
    du = mc.load_dmae_utils().DmaeUtils(Configuration(dict(mc.DMAE_CFG, l3_interaction="att_wti", l3_with_nfc=True, l3_sim_header="meanP")))
    W.fill_module_(du)
    du.train()
    sl = slice(rank * 2, rank * 2 + 2)
    t, w_, v = (g[k][sl].clone().requires_grad_(True) for k in ("text", "word", "video"))
    out = du.wti_interaction(t, w_, v, g["word_mask"][sl], g["video_mask"][sl])
    (out * g["g"]).sum().backward()
    return dict(out=out.detach(), dtext=t.grad, dvideo=v.grad, dword=w_.grad)


def test_dmae_wti_two_ranks_match_reference(golden):
    """wti_interaction with the batch split over 2 gloo ranks == the reference's single-process result on the whole batch:
    identical [4, 4] scores on both ranks, and local feature gradients = W x the single-process gradient slice (the gather's
    reduce-sum backward; the data-parallel mean divides it back)."""
    if not os.path.exists(os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")):
        pytest.skip("emulated kernel library not built")
    out = _spawn(_dmae_wti_case, 29665)
    g = golden("ops_dmae_wti.pt")
    for r in (0, 1):
        sl = slice(r * 2, r * 2 + 2)
        torch.testing.assert_close(out[r]["out"], g["att_wti.va1.out"], rtol=1e-3, atol=1e-3)
        for key, ref in (("dtext", "att_wti.va1.dtext"), ("dvideo", "att_wti.va1.dvideo"), ("dword", "att_wti.va1.dword")):
            torch.testing.assert_close(out[r][key], 2.0 * g[ref][sl], rtol=3e-2, atol=3e-2 * float(g[ref].abs().max()))


def _tiny_stage2_model(**extra):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "ant-multi-modal-framework_amd", "prj", "base_vtp"))
    import model_cases as mc
    import roi_univl  # noqa: F401
    from antmmf.common.configuration import Configuration
    from roi_univl.univl.model.univl_video_ret import UnivlForVideoTextRetrieval

    cfg = dict(mc.TINY_CLIP_CFG, training_stage="stage1+stage2", with_cross_encoder=True, hard_example_mining=True, re_sample_method="top_k",
               re_weight_method="median", **extra)
    return UnivlForVideoTextRetrieval(Configuration(cfg)).train()


def test_cnvid_scheduled_mining_gate_takes_the_reference_decisions(golden, monkeypatch):
    """prj/cnvid_vtp/roi_univl/univl/model/univl_video_ret.py:398-428: with `incre_num` given, stage 2 mines hard negatives only when the (rank-agreed) draw / 100 falls
    below it.  tests/golden/e2e_cnvid_gate.pt holds the decisions the REFERENCE class took for 16 seeds x 5 ratios (make_golden.py gen_cnvid_gate); the product draws with the
    same generator call, so a seeded single-process run must take the same branch every time.  The two similarity routines are stubbed (their parity is
    test_univl_stage2_*); the row re-weighting runs on both branches as in the reference."""
    if not os.path.exists(os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")):
        pytest.skip("emulated kernel library not built")
    monkeypatch.setenv("ANTMMF_HIP_LIB", os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so"))
    from antmmf.hip import _lib

    _lib.reset_for_tests()
    g = golden("e2e_cnvid_gate.pt")
    model = _tiny_stage2_model(change_iter=5000, change_rate=0.15)
    calls = []
    B = 4
    scores = torch.randn(B, B)
    monkeypatch.setattr(model, "_cross_similarity_hard_mining", lambda *a, **k: (calls.append(1), scores.clone().requires_grad_(True))[1])
    monkeypatch.setattr(model, "get_l2_simi_matrix", lambda *a, **k: (calls.append(0), scores.clone().requires_grad_(True))[1])
    cap_input, vis_input = (None, None, None, B, None), (None, None, None, 2, None)
    l1 = torch.randn(B, B)
    try:
        for si, seed in enumerate(g["seeds"].tolist()):
            torch.manual_seed(seed)
            assert abs(model.scheduled_mining_draw(torch.device("cpu")) * 100.0 - float(g["draw"][si])) < 1e-4
            for ii, inc in enumerate(g["incre_num"].tolist()):
                del calls[:]
                torch.manual_seed(seed)
                out = model.forward_stage2(vis_input, cap_input, {"losses": {}, "l1_simi": l1}, True, incre_num=inc)
                assert calls == [int(g["mined"][si, ii])] and model._last_mined == bool(g["mined"][si, ii]), (seed, inc, calls)
                assert torch.isfinite(out["losses"]["level2_similarity_loss"])
        # no schedule (prj/base_vtp): every training step mines; evaluation never does
        del calls[:]
        model.forward_stage2(vis_input, cap_input, {"losses": {}, "l1_simi": l1}, True)
        model.eval()
        model.forward_stage2(vis_input, cap_input, {"losses": {}, "l1_simi": l1}, True, incre_num=1.0)
        assert calls == [1, 0]
    finally:
        monkeypatch.undo()
        _lib.reset_for_tests()


def _gate_draw_case(rank, world):
    import sys

    sys.path.insert(0, os.path.join(ROOT, "ant-multi-modal-framework_amd", "prj", "base_vtp"))
    import roi_univl  # noqa: F401
    from roi_univl.univl.model.univl_video_ret import UnivlForVideoTextRetrieval

    out = []
    for step in range(6):
        torch.manual_seed(1000 * rank + step)   # the ranks' generators are NOT in step: agreement has to come from the collective
        mine = torch.randint(low=0, high=100, size=[1], dtype=torch.float32)
        torch.manual_seed(1000 * rank + step)
        out.append((float(mine), UnivlForVideoTextRetrieval.scheduled_mining_draw(None, torch.device("cpu"))))
    return out


def test_cnvid_gate_draw_is_rank_agreed_two_ranks():
    """the gate's draw on 2 gloo ranks: both ranks obtain the MEAN of the two local draws / 100 (reference: gather_tensor + torch.mean, :417-420), hence the same branch"""
    out = _spawn(_gate_draw_case, 29675)
    for step in range(6):
        want = (out[0][step][0] + out[1][step][0]) / 2 / 100.0
        assert abs(out[0][step][1] - want) < 1e-6 and abs(out[1][step][1] - want) < 1e-6, (step, out[0][step], out[1][step])
    assert any(out[0][s][0] != out[1][s][0] for s in range(6))


def test_m2_checkpoint_converters_match_reference(golden):
    """convert_pl_ckpt / convert_deepspeed_ckpt (released-weight loading of the M2 encoder) against the reference's own functions
    (tests/golden/m2_ckpt_convert.pt): position-table growth by area interpolation, truncation, prefix stripping."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "ant-multi-modal-framework_amd", "prj", "M2_Encoder"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import weightgen as W
    from vlmo.modules import vlmo_module as vm

    g = golden("m2_ckpt_convert.pt")
    dim = 8
    for tag, rows in (("grow", 3 + 16), ("shrink", 3 + 64), ("same", 3 + 36)):
        sd = {"backbone.encoder.embed_positions.A.weight": W.data_tensor(f"ckpt.{tag}.pos", (rows, dim)),
              "visual_tokenizer.x": torch.ones(2), "other.weight": W.data_tensor(f"ckpt.{tag}.o", (3, 2))}
        out = vm.convert_pl_ckpt(dict(sd), num_visual_token=37)
        torch.testing.assert_close(out["backbone.encoder.embed_positions.A.weight"], g[f"pl.{tag}.pos"], rtol=1e-6, atol=1e-7)
        assert len(out) == int(g[f"pl.{tag}.nkeys"])
    ds = {"_forward_module.backbone.encoder.embed_positions.A.weight": W.data_tensor("ckpt.ds.pos", (3 + 16, dim)),
          "_forward_module.visual_tokenizer.encoder.pos_embed": W.data_tensor("ckpt.ds.vt", (1, 1 + 16, dim)),
          "_forward_module.head.weight": W.data_tensor("ckpt.ds.h", (2, 2)), "plain.bias": torch.zeros(2)}
    out = vm.convert_deepspeed_ckpt(dict(ds), num_visual_token=37)
    torch.testing.assert_close(out["backbone.encoder.embed_positions.A.weight"], g["ds.pos"], rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(out["visual_tokenizer.encoder.pos_embed"], g["ds.vt"], rtol=1e-6, atol=1e-7)
    assert sorted(len(k) for k in out) == g["ds.keys"].tolist()


def _m2_step_case(rank, world):
    """One tiny-M2 ITC training step through the product stack on `world` gloo ranks (emulated kernels): VLMo towers, packed sharded ITC
    pair loss, gradient all-reduce over the flat arena (started from inside backward), fused AdamW with grad_scale = 1 / world."""
    os.environ["ANTMMF_HIP_LIB"] = os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so")
    sys.path.insert(0, os.path.join(PKG, "prj", "M2_Encoder"))
    import model_cases as mc
    import weightgen as W
    from antmmf.hip import _lib
    from antmmf.hip.arena import HipAdamW

    _lib.reset_for_tests()
    dev = torch.device("cpu")
    model = mc.build_tiny_m2(dev)
    opt = HipAdamW([{"params": list(model.parameters())}], lr=1e-2, weight_decay=0.01)
    pairs = int(os.environ.get("ANTMMF_TEST_DP_PAIRS", "4"))
    img = (W.data_tensor("m2dp.image", (pairs, 3, 32, 32)) * 0.25 + 0.5).clamp(0, 1)
    ids = W.data_ints("m2dp.ids", (pairs, 12), 1, 300)
    lengths = torch.tensor([12, 5, 8, 3, 7, 12, 4, 9])[:pairs]
    mask = (torch.arange(12)[None, :] < lengths[:, None]).long()
    ids = ids * mask
    per = pairs // world
    sl = slice(rank * per, (rank + 1) * per)
    mode = os.environ.get("ANTMMF_TEST_DP_MODE", "overlap")
    if world > 1 and mode != "plain":
        assert opt.arena.arm_overlap(bucket_bytes=64 << 10, reduce_dtype=torch.bfloat16 if mode == "bf16" else None)
    out = model({"image": [img[sl]], "text_ids": ids[sl], "text_masks": mask[sl]})
    loss = out["losses"]["itc_loss"] + out["losses"]["itc_vl_loss"]
    loss.backward()
    w = opt.arena.allreduce_grads()
    overlapped = getattr(opt.arena, "overlapped_buckets", 0)
    opt.grad_scale = 1.0 / w
    gsum = opt.arena.grad.clone() / w
    opt.step()
    return dict(loss=float(loss), grad=gsum, master=opt.arena.master.clone(), world=w, overlapped=overlapped,
                nbuckets=len(getattr(opt.arena, "_buckets", [])))


_SLOW = pytest.mark.skipif(not os.environ.get("ANTMMF_SLOW_TESTS"), reason="set ANTMMF_SLOW_TESTS=1 (three emulated M2 steps, ~3 min each variant)")


# (default run: the 4-rank twin below covers the overlap mode with more participants; the 2-rank variants are the slow set)
@pytest.mark.parametrize("mode", [pytest.param("overlap", marks=_SLOW), pytest.param("plain", marks=_SLOW), pytest.param("bf16", marks=_SLOW)])
def test_m2_step_two_ranks_equals_single_rank(mode):
    """the WHOLE M2 step on 2 ranks (2 pairs each) == the 1-rank step on the 4-pair batch: same global loss on both
    ranks, the averaged arena gradient equals the single-rank gradient, replicas hold identical weights after the fused AdamW.
    overlap: buckets all-reduced from inside the backward pass (some must really have gone early); plain: after backward; bf16: bf16 buckets."""
    os.environ["ANTMMF_TEST_DP_MODE"] = mode
    try:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(2) as ex:   # the 2-rank job and the 1-rank job side by side (emulated kernels: CPU-bound)
            f2 = ex.submit(_spawn, _m2_step_case, 29671 + ["overlap", "plain", "bf16"].index(mode))
            f1 = ex.submit(_spawn, _m2_step_case, 29675 + ["overlap", "plain", "bf16"].index(mode), 1)
            two, one = f2.result(), f1.result()[0]
    finally:
        os.environ.pop("ANTMMF_TEST_DP_MODE", None)
    assert two[0]["world"] == 2 and one["world"] == 1
    assert abs(two[0]["loss"] - two[1]["loss"]) < 1e-6 and abs(two[0]["loss"] - one["loss"]) <= 2e-5 * abs(one["loss"])
    torch.testing.assert_close(two[0]["master"], two[1]["master"], rtol=0, atol=0)      # replicas bit-identical
    tol = dict(rtol=2e-2, atol=2e-3 * float(one["grad"].abs().max())) if mode == "bf16" else dict(rtol=1e-3, atol=1e-5 * float(one["grad"].abs().max()))
    torch.testing.assert_close(two[0]["grad"], one["grad"], **tol)
    if mode == "overlap":
        assert two[0]["nbuckets"] >= 4 and two[0]["overlapped"] >= 1, (two[0]["nbuckets"], two[0]["overlapped"])
    if mode != "bf16":
        # AdamW's first update is lr * g / (|g| + eps): an element whose gradient is ~eps (1e-8) moves by anything in [-lr, lr] depending on the
        # last bit of g, so a handful of such elements may differ between the 2-rank and the 1-rank summation order -- bounded by 2 lr (= 2e-2)
        diff = (two[0]["master"] - one["master"]).abs()
        bad = diff > (1e-5 + 1e-4 * one["master"].abs())
        assert int(bad.sum()) <= max(1, diff.numel() // 100000) and float(diff.max()) <= 2e-2, (int(bad.sum()), float(diff.max()))


@pytest.mark.parametrize("world", [4, pytest.param(8, marks=_SLOW)])
def test_m2_step_many_ranks_equals_single_rank(world):
    """The 4- and 8-rank twins of test_m2_step_two_ranks_equals_single_rank: one pair per rank -- rank offsets row0 = rank * B, the x W
    factor of the embedding gradients, the packed gather / reduce-scatter and the bucketed all-reduce started from inside backward with more than two
    participants -- equal the single-rank step on the whole batch."""
    os.environ["ANTMMF_TEST_DP_MODE"] = "overlap"
    os.environ["ANTMMF_TEST_DP_PAIRS"] = str(world)
    try:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(2) as ex:
            fn = ex.submit(_spawn, _m2_step_case, 29681 + world, world)
            f1 = ex.submit(_spawn, _m2_step_case, 29691 + world, 1)
            many, one = fn.result(), f1.result()[0]
    finally:
        os.environ.pop("ANTMMF_TEST_DP_MODE", None)
        os.environ.pop("ANTMMF_TEST_DP_PAIRS", None)
    assert many[0]["world"] == world and one["world"] == 1
    for r in range(1, world):
        assert abs(many[0]["loss"] - many[r]["loss"]) < 1e-6
        torch.testing.assert_close(many[0]["master"], many[r]["master"], rtol=0, atol=0)      # replicas bit-identical
    assert abs(many[0]["loss"] - one["loss"]) <= 2e-5 * abs(one["loss"])
    torch.testing.assert_close(many[0]["grad"], one["grad"], rtol=1e-3, atol=1e-5 * float(one["grad"].abs().max()))
    assert many[0]["nbuckets"] >= 4 and many[0]["overlapped"] >= 1


@pytest.mark.parametrize("world,outside_gib", [(2, None), (8, 284)])
def test_bench_two_ranks_dry_run(world, outside_gib, tmp_path):
    """(world 8: the driver's full scaling point; outside_gib: the pretend device reports that much memory OUTSIDE torch's pool -- what RCCL's channel buffers are in
    a real N > 1 run -- so that the probe arithmetic of choose_keep_ffn has to turn the kept-activation policy OFF, on every rank alike.)
    VERDICT r3 item 5(ii): `python bench.py --gpus 2` end to end where there are no GPUs -- bench.py's dry-run mode (host, gloo, lane-emulated kernels, a toy M2)
    goes through its own self-launch (torch.distributed.run on 127.0.0.1), the rendezvous, choose_keep_ffn's probe step and the all-reduced decision, the
    trainer's step with the arena all-reduce, the barriers and the max-over-ranks timing, and rank 0 prints ONE JSON line with the contract's keys."""
    import json
    import subprocess

    from test_kernels_emu import _stale

    if _stale():
        subprocess.check_call([os.path.join(ROOT, "tests", "emu", "build_emu.sh")])
    env = dict(os.environ, ANTMMF_BENCH_DRY_RUN="1", ANTMMF_ALLOW_EMULATOR="1", ANTMMF_HIP_LIB=os.path.join(ROOT, "tests", "emu", "build", "libantmmf_emu.so"))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    if outside_gib is not None:
        env["ANTMMF_BENCH_DRY_OUTSIDE_GIB"] = str(outside_gib)
    env["OMP_NUM_THREADS"] = "1"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "1", "--warmup", "0", "--workload", "tiny", "--batch", "2",
                          "--no-cpu-baseline", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=2400)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
                "cpu_baseline"):
        assert key in j, key
    assert j["n_gpus"] == world and j["steps"] == 1 and j["scaling"] == "weak" and j["config"]["ranks_seen"] == world and j["config"]["global_batch"] == 2 * world
    assert "dry run" in j["data"] and "probe" in j["config"]["ffn_activation_policy"]     # N > 1: the policy came from the probe step
    assert j["config"]["ffn_activation_policy"].startswith("recompute" if outside_gib else "kept"), j["config"]["ffn_activation_policy"]
    log = j["config"]["grad_buckets"]                                                       # the step's bucket launch order made it into the line
    assert log and sorted(e["bucket"] for e in log) == list(range(len(log))) and all(e["when"] in ("bwd", "end") for e in log)
    assert j["config"]["loss"] == j["config"]["loss"] and j["value"] > 0
    # --dump-outputs: rank 0's last step as float32 .npy (the loss it returned, its meters, a seeded sample of the updated arena)
    import numpy as np

    dumped = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert {"loss", "meter_itc_loss", "master_weights_sample", "adam_exp_avg_sample"} <= set(dumped), sorted(dumped)
    assert all(v.dtype == np.float32 for v in dumped.values())
    assert abs(float(dumped["loss"]) - j["config"]["loss"]) <= 1e-5 * max(1.0, abs(j["config"]["loss"]))
    assert dumped["master_weights_sample"].shape == dumped["adam_exp_avg_sample"].shape and np.isfinite(dumped["master_weights_sample"]).all()


def test_bench_self_launches_n_ranks(monkeypatch):
    """`python bench.py --gpus N` without a launcher (how the driver may call it): bench.py starts N ranks of itself under
    torch.distributed.run on 127.0.0.1 and returns that job's exit code; it refuses when the node has fewer GPUs."""
    import subprocess

    import bench

    class A:
        gpus = 4

    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 8)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    with pytest.raises(SystemExit) as e:
        bench._self_launch(A())
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and 1024 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    with pytest.raises(SystemExit) as e:
        bench._self_launch(A())
    assert "exposes 1 GPU" in str(e.value.code)


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "prj")), reason="the reference tree is only present in the build container (it never travels to the GPU box)")
def test_every_shipped_reference_config_loads_unchanged():
    """north_star: the build "drops into prj/M2_Encoder and the prj/*_vtp configs unchanged".  Every yml the reference ships under prj/*_vtp/configs (91: base / cnvid / snps3 /
    dmae, their `includes:` chains resolved against the reference's own tree) goes through this build's build_config (antmmf/common/configuration.py:106-139,240-345 there), every
    prj/M2_Encoder/configs/*.json through the VLMo config loader (vlmo/config.py:22-165).  The files are READ where they lie; nothing of them is copied into the repo."""
    import glob

    from antmmf.common.build import build_config

    m2 = os.path.join(PKG, "prj", "M2_Encoder")
    if m2 not in sys.path:
        sys.path.insert(0, m2)
    from vlmo.config import default_config, load_json_config

    ymls = sorted(glob.glob(os.path.join(REF, "prj", "*_vtp", "configs", "**", "*.yml"), recursive=True))
    assert len(ymls) >= 91, len(ymls)
    heads = {}
    for y in ymls:
        cfg = build_config(y)
        # the framework defaults are underneath every file (training_parameters exists even where the yml has none)
        assert cfg.training_parameters.trainer, y
        ma = cfg.get("model_attributes", None)
        univl = ma.get("univl", None) if ma is not None else None
        if univl is None:
            continue
        # the model section resolves to a mapping with the keys the registry model reads; files that name a head inherit / carry the rest through `includes:`
        head = univl.get("training_head_type", None)
        heads[head] = heads.get(head, 0) + 1
        if head == "video_text_retrieval":
            assert univl.get("arch_type", None) in ("univl", "clip"), y
    # the four project trees all ship retrieval configs for this path (base 9, cnvid 7, snps3 7, dmae 9)
    assert heads.get("video_text_retrieval", 0) >= 32, heads
    jsons = sorted(glob.glob(os.path.join(REF, "prj", "M2_Encoder", "configs", "*.json")))
    assert len(jsons) >= 3
    known = set(default_config())
    sizes = {}
    for j in jsons:
        cfg = load_json_config(j)
        sizes[os.path.basename(j)] = (cfg["beit_version"], cfg["encoder_layers"], cfg["encoder_embed_dim"], cfg["beit3_vl_layers"])
        assert cfg["loss_names"]["itc"] in (0, 1) and cfg["image_size"] and cfg["patch_size"]
        # every key of a shipped json is either one this build's defaults know or one of the named off-path keys it carries through untouched (serving: modelscope /
        # model_file; data side: whole_word_masking, visual_mask_size; kernel choice of the reference: flash_attn, precision -- this build computes in bf16 on its own
        # attention kernels whatever they say).  A NEW key in a shipped file fails here instead of being silently ignored.
        import json as _json

        extra = set(_json.load(open(j))) - known
        assert extra <= {"flash_attn", "model_file", "modelscope", "precision", "whole_word_masking", "visual_mask_size"}, (j, extra)
        assert all(k in cfg for k in extra)
    assert sizes["Encoder_0.4B.json"][:3] == ("base", 9, 768) and sizes["Encoder_1B.json"][:3] == ("large", 21, 1024) and sizes["Encoder_10B.json"][:3] == ("huge", 21, 4096), sizes


def test_python_product_path_reads_no_switch_from_the_environment():
    """VERDICT r5 hygiene: the Python side of the product path reads two environment variables and no more -- ANTMMF_HIP_LIB (which build of the ABI to load; bench.py prints
    the answer as config.library) and, to warn that it is ignored, ANTMMF_FFN_FOLD.  Test switches are module attributes (contrastive.FORCE_COLLECTIVES, ...)."""
    import glob

    names = set()
    for f in glob.glob(os.path.join(PKG, "antmmf", "**", "*.py"), recursive=True) + glob.glob(os.path.join(PKG, "prj", "**", "*.py"), recursive=True):
        names |= set(re.findall(r"""environ(?:\.get|\.setdefault|\.pop)?[\[(]\s*["'](ANTMMF_\w+)["']""", open(f).read()))
    assert names == {"ANTMMF_HIP_LIB", "ANTMMF_ALLOW_EMULATOR", "ANTMMF_FFN_FOLD"}, names    # (ALLOW_EMULATOR: the loader refuses the CPU emulator build outside pytest without it)
