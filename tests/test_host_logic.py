"""CPU-only: host-side mirror of the reference interface, C-ABI export surface, sharding."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import distributed, native, sdes
from ditsep_amd.registry import Registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_registry_semantics():
    reg = Registry("Thing")

    @reg.register("a")
    class A:
        pass

    assert reg.get_by_name("a") is A and reg.get_all_names() == ["a"]
    with pytest.raises(ValueError, match="Thing with name 'b' unknown"):
        reg.get_by_name("b")
    with pytest.warns(UserWarning, match="doubly registered"):
        reg.register("a")(A)


def test_registered_names_match_reference():
    # reference src/sdes/predictors.py:39,55,69 and correctors.py:35,58,87,124
    assert set(sdes.PredictorRegistry.get_all_names()) == {"euler_maruyama", "reverse_diffusion", "none"}
    assert set(sdes.CorrectorRegistry.get_all_names()) == {"langevin", "ald", "ald2", "none"}
    # reference src/sdes/sdes.py:182,355,595,701
    assert set(sdes.SDERegistry.get_all_names()) == {"ouve", "mix", "priormix", "sbve"}


def test_ouve_closed_forms_match_reference_tables(golden):
    g = golden("sde_tables")
    sde = sdes.OUVESDE(theta=1.5, sigma_min=0.96, sigma_max=10.0, N=30)
    ts = torch.from_numpy(g["t_30"])
    np.testing.assert_allclose(sde._std(ts).numpy(), g["std_30"], rtol=1e-6)
    np.testing.assert_allclose(sde.sde(torch.zeros(30), ts, torch.zeros(30))[1].numpy(), g["g_30"], rtol=1e-6)
    c = sde.copy()
    c.N = 5
    assert sde.N == 30 and c.theta == sde.theta and sde.T == 1


def test_get_pc_sampler_error_behaviour():
    sde = sdes.OUVESDE(1.5, 0.96, 10.0, N=3)
    y = torch.zeros(1, 1, 64, 2)
    with pytest.raises(ValueError):          # unknown registry name -> ValueError as the reference
        sdes.get_pc_sampler("nope", "ald", sde, object(), y)
    with pytest.raises(NotImplementedError):  # python score functions are not executed (no fallback)
        sdes.get_pc_sampler("reverse_diffusion", "ald", sde, lambda x, t, y: x, y)


def test_shard_bounds_cover_batch():
    for B in (0, 1, 7, 64, 513):
        for world in (1, 2, 3, 8):
            spans = [distributed.shard_bounds(B, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == B
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_library_exports_every_declared_symbol():
    """The C-ABI library loads on a GPU-less host and exports every function
    include/ditsep_hip.h declares (no compute calls here)."""
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    declared = set(re.findall(r"\b(dsn_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 15
    lib = native.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/ditsep_hip.h but not exported"
    assert declared == set(native.EXPORTS)


def test_gemm_kernel_tests_cover_every_instantiation():
    """tests/test_gpu_gemm_kernels.py runs every igemm2 tile (CFGL / CFG lines of igemm2_launch_cfg) and every skinny
    MT (SK lines): an instantiation added to igemm.hip without a test entry fails here."""
    from tests.test_gpu_gemm_kernels import FULL, IGEMM_SRC, LEAN, SKINNY_MT

    src = open(IGEMM_SRC).read()

    def body(fn):
        b = src[src.index(fn):]
        return b[:b.index("\n}\n")]

    cfg = body("hipError_t igemm2_launch_cfg(")
    calls = lambda mac: sorted(tuple(int(x) for x in m.groups())
                               for m in re.finditer(r"\b" + mac + r"\((\d+), (\d+), (\d+), (\d+), (\d+)\)", cfg))
    assert calls("CFGL") == sorted(LEAN)
    assert calls("CFG") == sorted(FULL)
    assert re.findall(r"launch_cfg<\d[^>]*>", cfg) == [
        "launch_cfg<1, 1, 128, 64, 3, 64, 0, 32>", "launch_cfg<1, 0, 128, 64, 3, 64, 0, 32>"]  # the 128 x 64 tile
    sk = body("hipError_t igemm_skinny_launch(")
    assert sorted(int(m) for m in re.findall(r"\bSK\((\d+)\)", sk)) == SKINNY_MT


def _header_struct_fields(hdr, struct):
    body = hdr[hdr.index("typedef struct %s {" % struct):hdr.index("} %s;" % struct)]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*?[\s*]+(\w+)$", r"\1", d.strip()) if i == 0 else d.strip().lstrip("*")
                      for i, d in enumerate(decl.split(","))]
    return names


def test_test_gemm_struct_matches_header():
    """native.DsnTestGemm mirrors struct DsnTestGemm of include/ditsep_hip.h field by field"""
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    assert _header_struct_fields(hdr, "DsnTestGemm") == [f[0] for f in native.DsnTestGemm._fields_]


def test_test_kernel_struct_matches_header():
    """native.DsnTestKernel mirrors struct DsnTestKernel field by field, and TEST_KERNEL_KINDS the DSN_TK_* values"""
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    assert _header_struct_fields(hdr, "DsnTestKernel") == [f[0] for f in native.DsnTestKernel._fields_]
    kinds = dict(re.findall(r"DSN_TK_(\w+) = (\d+)", hdr))
    assert {k.lower(): int(v) for k, v in kinds.items()} == native.TEST_KERNEL_KINDS
    # same layout as the C struct: ints and floats 4 bytes, pointers and int64 8, natural alignment
    assert ctypes.sizeof(native.DsnTestKernel) % 8 == 0


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(native, "_lib", None)
    monkeypatch.setattr(native, "LIB_PATH", "/nonexistent/libditsep_hip.so")
    with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
        native.load_library()


def test_engine_requires_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="needs a ROCm GPU"):
        native.Engine()


def test_product_path_never_imports_oracle():
    """The oracle is test infrastructure: nothing under ditsep_amd/ may import it."""
    pkg = os.path.join(ROOT, "ditsep_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, re.M), f


def test_checkpoint_parameter_names_match_reference_module_order():
    """EMA shadow tensors are matched to names by parameters() order: the classification of state_dict entries into
    parameters and buffers must reproduce the reference modules' own order (fixture captured from the reference's
    DiffusionTransformer / Oobleck / LatentScoreModelNCSNpp by oracle/make_golden.py::gen_state_keys)."""
    import json
    import os

    from ditsep_amd import checkpoint

    keys = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "state_keys.json")))
    assert set(keys) >= {"dit_elu", "dit_snake", "ncsnpp_elu"}
    for tag, v in keys.items():
        assert checkpoint.parameter_names(v["state_dict"], "") == v["parameters"], tag
        assert checkpoint.parameter_names(v["state_dict"], "score_model.") == v["score_model_parameters"], tag
    bufs = [k for k in keys["dit_snake"]["state_dict"] if checkpoint.is_buffer(k)]
    assert len(bufs) == 5 and all(k.startswith("score_model.") for k in bufs)      # 2 layers x 2 betas + inv_freq
    assert not any(checkpoint.is_buffer(k) for k in keys["dit_snake"]["state_dict"] if k.startswith("vae."))


def test_oracle_si_bss_eval_decomposition_identities():
    """The oracle's SI-SDR / SI-SIR / SI-SAR restatement: energies of target, interference and artefact add up
    (1/SDR = 1/SIR + (1 + 1/SIR)/SAR), SI-SDR agrees with the plain si_sdr definition, scale invariance, and a
    perfect scrambled copy is recovered with the permutation."""
    import torch

    from oracle import metrics

    g = torch.Generator().manual_seed(3)
    ref = torch.randn((2, 3, 3000), generator=g)
    est = ref[:, [2, 0, 1]] + 0.4 * torch.randn((2, 3, 3000), generator=g) + 0.3 * ref[:, [0, 1, 2]]
    sdr, sir, sar, perm = metrics.si_bss_eval(ref, est, perm_by="sdr")
    inv = lambda x: 10 ** (-x / 10)
    assert float((inv(sdr) - (inv(sir) + inv(sar) * (1 + inv(sir)))).abs().max()) < 1e-9
    best, p2 = metrics.si_sdr_pit(ref, est)
    assert torch.equal(perm, p2) and float((sdr.mean(-1) - best).abs().max()) < 1e-9
    s2 = metrics.si_bss_eval(ref, 7.5 * est, perm_by="sdr")
    assert all(float((a - b).abs().max()) < 1e-6 for a, b in zip(s2[:3], (sdr, sir, sar)))
    _, _, _, p3 = metrics.si_bss_eval(ref, ref[:, [1, 2, 0]])
    assert torch.equal(p3, torch.tensor([[2, 0, 1]] * 2))


def test_score_model_config_targets_resolve_and_refuse_unbound_calls():
    """INTEGRATION.md names `ditsep_amd.score_models.DiTScoreModel` as the `_target_`: it must import, take the
    documented keywords (what hydra.utils.instantiate would call) and never compute without an engine."""
    import importlib

    import pytest

    mod = importlib.import_module("ditsep_amd.score_models")
    m = mod.DiTScoreModel(embed_dim=1024, depth=24, num_heads=16)
    assert m.kwargs == {"embed_dim": 1024, "depth": 24, "num_heads": 16}
    with pytest.raises(RuntimeError):
        m(None, None, None)
    with pytest.raises(ValueError):
        mod.DiTScoreModel(embed_dim=1024, depth=2, num_heads=8)        # 128-wide heads: not implemented
    n = mod.LatentScoreModelNCSNpp(num_sources=2, backbone_args={"nf": 128}, max_latent_length=16)
    assert n.kwargs["backbone_args"] == {"nf": 128}
