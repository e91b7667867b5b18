"""The plan of a DiT score call (ditsep_amd/csrc/dit_plan.h) through dsn_dit_plan: no GPU, no context.

dit_plan decides, from (configuration, precision, B, T) and the DSN_* switches alone, which kernel family and which
launch geometry every layer GEMM of dsn_ctx::dit_forward gets.  Checked here: over a grid, that every plan stays inside
what the launchers accept (igemm_panel_launch, igemm_panel_fp8_launch, igemm_skinny_launch, qkv_attention_launch, the
eight slabs of "dit_slabs"); the anchor plans worked out by hand from the rules; and a recorded table,
tests/golden/dit_plan.json, so that a change of any decision shows up as a diff of that table.

One property reads differently from a plain "qa_ipp <= B": DSN_QA_IPP takes the forced value as it is, also where the
batch has fewer items than a panel (tests/test_gpu_headline.py forces 16 items per panel on a batch of 7; the launcher
asks for ipp * S <= 240 only).  So qa_ipp <= B is asserted for every plan the rule itself makes, and a forced plan must
carry exactly the forced value."""
import ctypes as C
import itertools
import json
import os

import pytest

from ditsep_amd import native
from tests.test_host_logic import ROOT, _header_struct_fields

GOLDEN = os.path.join(ROOT, "tests", "golden")

BF16, BF16X3, FP16, FP16X3, FP8 = 1, 2, 3, 4, 5
PRECISIONS = {"bf16": BF16, "bf16x3": BF16X3, "fp16": FP16, "fp16x3": FP16X3, "fp8": FP8}
SWITCHES = ("DSN_SKINNY_MAX", "DSN_QA_IPP", "DSN_NO_LN_FOLD")
ENVS = [{}, {"DSN_SKINNY_MAX": "0"}, {"DSN_SKINNY_MAX": "128"}, {"DSN_QA_IPP": "1"}, {"DSN_QA_IPP": "2"},
        {"DSN_NO_LN_FOLD": "1"}]
FIELDS = [f[0] for f in native.DsnDitPlan._fields_]
# what the launchers take (igemm.h, kernels.h, qkv_attn.hip)
PANEL_ROWS, FP8_ROWS, FOLD_ROWS, QA_ROWS, SLABS = 272, 208, 80, 240, 8


def plan(prec, D, B, T, n_src=2, latent=64):
    cfg = native.DsnConfig()
    cfg.precision, cfg.n_src, cfg.latent_dim, cfg.score_kind = prec, n_src, latent, native.SCORE_DIT
    cfg.dit_embed_dim, cfg.dit_depth, cfg.dit_heads = D, 2, D // 64
    out = native.DsnDitPlan()
    assert native.load_library().dsn_dit_plan(C.byref(cfg), B, T, C.byref(out)) == 0
    return {k: getattr(out, k) for k in FIELDS}


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def test_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    assert _header_struct_fields(hdr, "DsnDitPlan") == FIELDS


def test_bad_arguments_are_refused():
    lib = native.load_library()
    cfg, out = native.DsnConfig(), native.DsnDitPlan()
    cfg.precision, cfg.dit_embed_dim, cfg.dit_heads = FP16, 256, 4
    assert lib.dsn_dit_plan(None, 1, 8, C.byref(out)) != 0
    assert lib.dsn_dit_plan(C.byref(cfg), 0, 8, C.byref(out)) != 0
    assert lib.dsn_dit_plan(C.byref(cfg), 1, 0, C.byref(out)) != 0
    assert lib.dsn_dit_plan(C.byref(cfg), 1, 8, None) != 0


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join(f"{k[4:]}={v}" for k, v in e.items()) or "default")
@pytest.mark.parametrize("pname", list(PRECISIONS))
def test_every_plan_is_one_the_launchers_accept(pname, env, monkeypatch):
    set_env(monkeypatch, env)
    prec = PRECISIONS[pname]
    single, fp8 = prec in (BF16, FP16, FP8), prec == FP8
    skinny_max = min(int(env.get("DSN_SKINNY_MAX", 80)), 128)
    forced = int(env.get("DSN_QA_IPP", 0))
    for D, B, T, n_src in itertools.product((256, 1024), (1, 2, 3, 8, 16, 64, 256), (1, 8, 16, 32, 40, 100, 235, 239),
                                            (2, 3)):
        p = plan(prec, D, B, T, n_src=n_src)
        what = f"{pname} D={D} B={B} T={T} n_src={n_src} {env}: {p}"
        S, M = T + 1, B * (T + 1)
        assert (p["S"], p["M"]) == (S, M), what
        if p["skinny"]:
            assert M <= skinny_max and single and not fp8 and D % 256 == 0, what
            assert p["fold_rows"] == 0 and p["qa_ipp"] == 0, what
            assert p["attn_out_ksplit"] == p["ff_out_ksplit"] == 8 <= D // 32, what
        if p["fold_rows"] > 0:
            assert p["fold_rows"] <= FOLD_ROWS and p["attn_out_ksplit"] == 1 and p["attn_out_rows"] == 0, what
            assert single and D % (128 if fp8 else 64) == 0 and "DSN_NO_LN_FOLD" not in env, what
        if p["qa_ipp"] > 0:
            assert p["qa_ipp"] * S <= QA_ROWS and p["qkv_rows"] == 0 and single, what
            if forced and forced * S <= QA_ROWS:
                assert p["qa_ipp"] == forced, what       # (taken as it is, see the module docstring)
            else:
                assert p["qa_ipp"] <= B, what
        for k in ("qkv_rows", "attn_out_rows", "ff_in_rows", "ff_out_rows", "project_out_rows"):
            assert p[k] == 0 or (p[k] % 8 == 0 and 8 <= p[k] <= PANEL_ROWS), (k, what)
        if fp8:
            assert p["qkv_rows"] <= FP8_ROWS and p["ff_out_rows"] <= FP8_ROWS, what
            # the fp8 launcher runs row panels only
            assert p["ff_in_rows"] > 0 and p["ff_out_rows"] > 0 and (p["qkv_rows"] > 0 or p["qa_ipp"] > 0), what
            assert p["fold_rows"] > 0 or p["attn_out_rows"] > 0, what
        assert 1 <= p["attn_out_ksplit"] <= SLABS and 1 <= p["ff_out_ksplit"] <= SLABS, what
        assert p["attn_out_ksplit"] <= D // 32 and p["ff_out_ksplit"] <= 4 * D // 32, what
        assert p["project_out_rows"] == (64 if single and n_src * 64 <= 128 and B * T >= 1024 else 0), what


# The plans of D = 1024, 16 heads, n_src 2, latent 64 worked out by hand from the rules; only the named fields
ANCHORS = [
    ("fp16", {}, 64, 32, dict(M=2112, skinny=0, fold_rows=66, qa_ipp=4, ff_in_rows=264, ff_out_ksplit=4, ff_out_rows=136,
                              project_out_rows=64)),
    ("fp16", {"DSN_NO_LN_FOLD": "1"}, 64, 32, dict(fold_rows=0, attn_out_ksplit=2, attn_out_rows=136)),
    ("fp16", {}, 64, 40, dict(fold_rows=41, qa_ipp=3, ff_in_rows=168, ff_out_rows=168)),
    ("fp16", {}, 3, 32, dict(M=99, skinny=0, fold_rows=4, qa_ipp=0, qkv_rows=8, ff_in_rows=16, ff_out_ksplit=4,
                             ff_out_rows=8)),
    ("fp16", {}, 1, 16, dict(skinny=1, attn_out_ksplit=8, ff_out_ksplit=8)),
    ("fp16", {}, 1, 235, dict(qa_ipp=0, qkv_rows=16, fold_rows=8)),
    ("fp16x3", {}, 64, 32, dict(fold_rows=0, qa_ipp=0, qkv_rows=0, attn_out_rows=0, ff_out_rows=0, attn_out_ksplit=3,
                                ff_out_ksplit=3, ff_in_rows=264)),
    ("fp16x3", {}, 256, 32, dict(attn_out_ksplit=1, ff_out_ksplit=1)),
    ("fp8", {}, 256, 32, dict(ff_out_rows=176)),
    ("fp16", {}, 256, 32, dict(ff_out_rows=264)),
]


@pytest.mark.parametrize("pname,env,B,T,want", ANCHORS)
def test_anchor_plans(pname, env, B, T, want, monkeypatch):
    set_env(monkeypatch, env)
    p = plan(PRECISIONS[pname], 1024, B, T)
    assert {k: p[k] for k in want} == want, p


def test_recorded_plans(monkeypatch):
    """tests/golden/dit_plan.json: plans recorded from this function when it was taken out of dit_forward unchanged"""
    rows = json.load(open(os.path.join(GOLDEN, "dit_plan.json")))
    assert len(rows) >= 40
    for r in rows:
        set_env(monkeypatch, r["env"])
        assert plan(PRECISIONS[r["precision"]], r["D"], r["B"], r["T"], n_src=r["n_src"]) == r["plan"], r
