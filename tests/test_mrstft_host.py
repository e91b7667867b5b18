"""CPU-only: the float64 restatement of the MR-STFT / L1 / L2 pair tables (tests/mrstft_restatement.py) against the
reference's own float64 values (tests/golden/mrstft.npz, scripts/make_golden_mrstft.py), the A-weighting design of
ditsep_amd/aweight.py against the reference's taps, the host-side combine, the config reading of LDM and every
refusal."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import aweight, latent, native
from tests import mrstft_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mrstft.npz")
# both sides are float64 with the same formulas on the same float32 inputs, taps and window: only the rounding of the
# FFT differs (measured 5.4e-15 at most)
TOL_F64 = 1e-9
# max |aweight.taps(fs) - reference taps| measured: 2.9e-11 (8 kHz), 2.4e-10 (16 kHz).  Both are float32 roundings
# of float64 designs that agree to 7.6e-12 (the 51 x 51 normal equations are solved by LU here, by Cholesky in scipy);
# a differing float32 rounding of the largest tap (0.85) would show as 6e-8.  Bound: 4x the measured maximum.
MEASURED_TAPS = 2.4e-10
TOL_TAPS = 4 * MEASURED_TAPS


@functools.lru_cache(maxsize=None)
def case(name):
    g = np.load(GOLDEN)
    fs, B, n, L, _ = R.CASES[name]
    reals, decoded = R.make_case(name)
    assert np.array_equal(reals, g[f"{name}_reals"]) and np.array_equal(decoded, g[f"{name}_decoded"])  # generator drift
    assert reals.shape == (B, n, L) and reals.dtype == np.float32
    return g, fs, n, R.pair_tables(reals, decoded, taps=g[f"{name}_taps"])


def rel(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) / np.asarray(want, dtype=np.float64) - 1.0).max())


def test_fixture_is_small_and_records_the_reference_error():
    assert os.path.getsize(GOLDEN) < 600_000
    g = np.load(GOLDEN)
    for name in R.CASES:
        own = rel(g[f"{name}_perm_values_f32"], g[f"{name}_perm_values_f64"])
        assert 5e-8 < own < 5e-7, own                     # the reference's own float32 error: 1.2e-7 and 2.7e-7


@pytest.mark.parametrize("name", ["fs8k", "fs16k"])
def test_restatement_matches_reference_float64(name):
    g, fs, n, tab = case(name)
    perms = [tuple(p) for p in g[f"{name}_perms"].tolist()]
    vals = np.array([R.spectral_item_values(tab, p).mean() for p in perms])
    errs = {"perm_values": rel(vals, g[f"{name}_perm_values_f64"])}
    assert len(perms) == {2: 2, 3: 6}[n] and int(np.argmin(vals)) != 0          # the identity is not the best order
    errs["sc"] = rel(np.stack([tab["sc"][:, :, i, i] for i in range(n)], -1), g[f"{name}_sc_f64"])
    errs["log_mag"] = rel(np.stack([tab["log_mag"][:, :, i, i] for i in range(n)], -1).mean((1, 2)),
                          g[f"{name}_log_mag_f64"])
    obj = R.objective(tab, n, l1_weight=15.0, l2_weight=1.0)
    for key in ("mrstft", "l1", "l2"):
        errs["pit_" + key] = rel(obj[f"pit_{key}_loss"], float(g[f"{name}_pit_{key}_f64"]))
    print(name, errs)
    assert max(errs.values()) <= TOL_F64, errs


@pytest.mark.parametrize("name", ["fs8k", "fs16k"])
@pytest.mark.parametrize("mode", ["batch", "item", None])
def test_host_combine_matches_restatement(name, mode):
    g, fs, n, tab = case(name)
    kw = dict(w_lin_mag=0.5, mrstft_weight=2.0, l1_weight=15.0, l2_weight=0.25)
    want = R.objective(tab, n, mode=mode, **kw)
    got = native.mrstft_combine(tab, pit=mode, **kw)
    for key in ("pit_mrstft", "pit_l1", "pit_l2"):
        assert abs(float(got[key + "_loss"]) - want[key + "_loss"]) <= 1e-14 * abs(want[key + "_loss"])
        assert np.array_equal(got[key + "_perm"].numpy(), want[key + "_perm"])
    assert np.abs(got["mrstft_values"].numpy() - want["mrstft_values"]).max() < 1e-13
    assert abs(float(got["loss"]) - want["loss"]) < 1e-13
    assert float(got["loss"]) == float(got["pit_mrstft_loss"] + got["pit_l1_loss"] + got["pit_l2_loss"])
    if mode == "batch":                                  # the reference's PITLoss: one permutation for the batch
        assert (got["pit_mrstft_perm"] == got["pit_mrstft_perm"][0]).all()
        if name == "fs16k":                              # chosen per term: the MSE term prefers another order here
            assert got["pit_l2_perm"][0].tolist() != got["pit_l1_perm"][0].tolist()


def test_combine_terms_and_single_source():
    g, fs, n, tab = case("fs8k")
    plain = native.mrstft_combine(tab)
    assert "pit_l1_loss" not in plain and "pit_l2_loss" not in plain and float(plain["loss"]) == float(plain["pit_mrstft_loss"])
    assert "pit_l1_loss" not in native.mrstft_combine(tab, l1_weight=0.0, l2_weight=1.0)
    one = {k: v[..., :1, :1] for k, v in tab.items()}
    got = native.mrstft_combine(one, l1_weight=3.0)
    assert got["perms"] == [(0,)] and got["pit_mrstft_perm"].tolist() == [[0], [0]]
    want = (one["sc"] + one["log_mag"]).mean()
    assert abs(float(got["pit_mrstft_loss"]) - want) < 1e-15 and abs(float(got["pit_l1_loss"]) - 3.0 * one["l1"].mean()) < 1e-15
    assert R.objective(one, 1, l1_weight=3.0)["loss"] == pytest.approx(float(got["loss"]), rel=1e-14)
    with pytest.raises(ValueError, match="pit"):
        native.mrstft_combine(tab, pit="best")
    off = native.mrstft_combine(tab, w_sc=0.0, w_log_mag=0.0)
    assert float(off["loss"]) == 0.0


def test_restatement_geometry():
    x = np.arange(1025, dtype=np.float64)[None]
    m = R.magnitudes(x, 2048, 512, 2048)
    assert m.shape == (1, 3, 1025)
    with pytest.raises(ValueError):
        R.magnitudes(x[:, :1024], 2048, 512, 2048)
    assert R.magnitudes(np.ones((1, 4001)), 64, 16, 64).shape == (1, 251, 33)
    w = R.padded_window(1024, 600)
    assert w[:212].sum() == 0 and w[812:].sum() == 0 and w[212] == 0 and w[212 + 300] == 1.0
    tw = torch.stft(torch.ones(1, 4001), 64, 16, 64, torch.hann_window(64), return_complex=True)
    assert tw.shape == (1, 33, 251)
    sig = np.random.default_rng(0).standard_normal((1, 3000)).astype(np.float32)
    want = torch.stft(torch.from_numpy(sig).double(), 1024, 256, 600, torch.hann_window(600).double(), return_complex=True).abs()
    assert np.abs(R.magnitudes(sig, 1024, 256, 600)[0].T - want[0].numpy()).max() < 1e-10
    taps = np.arange(1.0, 6.0)
    want = torch.nn.functional.conv1d(torch.from_numpy(sig).double()[None], torch.from_numpy(taps)[None, None], padding=2)
    assert np.abs(R.prefilter(sig, taps) - want[0].numpy()).max() < 1e-12


@pytest.mark.parametrize("name", ["fs8k", "fs16k"])
def test_aweighting_taps_match_reference(name):
    g = np.load(GOLDEN)
    fs = R.CASES[name][0]
    ref = g[f"{name}_taps"]
    got = aweight.taps(fs)
    assert got.dtype == np.float32 and got.shape == ref.shape == (101,) and not got.flags.writeable
    assert aweight.taps(fs) is got                                           # cached per fs
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"{name}: max |taps - reference taps| = {err:.3e} (bound {TOL_TAPS:.1e}); largest tap {np.abs(ref).max():.3f}")
    assert err <= TOL_TAPS
    assert np.array_equal(got, got[::-1])                                    # linear phase
    with pytest.raises(ValueError, match="odd"):
        aweight.least_squares_fir(100, [0, 1], [1, 1], 2.0)


@pytest.mark.parametrize("fs", [8000, 16000, 44100])
def test_aweighting_design_matches_scipy(fs):
    sig = pytest.importorskip("scipy.signal")
    num, den = aweight.analog_prototype()
    b, a = sig.bilinear(num, den, fs=fs)
    b2, a2 = aweight.bilinear(num, den, fs)
    assert np.abs(b - b2).max() < 1e-13 and np.abs(a - a2).max() < 1e-13
    w, h = sig.freqz(b, a, worN=512, fs=fs)
    w2, m2 = aweight.magnitude_response(b2, a2, fs)
    # the numerator has a quadruple zero at z = 1: near DC its evaluation cancels coefficients of size 1e7 * b[0], and
    # the two evaluation orders differ by that rounding (measured 1.8e-9 at DC, 1e-16 in the pass band)
    assert np.abs(w - w2).max() < 1e-9 and np.abs(np.abs(h) - m2).max() < 1e-8
    want = sig.firls(101, w, abs(h), fs=fs)
    err = float(np.abs(aweight.design(fs) - want).max())
    print(f"fs {fs}: max |design - scipy firls| in float64 = {err:.3e}")      # measured 7.6e-12 at most
    assert err < 4 * 7.6e-12
    assert np.abs(aweight.taps(fs) - want.astype(np.float32)).max() <= TOL_TAPS


def _ldm_config(**spectral):
    cfg = {"sample_rate": 16000, "fft_sizes": [2048, 1024, 512, 256, 128, 64, 32],
           "hop_sizes": [512, 256, 128, 64, 32, 16, 8], "win_lengths": [2048, 1024, 512, 256, 128, 64, 32],
           "_target_": "stable_audio_tools.training.losses.auraloss.MultiResolutionSTFTLoss",
           "perceptual_weighting": True}
    cfg.update(spectral)
    return {"training": {"loss": {"spectral": {"type": "mrstft", "decay": 1.0, "weights": {"mrstft": 1.0}, "config": cfg},
                                  "time": {"type": "l1", "weights": {"l1": 15.0}}}}}


def test_ldm_config_parsing():
    kw = latent.reconstruction_loss_config(_ldm_config())                    # src/config/ldm/training/default.yaml
    assert kw == dict(fs=16000, fft_sizes=R.FFT_SIZES, hop_sizes=R.HOP_SIZES, win_lengths=R.FFT_SIZES,
                      perceptual_weighting=True, w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, mrstft_weight=1.0,
                      l1_weight=15.0, l2_weight=0.0)
    cfg = _ldm_config(w_lin_mag=0.5, perceptual_weighting=False)
    cfg["training"]["loss"]["spectral"]["weights"]["mrstft"] = 2.0
    cfg["training"]["loss"]["time"]["weights"] = {"l2": 3.0}
    kw = latent.reconstruction_loss_config(cfg)
    assert (kw["w_lin_mag"], kw["mrstft_weight"], kw["l1_weight"], kw["l2_weight"]) == (0.5, 2.0, 0.0, 3.0)
    bare = {"training": {"loss": {"spectral": {"decay": 1.0, "weights": {"mrstft": 1.0}, "config": {}},
                                  "time": {"weights": {}}}}}
    kw = latent.reconstruction_loss_config(bare)                             # auraloss.py's constructor defaults
    assert kw["fft_sizes"] == (1024, 2048, 512) and kw["win_lengths"] == (600, 1200, 240) and not kw["perceptual_weighting"]
    from ditsep_amd import LDM
    assert issubclass(LDM, latent.LatentDiffSep) and LDM is latent.LDM


def test_ldm_config_refusals():
    with pytest.raises(ValueError, match="training.loss.spectral"):
        latent.reconstruction_loss_config({"model": {}})
    cfg = _ldm_config()
    cfg["training"]["discriminator"] = {"_target_": "EncodecDiscriminator"}
    latent.reconstruction_loss_config(cfg)                                   # the reference needs both sections (:92)
    cfg["training"]["loss"]["discriminator"] = {"weights": {"adversarial": 0.1}}
    with pytest.raises(NotImplementedError, match="discriminator"):
        latent.reconstruction_loss_config(cfg)
    with pytest.raises(NotImplementedError, match="_target_"):
        latent.reconstruction_loss_config(_ldm_config(_target_="auraloss.MelSTFTLoss"))
    cfg = _ldm_config()
    cfg["training"]["loss"]["spectral"]["decay"] = 0.99
    with pytest.raises(NotImplementedError, match="decay"):
        latent.reconstruction_loss_config(cfg)
    with pytest.raises(ValueError, match="sample_rate"):
        latent.reconstruction_loss_config(_ldm_config(sample_rate=None))
    with pytest.raises(NotImplementedError):
        latent.LDM(_ldm_config(scale="mel", n_bins=[64] * 7))                # refused before any engine is built


@pytest.mark.parametrize("kw,match", [({"scale": "mel"}, "scale"), ({"scale": "chroma"}, "scale"), ({"w_phs": 1.0}, "phase"),
                                      ({"scale_invariance": True}, "scale_invariance"),
                                      ({"window": "hamming_window"}, "window"), ({"decay": 0.5}, "decay"),
                                      ({"mag_distance": "L2"}, "mag_distance")])
def test_unsupported_options_raise(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        native.mrstft_unsupported(**kw)
    native.mrstft_unsupported(window="hann_window", w_phs=0.0, scale=None, scale_invariance=False, decay=1.0)


def test_default_evaluate_records_unchanged(monkeypatch):
    """evaluate_batches without mrstft=True calls nothing new and writes the fields it wrote before."""
    from ditsep_amd import evaluate

    calls = []

    class Eng:
        device = torch.device("cpu")

        def si_bss_eval(self, target, est, perm_by, clamp_db):
            B, n = target.shape[:2]
            z = torch.zeros(B, n)
            return z, z + 1, z + 2, torch.arange(n).flip(0).expand(B, n)

        def mrstft_loss(self, reals, decoded, fs, pit):
            calls.append((fs, pit))
            B, n = reals.shape[:2]
            t = torch.arange(B * n * n, dtype=torch.float64).reshape(B, n, n)
            return {"sc": torch.stack([t, t + 2]), "log_mag": torch.stack([t, t]), "l1": 10 * t}

    class Model:
        engine, config, sde = Eng(), {"model": {"sampler": {"N": 2}}}, type("Sde", (), {"N": 2})

        def encode(self, mix, target, seed):
            return mix, None

        def get_pc_sampler(self, *a, **k):
            return lambda: (torch.zeros(2, 2, 8), 4)

        def decode(self, x, L):
            return x

    batches = [(torch.zeros(2, 1, 8), torch.zeros(2, 2, 8))]
    keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    plain = evaluate.evaluate_batches(Model(), batches, fs=8000)
    assert not calls and all(list(r) == keys for r in plain.values())
    assert "mrstft_impl" not in _summary(evaluate, plain)
    res = evaluate.evaluate_batches(Model(), batches, fs=8000, mrstft=True)
    assert calls == [(8000, None)] and all(list(r) == keys + ["mrstft", "l1"] for r in res.values())
    # source i is scored against estimate perm[i] = 1 - i: entries [b, 0, 1] and [b, 1, 0] of mean_r (sc + log_mag)
    assert res[0]["mrstft"] == [2 * 1 + 1.0, 2 * 2 + 1.0] and res[1]["l1"] == [50.0, 60.0]
    assert "mrstft_impl" in _summary(evaluate, res)


def _summary(evaluate, results):
    import json
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        evaluate.write_results(os.path.join(d, "r.json"), results)
        return json.load(open(os.path.join(d, "r_summary.json")))


def test_dsn_mrstft_loss_binding_matches_header():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    m = re.search(r"\bint\s+dsn_mrstft_loss\s*\(([^)]*)\)\s*;", hdr)
    assert m, "dsn_mrstft_loss is not declared in include/ditsep_hip.h"
    names = [re.findall(r"\w+", p)[-1] for p in m.group(1).split(",")]
    assert names == ["ctx", "reals", "decoded", "B", "n", "L", "cfg", "out", "stream"]
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib = native.load_library()
    assert list(lib.dsn_mrstft_loss.argtypes) == [vp, vp, vp, ci, ci, ci, ctypes.POINTER(native.DsnMrstftConfig),
                                                  ctypes.POINTER(native.DsnMrstftOut), vp]
    s = re.search(r"typedef\s+struct\s+DsnMrstftOut\s*\{(.*?)\}\s*DsnMrstftOut\s*;", hdr, re.S)
    assert re.findall(r"\*\s*(\w+)", s.group(1)) == [f[0] for f in native.DsnMrstftOut._fields_]
    s = re.search(r"typedef\s+struct\s+DsnMrstftConfig\s*\{(.*?)\}\s*DsnMrstftConfig\s*;", hdr, re.S)
    body = re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S)
    fields = [nm for decl in body.split(";") for nm in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert fields == [f[0] for f in native.DsnMrstftConfig._fields_]
    assert "dsn_mrstft_loss" in native.EXPORTS
