"""dsn_mrstft_loss (ditsep_amd/csrc/mrstft.hip) through Engine.mrstft_loss, LDM.losses_gen and evaluate_batches, against
the reference's own float64 values (tests/golden/mrstft.npz, scripts/make_golden_mrstft.py) and the float64 restatement
(tests/mrstft_restatement.py).

Parity bound of the two fixture cases: the device's relative distance from the reference's float64 record may not
exceed 8x the reference's own float32-to-float64 distance stored in the fixture (8.1e-8 for fs8k, 2.70e-7 for fs16k),
with a floor of 1e-6 -- bounds 1.0e-6 and 2.16e-6.  The margin covers another FFT factorisation and log implementation.
Measured device distance: none recorded yet for the fp64 transform (MEASURED below is empty); its fp32 predecessor
passed both cases on an MI355X."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import mrstft_restatement as R
from tests.util import make_engine

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mrstft.npz")
# largest relative distance of any compared quantity from the reference's float64 record, measured on an MI355X
MEASURED = {"fs8k": None, "fs16k": None}
# The other cases compare with the float64 restatement, which forms the same sums from the same float32 inputs, float32
# taps and float32 window.  The bound is the parity cases' floor, 1e-6.  A float32 workspace for the filtered signal and
# a float32 FFT do not meet it on one resolution with few frames (log_mag 1.6e-6 at fft 2048 on 3000 samples,
# measured): the A-weighted spectra span 80 dB and the log term weighs every bin alike.  The device therefore keeps
# the filtered signal, the frames and the transforms in fp64, and its distance is that of two fp64 FFT orders.
TOL_RESTATEMENT = 1e-6


@pytest.fixture(scope="module")
def eng():
    e = make_engine(precision=2)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(GOLDEN)


def rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got / want - 1.0).max())


@functools.lru_cache(maxsize=None)
def signals(fs, B, n, L, seed):
    return R.make_signals(fs, B, n, L, seed)


def check_tables(tag, got, want, tol=TOL_RESTATEMENT, keys=("sc", "log_mag", "lin_mag", "l1", "l2")):
    bad = []
    for k in keys:
        if want[k].size == 0 or not np.any(want[k]):
            assert not np.any(got[k].numpy()), k
            continue
        err = rel(got[k].numpy(), want[k])
        print(f"{tag}: {k} max relative |device / restatement - 1| = {err:.3e} (bound {tol:.1e})")
        if not err <= tol:
            bad.append((k, err))
    assert not bad, bad


@pytest.mark.parametrize("name", ["fs8k", "fs16k"])
def test_parity_with_reference_float64(eng, name):
    g = golden()
    fs, B, n, L, _ = R.CASES[name]
    reals, decoded = g[f"{name}_reals"], g[f"{name}_decoded"]
    own = float(np.abs(g[f"{name}_perm_values_f32"] / g[f"{name}_perm_values_f64"] - 1.0).max())
    tol = max(8.0 * own, 1e-6)
    res = eng.mrstft_loss(torch.from_numpy(reals), torch.from_numpy(decoded), fs, l1_weight=15.0, l2_weight=1.0)
    perms = [tuple(p) for p in g[f"{name}_perms"].tolist()]
    assert res["perms"] == perms
    errs = {}
    # per-resolution terms of the identity permutation (output="full"): sc per (b, channel), log_mag per resolution
    diag = np.stack([res["sc"][:, :, i, i].numpy() for i in range(n)], -1)
    errs["sc"] = rel(diag, g[f"{name}_sc_f64"])
    lg = np.stack([res["log_mag"][:, :, i, i].numpy() for i in range(n)], -1).mean((1, 2))
    errs["log_mag"] = rel(lg, g[f"{name}_log_mag_f64"])
    errs["perm_values"] = rel(res["mrstft_values"].numpy(), g[f"{name}_perm_values_f64"])
    for key in ("mrstft", "l1", "l2"):
        errs["pit_" + key] = rel(float(res[f"pit_{key}_loss"]), float(g[f"{name}_pit_{key}_f64"]))
    errs["loss"] = rel(float(res["loss"]), sum(float(g[f"{name}_pit_{k}_f64"]) for k in ("mrstft", "l1", "l2")))
    for k, v in errs.items():
        print(f"{name}: {k} relative distance from the reference's float64 = {v:.3e} (bound {tol:.3e}; the "
              f"reference's own float32 is {own:.3e} away)")
    # the chosen permutations: the restatement's, and the minimum of the reference's recorded values
    want = R.objective(R.pair_tables(reals, decoded, taps=g[f"{name}_taps"]), n, l1_weight=15.0, l2_weight=1.0)
    for key in ("mrstft", "l1", "l2"):
        assert np.array_equal(res[f"pit_{key}_perm"].numpy(), want[f"pit_{key}_perm"]), key
    assert res["pit_mrstft_perm"][0].tolist() == list(perms[int(np.argmin(g[f"{name}_perm_values_f64"]))])
    assert res["pit_mrstft_perm"][0].tolist() != list(range(n)), "the case must need a permutation"
    assert max(errs.values()) <= tol, errs


@functools.lru_cache(maxsize=None)
def small_tables(fft, hop, win, L, weighted, B=2, n=2):
    reals, decoded = signals(8000, B, n, L, 40 + n)
    taps = None
    if weighted:
        from ditsep_amd import aweight
        taps = aweight.taps(8000)
    return reals, decoded, R.pair_tables(reals, decoded, (fft,), (hop,), (win,), taps=taps)


@pytest.mark.parametrize("fft", [2048, 1024, 512, 256, 128, 64, 32])
def test_each_fft_size_alone(eng, fft):
    reals, decoded, want = small_tables(fft, fft // 4, fft, 3000, True)
    got = eng.mrstft_loss(reals_t(reals), reals_t(decoded), 8000, fft_sizes=(fft,), hop_sizes=(fft // 4,), w_lin_mag=1.0)
    assert got["sc"].shape == (1, 2, 2, 2)
    check_tables(f"fft{fft}", got, want)


def reals_t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("fft,hop,win,L,weighted", [
    (2048, 512, 2048, 1025, True),      # the shortest legal length: reflect padding spans nearly the whole signal
    (512, 128, 512, 4001, True),        # not a multiple of any hop
    (64, 24, 64, 4001, False),          # a hop that is no power of two, no prefilter
    (1024, 256, 600, 3000, True),       # win_length < fft
    (2048, 500, 1200, 2500, False),
])
def test_geometry_cases(eng, fft, hop, win, L, weighted):
    reals, decoded, want = small_tables(fft, hop, win, L, weighted)
    got = eng.mrstft_loss(reals_t(reals), reals_t(decoded), 8000, fft_sizes=(fft,), hop_sizes=(hop,), win_lengths=(win,),
                          perceptual_weighting=weighted, w_lin_mag=1.0)
    check_tables(f"fft{fft} hop{hop} win{win} L{L}", got, want)


@pytest.mark.parametrize("B,n", [(1, 2), (3, 2), (1, 1), (2, 4)])
def test_batch_and_source_counts(eng, B, n):
    reals, decoded = signals(8000, B, n, 2100, 60 + 4 * B + n)
    from ditsep_amd import aweight
    ffts, hops = (1024, 128, 32), (256, 32, 8)
    want = R.pair_tables(reals, decoded, ffts, hops, taps=aweight.taps(8000))
    got = eng.mrstft_loss(reals_t(reals), reals_t(decoded), 8000, fft_sizes=ffts, hop_sizes=hops, l1_weight=2.0)
    check_tables(f"B{B} n{n}", got, want, keys=("sc", "log_mag", "l1", "l2"))
    assert not np.any(got["lin_mag"].numpy())                    # w_lin_mag = 0: the reference skips the term
    obj = R.objective(want, n, l1_weight=2.0)
    assert rel(float(got["loss"]), obj["loss"]) <= TOL_RESTATEMENT
    assert np.array_equal(got["pit_mrstft_perm"].numpy(), obj["pit_mrstft_perm"])
    if n == 1:
        assert got["perms"] == [(0,)] and got["pit_l1_perm"].tolist() == [[0]]


@pytest.mark.parametrize("mode", ["item", None, "batch"])
def test_pit_modes(eng, mode):
    reals, decoded = signals(8000, 3, 3, 2100, 77)               # the items' estimates are rolled differently: per-item optima differ
    ffts, hops = (512, 64), (128, 16)
    want = R.pair_tables(reals, decoded, ffts, hops)
    obj = R.objective(want, 3, l1_weight=15.0, l2_weight=0.5, mode=mode)
    got = eng.mrstft_loss(reals_t(reals), reals_t(decoded), 8000, fft_sizes=ffts, hop_sizes=hops,
                          perceptual_weighting=False, l1_weight=15.0, l2_weight=0.5, pit=mode)
    for key in ("pit_mrstft", "pit_l1", "pit_l2"):
        assert rel(float(got[key + "_loss"]), obj[key + "_loss"]) <= TOL_RESTATEMENT, key
        assert np.array_equal(got[key + "_perm"].numpy(), obj[key + "_perm"]), key
    assert rel(got["mrstft_values"].numpy(), obj["mrstft_values"]) <= TOL_RESTATEMENT
    if mode == "item":
        assert len({tuple(r) for r in got["pit_mrstft_perm"].tolist()}) == 2      # batch PIT could not give this
    if mode is None:
        assert got["pit_mrstft_perm"].tolist() == [[0, 1, 2]] * 3


def test_zero_weights_drop_terms(eng):
    reals, decoded, want = small_tables(256, 64, 256, 3000, True)
    got = eng.mrstft_loss(reals_t(reals), reals_t(decoded), 8000, fft_sizes=(256,), hop_sizes=(64,), w_sc=0.0, w_lin_mag=1.0)
    assert not np.any(got["sc"].numpy())
    check_tables("w_sc=0", got, want, keys=("log_mag", "lin_mag"))
    obj = R.objective(want, 2, w_sc=0.0, w_lin_mag=1.0)
    assert rel(float(got["loss"]), obj["loss"]) <= TOL_RESTATEMENT


def test_two_calls_are_bit_identical(eng):
    g = golden()
    x, y = torch.from_numpy(g["fs16k_reals"]).cuda(), torch.from_numpy(g["fs16k_decoded"]).cuda()
    a = eng.mrstft_loss(x, y, 16000, w_lin_mag=1.0, l1_weight=1.0)
    eng.mrstft_loss(y, x, 16000, fft_sizes=(64,), hop_sizes=(16,))          # another call in between reuses the workspace
    b = eng.mrstft_loss(x, y, 16000, w_lin_mag=1.0, l1_weight=1.0)
    for k in ("sc", "log_mag", "lin_mag", "l1", "l2", "loss"):
        assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k


def test_invalid_arguments_fail_before_any_launch(eng):
    from ditsep_amd import native

    x = torch.zeros((1, 5, 2100), device="cuda")
    tabs = np.zeros(4096)

    def call(n, L, fft, hop, win, taps=None, ntaps=0):
        R_ = len(fft)
        cfg = native.DsnMrstftConfig(n_res=R_, fft=(C.c_int * R_)(*fft), hop=(C.c_int * R_)(*hop),
                                     win=(C.c_int * R_)(*win), w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0,
                                     taps=taps, n_taps=ntaps)
        out = native.DsnMrstftOut(sc=tabs.ctypes.data_as(C.POINTER(C.c_double)))
        return eng.lib.dsn_mrstft_loss(eng.ctx, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()), 1, n, L,
                                       C.byref(cfg), C.byref(out), None)

    t100 = (C.c_float * 100)()
    for args, what in (((5, 2100, [64], [16], [64]), "n = 5"),
                       ((2, 2100, [48], [12], [48]), "fft"), ((2, 2100, [4096], [1024], [4096]), "fft"),
                       ((2, 2100, [16], [4], [16]), "fft"), ((2, 2100, [64], [16], [65]), "win"),
                       ((2, 2100, [64], [0], [64]), "hop"), ((2, 1024, [64, 2048], [16, 512], [64, 2048]), "reflect"),
                       ((2, 2100, [64], [16], [64], t100, 100), "taps")):
        assert call(*args) == -1, what
        with pytest.raises(RuntimeError, match="dsn_mrstft_loss.*" + what):
            eng._check(-1, "dsn_mrstft_loss")
    assert not np.any(tabs)
    with pytest.raises(RuntimeError, match="L = 1024"):
        eng.mrstft_loss(torch.zeros(1, 2, 1024), torch.zeros(1, 2, 1024), 8000)
    with pytest.raises(ValueError, match="B,n,L"):
        eng.mrstft_loss(torch.zeros(1, 2, 2100), torch.zeros(1, 3, 2100), 8000)
    with pytest.raises(NotImplementedError, match="scale"):
        eng.mrstft_loss(torch.zeros(1, 2, 2100), torch.zeros(1, 2, 2100), 8000, scale="mel")


def test_ldm_losses_gen_and_evaluate_harness(tmp_path):
    from ditsep_amd import LDM, evaluate
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights
    from tests.test_gpu_kernels import _tiny_config

    cfg = dict(_tiny_config(tmp_path))
    cfg["training"] = {"loss": {"spectral": {"type": "mrstft", "decay": 1.0, "weights": {"mrstft": 1.0},
                                             "config": {"sample_rate": 8000, "fft_sizes": [2048, 1024, 512, 256, 128, 64, 32],
                                                        "hop_sizes": [512, 256, 128, 64, 32, 16, 8],
                                                        "win_lengths": [2048, 1024, 512, 256, 128, 64, 32],
                                                        "perceptual_weighting": True}},
                                "time": {"type": "l1", "weights": {"l1": 15.0}}}}
    vcfg = ovae.OobleckConfig(channels=32)
    vsd = tiny_vae_weights(vcfg, 31)
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    dsd = odit.random_dit_weights(dcfg, 32, out_gain=0.005)
    model = LDM(cfg, precision="fp16")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)

    g = golden()
    reals, decoded = g["fs8k_reals"], g["fs8k_decoded"]
    loss, losses = model.losses_gen(torch.from_numpy(decoded), torch.from_numpy(reals))
    assert list(losses) == ["pit_mrstft_loss", "pit_l1_loss"]
    want = float(g["fs8k_pit_mrstft_f64"]) + float(g["fs8k_pit_l1_f64"])
    assert rel(float(loss), want) <= 1e-6 and float(loss) == float(losses["pit_mrstft_loss"] + losses["pit_l1_loss"])

    gen = torch.Generator().manual_seed(1)
    batches = [(0.3 * torch.randn((2, 1, 4000), generator=gen), 0.3 * torch.randn((2, 2, 4000), generator=gen))]
    gl, gls, dec = model.generator_loss(batches[0][0], batches[0][1], N=2, seed=3)
    again, _ = model.losses_gen(dec, batches[0][1])
    assert dec.shape == (2, 2, 4000) and float(gl) == float(again) and np.isfinite(float(gl))

    decoded_b = []
    decode = model.decode

    def capture(*a, **k):
        out = decode(*a, **k)
        decoded_b.append(out.clone())
        return out

    model.decode = capture
    plain = evaluate.evaluate_batches(model, batches, fs=8000)
    plain_keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    assert all(list(r) == plain_keys for r in plain.values())
    evaluate.write_results(str(tmp_path / "plain.json"), plain)
    assert "mrstft_impl" not in json.loads((tmp_path / "plain_summary.json").read_text())
    decoded_b.clear()
    res = evaluate.evaluate_batches(model, batches, fs=8000, mrstft=True)
    mix, target = batches[0]
    tabs = model.engine.mrstft_loss(target, decoded_b[0], 8000, pit=None)
    for b in range(2):
        rec = res[b]
        assert list(rec) == plain_keys + ["mrstft", "l1"]
        for i in range(2):
            j = rec["perm"][i]
            assert rec["mrstft"][i] == float((tabs["sc"] + tabs["log_mag"]).mean(0)[b, i, j])
            assert rec["l1"][i] == float(tabs["l1"][b, i, j]) and rec["l1"][i] > 0
    evaluate.write_results(str(tmp_path / "out.json"), res)
    assert "mrstft_impl" in json.loads((tmp_path / "out_summary.json").read_text())
    assert {"mrstft", "l1"} <= set(evaluate.summarize(res))
    model.close()
