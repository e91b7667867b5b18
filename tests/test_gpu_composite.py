"""dsn_composite (ditsep_amd/csrc/composite.hip) against the float64 restatement of LLR / WSS / segmental SNR
(tests/composite_restatement.py) and against the reference's own functions (tests/golden/composite.npz).

Every frame of every item is compared: the per-frame values are read back from the call's workspace buffers.  The
device decides one thing on its own arithmetic, the sign of a band slope (it steers the WSS peak search), so every
input is checked on the CPU to keep all its non-zero slopes MARGIN_DB away from zero; the rows of a case are (source
seed, noise seed) pairs found by that check (tests/composite_restatement.py CASES)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import composite_restatement as R
from tests.util import make_engine

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "composite.npz")
MARGIN_DB = 1e-3
MEASURES = ("llr", "wss", "segsnr", "snr")
FRAME_BUFS = {"llr": "comp_llr", "wss": "comp_wss", "segsnr": "comp_ssnr"}
CASES, SILENCE = R.CASES, R.SILENCE

# max |device - restatement| measured on an MI355X over the cases fs16k and fs8k, and the bounds at 4x that:
#                          fs16k     fs8k
#   llr     aggregate      8.9e-9    6.2e-9      every frame  6.9e-15   3.3e-15    (fp64 throughout)
#   wss     aggregate      4.5e-7    8.2e-7      every frame  1.83e-5   1.09e-5    (fp32 FFT; values up to 92)
#   segsnr  aggregate      2.6e-7    3.7e-7      every frame  7.1e-15   7.1e-15    (fp64 throughout)
#   snr     aggregate      7.1e-7    7.5e-7
# The aggregates come back as float32, whose rounding is what their error shows.  The other cases stay inside (long:
# wss 8.9e-6 per frame; short 6.5e-6; silence 6.1e-6).  No TOL_AGG may exceed 1e-4 of the measure's spread over the
# items (asserted in test_matches_restatement: 2.9e-5 for llr, 2.6e-3 for wss).
MEASURED_AGG = {"llr": 8.9e-9, "wss": 8.2e-7, "segsnr": 3.7e-7, "snr": 7.5e-7}
MEASURED_FRAME = {"llr": 6.9e-15, "wss": 1.83e-5, "segsnr": 7.1e-15}
TOL_AGG = {k: 4 * v for k, v in MEASURED_AGG.items()}
TOL_FRAME = {k: 4 * v for k, v in MEASURED_FRAME.items()}
# max |restatement - golden| on the same inputs (tests/test_composite_host.py) at 4x
from tests.test_composite_host import TOL_GOLDEN_AGG, TOL_GOLDEN_FRAME  # noqa: E402


@pytest.fixture(scope="module")
def eng():
    e = make_engine(precision=2)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def items(name):
    fs, n, L, rows = CASES[name]
    ref, est = R.make_items(n, L, fs, rows)
    if name == "silence":
        ref, est = R.with_silence(ref, est, *SILENCE)
    for b in range(ref.shape[0]):
        for i in range(n):
            m = R.wss_slope_margin_db(ref[b, i].double().numpy(), est[b, i].double().numpy(), fs)
            assert m > MARGIN_DB, f"{name} item ({b}, {i}): a band slope of {m:.2e} dB is too close to a sign change"
    return ref, est, fs


def restate(ref, est, fs):
    """{measure: [B, n]} and {measure: [B, n, F]} in float64"""
    B, n, _ = ref.shape
    out = [[R.measures(ref[b, i].double().numpy(), est[b, i].double().numpy(), fs) for i in range(n)]
           for b in range(B)]
    agg = {k: np.array([[o[k] for o in row] for row in out]) for k in MEASURES + ("frames",)}
    per = {k: np.array([[o[f] for o in row] for row in out])
           for k, f in (("llr", "llr_frames"), ("wss", "wss_frames"), ("segsnr", "ssnr_frames"))}
    return agg, per


@functools.lru_cache(maxsize=None)
def restated(name):
    return restate(*items(name))


def device(eng, ref, est, fs, **kw):
    res = eng.composite(ref, est, fs, **kw)
    B, n, _ = ref.shape
    F = int(res["frames"][0, 0])
    per = {k: eng.debug_read(buf, (B * n * F * 2,)).view(torch.float64).reshape(B, n, F).numpy()
           for k, buf in FRAME_BUFS.items()}
    return res, per


def compare(tag, got, got_per, want, want_per, tol_agg, tol_frame):
    assert np.array_equal(got["frames"].numpy(), want["frames"])
    bad = []
    for k in MEASURES:
        err = float(np.abs(got[k].double().numpy() - want[k]).max())
        print(f"{tag}: {k} max |device - expected| = {err:.3e} (bound {tol_agg[k]:.3e}), "
              f"values {want[k].min():.4f} .. {want[k].max():.4f}")
        if not err <= tol_agg[k]:
            bad.append((k, err))
    for k in FRAME_BUFS:
        err = float(np.abs(got_per[k] - want_per[k]).max())
        print(f"{tag}: {k} per frame max |device - expected| = {err:.3e} (bound {tol_frame[k]:.3e})")
        if not err <= tol_frame[k]:
            bad.append((k + "_frames", err))
    assert not bad, bad


@pytest.mark.parametrize("name", ["fs16k", "fs8k"])
def test_matches_restatement(eng, name):
    ref, est, fs = items(name)
    assert ref.shape[:2] == (3, 2)
    want, want_per = restated(name)
    assert int(want["frames"][0, 0]) == 263
    for k in MEASURES:      # no bound wider than 1e-4 of the spread of the measure over the items
        assert TOL_AGG[k] <= 1e-4 * float(want[k].max() - want[k].min()), k
    assert float(want["llr"].max() - want["llr"].min()) > 0.15
    assert float(want["wss"].max() - want["wss"].min()) > 10
    got, got_per = device(eng, ref, est, fs)
    compare(name, got, got_per, want, want_per, TOL_AGG, TOL_FRAME)


@pytest.mark.parametrize("name", ["fs16k", "fs8k"])
def test_matches_golden(eng, name):
    g = np.load(GOLDEN)
    ref, est, fs = items(name)
    assert np.array_equal(g[f"{name}_ref_head"], ref[..., :16].numpy())        # the inputs the golden was made from
    assert np.array_equal(g[f"{name}_est_head"], est[..., :16].numpy())
    want = {k: g[f"{name}_{k}"] for k in MEASURES}
    want["frames"] = np.full(ref.shape[:2], g[f"{name}_llr_frames"].shape[-1])
    want_per = {"llr": g[f"{name}_llr_frames"], "wss": g[f"{name}_wss_frames"], "segsnr": g[f"{name}_ssnr_frames"]}
    got, got_per = device(eng, ref, est, fs)
    compare(name + " golden", got, got_per, want, want_per,
            {k: TOL_AGG[k] + TOL_GOLDEN_AGG[k] for k in MEASURES},
            {k: TOL_FRAME[k] + TOL_GOLDEN_FRAME[k] for k in FRAME_BUFS})
    if name == "fs16k":
        pesq = torch.tensor(g[f"{name}_pesq"], dtype=torch.float32)
        res = eng.composite(ref, est, fs, pesq=pesq)
        comp = np.stack([res[k].double().numpy() for k in ("csig", "cbak", "covl")], axis=-1)
        # the regressions weigh llr by about 1, wss by 0.009, segsnr by 0.063; float32 results
        tol = 1.1 * TOL_GOLDEN_AGG["llr"] + 1.1 * TOL_AGG["llr"] + 0.01 * (TOL_AGG["wss"] + TOL_GOLDEN_AGG["wss"]) \
            + 0.07 * (TOL_AGG["segsnr"] + TOL_GOLDEN_AGG["segsnr"]) + 1e-6
        assert float(np.abs(comp - g[f"{name}_composite"]).max()) <= tol


def test_long_item(eng):
    """1329 frames: the rank selection of the finish step runs over more than one tile and more than one workgroup's
    worth of frames"""
    ref, est, fs = items("long")
    want, want_per = restated("long")
    assert int(want["frames"][0, 0]) == 1329 and R.trimmed_count(1329) == 1263
    got, got_per = device(eng, ref, est, fs)
    compare("long", got, got_per, want, want_per, TOL_AGG, TOL_FRAME)


def test_short_item(eng):
    ref, est, fs = items("short")
    want, want_per = restated("short")
    assert int(want["frames"][0, 0]) == 10 and R.trimmed_count(10) == 10
    got, got_per = device(eng, ref, est, fs)
    compare("short", got, got_per, want, want_per, TOL_AGG, TOL_FRAME)


def test_exact_silence(eng):
    ref, est, fs = items("silence")
    want, want_per = restated("silence")
    inside = [f for f in range(int(want["frames"][0, 0]))
              if f * 120 >= SILENCE[0] and f * 120 + 480 <= SILENCE[0] + SILENCE[1]]
    assert len(inside) >= 10
    assert np.all(want_per["wss"][..., inside] == 0.0) and np.all(want_per["llr"][..., inside] == 0.0)
    got, got_per = device(eng, ref, est, fs)
    assert np.all(got_per["wss"][..., inside] == 0.0) and np.all(got_per["llr"][..., inside] == 0.0)
    compare("silence", got, got_per, want, want_per, TOL_AGG, TOL_FRAME)


def test_all_zero_estimate(eng):
    """the documented rule: segsnr and snr are NaN (the reference divides by max|est| = 0), llr and wss defined"""
    ref, _, fs = items("fs16k")
    est = torch.zeros_like(ref)
    want, want_per = restate(ref[:1], est[:1], fs)
    got, got_per = device(eng, ref[:1], est[:1], fs, pesq=torch.full((1, 2), 2.5))
    assert np.isnan(want["segsnr"]).all() and np.isnan(want["snr"]).all()
    assert torch.isnan(got["segsnr"]).all() and torch.isnan(got["snr"]).all() and torch.isnan(got["cbak"]).all()
    for k in ("llr", "wss"):
        assert torch.isfinite(got[k]).all()
        assert float(np.abs(got[k].double().numpy() - want[k]).max()) <= TOL_AGG[k]
        assert float(np.abs(got_per[k] - want_per[k]).max()) <= TOL_FRAME[k]
    assert torch.isfinite(got["csig"]).all() and torch.isfinite(got["covl"]).all()
    # the engine is unharmed
    ref2, est2, _ = items("short")
    assert torch.isfinite(eng.composite(ref2, est2, fs)["segsnr"]).all()


def test_invariances_and_refusals(eng):
    fs = 16000
    ref, est = R.make_items(2, fs + 61, fs, ((600, 607), (1600, 1607), (2600, 2607), (3600, 3607)))
    pesq = torch.tensor([[1.2, 2.0], [2.8, 3.3], [4.1, 4.5], [0.2, 5.0]])
    base = eng.composite(ref, est, fs, pesq=pesq)
    again = eng.composite(ref, est, fs, pesq=pesq)
    for k, v in base.items():                                                   # bit-identical reruns
        assert torch.equal(v, again[k]), k
    perm = torch.tensor([[1, 0], [0, 1], [1, 0], [1, 0]])
    swapped = torch.stack([est[b, perm[b]] for b in range(4)])
    by_perm = eng.composite(ref, est, fs, perm=perm)
    direct = eng.composite(ref, swapped, fs)
    for k, v in by_perm.items():
        assert torch.equal(v, direct[k]), k
    assert not torch.equal(by_perm["llr"], base["llr"])
    for b in range(4):
        for i in range(2):
            want = R.composites(float(base["llr"][b, i]), float(base["wss"][b, i]), float(base["segsnr"][b, i]),
                                float(pesq[b, i]))
            got = [float(base[k][b, i]) for k in ("csig", "cbak", "covl")]
            assert all(1.0 <= g <= 5.0 for g in got)
            assert max(abs(g - w) for g, w in zip(got, want)) <= 1e-6     # float32 rounding of a value <= 5
    assert "csig" not in by_perm
    with pytest.raises(RuntimeError, match="dsn_composite.*fs = 44100"):
        eng.composite(ref, est, 44100)
    with pytest.raises(RuntimeError, match="dsn_composite.*shorter than one frame"):
        eng.composite(ref[..., :599], est[..., :599], fs)
    assert int(eng.composite(ref[..., :600], est[..., :600], fs)["frames"][0, 0]) == 1
    with pytest.raises(RuntimeError, match="dsn_composite.*perm"):
        eng.composite(ref, est, fs, perm=torch.tensor([[1, 0], [0, 2], [1, 0], [1, 0]]))
    # composite outputs without pesq, at the C boundary
    import ctypes as C

    from ditsep_amd import native
    buf = (C.c_float * 8)()
    out = native.DsnCompositeOut(csig=buf)
    r, e = ref.cuda(), est.cuda()
    rc = eng.lib.dsn_composite(eng.ctx, C.c_void_p(r.data_ptr()), C.c_void_p(e.data_ptr()), 4, 2, ref.shape[-1], fs,
                               None, None, C.byref(out), None)
    assert rc == -1
    with pytest.raises(RuntimeError, match="dsn_composite.*need pesq"):
        eng._check(rc, "dsn_composite")


def test_evaluate_harness_composite(tmp_path):
    from ditsep_amd import LatentDiffSep, evaluate
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights
    from tests.test_gpu_kernels import _tiny_config

    vcfg = ovae.OobleckConfig(channels=32)
    vsd = tiny_vae_weights(vcfg, 31)
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    dsd = odit.random_dit_weights(dcfg, 32, out_gain=0.005)
    model = LatentDiffSep(_tiny_config(tmp_path), precision="fp16")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(1)
    batches = [(0.3 * torch.randn((2, 1, 4000), generator=g), 0.3 * torch.randn((2, 2, 4000), generator=g))
               for _ in range(2)]
    decoded = []
    decode = model.decode

    def capture(*a, **k):
        out = decode(*a, **k)
        decoded.append(out.clone())
        return out

    model.decode = capture
    plain = evaluate.evaluate_batches(model, batches[:1], fs=8000)
    plain_keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    assert all(list(r) == plain_keys and r["pesq"] is None for r in plain.values())
    evaluate.write_results(str(tmp_path / "plain.json"), plain)
    assert "composite_impl" not in json.loads((tmp_path / "plain_summary.json").read_text())

    decoded.clear()
    res = evaluate.evaluate_batches(model, batches, fs=8000, composite=True)
    assert sorted(res) == [0, 1, 2, 3] and len(decoded) == 2
    for k, (mix, target) in enumerate(batches):
        for b in range(2):
            rec = res[2 * k + b]
            assert list(rec) == plain_keys + ["llr", "wss", "segsnr"] and rec["pesq"] is None
            want = model.engine.composite(target[b:b + 1], decoded[k][b:b + 1], 8000, perm=[rec["perm"]])
            for key in ("llr", "wss", "segsnr"):
                assert rec[key] == want[key][0].tolist() and len(rec[key]) == 2
    evaluate.write_results(str(tmp_path / "out.json"), res)
    assert "composite_impl" in json.loads((tmp_path / "out_summary.json").read_text())

    seen = []

    def toy_pesq(fs, ref, est):
        assert fs == 8000 and ref.shape == est.shape == (4000,) and ref.dtype == np.float32
        assert abs(float(ref.mean())) < 1e-6 and abs(float(np.abs(est).max() / np.abs(ref).max()) - 1.0) < 1e-5
        seen.append(1)
        return 1.0 + 0.5 * (len(seen) % 5)

    decoded.clear()
    full = evaluate.evaluate_batches(model, batches[:1], fs=8000, composite=True, pesq_fn=toy_pesq)
    assert len(seen) == 4
    for b, rec in full.items():
        assert list(rec) == plain_keys + ["llr", "wss", "segsnr", "csig", "cbak", "covl"]
        assert rec["pesq"] == [1.0 + 0.5 * ((2 * b + i + 1) % 5) for i in range(2)]
        for i in range(2):
            want = R.composites(rec["llr"][i], rec["wss"][i], rec["segsnr"][i], rec["pesq"][i])
            assert max(abs(rec[k][i] - w) for k, w in zip(("csig", "cbak", "covl"), want)) <= 1e-6
    with pytest.raises(ValueError, match="pesq_fn"):
        evaluate.evaluate_batches(model, batches[:1], fs=8000, pesq_fn=toy_pesq)
    model.close()
