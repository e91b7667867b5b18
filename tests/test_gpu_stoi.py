"""dsn_stoi (ditsep_amd/csrc/stoi.hip) against the float64 restatement of pystoi's STOI / ESTOI
(tests/stoi_restatement.py; parity with the pystoi package itself is unpinned)."""
import functools

import numpy as np
import pytest
import torch

from ditsep_amd import synthetic
from tests import stoi_restatement as R
from tests.util import make_engine

pytestmark = pytest.mark.gpu

TOL = 1e-4
MARGIN_DB = 0.01       # no clean frame may lie this close to the silent-frame threshold (a hard decision)
SNRS_DB = (-5.0, 0.0, 5.0, 10.0, 15.0, 20.0, 2.5, 12.5)
SEEDS = {8000: 100, 10000: 101, 16000: 100}      # inputs whose clean frames all clear MARGIN_DB (make_items checks)
GAP_SEEDS = {10000: 401, 16000: 400}


@pytest.fixture(scope="module")
def eng():
    e = make_engine(precision=2)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def make_items(B, n, L, fs, seed, gaps=False):
    """ref = synthetic_sources; est_i = ref_i + leakage of the other source + white noise, at SNRs from -5 to +20 dB.
    gaps=True inserts -60 dB stretches into every item (their frames must be removed)."""
    ref = synthetic.synthetic_sources(B, n, L, fs=fs, seed=seed).double()
    g = torch.Generator().manual_seed(seed + 7)
    noise = torch.randn((B, n, L), generator=g, dtype=torch.float64)
    est = torch.empty_like(ref)
    for b in range(B):
        for i in range(n):
            s = ref[b, i]
            snr = SNRS_DB[(b * n + i) % len(SNRS_DB)]
            d = 0.5 * ref[b, (i + 1) % n] + 0.3 * s.abs().max() * noise[b, i]
            est[b, i] = s + d * (s.norm() / d.norm()) * 10 ** (-snr / 20)
    if gaps:
        for b in range(B):
            for i in range(n):
                a = int(L * (0.2 + 0.1 * ((b + i) % 3)))
                ref[b, i, a:a + L // 6] *= 1e-3
                est[b, i, a:a + L // 6] *= 1e-3
    ref, est = ref.float(), est.float()
    for b in range(B):
        for i in range(n):
            m = R.silence_margin_db(ref[b, i].double().numpy(), fs)
            assert m > MARGIN_DB, f"test input item ({b}, {i}) lies {m:.4f} dB from the silent-frame threshold"
    return ref, est


@functools.lru_cache(maxsize=None)
def restated(B, n, L, fs, seed, extended, gaps=False):
    ref, est = make_items(B, n, L, fs, seed, gaps)
    out = [[R.stoi_details(ref[b, i].double().numpy(), est[b, i].double().numpy(), fs, extended)
            for i in range(n)] for b in range(B)]
    return (torch.tensor([[o[0] for o in row] for row in out], dtype=torch.float64),
            torch.tensor([[o[1] for o in row] for row in out], dtype=torch.long))


@pytest.mark.parametrize("extended", [0, 1])
@pytest.mark.parametrize("fs", [8000, 10000, 16000])
@pytest.mark.parametrize("seconds", [4.0, 2.73])
def test_stoi_matches_restatement(eng, fs, extended, seconds):
    L = int(seconds * fs) + (0 if seconds == 4.0 else 61)
    ref, est = make_items(4, 2, L, fs, SEEDS[fs])
    want, want_frames = restated(4, 2, L, fs, SEEDS[fs], extended)
    got, frames = eng.stoi(ref, est, fs, extended=bool(extended), return_frames=True)
    assert torch.equal(frames, want_frames)
    err = float((got.double() - want).abs().max())
    print(f"fs={fs} extended={extended} L={L}: max |native - restatement| = {err:.3e}, "
          f"scores {float(want.min()):.3f} .. {float(want.max()):.3f}")
    assert err <= TOL
    assert float(want.max() - want.min()) > 0.3      # the items spread over a real range of scores


def test_stoi_30s_item(eng):
    fs, L = 16000, 30 * 16000
    ref, est = make_items(1, 2, L, fs, 300)
    for extended in (0, 1):
        want, want_frames = restated(1, 2, L, fs, 300, extended)
        got, frames = eng.stoi(ref, est, fs, extended=bool(extended), return_frames=True)
        assert torch.equal(frames, want_frames) and int(frames.min()) > 2000
        err = float((got.double() - want).abs().max())
        print(f"30 s, extended={extended}: max |native - restatement| = {err:.3e}")
        assert err <= TOL


@pytest.mark.parametrize("fs", [10000, 16000])
def test_silent_frames_are_removed(eng, fs):
    L = 4 * fs
    ref, est = make_items(4, 2, L, fs, GAP_SEEDS[fs], gaps=True)
    want, want_frames = restated(4, 2, L, fs, GAP_SEEDS[fs], 1, gaps=True)
    got, frames = eng.stoi(ref, est, fs, extended=True, return_frames=True)
    assert torch.equal(frames, want_frames)
    full = 4 * 10000 // 128 - 2    # STFT frames of a 4 s item with nothing removed
    assert int(frames.max()) < full - 40
    assert float((got.double() - want).abs().max()) <= TOL


def test_short_input_scores_floor_and_warns(eng):
    fs = 16000
    ref, est = make_items(2, 2, 4 * fs, fs, 502)
    ref, est = ref.clone(), est.clone()
    ref[1, 0] = 0.0
    ref[1, 0, fs:fs + 3000] = 0.3 * torch.sin(torch.arange(3000) * 0.05)  # one short burst: < 30 frames survive
    assert R.silence_margin_db(ref[1, 0].double().numpy(), fs) > MARGIN_DB
    want, want_frames = [], []
    for b in range(2):
        for i in range(2):
            s, f, _ = R.stoi_details(ref[b, i].double().numpy(), est[b, i].double().numpy(), fs, True)
            want.append(s)
            want_frames.append(f)
    assert want_frames[2] < 30 and min(want_frames[:2] + want_frames[3:]) >= 30
    with pytest.warns(RuntimeWarning, match="fewer than 30 frames"):
        got, frames = eng.stoi(ref, est, fs, extended=True, return_frames=True)
    assert frames.reshape(-1).tolist() == want_frames
    assert float(got[1, 0]) == np.float32(1e-5)
    assert float((got.double().reshape(-1) - torch.tensor(want)).abs().max()) <= TOL
    with pytest.warns(RuntimeWarning):
        tiny = eng.stoi(ref[:, :, :3000], est[:, :, :3000], fs)      # 1875 samples at 10 kHz: < 30 frames anywhere
    assert torch.equal(tiny, torch.full((2, 2), 1e-5, dtype=torch.float32))


@pytest.mark.parametrize("extended", [False, True])
def test_stoi_invariances(eng, extended):
    fs = 16000
    ref, est = make_items(4, 2, 4 * fs, fs, 600)
    base = eng.stoi(ref, est, fs, extended=extended)
    assert torch.equal(base, eng.stoi(ref, est, fs, extended=extended))                 # bit-identical reruns
    assert float((eng.stoi(ref, 3.7 * est, fs, extended=extended) - base).abs().max()) < 1e-5
    perm = torch.tensor([[1, 0], [0, 1], [1, 0], [1, 0]])
    swapped = torch.stack([est[b, perm[b]] for b in range(4)])
    by_perm = eng.stoi(ref, est, fs, extended=extended, perm=perm)
    assert torch.equal(by_perm, eng.stoi(ref, swapped, fs, extended=extended))
    zero = eng.stoi(ref, torch.zeros_like(est), fs, extended=extended)
    assert torch.equal(zero, torch.zeros_like(zero))
    with pytest.raises(RuntimeError, match="dsn_stoi"):
        eng.stoi(ref, est, 0)
    with pytest.raises(RuntimeError, match="tap resampling filter"):
        eng.stoi(ref, est, 44101)


def test_evaluate_harness_stoi(tmp_path):
    import json

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
    res = evaluate.evaluate_batches(model, batches, fs=8000, stoi=True)
    assert sorted(res) == [0, 1, 2, 3] and len(decoded) == 2
    for k, (mix, target) in enumerate(batches):
        for b in range(2):
            rec = res[2 * k + b]
            assert len(rec["stoi"]) == 2 and rec["pesq"] is None
            want = model.engine.stoi(target[b:b + 1], decoded[k][b:b + 1], 8000, perm=[rec["perm"]])
            assert rec["stoi"] == want[0].tolist()
    s = evaluate.summarize(res)
    assert abs(s["stoi"] - np.mean([np.mean(r["stoi"]) for r in res.values()])) < 1e-12
    evaluate.write_results(str(tmp_path / "out.json"), res)
    assert "stoi_impl" in json.loads((tmp_path / "out_summary.json").read_text())
    plain = evaluate.evaluate_batches(model, batches[:1], fs=8000)
    assert all(r["stoi"] is None for r in plain.values())
    evaluate.write_results(str(tmp_path / "plain.json"), plain)
    assert "stoi_impl" not in json.loads((tmp_path / "plain_summary.json").read_text())
    model.close()
