"""The `loudness` keyword of LatentDiffSep.separate / separate_batch / separate_long / separate_files with the tiny
model of tests/test_gpu_separate_files.py (hop 8, fs = 16000, bf16x3), on clips of half a second and more (a 400 ms
block must fit): None is the call without the keyword to the bit and to the byte; link "mixture" is Engine.loudness on
the mixture, native.loudness_gain and Engine.apply_gain done by hand; link "stem" brings every stem to the target."""
import math
import os

import numpy as np
import pytest
import torch

from ditsep_amd import native, wavio
from tests import pcm_restatement as pr

pytestmark = pytest.mark.gpu

FS = 16000
N_STEPS = 4
ROUND_DB = 20.0 * math.log10(1.0 + 2.0 ** -23)       # what rounding the gain to float32 can move a level by


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import json

    from ditsep_amd import LatentDiffSep
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights

    tmp = tmp_path_factory.mktemp("loud")
    vcfg = ovae.OobleckConfig(channels=128, c_mults=(1, 2), strides=(2, 4))
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    blk = {"channels": 128, "c_mults": [1, 2], "strides": [2, 4]}
    vae_json = {"model_type": "autoencoder", "sample_rate": FS,
                "model": {"encoder": {"type": "oobleck", "config": {"in_channels": 1, "latent_dim": 128, **blk}},
                          "decoder": {"type": "oobleck", "config": {"out_channels": 1, "latent_dim": 64, **blk}},
                          "bottleneck": {"type": "vae"}, "latent_dim": 64, "downsampling_ratio": vcfg.hop,
                          "io_channels": 1}}
    (tmp / "vae.json").write_text(json.dumps(vae_json))
    cfg = {"model": {"n_speakers": 2, "t_eps": 0.03, "fs": FS,
                     "score_model": {"_target_": "ditsep_amd.score_models.DiTScoreModel", "embed_dim": 128, "depth": 2,
                                     "num_heads": 2},
                     "vae": {"config_path": str(tmp / "vae.json"), "ckpt_path": None, "trainable_vae": False},
                     "sde": {"_target_": "sdes.sdes.OUVESDE", "theta": 1.5, "sigma_min": 0.96, "sigma_max": 10.0,
                             "N": N_STEPS},
                     "sampler": {"N": N_STEPS, "snr": 0.5, "corrector_steps": 1}}}
    sd = {"score_model." + k: v for k, v in odit.random_dit_weights(dcfg, 32, out_gain=0.005).items()}
    sd.update({"vae." + k: v for k, v in tiny_vae_weights(vcfg, 23).items()})
    m = LatentDiffSep(cfg, precision="bf16x3")
    m.load_state_dict(sd)
    assert m.fs == FS and m.hop_length == 8

    g = np.random.default_rng(61)
    src = tmp / "in"
    src.mkdir()
    wavio.write_wav(src / "a_mono.wav", (0.2 * g.standard_normal(8000) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    wavio.write_wav(src / "b_stereo.wav", (0.2 * g.standard_normal(2 * 4100) * 2 ** 15).astype("<i2").tobytes(), 8000, 2,
                    "s16")
    paths = sorted(src.glob("*.wav"))
    yield {"model": m, "tmp": tmp, "paths": paths, "headers": [wavio.read_header(p) for p in paths]}
    m.close()


def clip_of(path, h):
    return torch.from_numpy(pr.decode(wavio.read_payload(path, h), h.frames, h.channels, h.encoding))


def floats_of(path):
    """an f32 WAV -> (header, [C, frames] float32: the bits that were written)"""
    h = wavio.read_header(path)
    assert h.encoding == "f32"
    x = np.frombuffer(wavio.read_payload(path, h), dtype="<f4").reshape(h.frames, h.channels).T
    return h, torch.from_numpy(np.array(x, dtype=np.float32, order="C"))


def by_hand(eng, mixes, ests, rates, target=-23.0, peak=-1.0, link="mixture"):
    """the keyword's step from the public calls, item by item: -> (list of tensors, gains in dB per item)"""
    outs, gains = [], []
    for m, e, r in zip(mixes, ests, rates):
        n = int(e.shape[0])
        rows = e.reshape(n, -1, e.shape[-1])
        st = eng.loudness(rows, [r] * n)
        if link == "mixture":
            I = eng.loudness(m.reshape(-1, m.shape[-1]), r, true_peak=False)["loudness"].tolist() * n
            g = native.loudness_gain(I, st["true_peak"].tolist(), [0] * n, target, peak)
        else:
            g = native.loudness_gain(st["loudness"].tolist(), st["true_peak"].tolist(), None, target, peak)
        outs.append(eng.apply_gain(rows, g["gain"]).reshape(e.shape))
        gains.append(g["gain_db"])
    return outs, gains


@pytest.fixture(scope="module")
def mix():
    return 0.2 * torch.randn((2, 1, 8000), generator=torch.Generator().manual_seed(7))


def test_none_returns_the_bits_of_the_call_without_the_keyword(setup, mix):
    m = setup["model"]
    a, nfe = m.separate(mix, seed=3)
    b, _ = m.separate(mix, seed=3, loudness=None)
    assert torch.equal(a, b) and nfe == 2 * N_STEPS
    clips = [mix[0], mix[1, :, :7001]]
    a, _ = m.separate_batch(clips, codec="padded", seed=4)
    b, _ = m.separate_batch(clips, codec="padded", seed=4, loudness=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, _ = m.separate_long(mix[0], 4096, seed=5)
    b, _ = m.separate_long(mix[0], 4096, seed=5, loudness=None)
    assert torch.equal(a, b)


def test_none_writes_the_bytes_of_the_call_without_the_keyword(setup):
    m, paths = setup["model"], setup["paths"]
    o1, o2 = setup["tmp"] / "plain", setup["tmp"] / "none"
    r1 = m.separate_files(paths, o1, batch=2, seed=5)
    r2 = m.separate_files(paths, o2, batch=2, seed=5, loudness=None)
    for a, b in zip(r1, r2):
        assert "gain_db" not in b and a["clipped"] == b["clipped"]
        for p, q in zip(a["outputs"], b["outputs"]):
            assert open(p, "rb").read() == open(q, "rb").read()


def test_mixture_link_is_the_calls_by_hand(setup, mix):
    m = setup["model"]
    eng = m.engine
    est, _ = m.separate(mix, seed=3)
    got, _, info = m.separate(mix, seed=3, loudness=True, return_info=True)
    want, gains = by_hand(eng, [mix[0], mix[1]], [est[0], est[1]], [FS, FS])
    assert torch.equal(got, torch.stack(want))
    assert info["gain_db"] == gains and all(math.isfinite(g) and g != 0.0 for row in gains for g in row)
    for b in range(2):
        assert info["gain_db"][b][0] == info["gain_db"][b][1]                       # one gain per item
        assert info["loudness_out"][b][0] == info["loudness_in"][b][0] + info["gain_db"][b][0]
        if not info["limited"][b][0]:
            assert abs(info["loudness_out"][b][0] - (-23.0)) <= 1e-12
        assert max(info["true_peak_db"][b]) <= -1.0 + 1e-9
        # stems that summed to s now sum to g s, up to the rounding of the two products and of the sums
        g = float(np.float32(10.0 ** (gains[b][0] / 20.0)))
        s_before, s_after = est[b].double().sum(0), got[b].double().sum(0)
        slack = 3.0 * 2.0 ** -24 * g * est[b].abs().sum(0).double()
        assert bool(((s_after - g * s_before).abs() <= slack).all())
    assert info["silent"] == [] and info["nonfinite"] == []


def test_stem_link_brings_every_stem_to_the_target(setup, mix):
    m = setup["model"]
    eng = m.engine
    clips = [mix[0], torch.cat([mix[1, :, :7001], 0.5 * mix[1, :, 999:8000]])]      # mono, and stereo at 8 kHz
    rates = [FS, 8000]
    got, _, info = m.separate_batch(clips, codec="padded", sample_rates=rates, seed=4, return_info=True,
                                    loudness=dict(target=-30.0, peak=None, link="stem"))
    for b in range(2):
        again = eng.loudness(got[b][:, None], [rates[b]] * 2)
        for i in range(2):
            assert math.isfinite(info["loudness_in"][b][i])
            # the re-measurement works in float64 on float32 products, each off by at most 2^-24 relative: the mean
            # square moves by at most 2^-23 relative, 10 log10(1 + 2^-23) LU
            assert abs(float(again["loudness"][i]) - (-30.0)) <= ROUND_DB + 10.0 * math.log10(1.0 + 2.0 ** -23) + 1e-9
    # a target the ceiling forbids: every stem's true peak lands on the ceiling instead
    got, _, info = m.separate_batch(clips, codec="padded", sample_rates=rates, seed=4, return_info=True,
                                    loudness=dict(target=0.0, peak=-1.0, link="stem"))
    for b in range(2):
        again = eng.loudness(got[b][:, None], [rates[b]] * 2)
        for i in range(2):
            assert info["limited"][b][i]
            # |h| sums to less than 3 over a phase, so the interpolated values of g x and g times those of x differ by
            # at most (S + 2) 2^-24 3 max|x| <= 3e-6 of the peak: 3e-5 dB; the gain's rounding adds ROUND_DB
            assert abs(20.0 * math.log10(float(again["true_peak"][i])) - (-1.0)) <= 1e-4
            assert abs(info["true_peak_db"][b][i] - (-1.0)) <= 1e-9


def test_separate_long_with_loudness(setup, mix):
    m = setup["model"]
    est, _ = m.separate_long(mix[0], 4096, seed=5)
    got, _ = m.separate_long(mix[0], 4096, seed=5, loudness=-20.0)
    want, gains = by_hand(m.engine, [mix[0]], [est], [FS], target=-20.0)
    assert torch.equal(got, want[0]) and gains[0][0] != 0.0


def test_stereo_stems_file_in_a_batch_with_a_mono_file(setup):
    """f32 outputs hold the very floats: the files written with loudness= are gain times the files written without"""
    m, paths, hs = setup["model"], setup["paths"], setup["headers"]
    eng = m.engine
    o1, o2 = setup["tmp"] / "stems", setup["tmp"] / "stems_loud"
    r1 = m.separate_files(paths, o1, batch=2, seed=5, stems="wiener", encoding="f32")
    r2 = m.separate_files(paths, o2, batch=2, seed=5, stems="wiener", encoding="f32", loudness=True)
    for i, (a, b) in enumerate(zip(r1, r2)):
        before = [floats_of(p) for p in a["outputs"]]
        after = [floats_of(p) for p in b["outputs"]]
        assert all(h.channels == hs[i].channels and h.frames == hs[i].frames and h.rate == hs[i].rate for h, _ in after)
        stems = torch.stack([x for _, x in before])                                  # [n, C, frames]
        want, gains = by_hand(eng, [clip_of(paths[i], hs[i])], [stems], [hs[i].rate])
        assert torch.equal(torch.stack([x for _, x in after]), want[0].cpu())
        assert b["gain_db"] == gains[0] and gains[0][0] == gains[0][1] and gains[0][0] != 0.0
        assert set(b) - set(a) == {"loudness_in", "loudness_out", "gain_db", "true_peak_db"}
        assert max(b["true_peak_db"]) <= -1.0 + 1e-9
    assert hs[1].channels == 2 and hs[0].channels == 1


def test_mono_files_with_mixture_link_measure_the_file_with_its_channels(setup):
    m, paths, hs = setup["model"], setup["paths"], setup["headers"]
    o1, o2 = setup["tmp"] / "mono", setup["tmp"] / "mono_loud"
    r1 = m.separate_files(paths, o1, batch=2, seed=5, encoding="f32")
    r2 = m.separate_files(paths, o2, batch=2, seed=5, encoding="f32", loudness=dict(target=-18.0))
    for i, (a, b) in enumerate(zip(r1, r2)):
        stems = torch.stack([floats_of(p)[1][0] for p in a["outputs"]])               # [n, frames]
        want, gains = by_hand(m.engine, [clip_of(paths[i], hs[i])], [stems], [hs[i].rate], target=-18.0)
        got = torch.stack([floats_of(p)[1][0] for p in b["outputs"]])
        assert torch.equal(got, want[0].cpu()) and b["gain_db"] == gains[0]


def test_refusals(setup, mix):
    m = setup["model"]
    with pytest.raises(ValueError, match="latent=True"):
        m.separate(mix, latent=True, loudness=True)
    with pytest.raises(ValueError, match="intermediate"):
        m.separate(mix, loudness=True, intermediate=2)
    with pytest.raises(ValueError, match="intermediate"):
        m.separate_batch([mix[0]], loudness=True, intermediate=2)
    with pytest.raises(ValueError, match="loudness must be"):
        m.separate(mix, loudness=False)
    with pytest.raises(ValueError, match="3 channels"):
        m.separate(torch.zeros((1, 3, 8000)), sample_rate=8000, loudness=True)
    with pytest.raises(ValueError, match="link must be one of"):
        m.separate_files(setup["paths"], setup["tmp"] / "never", loudness={"link": "file"})
    assert not (setup["tmp"] / "never").exists()
