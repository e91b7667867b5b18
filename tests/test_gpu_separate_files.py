"""LatentDiffSep.separate_files and `python -m ditsep_amd.separate` on five tiny WAV files of different formats, rates
and channel counts, with the tiny model of tests/test_gpu_resample.py (hop 8, fs = 16000, bf16x3): the files written
equal, byte for byte, the route done by hand with the same batches and seeds -- the restatement's decode
(tests/pcm_restatement.py), separate_batch(sample_rates=..., seed=...) and the restatement's quantiser."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from ditsep_amd import files, wavio
from tests import pcm_restatement as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 16000
N_STEPS = 4


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """the model fixture of tests/test_gpu_resample.py, with its configuration and weights also on disk for the command
    line, and the input folder"""
    from ditsep_amd import LatentDiffSep
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights

    tmp = tmp_path_factory.mktemp("files")
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
    (tmp / "config.json").write_text(json.dumps(cfg))
    sd = {"score_model." + k: v for k, v in odit.random_dit_weights(dcfg, 32, out_gain=0.005).items()}
    sd.update({"vae." + k: v for k, v in tiny_vae_weights(vcfg, 23).items()})
    torch.save({"state_dict": {k: v.contiguous() for k, v in sd.items()}}, tmp / "model.pt")
    m = LatentDiffSep(cfg, precision="bf16x3")
    m.load_state_dict(sd)
    assert m.fs == FS and m.hop_length == 8

    g = np.random.default_rng(59)
    src = tmp / "in"
    src.mkdir()
    wavio.write_wav(src / "a_mono16.wav", (0.3 * g.standard_normal(203) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    s24 = (0.3 * g.standard_normal(2 * 611) * 2 ** 23).astype(np.int64)
    wavio.write_wav(src / "b_stereo24.wav", b"".join(int(v & 0xFFFFFF).to_bytes(3, "little") for v in s24), 44100, 2,
                    "s24")
    wavio.write_wav(src / "c_float.wav", (0.3 * g.standard_normal(417)).astype("<f4").tobytes(), 32000, 1, "f32")
    with wave.open(str(src / "d_stereo8.wav"), "wb") as w:
        w.setnchannels(2), w.setsampwidth(1), w.setframerate(8000)
        w.writeframes(np.clip(128 + 40 * g.standard_normal(2 * 90), 0, 255).astype(np.uint8).tobytes())
    wavio.write_wav(src / "e_longer.wav", (0.3 * g.standard_normal(700) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    paths = sorted(src.glob("*.wav"))
    yield {"model": m, "tmp": tmp, "paths": paths, "headers": [wavio.read_header(p) for p in paths]}
    m.close()


@pytest.fixture(scope="module")
def plain(setup):
    """separate_files(batch=3, seed=5) on the five files: (the output folder, the records)"""
    out = setup["tmp"] / "out"
    return out, setup["model"].separate_files(setup["paths"], out, batch=3, seed=5)


def clip_of(path, h):
    """the restatement's decode of a file: [C, frames] float32 at the file's own rate"""
    return torch.from_numpy(pr.decode(wavio.read_payload(path, h), h.frames, h.channels, h.encoding))


def check_outputs(out_dir, path, h, est, encoding="s16"):
    """est [n, frames] at the file's rate -> the two files hold the restatement's quantisation of it"""
    assert tuple(est.shape) == (2, h.frames)
    clipped = []
    for s in range(2):
        p = os.path.join(out_dir, f"s{s}", os.path.splitext(os.path.basename(path))[0] + ".wav")
        ho = wavio.read_header(p)
        assert ho[:4] == (h.rate, 1, h.frames, encoding), p
        want, c = pr.quantise(est[s].cpu().numpy(), encoding)
        assert wavio.read_payload(p, ho) == want, f"{p} is not the route done by hand"
        clipped.append(c)
    return clipped


def test_separate_files_is_the_route_by_hand(setup, plain):
    m, paths, hs = setup["model"], setup["paths"], setup["headers"]
    out, recs = plain
    plan = files.plan_files(hs, FS, 8, batch=3)
    assert plan["batches"] == [[3, 0, 2], [1, 4]] and plan["lengths"] == [203, 222, 209, 180, 700]
    assert sorted(os.listdir(out)) == ["s0", "s1"] and len(os.listdir(out / "s0")) == len(os.listdir(out / "s1")) == 5
    for k, idx in enumerate(plan["batches"]):
        clips = [clip_of(paths[i], hs[i]) for i in idx]
        est, nfe = m.separate_batch(clips, codec="padded", sample_rates=[hs[i].rate for i in idx], seed=5 + k)
        assert nfe == 2 * N_STEPS
        for j, i in enumerate(idx):
            r = recs[i]
            assert (r["path"], r["rate"], r["channels"], r["frames"], r["batch"]) == (
                str(paths[i]), hs[i].rate, hs[i].channels, hs[i].frames, k) and "alpha" not in r
            assert r["outputs"] == [str(out / f"s{s}" / paths[i].name) for s in range(2)]
            assert r["clipped"] == check_outputs(out, paths[i], hs[i], est[j])
            assert float(est[j].abs().max()) > 0


def test_rescale_and_encodings(setup):
    m, paths, hs = setup["model"], setup["paths"][:3], setup["headers"][:3]
    eng = m.engine
    out = setup["tmp"] / "out_rescale"
    recs = m.separate_files(paths, out, batch=3, seed=7, rescale=True, encoding="s24")
    idx = files.plan_files(hs, FS, 8, batch=3)["batches"][0]
    assert idx == [0, 2, 1]
    at_fs = eng.to_model_rate([clip_of(paths[i], hs[i]) for i in idx], [hs[i].rate for i in idx], FS)
    est, _ = m.separate_batch(at_fs, codec="padded", seed=7)
    lens = [int(e.shape[-1]) for e in est]
    sep = torch.zeros((3, 2, max(lens)), device=eng.device)
    mix = torch.zeros((3, max(lens)), device=eng.device)
    for j in range(3):
        sep[j, :, :lens[j]], mix[j, :lens[j]] = est[j], at_fs[j][0]
    scaled, alpha = eng.scale_output(mix, sep, lens)
    back = eng.from_model_rate([scaled[j, :, :lens[j]] for j in range(3)], [hs[i].rate for i in idx], FS,
                               [hs[i].frames for i in idx])
    for j, i in enumerate(idx):
        assert recs[i]["alpha"] == [float(a) for a in alpha[j]] and all(a != 1.0 for a in recs[i]["alpha"])
        assert recs[i]["clipped"] == check_outputs(out, paths[i], hs[i], back[j], "s24")


def test_long_files_go_through_separate_long(setup, plain):
    m, paths, hs = setup["model"], setup["paths"], setup["headers"]
    out = setup["tmp"] / "out_long"
    kw = dict(window=256, overlap=64)
    recs = m.separate_files(paths, out, batch=3, seed=5, long_after=0.03, **kw)
    plan = files.plan_files(hs, FS, 8, batch=3, long_after=0.03)
    assert plan["long"] == [4] and plan["batches"] == [[3, 0, 2], [1]]
    assert [r["batch"] for r in recs] == [0, 1, 0, 0, "long"]
    est, _ = m.separate_long([clip_of(paths[4], hs[4])], mode="stitch", batch=3, sample_rates=[hs[4].rate], seed=5, **kw)
    assert recs[4]["clipped"] == check_outputs(out, paths[4], hs[4], est[0])
    # the short files are what they are without the long one in their batches: batch 0 is the same three files
    for i in (3, 0, 2):
        for s in range(2):
            assert (out / f"s{s}" / paths[i].name).read_bytes() == (plain[0] / f"s{s}" / paths[i].name).read_bytes()


def test_command_line_writes_the_same_files(setup, plain):
    tmp = setup["tmp"]
    out = tmp / "out_cli"
    run = subprocess.run([sys.executable, "-m", "ditsep_amd.separate", str(tmp / "in"), str(out), "--config",
                          str(tmp / "config.json"), "--checkpoint", str(tmp / "model.pt"), "--precision", "bf16x3",
                          "--batch", "3", "--seed", "5"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert len(run.stdout.strip().splitlines()) == 5 and "b_stereo24.wav: 611 frames at 44100 Hz, 2 ch" in run.stdout
    for s in range(2):
        for p in setup["paths"]:
            assert (out / f"s{s}" / p.name).read_bytes() == (plain[0] / f"s{s}" / p.name).read_bytes(), p.name


def test_one_bad_file_raises_before_anything_is_written(setup):
    tmp = setup["tmp"]
    bad = tmp / "bad_mulaw.wav"
    good = setup["paths"][0].read_bytes()
    bad.write_bytes(good[:20] + (7).to_bytes(2, "little") + good[22:])          # format tag 7: mu-law
    out = tmp / "out_bad"
    with pytest.raises(ValueError, match="bad_mulaw.wav.*mu-law"):
        setup["model"].separate_files(setup["paths"] + [bad], out, batch=3, seed=5)
    assert not out.exists()
    with pytest.raises(ValueError, match="same stem"):
        setup["model"].separate_files([setup["paths"][0], setup["paths"][0]], out)
    assert not out.exists()
