"""dsn_resample (ditsep_amd/csrc/resample.hip) through Engine.resample on an engine with no score network and no codec,
against the float64 restatement A (tests/resample_restatement.py) fed the plan's own float32 taps, and the rate
keywords of LatentDiffSep against the same steps done by hand.

Bounds (u = 2^-24, A[j] = sum_k |h_k| |x_k| over output j's taps).
* One output is S float32 products and S - 1 additions, in any order, fused or not.  With every one of the 2 S - 1
  operations rounding once, |out - want| <= ((1 + u)^S - 1) A <= (S + 1) u A for S <= 73 (S^2 u / 2 < 1e-3 S).  The
  restatement's own float64 rounding is 2^-29 of that.
* With downmix the staged sample is fl(fl(x_0 + .. + x_{C-1}) / C): C - 1 additions and one division, each rounding
  once, so it is within ((1 + u)^C - 1) mean|x| <= (C + 1/2) u mean|x| of the exact mean, and the filter adds its own
  (S + 1) u on top: (S + C + 2) u A with A taken on the channel mean of |x|.
* Everything else -- a ragged item against the same item alone, reruns, equal rates, C = 1 with downmix -- is bit for
  bit: an output depends on its index and the staged samples only."""
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import resample_restatement as rr
from tests.util import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "ditsep_amd", "csrc", "resample.hip")).read()
TILE = int(re.search(r"constexpr int RS_TILE = (\d+);", SRC).group(1))              # output samples per tile
TILES_PER_WG = int(re.search(r"constexpr int RS_TILES_PER_WG = (\d+);", SRC).group(1))
U = 2.0 ** -24

# the smallest and the largest support (13, 73), the largest table (11025 -> 16000), orig = 1, both directions of 441:160
PAIRS = [(8000, 16000), (16000, 8000), (48000, 16000), (44100, 16000), (16000, 44100), (11025, 16000), (48000, 8000)]


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


_plans = {}


def plan_of(fs_in, fs_out):
    """the plan, and the dense float32 table its compact taps stand for (what the restatement is fed)"""
    if (fs_in, fs_out) not in _plans:
        p = native.resample_plan(fs_in, fs_out)
        _plans[(fs_in, fs_out)] = (p, rr.dense_from_compact(p["k0"], p["taps"], p["K"]))
    return _plans[(fs_in, fs_out)]


def in_len(fs_in, fs_out, Lout):
    """the shortest input whose output has at least Lout samples"""
    o, n = rr.params(fs_in, fs_out)[:2]
    return -(-Lout * o // n)


def lengths(fs_in, fs_out):
    o, _, _, width, _ = rr.params(fs_in, fs_out)
    return [1, width - 1, o + 1, 3 * o + 17,
            in_len(fs_in, fs_out, 3 * TILE + 37),                       # three tiles and an odd remainder
            in_len(fs_in, fs_out, (TILES_PER_WG + 1) * TILE + 301)]    # .. and into a second workgroup's first tile


def check(out, x64, fs_in, fs_out, what, absx=None, extra=1):
    """out [Lout] float32 against restatement A of x64 within (S + extra) u A; A on absx when given"""
    plan, h = plan_of(fs_in, fs_out)
    want, A = rr.resample_a(x64, fs_in, fs_out, h)
    if absx is not None:
        A = rr.resample_a(absx, fs_in, fs_out, np.abs(h))[0]
    assert out.shape == want.shape, (what, out.shape, want.shape)
    bound = (plan["support"] + extra) * U * A
    err = np.abs(out.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: error / bound, worst {worst:.3f}")
    assert np.all(err <= bound), f"{what}: {worst:.3f} x the bound"


@pytest.mark.parametrize("fs_in,fs_out", PAIRS, ids=lambda v: str(v))
def test_against_the_restatement(eng, fs_in, fs_out):
    g = torch.Generator().manual_seed(fs_in // 25 + fs_out)
    for L in lengths(fs_in, fs_out):
        x = torch.randn(L, generator=g)
        out = eng.resample(x, fs_in, fs_out)
        assert out.is_cuda and out.dtype == torch.float32
        assert tuple(out.shape) == (native.resample_length(fs_in, fs_out, L),) == (rr.length(*rr.params(fs_in, fs_out)[:2], L),)
        check(out.cpu().numpy(), x.double().numpy(), fs_in, fs_out, f"{fs_in} -> {fs_out} L {L}")


@pytest.mark.parametrize("fs_in,fs_out", PAIRS, ids=lambda v: str(v))
def test_ragged(eng, fs_in, fs_out):
    """B = 3, C = 2, NaN in the padding: every item is the dense call on that item alone"""
    o, n = rr.params(fs_in, fs_out)[:2]
    L = in_len(fs_in, fs_out, TILE + TILE // 2) + 1
    lens = [L, (L // 2) | 1, 1]
    g = torch.Generator().manual_seed(7)
    x = torch.randn((3, 2, L), generator=g)
    for b, v in enumerate(lens):
        x[b, :, v:] = float("nan")
    out, out_lens = eng.resample(x, fs_in, fs_out, lens=lens)
    assert out_lens == [rr.length(o, n, v) for v in lens]
    assert tuple(out.shape) == (3, 2, rr.length(o, n, L)) and not bool(torch.isnan(out).any())
    for b, v in enumerate(lens):
        alone = eng.resample(x[b:b + 1, :, :v].contiguous(), fs_in, fs_out)
        assert torch.equal(out[b, :, :out_lens[b]], alone[0]), f"item {b} differs from the item alone"
        assert bool((out[b, :, out_lens[b]:] == 0).all()), f"item {b}: not zero past its end"
    check(out[1, 1, :out_lens[1]].cpu().numpy(), x[1, 1, :lens[1]].double().numpy(), fs_in, fs_out,
          f"ragged {fs_in} -> {fs_out} item 1 channel 1")


@pytest.mark.parametrize("fs_in,fs_out", PAIRS, ids=lambda v: str(v))
def test_downmix(eng, fs_in, fs_out):
    o = rr.params(fs_in, fs_out)[0]
    g = torch.Generator().manual_seed(11)
    L4 = 4 * ((3 * o + 17) // 4 + 1)
    for L in (L4, L4 + 1):                        # rows 16-byte aligned, and not
        x1 = torch.randn((2, 1, L), generator=g)
        assert torch.equal(eng.resample(x1, fs_in, fs_out, downmix=True), eng.resample(x1, fs_in, fs_out))
        for Cn in (2, 3):
            x = torch.randn((2, Cn, L), generator=g)
            out = eng.resample(x, fs_in, fs_out, downmix=True)
            assert tuple(out.shape) == (2, 1, native.resample_length(fs_in, fs_out, L))
            for b in range(2):
                x64 = x[b].double().numpy()
                check(out[b, 0].cpu().numpy(), x64.sum(axis=0) / Cn, fs_in, fs_out,
                      f"downmix {fs_in} -> {fs_out} C {Cn} L {L} item {b}", absx=np.abs(x64).sum(axis=0) / Cn,
                      extra=Cn + 2)
    # a ragged batch with downmix: each item is the item alone
    x = torch.randn((2, 2, L4), generator=g)
    lens = [L4, L4 // 2 + 1]
    x[1, :, lens[1]:] = float("nan")
    out, ol = eng.resample(x, fs_in, fs_out, lens=lens, downmix=True)
    for b in range(2):
        alone = eng.resample(x[b:b + 1, :, :lens[b]].contiguous(), fs_in, fs_out, downmix=True)
        assert torch.equal(out[b, :, :ol[b]], alone[0]) and bool((out[b, :, ol[b]:] == 0).all())


def test_repeatable_and_layouts(eng):
    g = torch.Generator().manual_seed(13)
    x = torch.randn((2, 2, 3 * TILE + 5), generator=g)
    a = eng.resample(x, 44100, 16000)
    assert torch.equal(a, eng.resample(x, 44100, 16000))
    # [C, L] and [L] are the batch's rows
    assert torch.equal(eng.resample(x[1], 44100, 16000), a[1]) and torch.equal(eng.resample(x[1, 0], 44100, 16000), a[1, 0])
    assert tuple(eng.resample(x[1], 44100, 16000, downmix=True).shape) == (1, a.shape[-1])
    # a base that is not 16-byte aligned takes the scalar loads: the same bits
    flat = torch.randn(2 * TILE + 2, generator=g).to(eng.device)
    assert flat[1:].data_ptr() % 16 == 4
    assert torch.equal(eng.resample(flat[1:], 48000, 16000), eng.resample(flat[1:].clone(), 48000, 16000))
    # equal rates: the input bits (a negative zero included); with lens, zero past each item; with downmix, the mean
    x[0, 0, 3] = -0.0
    same = eng.resample(x, 16000, 16000)
    assert torch.equal(same.view(torch.int32), x.to(eng.device).view(torch.int32))
    x[1, :, 100:] = float("nan")
    out, ol = eng.resample(x, 16000, 16000, lens=[x.shape[-1], 100])
    assert ol == [x.shape[-1], 100] and torch.equal(out[1, :, :100], x[1, :, :100].to(eng.device))
    assert bool((out[1, :, 100:] == 0).all()) and torch.equal(out[0], x[0].to(eng.device))
    mean = eng.resample(x[0], 16000, 16000, downmix=True)
    assert torch.equal(mean, ((x[0, 0] + x[0, 1]) / 2.0)[None].to(eng.device))


def test_refusals_launch_nothing(eng):
    x = torch.zeros((1, 1, 480), device=eng.device)
    out = torch.full((1, 1, 160), 7.0, device=eng.device)

    def call(fs_in, fs_out, Lout):
        return eng.lib.dsn_resample(eng.ctx, native._ptr(x), 1, 1, 480, None, fs_in, fs_out, 0, native._ptr(out), Lout,
                                    eng._stream())

    assert call(48000, 16000, 159) != 0
    assert "Lout = 159 < ceil(new * L / orig) = 160" in eng.lib.dsn_last_error(eng.ctx).decode()
    # more phases than the LDS budget has room for (refused before the table is computed), and a tile span too long
    with pytest.raises(RuntimeError, match="words of LDS"):
        eng.resample(x, 48000, 47999)
    with pytest.raises(RuntimeError, match=r"orig 24, new 1\) needs \d+ words of LDS"):
        eng.resample(x, 192000, 8000)
    with pytest.raises(RuntimeError, match=r"B \* C = 65536 > 65535 rows"):
        eng.resample(torch.zeros((32768, 2, 1)), 8000, 16000)
    assert call(0, 16000, 160) != 0 and "sample rates must be positive" in eng.lib.dsn_last_error(eng.ctx).decode()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(48000, 16000, 160) == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())


# ------------------------------------------------------------------ the rate keywords of LatentDiffSep
FS = 16000
N_STEPS = 4
DRAWS = 1 + 2 * N_STEPS


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """a two-block Oobleck with hop 8 (the 128-channel configuration of tests/test_gpu_ragged_codec.py) and the tiny DiT
    of tests/test_gpu_separate_long.py behind LatentDiffSep, with config.model.fs = 16000"""
    import json

    from ditsep_amd import LatentDiffSep
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights

    vcfg = ovae.OobleckConfig(channels=128, c_mults=(1, 2), strides=(2, 4))
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    blk = {"channels": 128, "c_mults": [1, 2], "strides": [2, 4]}
    vae_json = {"model_type": "autoencoder", "sample_rate": FS,
                "model": {"encoder": {"type": "oobleck", "config": {"in_channels": 1, "latent_dim": 128, **blk}},
                          "decoder": {"type": "oobleck", "config": {"out_channels": 1, "latent_dim": 64, **blk}},
                          "bottleneck": {"type": "vae"}, "latent_dim": 64, "downsampling_ratio": vcfg.hop,
                          "io_channels": 1}}
    p = tmp_path_factory.mktemp("resample") / "vae.json"
    p.write_text(json.dumps(vae_json))
    cfg = {"model": {"n_speakers": 2, "t_eps": 0.03, "fs": FS,
                     "score_model": {"_target_": "ditsep_amd.score_models.DiTScoreModel", "embed_dim": 128, "depth": 2,
                                     "num_heads": 2},
                     "vae": {"config_path": str(p), "ckpt_path": None, "trainable_vae": False},
                     "sde": {"_target_": "sdes.sdes.OUVESDE", "theta": 1.5, "sigma_min": 0.96, "sigma_max": 10.0,
                             "N": N_STEPS},
                     "sampler": {"N": N_STEPS, "snr": 0.5, "corrector_steps": 1}}}
    m = LatentDiffSep(cfg, precision="bf16x3")
    sd = {"score_model." + k: v for k, v in odit.random_dit_weights(dcfg, 32, out_gain=0.005).items()}
    sd.update({"vae." + k: v for k, v in tiny_vae_weights(vcfg, 23).items()})
    m.load_state_dict(sd)
    assert m.fs == FS and m.hop_length == 8
    yield m
    m.close()


@pytest.fixture(scope="module")
def clips():
    """at the model's rate, at twice that rate, and stereo with the ratio 441:160"""
    g = torch.Generator().manual_seed(17)
    return [0.3 * torch.randn((1, 203), generator=g), 0.3 * torch.randn((1, 417), generator=g),
            0.3 * torch.randn((2, 611), generator=g)], [FS, 2 * FS, 44100]


def by_hand_in(model, clips, rates):
    return [c.to(model.engine.device) if (r == FS and c.shape[0] == 1) else
            model.engine.resample(c, r, FS, downmix=True) for c, r in zip(clips, rates)]


def by_hand_out(model, ests, clips, rates):
    return [e[:, :c.shape[-1]] if r == FS else model.engine.resample(e, FS, r)[:, :c.shape[-1]]
            for e, c, r in zip(ests, clips, rates)]


def test_separate_batch_at_any_rate(model, clips):
    cl, rates = clips
    hand = by_hand_in(model, cl, rates)
    assert [tuple(h.shape) for h in hand] == [(1, 203), (1, 209), (1, 222)]
    frames = [native.latent_frames_of(h.shape[-1], 8) for h in hand]
    g = torch.Generator().manual_seed(19)
    kw = dict(seed=3, vae_noise=[torch.randn((64, f), generator=g) for f in frames],
              noise=torch.randn((DRAWS, 3, 2, 64, max(frames)), generator=g))
    est, nfe = model.separate_batch(cl, sample_rates=rates, **kw)
    at_fs, nfe_fs = model.separate_batch(hand, **kw)
    want = by_hand_out(model, at_fs, cl, rates)
    assert nfe == nfe_fs == 2 * N_STEPS
    for b in range(3):
        assert tuple(est[b].shape) == (2, cl[b].shape[-1])                  # the input's own length
        assert torch.equal(est[b], want[b]), f"clip {b} is not the composition done by hand"
        assert bool(torch.isfinite(est[b]).all()) and float(est[b].abs().max()) > 0
    assert torch.equal(est[0], at_fs[0])            # the clip at the model's rate: what the call without rates gives it
    # one rate for all
    same, _ = model.separate_batch([cl[1], cl[1][:, :300]], sample_rates=2 * FS, seed=3)
    assert [tuple(s.shape) for s in same] == [(2, 417), (2, 300)]


def test_separate_at_a_rate(model):
    g = torch.Generator().manual_seed(23)
    mix = 0.3 * torch.randn((2, 2, 441), generator=g)
    est, nfe = model.separate(mix, sample_rate=44100, seed=5)
    m = model.engine.resample(mix, 44100, FS, downmix=True)
    assert tuple(m.shape) == (2, 1, 160)
    at_fs, _ = model.separate(m, seed=5)
    assert tuple(est.shape) == (2, 2, 441) and nfe == 2 * N_STEPS
    assert torch.equal(est, model.engine.resample(at_fs, FS, 44100)[..., :441])


def test_separate_long_at_any_rate(model):
    g = torch.Generator().manual_seed(29)
    cl = [0.3 * torch.randn((1, 803), generator=g), 0.3 * torch.randn((2, 290), generator=g)]
    rates = [2 * FS, FS]                                       # (stereo at the model's rate: mixed down, not resampled)
    kw = dict(window=128, overlap=32, mode="score", seed=7)
    est, nfe = model.separate_long(cl, sample_rates=rates, **kw)
    hand = by_hand_in(model, cl, rates)
    assert [tuple(h.shape) for h in hand] == [(1, 402), (1, 290)]
    at_fs, nfe_fs = model.separate_long(hand, **kw)
    want = by_hand_out(model, at_fs, cl, rates)
    assert nfe == nfe_fs
    for r in range(2):
        assert tuple(est[r].shape) == (2, cl[r].shape[-1]) and torch.equal(est[r], want[r])
    one, _ = model.separate_long(cl[0], sample_rates=2 * FS, **kw)
    assert torch.is_tensor(one) and tuple(one.shape) == (2, 803)


def test_preprocess_audio_list_for_encoder(model, clips):
    cl, rates = clips
    out = model.preprocess_audio_list_for_encoder(cl, rates)
    hand = by_hand_in(model, cl, rates)
    max_len = max(h.shape[-1] for h in hand)
    Lpad = max_len + (8 - max_len % 8) % 8
    assert tuple(out.shape) == (3, 1, Lpad) and Lpad == 224
    for b, h in enumerate(hand):
        assert torch.equal(out[b, :, :h.shape[-1]], h) and bool((out[b, :, h.shape[-1]:] == 0).all())
    # a [1, C, L] clip is squeezed, a 1-D clip gains its channel axis, one rate serves all
    one = model.preprocess_audio_for_encoder(cl[2][None], 44100)
    assert tuple(one.shape) == (1, 1, 224) and torch.equal(one[0], out[2])
    two = model.preprocess_audio_list_for_encoder([cl[1][0], cl[1]], 2 * FS)
    assert tuple(two.shape) == (2, 1, 216) and torch.equal(two[0], two[1])
