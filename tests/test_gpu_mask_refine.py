"""dsn_mask_refine (ditsep_amd/csrc/maskrefine.hip) through Engine.mask_refine on an engine with no score network and no
codec, against the float64 restatement (tests/mask_refine_restatement.py), and the `refine` keyword of LatentDiffSep
against the same steps done by hand.

Bounds.  The error of a result is its largest absolute difference from the float64 restatement divided by the peak of
|mix|.  The allowed error is 8 x the error that the float32 run of the same restatement (torch.stft / torch.istft in
float32 on the CPU) shows on the same inputs: the device's radix-2 butterfly order and its fused multiply-adds differ
from pocketfft's, so a small factor over another float32 implementation is what can be justified; 8 is the margin the
multi-resolution STFT loss uses here.  Mixture consistency (sum_i out_i - mix) is held to 8 x the float32 run's own
consistency error in the same way.  Everything else -- silent estimates, n = 1, a ragged item against the item alone,
a permuted batch, a rerun, the keyword against the call done by hand -- is bit for bit.

Measured on an MI355X (device error / float32 CPU error, the allowed ratio being 8): see the README paragraph
"Mixture-consistent masks"."""
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import files, native, wavio
from tests import mask_refine_restatement as mr
from tests import pcm_restatement as pr
from tests.util import make_engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "ditsep_amd", "csrc", "maskrefine.hip")).read()
_m = re.search(r"constexpr int mr_span\(\) \{ return NFFT >= (\d+) \? (\d+) : (\d+); \}", SRC)
SPAN_FROM, SPAN_WIDE, SPAN_BASE = (int(v) for v in _m.groups())
FACTOR = 8.0


def span_of(n_fft):
    """output samples one workgroup owns"""
    return SPAN_WIDE if n_fft >= SPAN_FROM else SPAN_BASE


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    assert e.cfg.score_kind == native.SCORE_NONE
    yield e
    e.close()


def run(eng, mix, est, **kw):
    """mix [L], est [n, L] numpy float32 -> [n, L] numpy float32 from the device"""
    out = eng.mask_refine(torch.from_numpy(mix)[None], torch.from_numpy(est)[None], **kw)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (1,) + est.shape
    return out[0].cpu().numpy()


def check(eng, mix, est, n_fft, hop, power, what):
    """parity and mixture consistency of one case, each within FACTOR x the float32 CPU run's own error"""
    ref = mr.refine_torch(mix, est, n_fft, hop, power)
    cpu32 = mr.refine_torch(mix, est, n_fft, hop, power, dtype=np.float32)
    out = run(eng, mix, est, n_fft=n_fft, hop=hop, power=power)
    assert np.all(np.isfinite(out))
    e_dev, e_cpu = mr.rel_err(out, ref, mix), mr.rel_err(cpu32, ref, mix)
    c_dev = mr.rel_err(out.astype(np.float64).sum(axis=0), mix, mix)
    c_cpu = mr.rel_err(cpu32.astype(np.float64).sum(axis=0), mix, mix)
    print(f"{what}: parity {e_dev:.3e} (float32 CPU {e_cpu:.3e}, ratio {e_dev / e_cpu:.2f}); "
          f"consistency {c_dev:.3e} (float32 CPU {c_cpu:.3e}, ratio {c_dev / c_cpu:.2f})")
    assert e_dev <= FACTOR * e_cpu, f"{what}: parity {e_dev / e_cpu:.2f} x the float32 CPU error"
    assert c_dev <= FACTOR * c_cpu, f"{what}: consistency {c_dev / c_cpu:.2f} x the float32 CPU error"
    return e_dev / e_cpu, c_dev / c_cpu


@pytest.mark.parametrize("n_fft", [64, 512, 2048])
def test_against_the_restatement(eng, n_fft):
    """reflection at both ends (n_fft / 2 + 1: every frame reflects), the partial last hop (3 hop + 1, 5 n_fft + 7), the
    thin envelope at the edges, every source count and both powers.  3 hop + 1 at n_fft / hop = 8 is shorter than
    n_fft / 2 + 1 and refused by the definition (tests/test_mask_refine_host.py)."""
    worst = (0.0, 0.0)
    for r in (2, 4, 8):
        hop = n_fft // r
        for L in (n_fft // 2 + 1, 3 * hop + 1, 5 * n_fft + 7):
            if L < n_fft // 2 + 1:
                continue
            for n in (1, 2, 3, 4):
                mix, est = mr.make_case(n_fft + 31 * r + 7 * n + L, n, L)
                for power in (1, 2):
                    got = check(eng, mix, est, n_fft, hop, power, f"n_fft {n_fft} hop {hop} L {L} n {n} power {power}")
                    worst = (max(worst[0], got[0]), max(worst[1], got[1]))
    print(f"n_fft {n_fft}: worst parity ratio {worst[0]:.2f}, worst consistency ratio {worst[1]:.2f} (allowed {FACTOR})")


@pytest.mark.parametrize("n_fft,r,n,power", [(64, 8, 3, 1), (512, 4, 3, 2), (512, 2, 4, 2), (2048, 8, 2, 2),
                                             (2048, 4, 1, 1)])
def test_more_than_three_workgroup_spans(eng, n_fft, r, n, power):
    """three whole spans and a remainder that is no multiple of the hop or of 4: halo frames on both sides of every
    span boundary, the odd source count, the scalar store path"""
    hop = n_fft // r
    L = 3 * span_of(n_fft) + 2 * hop + 37
    mix, est = mr.make_case(n_fft + r + n, n, L)
    check(eng, mix, est, n_fft, hop, power, f"long n_fft {n_fft} hop {hop} L {L} n {n} power {power}")


def test_exact_cases(eng):
    for n_fft, hop, L in ((512, 128, 2 * SPAN_BASE + 301), (64, 8, 33), (2048, 1024, 3000)):
        mix, est = mr.make_case(n_fft + L, 4, L)
        one = run(eng, mix, np.zeros_like(est[:1]), n_fft=n_fft, hop=hop)
        assert float(np.abs(one).max()) > 0
        # silent estimates: M_i = eps / (n eps) = 1 / n exactly for n = 2, 4, and a power of two scales every bit
        for n in (1, 2, 4):
            out = run(eng, mix, np.zeros_like(est[:n]), n_fft=n_fft, hop=hop)
            for i in range(n):
                assert np.array_equal(out[i].view(np.int32), (one[0] / np.float32(n)).view(np.int32)), (n_fft, n, i)
        # n = 1: (a + eps) / (a + eps) = 1 exactly, whatever the estimate holds
        for power in (1, 2):
            got = run(eng, mix, est[:1], n_fft=n_fft, hop=hop, power=power)
            assert np.array_equal(got.view(np.int32), one.view(np.int32)), (n_fft, power)
        assert mr.rel_err(one[0], mix, mix) < 1e-5


@pytest.mark.parametrize("n_fft,hop,n", [(512, 128, 3), (2048, 256, 2), (64, 32, 4)])
def test_ragged(eng, n_fft, hop, n):
    """5 items of distinct lengths, one at the minimum, one over two spans, NaN past every end"""
    S, need = span_of(n_fft), n_fft // 2 + 1
    lens = [2 * S + 3 * hop + 5, need, S, S + 1, need + hop + 2]
    Lmax = max(lens) + 3
    g = np.random.default_rng(n_fft + n)
    mix = torch.full((5, Lmax), float("nan"))
    est = torch.full((5, n, Lmax), float("nan"))
    for b, v in enumerate(lens):
        m, e = mr.make_case(int(g.integers(1 << 30)), n, v)
        mix[b, :v], est[b, :, :v] = torch.from_numpy(m), torch.from_numpy(e)
    out = eng.mask_refine(mix, est, lens=lens, n_fft=n_fft, hop=hop)
    assert tuple(out.shape) == (5, n, Lmax) and not bool(torch.isnan(out).any())
    for b, v in enumerate(lens):
        alone = eng.mask_refine(mix[b:b + 1, :v].contiguous(), est[b:b + 1, :, :v].contiguous(), n_fft=n_fft, hop=hop)
        assert torch.equal(out[b, :, :v].view(torch.int32), alone[0].view(torch.int32)), f"item {b} differs from the item alone"
        assert bool((out[b, :, v:] == 0).all()), f"item {b}: not zero past its end"
        assert float(alone.abs().max()) > 0
    perm = [3, 0, 4, 2, 1]
    again = eng.mask_refine(mix[perm].contiguous(), est[perm].contiguous(), lens=[lens[p] for p in perm], n_fft=n_fft,
                            hop=hop)
    assert torch.equal(again.view(torch.int32), out[perm].view(torch.int32))
    twice = eng.mask_refine(mix, est, lens=lens, n_fft=n_fft, hop=hop)
    assert torch.equal(twice.view(torch.int32), out.view(torch.int32))
    # lists are padded once and come back as a list
    as_list = eng.mask_refine([mix[b, None, :v] for b, v in enumerate(lens)], [est[b, :, :v] for b, v in enumerate(lens)],
                              n_fft=n_fft, hop=hop)
    for b, v in enumerate(lens):
        assert tuple(as_list[b].shape) == (n, v) and torch.equal(as_list[b], out[b, :, :v])


def test_refusals_launch_nothing(eng):
    B, n, L = 2, 2, 600
    mix = torch.zeros((B, L), device=eng.device)
    est = torch.zeros((B, n, L), device=eng.device)
    out = torch.full((B, n, L), 7.0, device=eng.device)
    good = dict(mix=mix, est=est, B=B, n=n, Lmax=L, lens=None, n_fft=512, hop=128, power=2, eps=1e-10, out=out)

    def call(**kw):
        a = dict(good, **kw)
        lens = None if a["lens"] is None else (native.C.c_int32 * len(a["lens"]))(*a["lens"])
        return eng.lib.dsn_mask_refine(eng.ctx, native._ptr(a["mix"]), native._ptr(a["est"]), a["B"], a["n"], a["Lmax"],
                                       lens, a["n_fft"], a["hop"], a["power"], a["eps"], native._ptr(a["out"]),
                                       eng._stream())

    flat = torch.zeros(B * (n + 1) * L + 8, device=eng.device)
    for kw, msg in ((dict(mix=None), "mix, est or out is null"), (dict(est=None), "mix, est or out is null"),
                    (dict(out=None), "mix, est or out is null"),
                    (dict(B=0), "B = 0 outside [1, 65535]"),
                    (dict(n=0), "n = 0 outside [1, 4]"), (dict(n=5), "n = 5 outside [1, 4]"),
                    (dict(n_fft=32, hop=8), "n_fft = 32 is not a power of two in [64, 2048]"),
                    (dict(n_fft=4096, hop=1024), "n_fft = 4096 is not a power of two in [64, 2048]"),
                    (dict(n_fft=384, hop=96), "n_fft = 384 is not a power of two"),
                    (dict(hop=512), "n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
                    (dict(hop=32), "n_fft / hop = 512 / 32 is not one of 2, 4, 8"),
                    (dict(hop=0), "n_fft / hop = 512 / 0 is not one of 2, 4, 8"),
                    (dict(power=3), "power = 3 is not 1 or 2"),
                    (dict(eps=0.0), "eps = 0 is not a finite positive number"),
                    (dict(eps=float("nan")), "is not a finite positive number"),
                    (dict(eps=float("inf")), "is not a finite positive number"),
                    (dict(lens=[600, 256]), "item 1 has 256 samples, outside [n_fft / 2 + 1 = 257, Lmax = 600] (257 "
                                            "samples needed"),
                    (dict(lens=[601, 600]), "item 0 has 601 samples, outside"),
                    (dict(n_fft=2048, hop=512), "item 0 has 600 samples, outside [n_fft / 2 + 1 = 1025, Lmax = 600]"),
                    (dict(mix=out[0, 1]), "out overlaps mix or est"),
                    (dict(est=flat[4:], out=flat), "out overlaps mix or est"),
                    (dict(est=out), "out overlaps mix or est")):
        assert call(**kw) != 0, kw
        assert msg in eng.lib.dsn_last_error(eng.ctx).decode(), (kw, eng.lib.dsn_last_error(eng.ctx).decode())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flat == 0.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0.0).all())                 # a silent mixture gives silence


# ------------------------------------------------------------------ the refine keyword of LatentDiffSep
FS = 16000
N_STEPS = 4


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """the tiny DiT and the two-block Oobleck with hop 8 of tests/test_gpu_separate_files.py behind LatentDiffSep"""
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
    p = tmp_path_factory.mktemp("refine") / "vae.json"
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


def test_separate_with_refine(model):
    eng = model.engine
    g = torch.Generator().manual_seed(41)
    mix = 0.3 * torch.randn((2, 1, 600), generator=g)
    plain, nfe = model.separate(mix, seed=3)
    got, nfe_r = model.separate(mix, seed=3, refine=True)
    # without target_dim the codec hands back whole hops: the mixture is zero-extended to that, as the encoder saw it
    assert nfe == nfe_r == 2 * N_STEPS and tuple(got.shape) == tuple(plain.shape) == (2, 2, 608)
    padded = torch.nn.functional.pad(mix, (0, 8))
    assert torch.equal(got, eng.mask_refine(padded, plain)) and not torch.equal(got, plain)
    assert torch.equal(model.separate(mix, seed=3, refine="mask")[0], got)
    opts = dict(n_fft=64, hop=16, power=1)
    assert torch.equal(model.separate(mix, seed=3, refine=opts)[0], eng.mask_refine(padded, plain, **opts))
    cut, _ = model.separate(mix, target_dim=600, seed=3)
    assert torch.equal(model.separate(mix, target_dim=600, seed=3, refine=True)[0], eng.mask_refine(mix, cut))
    # refine=None is the old path, before and after
    assert torch.equal(model.separate(mix, seed=3)[0], plain)
    assert torch.equal(model.separate(mix, seed=3, refine=None)[0], plain)
    # the outputs add up to the mixture; the decoder's own do not
    peak = float(mix.abs().max())
    assert float((got.sum(dim=1).cpu() - padded[:, 0]).abs().max()) < 1e-5 * peak
    assert float((plain.sum(dim=1).cpu() - padded[:, 0]).abs().max()) > 1e-2 * peak
    # at another rate: refined at the model's rate, then taken back
    x = 0.3 * torch.randn((1, 2, 1300), generator=g)
    at_fs = eng.resample(x, 32000, FS, downmix=True)
    sep = model.separate(at_fs, seed=5)[0]
    hand = eng.resample(eng.mask_refine(torch.nn.functional.pad(at_fs, (0, sep.shape[-1] - at_fs.shape[-1])), sep),
                        FS, 32000)[..., :1300]
    assert torch.equal(model.separate(x, seed=5, sample_rate=32000, refine=True)[0], hand)
    with pytest.raises(ValueError, match="with latent=True there is no waveform mixture"):
        model.separate(torch.zeros(1, 64, 75), latent=True, refine=True)
    with pytest.raises(ValueError, match=r"the estimates \(592 samples\) are shorter than the mixture \(600\)"):
        model.separate(mix, target_dim=592, seed=3, refine=True)


def test_separate_batch_and_long_with_refine(model):
    eng = model.engine
    g = torch.Generator().manual_seed(43)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in (300, 611, 417)]
    for codec in ("grouped", "padded"):
        plain, nfe = model.separate_batch(mixes, codec=codec, seed=7)
        got, nfe_r = model.separate_batch(mixes, codec=codec, seed=7, refine=True)
        assert nfe == nfe_r
        want = eng.mask_refine(mixes, plain)
        for b in range(3):
            assert tuple(got[b].shape) == (2, mixes[b].shape[-1]) and torch.equal(got[b], want[b])
            assert torch.equal(got[b], eng.mask_refine(mixes[b], plain[b][None])[0])         # .. and the item alone
        again, _ = model.separate_batch(mixes, codec=codec, seed=7)
        assert all(torch.equal(a, p) for a, p in zip(again, plain))
    opts = dict(n_fft=128, hop=32)
    got, _ = model.separate_batch(mixes, seed=7, refine=opts)
    plain, _ = model.separate_batch(mixes, seed=7)
    assert all(torch.equal(a, b) for a, b in zip(got, eng.mask_refine(mixes, plain, **opts)))
    # long recordings: after the stitch (or the single decode of mode="score")
    rec = [0.3 * torch.randn((1, L), generator=g) for L in (700, 450)]
    for mode in ("stitch", "score"):
        kw = dict(window=256, overlap=64, mode=mode, batch=3, seed=9)
        plain, nfe = model.separate_long(rec, **kw)
        got, nfe_r = model.separate_long(rec, refine=True, **kw)
        assert nfe == nfe_r
        want = eng.mask_refine(rec, plain)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        one, _ = model.separate_long(rec[0], refine=True, **kw)
        assert tuple(one.shape) == (2, 700) and torch.equal(one, eng.mask_refine(rec[0], model.separate_long(rec[0], **kw)[0][None])[0])
        again, _ = model.separate_long(rec, **kw)
        assert all(torch.equal(a, b) for a, b in zip(again, plain))


def test_separate_files_with_refine(model, tmp_path):
    eng = model.engine
    g = np.random.default_rng(47)
    src = tmp_path / "in"
    src.mkdir()
    wavio.write_wav(src / "a.wav", (0.3 * g.standard_normal(300) * 2 ** 15).astype("<i2").tobytes(), FS, 1, "s16")
    wavio.write_wav(src / "b.wav", (0.3 * g.standard_normal(2 * 900)).astype("<f4").tobytes(), 32000, 2, "f32")
    wavio.write_wav(src / "c.wav", (0.3 * g.standard_normal(260) * 2 ** 15).astype("<i2").tobytes(), 8000, 1, "s16")
    paths = sorted(src.glob("*.wav"))
    hs = [wavio.read_header(p) for p in paths]
    out = tmp_path / "out"
    recs = model.separate_files(paths, out, batch=2, seed=5, refine=True)
    assert set(recs[0]) == {"path", "rate", "channels", "frames", "outputs", "clipped", "batch"}
    plan = files.plan_files(hs, FS, 8, batch=2)
    assert sorted(i for b in plan["batches"] for i in b) == [0, 1, 2] and len(plan["batches"]) == 2
    differs = False
    for k, idx in enumerate(plan["batches"]):
        clips = [torch.from_numpy(pr.decode(wavio.read_payload(paths[i], hs[i]), hs[i].frames, hs[i].channels,
                                            hs[i].encoding)) for i in idx]
        at_fs = eng.to_model_rate(clips, [hs[i].rate for i in idx], FS)
        est, _ = model.separate_batch(at_fs, codec="padded", seed=5 + k)
        back = eng.from_model_rate(eng.mask_refine(at_fs, est), [hs[i].rate for i in idx], FS,
                                   [hs[i].frames for i in idx])
        raw = eng.from_model_rate(est, [hs[i].rate for i in idx], FS, [hs[i].frames for i in idx])
        for j, i in enumerate(idx):
            assert tuple(back[j].shape) == (2, hs[i].frames)
            for s in range(2):
                p = out / f"s{s}" / paths[i].name
                ho = wavio.read_header(p)
                assert ho[:4] == (hs[i].rate, 1, hs[i].frames, "s16")
                want, clipped = pr.quantise(back[j][s].cpu().numpy(), "s16")
                assert wavio.read_payload(p, ho) == want, f"{p} is not the quantised refined estimate"
                assert recs[i]["clipped"][s] == clipped
                differs |= want != pr.quantise(raw[j][s].cpu().numpy(), "s16")[0]
    assert differs
    with pytest.raises(ValueError, match="refine must be"):
        model.separate_files(paths, tmp_path / "never", refine="wiener")
    with pytest.raises(ValueError, match=r"power = 3 is not 1 or 2"):
        model.separate_files(paths, tmp_path / "never", refine={"power": 3})
    # a file too short for one reflection is refused by name before anything is written
    with pytest.raises(ValueError, match=r"a\.wav: 300 samples at the model's rate; refine= needs at least n_fft / 2 \+ 1 "
                                         r"= 513"):
        model.separate_files(paths, tmp_path / "never", refine={"n_fft": 1024, "hop": 256})
    assert not (tmp_path / "never").exists()
