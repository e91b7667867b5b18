"""GPU: the native score-matching loss (dsn_score_loss, ditsep_amd/csrc/loss.hip) against the float64 restatement of
the reference's methods (tests/score_loss_restatement.py).

Two tiers.  (1) Perturb and reduce in isolation, bound 1e-6 relative: x_t and sigma with injected t, z, perm against
the restatement (x_t against the largest magnitude of the tensor: mean + sigma z cancels per element, and the device
forms it in fp32 as the reference does); the loss against the restatement fed the device's OWN score output
(Engine.score on the returned x_t), so no network rounding is in the way -- fp64 sums on both sides, one rounding to
fp32 at the end (6e-8).  (2) End to end against the CPU oracle networks: the relative difference per item of the
[B, n] loss against the restatement driven by oracle.dit.DiTScore / oracle.ncsnpp.NCSNppScore in fp32 on the same
injected t and z.  That is the score call's operand rounding seen through (sigma s + z)^2; it cannot be derived, so it
was measured over 3 seeds per case and the tests assert 4x the worst value seen (E2E_BOUND); every margin is printed as
a "loss-margin {json}" line (visible with -s).

Measured (worst relative difference per item over seeds 0, 1, 2; B x T in brackets):
  tiny DiT, bf16x3 [5 x 12]:        DSM 1.5e-7, 6.8e-8, 1.2e-7   PIT 3.9e-7, 1.0e-7, 2.3e-7   worst 3.94e-7 -> bound 1.6e-6
  tiny NCSN++, bf16x3 [3 x 6]:      DSM 1.2e-5, 3.8e-6, 7.4e-6   PIT 4.1e-6, 3.9e-6, 4.8e-6   worst 1.21e-5 -> bound 4.9e-5
  full-size DiT, fp16 [64 x 32]:    DSM 2.9e-5, 3.2e-5, 5.5e-5   PIT 2.3e-5, 5.2e-5, 2.2e-5   worst 5.52e-5 -> bound 2.2e-4
(PIT on the first two items of each batch.)  All are below the score-call tolerances the existing tests hold for the
same network and precision (1e-4 rel-L2 for the tiny networks in bf16x3, 3e-3 for the full-size DiT in fp16), as
they should be: sigma s is one of two terms of comparable size, and the mean over D T elements averages the
rounding.
"""
import itertools
import json

import numpy as np
import pytest
import torch

from oracle import dit as odit
from oracle import oobleck as ovae
from oracle.make_golden import tiny_vae_weights
from tests import score_loss_restatement as R
from tests.util import make_engine

pytestmark = pytest.mark.gpu

X3, FP16 = 2, 3
THETA, SMIN, SMAX = 1.5, float(np.float32(0.96)), 10.0   # the engine holds the SDE parameters as float32
T_EPS = 0.03
TOL = 1e-6
SDE = R.SDE(THETA, SMIN, SMAX)
# 4 x the worst per-item relative difference measured over seeds 0, 1, 2 (module docstring)
E2E_BOUND = {"tiny_dit/bf16x3": 4 * 3.94e-7, "tiny_ncsnpp/bf16x3": 4 * 1.21e-5, "full_dit/fp16": 4 * 5.52e-5}


def rel_max(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def rel_each(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(((a - b).abs() / b.abs()).max())


def _tiny_dit(n_src=2):
    cfg = odit.DiTConfig(n_src=n_src, embed_dim=128, depth=2, num_heads=2)
    sd = odit.random_dit_weights(cfg, 32 + n_src, out_gain=0.005)
    return cfg, sd


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(n_src):
        if n_src not in made:
            cfg, sd = _tiny_dit(n_src)
            made[n_src] = (cfg, sd, make_engine(cfg, sd, precision=X3))
        return made[n_src]

    yield get
    for _, _, eng in made.values():
        eng.close()


def _inputs(B, n, T, seed, D=64):
    g = torch.Generator().manual_seed(seed)
    mix = torch.randn((B, 1, D, T), generator=g)
    target = 0.7 * torch.randn((B, n, D, T), generator=g)
    t = T_EPS + (1 - T_EPS) * torch.rand(B, generator=g)
    z = torch.randn((B, n, D, T), generator=g)
    perm = torch.argsort(torch.rand((B, n), generator=g), dim=1)
    return mix, target, t, z, perm


# ------------------------------------------------------------------ perturb and reduce in isolation
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("T", [5, 40])      # D T = 320: a fraction of one 2048-element chunk; 2560: one chunk and a quarter
def test_perturb_and_reduce_in_isolation(engines, B, n, T):
    from ditsep_amd import sdes

    _, _, eng = engines(n)
    mix, target, t, z, perm = _inputs(B, n, T, 100 * B + 10 * n + T)
    # ---- DSM, with and without a source permutation
    for p in (None, perm):
        tgt = target if p is None else R.shuffle_sources(target, p)
        for red in ("none", "mean"):
            loss, aux = eng.score_loss(mix, target, reduction=red, time=t, noise=z, perm=p, return_aux=True)
            x_ref, _, s_ref, _ = R.sample_prior(SDE, mix, tgt, t, z)
            assert torch.equal(aux["t"].cpu(), t) and torch.equal(aux["z"].cpu(), z)
            assert rel_each(aux["sigma"], s_ref.reshape(-1)) <= TOL
            assert rel_max(aux["x_t"], x_ref) <= TOL
            # the host closed forms of the package agree with both
            hm, hs = sdes.OUVESDE(THETA, SMIN, SMAX).marginal_prob(tgt.double(), t.double(), mix.double())
            assert rel_each(aux["sigma"], hs) <= TOL and rel_max(aux["x_t"], hm + hs.reshape(-1, 1, 1, 1) * z) <= TOL
            dev = eng.score(aux["x_t"], aux["t"], mix).cpu().double()
            want = R.compute_score_loss(SDE, lambda *a: dev, mix, tgt, t, z, reduction=red)
            assert loss.shape == want.shape == ((B, n) if red == "none" else ())
            assert rel_each(loss, want) <= TOL, (red, p is not None)
    # ---- PIT variant: the restatement's n! enumeration on the device's own score
    loss, aux = eng.score_loss(mix, target, mode="init_pit", noise=z, return_aux=True)
    ones = torch.ones(B, dtype=torch.float64)
    assert torch.equal(aux["t"].cpu().double(), ones)
    assert rel_each(aux["sigma"], SDE.std(ones)) <= TOL
    assert rel_max(aux["x_t"], mix.double() + SDE.std(ones).reshape(-1, 1, 1, 1) * z.double()) <= TOL
    dev = eng.score(aux["x_t"], aux["t"], mix).cpu().double()
    count = {}
    want = R.compute_score_loss_init_hack_pit(SDE, lambda *a: dev, mix, target, z, count=count)
    assert count["calls"] == len(list(itertools.permutations(range(n))))
    assert loss.shape == want.shape == (B, n)
    assert rel_each(loss, want) <= TOL
    mean = eng.score_loss(mix, target, mode="init_pit", reduction="mean", noise=z)
    assert mean.shape == () and rel_each(mean, want.mean()) <= TOL


def test_pit_variant_makes_one_score_call(engines):
    """n = 3: the reference evaluates the network 3! = 6 times; the native call launches exactly the GEMMs of one
    Engine.score call, and its result equals the enumeration."""
    _, _, eng = engines(3)
    mix, target, _, z, _ = _inputs(4, 3, 8, 7)
    eng.profile_begin()
    eng.score(torch.zeros_like(target), torch.ones(4), mix)
    one = eng.profile_end()["gemm_launches"]
    eng.profile_begin()
    loss, aux = eng.score_loss(mix, target, mode="init_pit", noise=z, return_aux=True)
    got = eng.profile_end()["gemm_launches"]
    assert one > 0 and got == one
    dev = eng.score(aux["x_t"], aux["t"], mix).cpu().double()
    count = {}
    want = R.compute_score_loss_init_hack_pit(SDE, lambda *a: dev, mix, target, z, count=count)
    assert count["calls"] == 6 and rel_each(loss, want) <= TOL


# ------------------------------------------------------------------ end to end against the CPU oracle networks
def _e2e(name, eng, net, B, n, T, seeds=(0, 1, 2)):
    worst = 0.0
    for seed in seeds:
        mix, target, t, z, _ = _inputs(B, n, T, 1000 + seed)
        with torch.no_grad():
            ref = R.compute_score_loss(SDE, net, mix, target, t, z, score_dtype=torch.float32)
            ref_pit = R.compute_score_loss_init_hack_pit(SDE, net, mix[:2], target[:2], z[:2],
                                                         score_dtype=torch.float32)
        got = eng.score_loss(mix, target, time=t, noise=z).cpu().double()
        got_pit = eng.score_loss(mix[:2], target[:2], mode="init_pit", noise=z[:2]).cpu().double()
        d = float(((got - ref).abs() / ref).max())
        dp = float(((got_pit - ref_pit).abs() / ref_pit).max())
        worst = max(worst, d, dp)
        print("loss-margin " + json.dumps({"case": name, "B": B, "T": T, "seed": seed, "dsm_rel": d, "pit_rel": dp,
                                           "bound": E2E_BOUND[name]}))
    return worst


def test_e2e_tiny_dit_bf16x3(engines):
    torch.set_num_threads(16)
    cfg, sd, eng = engines(2)
    worst = _e2e("tiny_dit/bf16x3", eng, odit.DiTScore(sd, cfg), 5, 2, 12)
    assert worst <= E2E_BOUND["tiny_dit/bf16x3"]


def test_e2e_tiny_ncsnpp_bf16x3():
    from oracle import ncsnpp as oncs

    torch.set_num_threads(16)
    cfg = oncs.NCSNppConfig(n_src=2, nf=32)
    sd = oncs.random_ncsnpp_weights(cfg, 41)
    eng = make_engine(ncfg=cfg, nsd=sd, precision=X3)
    worst = _e2e("tiny_ncsnpp/bf16x3", eng, oncs.NCSNppScore(sd, cfg), 3, 2, 6)
    eng.close()
    assert worst <= E2E_BOUND["tiny_ncsnpp/bf16x3"]


def test_e2e_full_size_dit_batch64_fp16():
    """The benchmarked score network and shape (B = 64, T = 32, fp16) as tests/test_gpu_headline.py builds it."""
    from ditsep_amd import synthetic

    torch.set_num_threads(16)
    dcfg = synthetic.DiTConfig()
    dsd = synthetic.random_dit_weights(dcfg, 1, out_gain=0.002, skip_gain=0.02)
    eng = make_engine(dcfg, dsd, precision=FP16)
    worst = _e2e("full_dit/fp16", eng, odit.DiTScore(dsd, dcfg), 64, 2, 32)
    eng.close()
    assert worst <= E2E_BOUND["full_dit/fp16"]


# ------------------------------------------------------------------ determinism, RNG, argument checks
def test_bit_reproducible_eager_and_graph_replayed(engines):
    _, _, eng = engines(2)
    mix, target, t, z, perm = _inputs(5, 2, 12, 3)
    for kw in (dict(seed=11), dict(seed=11, mode="init_pit"), dict(seed=11, reduction="mean"),
               dict(time=t, noise=z, perm=perm)):
        eng.enable_graphs(False)
        a, aux_a = eng.score_loss(mix, target, return_aux=True, **kw)
        b = eng.score_loss(mix, target, **kw)
        assert torch.equal(a, b)
        eng.enable_graphs(True)
        for _ in range(3):                    # eager warm-up, capture, replay
            c, aux_c = eng.score_loss(mix, target, return_aux=True, **kw)
            assert torch.equal(a, c) and all(torch.equal(aux_a[k], aux_c[k]) for k in aux_a)
        other = eng.score_loss(mix * 0.5, target, **kw)      # a different input through the captured graph
        eng.enable_graphs(False)
        assert torch.equal(other, eng.score_loss(mix * 0.5, target, **kw))
    assert not torch.equal(eng.score_loss(mix, target, seed=11), eng.score_loss(mix, target, seed=12))


def test_seeded_draws(engines):
    """t inside [t_eps, T] for every item, different per item and per seed; z is draw 0 of the samplers' stream (the
    prior noise pc_sample uses for the same seed); the perturbation-only call returns the same draws."""
    _, _, eng = engines(2)
    mix, target, *_ = _inputs(64, 2, 8, 4)
    seen = []
    for seed in range(8):
        _, aux = eng.score_loss(mix, target, seed=seed, t_eps=T_EPS, return_aux=True)
        t = aux["t"].cpu()
        assert float(t.min()) >= np.float32(T_EPS) and float(t.max()) <= 1.0 and t.unique().numel() == 64
        seen.append(t)
        _, aux2 = eng.score_loss(mix, target, seed=seed, t_eps=T_EPS, loss=False, return_aux=True)
        assert all(torch.equal(aux[k], aux2[k]) for k in aux)
    assert len({tuple(t.tolist()) for t in seen}) == 8
    allt = torch.cat(seen)
    assert abs(float(allt.mean()) - 0.5 * (1 + T_EPS)) < 0.05          # 512 uniform draws: sd of the mean 0.012
    # x_T of the PC sampler for seed 5 is mix + std(1) z with the same z
    _, aux = eng.score_loss(mix, target, seed=5, mode="init_pit", return_aux=True)
    pc_x, _ = eng.pc_sample(mix, None, N=1, corrector_steps=0, predictor="none", denoise=False, seed=5)
    assert rel_max(aux["x_t"], pc_x) <= TOL


def test_invalid_arguments_rejected_by_the_engine(engines):
    _, _, eng = engines(2)
    mix, target, t, z, perm = _inputs(3, 2, 4, 5)
    bad_t = t.clone()
    bad_t[1] = 1.5
    bad_p = perm.clone()
    bad_p[2] = 0
    for kw in (dict(time=bad_t), dict(time=torch.zeros(3)), dict(time=torch.full((3,), float("nan"))),
               dict(perm=bad_p), dict(perm=perm + 1), dict(mode="init_pit", time=t), dict(mode="init_pit", perm=perm),
               dict(t_eps=0.0), dict(t_eps=1.0)):
        with pytest.raises(RuntimeError, match="dsn_score_loss"):
            eng.score_loss(mix, target, **kw)
    assert torch.isfinite(eng.score_loss(mix, target, time=t, noise=z, perm=perm)).all()     # the engine recovers


# ------------------------------------------------------------------ API mirror
def _tiny_config(tmp_path, **model_extra):
    vae_json = {"model_type": "autoencoder", "sample_rate": 16000,
                "model": {"encoder": {"type": "oobleck", "config": {"in_channels": 1, "channels": 32,
                                                                     "c_mults": [1, 2, 4, 8, 16],
                                                                     "strides": [2, 4, 4, 8, 8], "latent_dim": 128}},
                          "decoder": {"type": "oobleck", "config": {"out_channels": 1, "channels": 32,
                                                                     "c_mults": [1, 2, 4, 8, 16],
                                                                     "strides": [2, 4, 4, 8, 8], "latent_dim": 64}},
                          "bottleneck": {"type": "vae"}, "latent_dim": 64, "downsampling_ratio": 2048,
                          "io_channels": 1}}
    p = tmp_path / "vae.json"
    p.write_text(json.dumps(vae_json))
    return {"model": {"n_speakers": 2, "t_eps": T_EPS,
                      "score_model": {"_target_": "ditsep_amd.score_models.DiTScoreModel", "embed_dim": 128,
                                      "depth": 2, "num_heads": 2},
                      "vae": {"config_path": str(p), "ckpt_path": None, "trainable_vae": False},
                      "sde": {"_target_": "sdes.sdes.OUVESDE", "theta": 1.5, "sigma_min": 0.96, "sigma_max": 10.0,
                              "N": 4}, **model_extra}}


def _model(tmp_path, **model_extra):
    from ditsep_amd import LatentDiffSep

    vcfg = ovae.OobleckConfig(channels=32)
    vsd = tiny_vae_weights(vcfg, 31)
    _, dsd = _tiny_dit()
    model = LatentDiffSep(_tiny_config(tmp_path, **model_extra), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    return model


def test_latentdiffsep_mirrors_the_reference_methods(tmp_path):
    model = _model(tmp_path, loss={"_target_": "torch.nn.MSELoss"})
    eng = model.engine
    g = torch.Generator().manual_seed(21)
    L = 8000
    mix = 0.3 * torch.randn((3, 1, L), generator=g)
    target = 0.3 * torch.randn((3, 2, L), generator=g)
    assert model.loss_reduction == "mean" and model.init_hack is False and model.init_hack_p == 0.25
    out = model.validation_step((mix, target), 0, seed=5)
    y, x = model.encode(mix, target, seed=5)
    want = eng.score_loss(y, x, reduction="mean", t_eps=T_EPS, seed=5)
    assert out["val/score_loss"].shape == () and torch.equal(out["val/score_loss"], want)
    est, _ = model.separate(y, latent=True, target_dim=L, seed=5)
    si, _ = eng.si_sdr_pit(target, est)
    assert torch.equal(out["val/si_sdr"], si.clamp(-30.0, 30.0).mean())
    assert set(model.validation_step((mix, target), 1, seed=5)) == {"val/score_loss"}     # valid_max_sep_batches = 1
    model.on_validation_epoch_start()
    assert "val/si_sdr" in model.test_step((mix, target), 0, seed=5)
    # sample_time / sample_prior: the draws of the loss call for the same seed, reference shapes
    x_t, t, sigma, z = model.sample_prior(y, x, seed=9)
    _, aux = eng.score_loss(y, x, t_eps=T_EPS, seed=9, return_aux=True)
    assert sigma.shape == (3, 1, 1, 1) and torch.equal(x_t, aux["x_t"]) and torch.equal(z, aux["z"])
    assert torch.equal(model.sample_time(x, seed=9), t) and torch.equal(t, aux["t"])
    # minibatches: per-minibatch calls; the mean weighs them by size
    full = model.compute_score_loss(y, x, time=t, noise=z)
    split = model.compute_score_loss(y, x, time=t, noise=z, minibatch=2)
    assert abs(float(full) - float(split)) <= 1e-6 * float(full)
    with pytest.raises(IndexError):
        model.compute_score_loss_init_hack_pit(y, x)
    with pytest.raises(ValueError):
        model.train_step_init_5(y, x)
    model.close()


def test_latentdiffsep_init_hack_5_validation(tmp_path):
    model = _model(tmp_path, loss={"_target_": "torch.nn.MSELoss"}, init_hack=5, init_hack_p=0.5)
    eng = model.engine
    assert model.loss_reduction == "none"
    g = torch.Generator().manual_seed(22)
    y = torch.randn((5, 1, 64, 6), generator=g).cuda()
    x = 0.7 * torch.randn((5, 2, 64, 6), generator=g).cuda()
    mask = torch.tensor([True, False, False, True, False])
    perm = torch.tensor([[1, 0], [0, 1], [1, 0]])
    z = torch.randn((5, 2, 64, 6), generator=g)
    t = torch.tensor([0.2, 0.9, 0.5])
    got = model.train_step_init_5(y, x, pit_mask=mask, perm=perm, time=t, noise=z)
    a = eng.score_loss(y[mask], x[mask], mode="init_pit", noise=z[mask])
    b = eng.score_loss(y[~mask], x[~mask], time=t, noise=z[~mask], perm=perm)
    assert got.shape == () and torch.equal(got, torch.cat([a, b]).mean())
    assert model.compute_score_loss(y, x, seed=1).shape == (5, 2)
    assert model.compute_score_loss_init_hack_pit(y, x, seed=1, minibatch=2).shape == (5, 2)
    # seed-only: reproducible
    assert torch.equal(model.train_step_init_5(y, x, seed=3), model.train_step_init_5(y, x, seed=3))

    def dev_score(xt, tt, yy):      # the restatement on the device's score of the restatement's own float64 x_t
        return eng.score(xt.float(), tt.float(), yy.float()).cpu().double()

    want = R.train_step_init_5(SDE, dev_score, y.cpu(), x.cpu(), mask, z[mask], perm, t, z[~mask])
    assert abs(float(got) - float(want)) <= 1e-4 * float(want)   # (x_t is rounded to fp32 ahead of the network)
    model.close()


def test_evaluate_batches_score_loss_flag(tmp_path):
    from ditsep_amd import evaluate

    model = _model(tmp_path)
    g = torch.Generator().manual_seed(23)
    batches = [(0.3 * torch.randn((2, 1, 8000), generator=g), 0.3 * torch.randn((2, 2, 8000), generator=g))]
    base = evaluate.evaluate_batches(model, batches, 16000, N=2, seed=4)
    again = evaluate.evaluate_batches(model, batches, 16000, N=2, seed=4, score_loss=False)
    with_loss = evaluate.evaluate_batches(model, batches, 16000, N=2, seed=4, score_loss=True)
    keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    for i in base:
        assert list(base[i]) == keys == list(again[i]) and list(with_loss[i]) == keys + ["score_loss"]
        for k in keys:
            if k != "runtime":
                assert base[i][k] == again[i][k] == with_loss[i][k], k
        sl = with_loss[i]["score_loss"]
        assert len(sl) == 2 and all(np.isfinite(v) and v > 0 for v in sl)
    assert "score_loss" in evaluate.summarize(with_loss)
    model.close()
