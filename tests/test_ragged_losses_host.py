"""CPU: the mixed-length forms of the MR-STFT and score-matching losses, before any device work.

(1) The yardstick of tests/test_gpu_ragged_losses.py: on the float64 restatements, the padded-and-masked formulation
the device implements equals the per-item definition (tests/ragged_losses_restatement.py).  (2) Argument checking of
lens / frames and of the list forms.  (3) evaluate_batches on a list batch against a stub engine: with
ragged_losses=True, score_loss=True and mrstft=True are honoured with one call each (a TypeError before this feature:
the keyword did not exist); without it the refusal stands."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mrstft_restatement as M
from tests import ragged_losses_restatement as RL
from tests import score_loss_restatement as S

SDE = S.SDE(1.5, 0.96, 10.0)


# ------------------------------------------------------------------ the restatements agree
@pytest.mark.parametrize("weighted", [False, True])
def test_mrstft_masked_formulation_equals_per_item(weighted):
    lens = (1025, 1031, 2047, 2100)
    B, n, Lmax = len(lens), 2, 2300
    reals, decoded = M.make_signals(8000, B, n, Lmax, 5)
    for b, v in enumerate(lens):                       # the padding is never read by either formulation
        reals[b, :, v:] = np.nan
        decoded[b, :, v:] = np.nan
    taps = None
    if weighted:
        from ditsep_amd import aweight
        taps = aweight.taps(8000)
    res = dict(fft_sizes=(2048, 256, 64), hop_sizes=(512, 64, 24), win_lengths=(2048, 200, 64), taps=taps)
    want = RL.mrstft_items(reals, decoded, lens, **res)
    got = RL.mrstft_masked(reals, decoded, lens, **res)
    for k in RL.KEYS:
        assert want[k].shape == got[k].shape and np.isfinite(want[k]).all(), k
        assert float(np.abs(got[k] / want[k] - 1.0).max()) <= 1e-12, k
    # and a dense batch is the special case of equal lengths
    dense = M.pair_tables(reals[:, :, :1025], decoded[:, :, :1025], res["fft_sizes"], res["hop_sizes"],
                          res["win_lengths"], taps)
    same = RL.mrstft_masked(reals, decoded, (1025,) * B, **res)
    for k in RL.KEYS:
        assert float(np.abs(same[k] / dense[k] - 1.0).max()) <= 1e-12, k


@pytest.mark.parametrize("n", [2, 3])
def test_score_loss_masked_formulation_equals_per_item(n):
    frames, T, D = (40, 32, 33, 1, 17), 48, 8
    B = len(frames)
    g = torch.Generator().manual_seed(3)
    y = torch.randn((B, 1, D, T), generator=g, dtype=torch.float64)
    x = torch.randn((B, n, D, T), generator=g, dtype=torch.float64)
    z = torch.randn((B, n, D, T), generator=g, dtype=torch.float64)
    t = 0.03 + 0.97 * torch.rand(B, generator=g, dtype=torch.float64)
    for b, f in enumerate(frames):
        x[b, ..., f:] = float("nan")
        z[b, ..., f:] = float("nan")
    for mode in ("dsm", "init_pit"):
        tt = t if mode == "dsm" else torch.ones(B, dtype=torch.float64)
        # the toy score acts per element, so the padded evaluation restricted to an item's frames is the item's own
        xt = torch.nan_to_num(S.sample_prior(SDE, y, x, tt, z)[0] if mode == "dsm"
                              else y + SDE.std(tt).reshape(-1, 1, 1, 1) * z)
        padded = S.toy_score(xt, tt, y)
        want = RL.score_loss_items(SDE, lambda b: S.toy_score, y, x, t, z, frames, mode=mode)
        got = RL.score_loss_masked(SDE, padded, y, x, t, z, frames, mode=mode)
        assert want.shape == got.shape == (B, n) and torch.isfinite(want).all()
        assert float(((got - want).abs() / want).max()) <= 1e-12, mode
        assert float(RL.reduce_mean(got)) == pytest.approx(float(want.mean()), rel=1e-12)
    # equal lengths: the mean of the row means is MSELoss()
    full = S.compute_score_loss(SDE, S.toy_score, y[..., :1], x[..., :1], t, z[..., :1], reduction="mean")
    rows = RL.score_loss_items(SDE, lambda b: S.toy_score, y, x, t, z, (1,) * B)
    assert float(RL.reduce_mean(rows)) == pytest.approx(float(full), rel=1e-12)


def test_sum_terms():
    assert RL.sum_terms("l1", 64, 16, 1031) == 1031
    assert RL.sum_terms("log_mag", 2048, 512, 1025) == 1025 * 3


# ------------------------------------------------------------------ argument checking
def test_lens_and_frames_are_validated():
    from ditsep_amd import native

    assert native.check_lens((1025, 2000), 2, 2000, 1025) == [1025, 2000]
    for bad, match in (((1025,), "one sample count per item"), ((0, 2000), r"lens\[0\] = 0 outside"),
                       ((1025, 2001), r"lens\[1\] = 2001 outside"), ((1024, 2000), "item 0")):
        with pytest.raises(ValueError, match=match):
            native.check_lens(bad, 2, 2000, 1025, " for the reflect padding of the largest FFT")
    assert native.check_ragged(native.SCORE_DIT, (1, 40), 2, 40) == [1, 40]
    for kind, fr, match in ((native.SCORE_NCSNPP, (1, 40), "need the DiT"), (native.SCORE_DIT, (0, 40), "outside"),
                            (native.SCORE_DIT, (1, 41), "outside"), (native.SCORE_DIT, (1,), "one frame count")):
        with pytest.raises(ValueError, match=match):
            native.check_ragged(kind, fr, 2, 40)


def test_engine_methods_refuse_bad_lengths_before_the_library():
    """Engine.mrstft_loss / score_loss check lens / frames on the host: a stub `self` without a library gets that far"""
    from ditsep_amd import native

    stub = SimpleNamespace(device="cpu", n_src=2, latent_dim=4, cfg=SimpleNamespace(score_kind=native.SCORE_DIT))
    x = torch.zeros((2, 2, 3000))
    for lens, match in (((1024, 3000), "item 0"), ((0, 3000), "outside"), ((3000, 3001), "outside"),
                        ((3000,), "one sample count")):
        with pytest.raises(ValueError, match=match):
            native.Engine.mrstft_loss(stub, x, x, 8000, lens=lens)
    y, x0 = torch.zeros((2, 1, 4, 6)), torch.zeros((2, 2, 4, 6))
    for frames, match in (((0, 6), "outside"), ((6, 7), "outside"), ((6,), "one frame count")):
        with pytest.raises(ValueError, match=match):
            native.Engine.score_loss(stub, y, x0, frames=frames)
    stub.cfg.score_kind = native.SCORE_NCSNPP
    with pytest.raises(ValueError, match="need the DiT"):
        native.Engine.score_loss(stub, y, x0, frames=(6, 6))


def test_losses_gen_list_form_is_padded_once_or_refused():
    from ditsep_amd.latent import LDM, padded_pair

    g = torch.Generator().manual_seed(1)
    reals = [torch.randn((2, L), generator=g) for L in (1500, 1100, 1300)]
    decoded = [r + 0.1 for r in reals]
    d, r, lens = padded_pair(decoded, reals, None, "cpu")
    assert lens == [1500, 1100, 1300] and d.shape == r.shape == (3, 2, 1500)
    assert torch.equal(r[1, :, :1100], reals[1]) and not r[1, :, 1100:].any() and torch.equal(d[2, :, :1300], decoded[2])
    t = torch.zeros((3, 2, 1500))
    assert padded_pair(t, t, [1500, 2, 3], "cpu") == (t, t, [1500, 2, 3]) and padded_pair(t, t, None, "cpu")[2] is None
    for args in ((decoded, t, None), (decoded, reals[:2], None), (decoded, reals, [1, 2, 3]), ([], [], None),
                 (decoded, [x[:, :-1] for x in reals], None), ([x[:1] for x in decoded], reals, None)):
        with pytest.raises(ValueError):
            padded_pair(*args, "cpu")
    calls = []

    def mrstft_loss(reals, decoded, fs, **kw):
        calls.append((reals, decoded, fs, kw))
        return {"loss": 1.0, "pit_mrstft_loss": 1.0}

    ldm = SimpleNamespace(engine=SimpleNamespace(mrstft_loss=mrstft_loss, device="cpu"), loss_fs=16000, pit="batch",
                          loss_kwargs={"l1_weight": 0.0})
    LDM.losses_gen(ldm, decoded, reals)
    LDM.losses_gen(ldm, d, r, lens=lens)
    assert len(calls) == 2 and calls[0][3]["lens"] == calls[1][3]["lens"] == lens
    assert torch.equal(calls[0][0], calls[1][0]) and torch.equal(calls[0][1], calls[1][1])
    LDM.losses_gen(ldm, d, r)
    assert calls[2][3]["lens"] is None                                       # the dense call is what it was


def test_list_forms_of_the_score_loss_are_refused_before_encoding():
    from ditsep_amd.latent import LatentDiffSep

    stub = SimpleNamespace()
    stub._maybe_lists = lambda *a: LatentDiffSep._maybe_lists(stub, *a)
    stub.encode_lists = lambda *a, **k: LatentDiffSep.encode_lists(stub, *a, **k)
    mixes = [torch.zeros((1, 900)), torch.zeros((1, 700))]
    targets = [torch.zeros((2, 900)), torch.zeros((2, 700))]
    for m, t in ((mixes, targets[:1]), ([], []), (mixes, [targets[0], torch.zeros((2, 701))]),
                 (mixes, [targets[0], torch.zeros((3, 700))]), ([torch.zeros((2, 900)), mixes[1]], targets)):
        with pytest.raises(ValueError):
            stub.encode_lists(m, t, seed=0)
    with pytest.raises(ValueError, match="both be tensors"):
        stub._maybe_lists(mixes, torch.zeros((2, 2, 4, 4)), 0, "grouped")
    with pytest.raises(ValueError):
        stub.encode_lists(mixes, targets, seed=0, codec="nonsense")


# ------------------------------------------------------------------ evaluate_batches on a list batch (stub engine)
class StubEngine:
    device, hop, D, n = "cpu", 100, 4, 2

    def __init__(self):
        self.calls = []

    def encode_ragged(self, mixes, vae_noise, seed=0, codec="grouped"):
        frames = [m.shape[-1] // self.hop + 1 for m in mixes]
        self.calls.append(("encode_ragged", len(mixes), seed, codec))
        return torch.ones((len(mixes), 1, self.D, max(frames))), frames

    def decode_ragged(self, x, frames, lens, codec="grouped"):
        return [torch.full((self.n, L), 0.5) for L in lens]

    def si_bss_eval(self, tgt, est, perm_by="sir", clamp_db=100.0, lens=None):
        B = tgt.shape[0]
        v = torch.zeros((B, self.n))
        return v, v, v, torch.tensor([[1, 0]] * B)

    def score_loss(self, y, x0, **kw):
        self.calls.append(("score_loss", tuple(y.shape), tuple(x0.shape), kw))
        return torch.arange(x0.shape[0] * self.n, dtype=torch.float32).reshape(-1, self.n)

    def mrstft_loss(self, reals, decoded, fs, **kw):
        self.calls.append(("mrstft_loss", tuple(reals.shape), fs, kw))
        B, n = reals.shape[:2]
        tab = torch.arange(B * n * n, dtype=torch.float64).reshape(1, B, n, n)
        return {"sc": tab, "log_mag": 2 * tab, "l1": -tab[0]}


def test_evaluate_batches_list_batch_honours_score_loss_and_mrstft(monkeypatch):
    from ditsep_amd import evaluate

    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    eng = StubEngine()
    model = SimpleNamespace(engine=eng, t_eps=0.03, sde=SimpleNamespace(N=2),
                            get_pc_sampler=lambda *a, **k: (lambda: (torch.zeros((3, 2, 4, 16)), 4)))
    lens = (1500, 1100, 1300)
    batch = ([torch.zeros((1, L)) for L in lens], [torch.zeros((2, L)) for L in lens])
    for flags in (dict(score_loss=True), dict(mrstft=True), dict(score_loss=True, mrstft=True, ragged_losses=False)):
        with pytest.raises(NotImplementedError, match="score_loss / mrstft .* ragged_losses=True"):   # the default
            evaluate.evaluate_batches(model, [batch], 16000, **flags)
    assert not eng.calls                                                     # refused before any device work
    res = evaluate.evaluate_batches(model, [batch], 16000, seed=7, start_idx=10, score_loss=True, mrstft=True,
                                    codec="padded", ragged_losses=True)
    assert sorted(res) == [10, 11, 12]
    keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    for b, i in enumerate(sorted(res)):
        assert list(res[i]) == keys + ["score_loss", "mrstft", "l1"]
        assert res[i]["score_loss"] == [2.0 * b, 2.0 * b + 1]
        # the diagonal under perm (1, 0) of (sc + log_mag) and of l1
        assert res[i]["mrstft"] == [3.0 * (4 * b + 1), 3.0 * (4 * b + 2)] and res[i]["l1"] == [-(4.0 * b + 1), -(4.0 * b + 2)]
    by = lambda name: [c for c in eng.calls if c[0] == name]
    # the seeds of the dense branch: mixtures seed + idx, targets seed + idx + 1 as B n rows, loss draws seed + idx
    assert by("encode_ragged") == [("encode_ragged", 3, 17, "padded"), ("encode_ragged", 6, 18, "padded")]
    (sl,), (mr,) = by("score_loss"), by("mrstft_loss")
    assert sl[1] == (3, 1, 4, 16) and sl[2] == (3, 2, 4, 16)
    assert sl[3] == dict(reduction="none", t_eps=0.03, seed=17, frames=[16, 12, 14])
    assert mr[1] == (3, 2, 1500) and mr[2] == 16000 and mr[3] == dict(pit=None, lens=[1500, 1100, 1300])
    # without the flags the records and the calls are what they were
    eng.calls.clear()
    plain = evaluate.evaluate_batches(model, [batch], 16000, seed=7, start_idx=10, ragged_losses=True)
    assert all(list(r) == keys for r in plain.values()) and not by("score_loss") and not by("mrstft_loss")
    assert len(by("encode_ragged")) == 1
