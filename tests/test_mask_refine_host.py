"""The host side of the mixture-consistent STFT masks (no GPU): the two float64 restatements of
tests/mask_refine_restatement.py against each other and against the properties the definition promises, the refusals
of native.check_mask_refine before the library is touched, the declaration and export of dsn_mask_refine, and the
`refine` keyword and command-line flags, all of which default to "off"."""
import inspect
import os
import re
import warnings

import numpy as np
import pytest
import torch

from ditsep_amd import files, native
from ditsep_amd import separate as cli
from ditsep_amd.latent import LatentDiffSep
from tests import mask_refine_restatement as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes():
    """(n_fft, hop, L): n_fft in {64, 512, 2048}, n_fft / hop in {2, 4, 8}, L in {n_fft / 2 + 1, 3 hop + 1,
    5 n_fft + 7}.  At n_fft / hop = 8, 3 hop + 1 < n_fft / 2 + 1: the definition refuses that length (one reflection
    must reach the item), so it is checked as a refusal below and not here."""
    out = []
    for n_fft in (64, 512, 2048):
        for r in (2, 4, 8):
            hop = n_fft // r
            for L in (n_fft // 2 + 1, 3 * hop + 1, 5 * n_fft + 7):
                if L >= n_fft // 2 + 1:
                    out.append((n_fft, hop, L))
    return out


SHAPES = shapes()


def test_shape_list():
    assert len(SHAPES) == 24 and (64, 8, 25) not in SHAPES and (64, 16, 49) in SHAPES


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_the_two_restatements_agree_and_keep_their_promises(n):
    worst = {"pair": 0.0, "sum": 0.0, "silent": 0.0, "f32": 0.0}
    for k, (n_fft, hop, L) in enumerate(SHAPES):
        mix, est = mr.make_case(1000 * n + k, n, L)
        for power in (1, 2):
            with warnings.catch_warnings():
                warnings.simplefilter("error")                  # torch.istft's window-overlap complaint included
                a = mr.refine_torch(mix, est, n_fft, hop, power)
                a32 = mr.refine_torch(mix, est, n_fft, hop, power, dtype=np.float32)
            b = mr.refine_numpy(mix, est, n_fft, hop, power)
            assert a.shape == b.shape == (n, L) and a.dtype == np.float64 and a32.dtype == np.float32
            worst["pair"] = max(worst["pair"], mr.rel_err(a, b, mix))
            worst["sum"] = max(worst["sum"], mr.rel_err(a.sum(axis=0), mix, mix), mr.rel_err(b.sum(axis=0), mix, mix))
            worst["f32"] = max(worst["f32"], mr.rel_err(a32, a, mix))
        silent = mr.refine_torch(mix, np.zeros_like(est), n_fft, hop)
        worst["silent"] = max(worst["silent"], mr.rel_err(silent, np.tile(mix.astype(np.float64) / n, (n, 1)), mix))
    print(f"n = {n}: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["pair"] < 1e-12 and worst["sum"] < 1e-12 and worst["silent"] < 1e-12
    assert worst["f32"] <= 2.5e-7


def test_one_source_gives_back_istft_of_stft():
    for n_fft, hop, L in SHAPES[::5]:
        mix, est = mr.make_case(n_fft + L, 1, L)
        Lp = mr.padded_length(L, hop)
        x = torch.zeros(Lp, dtype=torch.float64)
        x[:L] = torch.from_numpy(mix).double()
        w = torch.from_numpy(mr.window(n_fft))
        X = torch.stft(x, n_fft, hop_length=hop, window=w, center=True, pad_mode="reflect", return_complex=True)
        want = torch.istft(X, n_fft, hop_length=hop, window=w, center=True, length=Lp)[:L].numpy()
        for fn in (mr.refine_torch, mr.refine_numpy):
            got = fn(mix, est, n_fft, hop)
            assert mr.rel_err(got[0], want, mix) < 1e-12 and mr.rel_err(got[0], mix, mix) < 1e-12


def test_window_and_padding():
    w = mr.window(512)
    assert w[0] == 0.0 and w[256] == 1.0 and np.array_equal(w[1:], w[1:][::-1])
    assert np.array_equal(w, torch.hann_window(512, periodic=True, dtype=torch.float64).float().double().numpy())
    assert [mr.padded_length(L, 128) for L in (257, 384, 385)] == [384, 384, 512]
    assert mr.DEFAULTS == native.MASK_REFINE_DEFAULTS == dict(n_fft=512, hop=128, power=2, eps=1e-10)


# ------------------------------------------------------------------ refusals before the library
class _Untouchable:
    """stands in for the loaded library: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the refusal")


def _engine():
    e = object.__new__(native.Engine)
    e.cfg = native.DsnConfig()
    e.cfg.score_kind = native.SCORE_NONE
    e.lib, e.ctx, e.n_src, e.latent_dim, e.device = _Untouchable(), None, 2, 64, torch.device("cpu")
    return e


def test_refusals_before_the_library():
    e = _engine()
    mix, est = torch.zeros(2, 1, 600), torch.zeros(2, 2, 600)
    for kw, msg in ((dict(n_fft=48, hop=12), r"n_fft = 48 is not a power of two in \[64, 2048\]"),
                    (dict(n_fft=32, hop=8), r"n_fft = 32 is not a power of two"),
                    (dict(n_fft=4096, hop=1024), r"n_fft = 4096 is not a power of two in \[64, 2048\]"),
                    (dict(n_fft=512, hop=512), r"n_fft / hop = 512 / 512 is not one of 2, 4, 8"),
                    (dict(n_fft=512, hop=32), r"n_fft / hop = 512 / 32 is not one of 2, 4, 8"),
                    (dict(n_fft=512, hop=100), r"n_fft / hop = 512 / 100 is not one of 2, 4, 8"),
                    (dict(n_fft=512, hop=0), r"n_fft / hop = 512 / 0 is not one of"),
                    (dict(power=3), r"power = 3 is not 1 or 2"),
                    (dict(power=0), r"power = 0 is not 1 or 2"),
                    (dict(eps=0.0), r"eps = 0.0 is not a finite positive number"),
                    (dict(eps=-1e-3), r"eps = -0.001 is not a finite positive"),
                    (dict(eps=float("inf")), r"eps = inf is not a finite positive"),
                    (dict(eps=float("nan")), r"eps = nan is not a finite positive"),
                    (dict(n_fft=2048, hop=512), r"item 0 has 600 samples, outside \[n_fft / 2 \+ 1 = 1025, L = 600\] "
                                                r"\(1025 samples needed"),
                    (dict(lens=[600, 256]), r"item 1 has 256 samples, outside \[n_fft / 2 \+ 1 = 257, L = 600\]"),
                    (dict(lens=[601, 300]), r"item 0 has 601 samples, outside"),
                    (dict(lens=[600]), r"one sample count per item \(B = 2\), got 1")):
        with pytest.raises(ValueError, match=msg):
            e.mask_refine(mix, est, **kw)
    for m, s, msg in ((torch.zeros(2, 600), torch.zeros(2, 5, 600), r"n = 5 outside \[1, 4\]"),
                      (torch.zeros(2, 600), torch.zeros(2, 0, 600), r"n = 0 outside \[1, 4\]"),
                      (torch.zeros(2, 2, 600), est, r"mix must be \[B, L\] or \[B, 1, L\] and est \[B, n, L\]"),
                      (torch.zeros(2, 599), est, r"of the same B and L"),
                      (torch.zeros(3, 600), est, r"of the same B and L"),
                      (torch.zeros(0, 600), torch.zeros(0, 2, 600), r"B = 0 < 1"),
                      (mix, torch.zeros(2, 600), r"est \[B, n, L\]")):
        with pytest.raises(ValueError, match=msg):
            e.mask_refine(m, s)
    # 3 hop + 1 at n_fft / hop = 8: shorter than one reflection reaches
    with pytest.raises(ValueError, match=r"item 0 has 25 samples, outside \[n_fft / 2 \+ 1 = 33"):
        e.mask_refine(torch.zeros(1, 25), torch.zeros(1, 2, 25), n_fft=64, hop=8)
    # lists: one estimate per mixture, of the mixture's length
    with pytest.raises(ValueError, match="a list of mixtures goes with a list of as many estimates"):
        e.mask_refine([torch.zeros(1, 300)], [torch.zeros(2, 300)] * 2)
    with pytest.raises(ValueError, match=r"item 1 must be mix \[1, L\] and est \[n, L\]"):
        e.mask_refine([torch.zeros(1, 300), torch.zeros(1, 301)], [torch.zeros(2, 300)] * 2)
    assert native.check_mask_refine((2, 1, 600), (2, 2, 600), [600, 257]) == ((2, 2, 600), [600, 257], 512, 128, 2, 1e-10)
    assert native.check_mask_refine((1, 33), (1, 4, 33), None, 64, 8, 1, 1e-3) == ((1, 4, 33), None, 64, 8, 1, 1e-3)


def test_refine_options():
    assert native.refine_options(None) is None
    assert native.refine_options(True) == native.refine_options("mask") == native.MASK_REFINE_DEFAULTS
    assert native.refine_options(True) is not native.MASK_REFINE_DEFAULTS
    assert native.refine_options({"hop": 64, "power": 1}) == dict(n_fft=512, hop=64, power=1, eps=1e-10)
    for bad in (False, "wiener", 1, 512):
        with pytest.raises(ValueError, match="refine must be None, True, 'mask' or a dict"):
            native.refine_options(bad)
    with pytest.raises(ValueError, match=r"unknown keys \['window'\]"):
        native.refine_options({"window": "hann"})


def test_latent_with_refine_is_refused_before_anything_runs():
    m = object.__new__(LatentDiffSep)           # no engine: the refusal comes first
    with pytest.raises(ValueError, match="with latent=True there is no waveform mixture"):
        m.separate(torch.zeros(1, 64, 8), latent=True, refine=True)
    with pytest.raises(ValueError, match="refine must be"):
        m.separate(torch.zeros(1, 1, 800), refine="wiener")


# ------------------------------------------------------------------ declaration, export, keywords, flags
def test_symbol_declared_exported_and_built():
    hdr = open(os.path.join(ROOT, "include", "ditsep_hip.h")).read()
    assert re.search(r"\bint dsn_mask_refine\(dsn_ctx\* ctx, const float\* mix, const float\* est, int B, int n, "
                     r"int Lmax, const int32_t\* lens,\s+int n_fft, int hop, int power, float eps, float\* out, "
                     r"void\* stream\);", hdr)
    lib = native.load_library()
    assert "dsn_mask_refine" in native.EXPORTS and hasattr(lib, "dsn_mask_refine")
    assert len(lib.dsn_mask_refine.argtypes) == 13
    assert callable(native.Engine.mask_refine)
    src = open(os.path.join(ROOT, "ditsep_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bmaskrefine\.hip\b", src, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "ditsep_amd", "csrc", "maskrefine.hip"))


def test_keywords_default_to_off():
    for fn in (LatentDiffSep.separate, LatentDiffSep.separate_batch, LatentDiffSep.separate_long,
               LatentDiffSep.separate_files, files.separate_files):
        assert inspect.signature(fn).parameters["refine"].default is None, fn
    sig = inspect.signature(native.Engine.mask_refine).parameters
    assert {k: sig[k].default for k in native.MASK_REFINE_DEFAULTS} == native.MASK_REFINE_DEFAULTS
    assert sig["lens"].default is None


def test_command_line_flags():
    p = cli.build_parser()
    a = p.parse_args(["in", "out", "--config", "c.json"])
    assert (a.refine, a.refine_nfft, a.refine_hop, a.refine_power) == (False, 512, 128, 2)
    assert cli.refine_of(a) is None
    # the flags that were there keep their defaults
    assert (a.N, a.snr, a.corrector_steps, a.denoise, a.schedule, a.device) == (None, None, None, True, None, "cuda:0")
    assert (a.checkpoint, a.ema, a.precision, a.batch, a.encoding, a.rescale) == (None, False, "fp16", 64, "s16", False)
    assert (a.long_after, a.window, a.overlap, a.long_mode, a.seed) == (None, None, None, "stitch", None)
    a = p.parse_args(["in", "out", "--config", "c.json", "--refine"])
    assert cli.refine_of(a) == dict(n_fft=512, hop=128, power=2)
    assert native.refine_options(cli.refine_of(a)) == native.MASK_REFINE_DEFAULTS
    a = p.parse_args(["in", "out", "--config", "c.json", "--refine", "--refine-nfft", "1024", "--refine-hop", "256",
                      "--refine-power", "1"])
    assert cli.refine_of(a) == dict(n_fft=1024, hop=256, power=1)
    with pytest.raises(SystemExit):
        p.parse_args(["in", "out", "--config", "c.json", "--refine-power", "3"])
