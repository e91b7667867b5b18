"""The metric calls on mixed-length batches (dsn_si_bss_eval_ragged, dsn_stoi_ragged, dsn_composite_ragged through
Engine.si_bss_eval / stoi / composite with lens=): items of different lengths padded to [B, 2, Lmax], THE PADDING SET TO
NaN, scored in one call.  Every case makes two comparisons:

1. against the dense call on the item alone (ref[b:b+1, :, :L_b]): equal bits (torch.equal) for scores, frames and
   perm.  The bound is derived: in all three families every reduction is per item, in an order fixed by the item's own
   length, and the padded batch only changes row strides and grid sizes.
2. against the float64 restatements run per item on the unpadded slice, at the bounds of the dense tests (imported):
   the oracle's definition-level SI-BSS restatement at the 2e-3 dB of test_si_bss_eval_matches_oracle, TOL of
   tests/test_gpu_stoi.py, TOL_AGG of tests/test_gpu_composite.py.

The inputs are seeded Gaussian references plus noisy estimates with cross-talk.  The composite seeds were searched on
the CPU, as the rows of tests/composite_restatement.py CASES were, so that no band slope lies within SLOPE_MARGIN_DB of
a sign change (the one hard decision the device takes on its own fp32 spectrum)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from ditsep_amd import native
from tests import composite_restatement as CR
from tests import stoi_restatement as SR
from tests.test_gpu_composite import TOL_AGG
from tests.test_gpu_stoi import MARGIN_DB as STOI_MARGIN_DB
from tests.test_gpu_stoi import TOL as STOI_TOL
from tests.util import make_engine

pytestmark = pytest.mark.gpu

SI_BSS_TOL_DB = 2e-3            # the bound of tests/test_gpu_kernels.py::test_si_bss_eval_matches_oracle
# a band energy off by the fp32 FFT's relative error (some 1e-6) moves a slope by 10 log10(1 + 1e-6) = 4e-6 dB; the
# inputs keep every non-zero slope 25 times that away from zero
SLOPE_MARGIN_DB = 1e-4
SI_BSS_LENS = (1, 255, 257, 4096)
STOI_LENS_16K = (12000, 11999, 9000, 6500, 300)
STOI_LENS_10K = (6500, 5000, 300)
COMP_LENS_8K = (61920, 5000, 359, 300)
COMP_LENS_16K = (5000, 719, 600)
COMP_SEEDS = {8000: 8441, 16000: 16001}


@pytest.fixture(scope="module")
def eng():
    e = make_engine(precision=2)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def ragged_items(lens, seed, swap=None):
    """-> (ref, est) [B, 2, Lmax] float32, NaN past every item's own length.  est_i = ref_i + cross-talk + noise; item
    `swap` has its estimate sources exchanged."""
    g = torch.Generator().manual_seed(seed)
    B, Lmax = len(lens), max(lens)
    ref = torch.randn((B, 2, Lmax), generator=g) * torch.tensor([1.0, 0.6])[None, :, None]
    est = ref + 0.25 * ref[:, [1, 0]] + 0.4 * torch.randn((B, 2, Lmax), generator=g)
    if swap is not None:
        est[swap] = est[swap][[1, 0]].clone()
    for b, L in enumerate(lens):
        ref[b, :, L:] = float("nan")
        est[b, :, L:] = float("nan")
    return ref, est


def alone(ref, est, lens, b):
    return ref[b:b + 1, :, :lens[b]].contiguous(), est[b:b + 1, :, :lens[b]].contiguous()


# ------------------------------------------------------------------ SI-SDR / SI-SIR / SI-SAR
@pytest.mark.parametrize("by", ["sir", "sdr"])
def test_si_bss_ragged(eng, by):
    from oracle import metrics

    lens = SI_BSS_LENS
    ref, est = ragged_items(lens, 71, swap=2)
    got = eng.si_bss_eval(ref, est, perm_by=by, lens=lens)
    again = eng.si_bss_eval(ref, est, perm_by=by, lens=lens)
    for a, b_ in zip(got, again):
        assert torch.equal(a, b_), "two ragged calls differ"
    assert all(torch.isfinite(v).all() for v in got[:3]), "the NaN padding was read"
    assert got[3][2].tolist() == [1, 0] and got[3][3].tolist() == [0, 1]      # the permutation is per item
    bad = []
    for b, L in enumerate(lens):
        r1, e1 = alone(ref, est, lens, b)
        dense = eng.si_bss_eval(r1, e1, perm_by=by)
        for name, a, d in zip(("si_sdr", "si_sir", "si_sar", "perm"), got, dense):
            assert torch.equal(a[b:b + 1], d), f"item {b} (L {L}) {name}: ragged {a[b].tolist()} dense {d[0].tolist()}"
        want = metrics.si_bss_eval(r1, e1, perm_by=by)
        assert torch.equal(got[3][b:b + 1], want[3])
        for name, a, w in zip(("si_sdr", "si_sir", "si_sar"), got[:3], want[:3]):
            err = float((a[b:b + 1].double() - w).abs().max())
            print(f"si_bss by {by} item {b} (L {L}) {name}: |ragged - float64| = {err:.3e} (bound {SI_BSS_TOL_DB:.0e})")
            if not err < SI_BSS_TOL_DB:
                bad.append((b, name, err))
    assert not bad, bad


# ------------------------------------------------------------------ STOI / ESTOI
@functools.lru_cache(maxsize=None)
def stoi_restated(lens, seed, fs, extended, perm=None):
    """float64 restatement per item on the unpadded slice -> ([B, 2] scores, [B, 2] frames); an item without one 10 kHz
    frame has no restatement (it raises there): None"""
    ref, est = ragged_items(lens, seed)
    scores, frames = [], []
    for b, L in enumerate(lens):
        if -(-L * 10000 // fs) < SR.N_FRAME:
            scores.append(None)
            frames.append(None)
            continue
        row = [SR.stoi_details(ref[b, i, :L].double().numpy(),
                               est[b, i if perm is None else perm[b][i], :L].double().numpy(), fs, bool(extended))
               for i in range(2)]
        for i in range(2):
            m = SR.silence_margin_db(ref[b, i, :L].double().numpy(), fs)
            assert m > STOI_MARGIN_DB, f"item ({b}, {i}) lies {m:.4f} dB from the silent-frame threshold"
        scores.append([r[0] for r in row])
        frames.append([r[1] for r in row])
    return scores, frames


def check_stoi(eng, lens, seed, fs, extended, perm=None, expect_frames=None):
    ref, est = ragged_items(lens, seed)
    with pytest.warns(RuntimeWarning, match="fewer than 30 frames"):
        got, frames = eng.stoi(ref, est, fs, extended=bool(extended), perm=perm, return_frames=True, lens=lens)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        again = eng.stoi(ref, est, fs, extended=bool(extended), perm=perm, lens=lens)
    assert torch.equal(got, again), "two ragged calls differ"
    assert torch.isfinite(got).all(), "the NaN padding was read"
    want, want_frames = stoi_restated(lens, seed, fs, extended, None if perm is None else tuple(map(tuple, perm)))
    if expect_frames is not None:
        assert [f[0] for f in want_frames if f is not None] == list(expect_frames)
    bad = []
    for b, L in enumerate(lens):
        r1, e1 = alone(ref, est, lens, b)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            d, df = eng.stoi(r1, e1, fs, extended=bool(extended), perm=None if perm is None else [perm[b]],
                             return_frames=True)
        for name, a, w in (("frames", frames, df), ("score", got, d)):
            assert torch.equal(a[b:b + 1], w), f"item {b} (L {L}) {name}: ragged {a[b].tolist()} dense {w[0].tolist()}"
        if want[b] is None:                                  # no frame at all: the dense call is the expectation
            assert frames[b].tolist() == [0, 0] and got[b].tolist() == [float(np.float32(1e-5))] * 2
            continue
        assert frames[b].tolist() == want_frames[b]
        err = float((got[b].double() - torch.tensor(want[b])).abs().max())
        print(f"stoi fs {fs} ext {extended} item {b} (L {L}, {want_frames[b][0]} frames): |ragged - float64| = "
              f"{err:.3e} (bound {STOI_TOL:.0e}), scores {want[b]}")
        if want_frames[b][0] < SR.N:
            assert got[b].tolist() == [float(np.float32(1e-5))] * 2
        if not err <= STOI_TOL:
            bad.append((b, err))
    assert not bad, bad


@pytest.mark.parametrize("extended", [1, 0], ids=["estoi", "stoi"])
def test_stoi_ragged_16k(eng, extended):
    check_stoi(eng, STOI_LENS_16K, 72, 16000, extended, expect_frames=(56, 56, 41, 29))


def test_stoi_ragged_10k(eng):
    """fs = 10000: no resampler, the frame kernels read the padded input rows themselves"""
    check_stoi(eng, STOI_LENS_10K, 73, 10000, 1)


def test_stoi_ragged_perm(eng):
    check_stoi(eng, STOI_LENS_16K, 72, 16000, 1, perm=[[1, 0], [0, 1], [1, 0], [0, 1], [1, 0]])


# ------------------------------------------------------------------ LLR / WSS / segmental SNR, composites
def check_composite(eng, lens, fs, expect_frames):
    seed = COMP_SEEDS[fs]
    ref, est = ragged_items(lens, seed)
    pesq = torch.linspace(1.2, 4.4, 2 * len(lens)).reshape(len(lens), 2)
    got = eng.composite(ref, est, fs, pesq=pesq, lens=lens)
    again = eng.composite(ref, est, fs, pesq=pesq, lens=lens)
    for k, v in got.items():
        assert torch.equal(v, again[k]), f"{k}: two ragged calls differ"
        assert torch.isfinite(v.double()).all(), f"{k}: the NaN padding was read"
    assert got["frames"][:, 0].tolist() == list(expect_frames)
    bad = []
    for b, L in enumerate(lens):
        r1, e1 = alone(ref, est, lens, b)
        dense = eng.composite(r1, e1, fs, pesq=pesq[b:b + 1])
        assert set(dense) == set(got)
        for k, v in got.items():
            assert torch.equal(v[b:b + 1], dense[k]), \
                f"item {b} (L {L}) {k}: ragged {v[b].tolist()} dense {dense[k][0].tolist()}"
        for i in range(2):
            x, y = ref[b, i, :L].double().numpy(), est[b, i, :L].double().numpy()
            m = CR.wss_slope_margin_db(x, y, fs)
            assert m > SLOPE_MARGIN_DB, f"item ({b}, {i}): a band slope of {m:.2e} dB is too close to a sign change"
            want = CR.measures(x, y, fs)
            assert int(got["frames"][b, i]) == want["frames"]
            for k in ("llr", "wss", "segsnr", "snr"):
                err = abs(float(got[k][b, i]) - want[k])
                print(f"composite fs {fs} item ({b}, {i}) (L {L}, {want['frames']} frames) {k}: |ragged - float64| = "
                      f"{err:.3e} (bound {TOL_AGG[k]:.3e}), value {want[k]:.4f}")
                if not err <= TOL_AGG[k]:
                    bad.append((b, i, k, err))
    assert not bad, bad


def test_composite_ragged_8k(eng):
    """1028 frames (past one 1024-frame rank tile), 79, and two items of exactly one frame"""
    check_composite(eng, COMP_LENS_8K, 8000, (1028, 79, 1, 1))


def test_composite_ragged_16k(eng):
    check_composite(eng, COMP_LENS_16K, 16000, (37, 1, 1))


# ------------------------------------------------------------------ refusals
def test_ragged_metric_refusals_launch_nothing(eng):
    """the C entry points refuse by name before anything is allocated or launched (the Python layer refuses the same
    cases earlier, tests/test_ragged_metrics_host.py: these calls go to the library directly)"""
    B, n, Lmax, fs = 4, 2, 5000, 8000
    ref = torch.zeros((B, n, Lmax), device="cuda")
    est = torch.zeros((B, n, Lmax), device="cuda")
    fbuf = [(C.c_float * (B * n))() for _ in range(4)]
    ibuf = (C.c_int * (B * n))()
    cout = native.DsnCompositeOut(llr=fbuf[0], wss=fbuf[1], segsnr=fbuf[2], snr=fbuf[3], frames=ibuf)

    def calls(lens):
        ln = None if lens is None else (C.c_int32 * B)(*lens)
        r, e = native._ptr(ref), native._ptr(est)
        return {
            "dsn_si_bss_eval_ragged": lambda: eng.lib.dsn_si_bss_eval_ragged(
                eng.ctx, r, e, B, n, Lmax, ln, 1, 100.0, fbuf[0], fbuf[1], fbuf[2], ibuf, eng._stream()),
            "dsn_stoi_ragged": lambda: eng.lib.dsn_stoi_ragged(
                eng.ctx, r, e, B, n, Lmax, ln, fs, 1, None, fbuf[0], ibuf, eng._stream()),
            "dsn_composite_ragged": lambda: eng.lib.dsn_composite_ragged(
                eng.ctx, r, e, B, n, Lmax, ln, fs, None, None, C.byref(cout), eng._stream()),
        }

    def refused(lens, reason, only=None):
        for name, call in calls(lens).items():
            if only is not None and name != only:
                continue
            before = eng.workspace_bytes()
            rc = call()
            msg = eng.lib.dsn_last_error(eng.ctx).decode()
            assert rc != 0 and msg.startswith(name + ":") and reason in msg, (name, rc, msg)
            assert eng.workspace_bytes() == before, f"{name}: a refused call grew the workspace"

    refused(None, "lens is null")
    refused((5000, 0, 4000, 3000), "lens[1] = 0 outside [1, Lmax = 5000]")
    refused((5000, 4000, 5001, 3000), "lens[2] = 5001 outside [1, Lmax = 5000]")
    refused((5000, 4000, 3000, 299),
            "item 3 (lens[3] = 299) is shorter than one frame (300 samples needed at fs = 8000)",
            only="dsn_composite_ragged")
    with pytest.raises(ValueError, match=r"lens\[2\] = 5001 outside"):
        eng.stoi(ref, est, fs, lens=(5000, 4000, 5001, 3000))
    with pytest.raises(ValueError, match="item 3 .* shorter than one frame"):
        eng.composite(ref, est, fs, lens=(5000, 4000, 3000, 299))


# ------------------------------------------------------------------ evaluation harness
HARNESS_LENS = (4000, 6143, 9000)


def test_evaluate_batches_ragged_metrics(tmp_path):
    """one list batch of three lengths through evaluate_batches with stoi and composite: every record holds what
    Engine.* gives for that item's own estimate alone"""
    from ditsep_amd import LatentDiffSep
    from ditsep_amd.evaluate import evaluate_batches
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights
    from tests.test_gpu_kernels import _tiny_config

    fs = 8000
    vcfg = ovae.OobleckConfig(channels=32)
    vsd = tiny_vae_weights(vcfg, 31)
    dcfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    dsd = odit.random_dit_weights(dcfg, 32, out_gain=0.005)
    model = LatentDiffSep(_tiny_config(tmp_path), precision="bf16x3")
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in vsd.items()})
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(35)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in HARNESS_LENS]
    targets = [0.3 * torch.randn((2, L), generator=g) for L in HARNESS_LENS]
    decoded = []
    decode_ragged = model.engine.decode_ragged

    def capture(*a, **k):
        out = decode_ragged(*a, **k)
        decoded.append([t.clone() for t in out])
        return out

    model.engine.decode_ragged = capture
    seen = []

    def toy_pesq(fs_, ref, est):
        assert fs_ == fs and ref.shape == est.shape and ref.shape[0] in HARNESS_LENS and ref.dtype == np.float32
        assert abs(float(ref.mean())) < 1e-6 and abs(float(np.abs(est).max() / np.abs(ref).max()) - 1.0) < 1e-5
        seen.append(ref.shape[0])
        return 1.0 + 0.5 * (len(seen) % 5)

    plain_keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    res = evaluate_batches(model, [(mixes, targets)], fs, N=4, seed=3, start_idx=10, stoi=True, composite=True)
    assert sorted(res) == [10, 11, 12] and len(decoded) == 1
    eng = model.engine
    for b, L in enumerate(HARNESS_LENS):
        rec = res[10 + b]
        assert list(rec) == plain_keys + ["llr", "wss", "segsnr"] and rec["pesq"] is None and rec["len_s"] == L / fs
        tgt, xr = targets[b][None], decoded[0][b][None]
        assert tuple(xr.shape) == (1, 2, L)
        sdr, sir, sar, perm = eng.si_bss_eval(tgt, xr, perm_by="sir", clamp_db=100.0)
        assert rec["perm"] == perm[0].tolist()
        assert rec["si_sdr"] == sdr[0].tolist() and rec["si_sir"] == sir[0].tolist()
        assert rec["si_sar"] == sar[0].tolist()
        assert rec["stoi"] == eng.stoi(tgt, xr, fs, perm=perm)[0].tolist()
        comp = eng.composite(tgt, xr, fs, perm=perm)
        for k in ("llr", "wss", "segsnr"):
            assert rec[k] == comp[k][0].tolist() and len(rec[k]) == 2, k
    full = evaluate_batches(model, [(mixes, targets)], fs, N=4, seed=3, composite=True, pesq_fn=toy_pesq)
    assert seen == [L for L in HARNESS_LENS for _ in range(2)]
    for b, rec in full.items():
        assert list(rec) == plain_keys + ["llr", "wss", "segsnr", "csig", "cbak", "covl"]
        assert rec["pesq"] == [1.0 + 0.5 * ((2 * b + i + 1) % 5) for i in range(2)]
        for i in range(2):
            want = CR.composites(rec["llr"][i], rec["wss"][i], rec["segsnr"][i], rec["pesq"][i])
            assert max(abs(rec[k][i] - w) for k, w in zip(("csig", "cbak", "covl"), want)) <= 1e-6
    with pytest.raises(NotImplementedError, match="score_loss / mrstft"):
        evaluate_batches(model, [(mixes, targets)], fs, N=4, mrstft=True)
    model.close()
