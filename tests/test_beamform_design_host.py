"""The host side of the beamforming designs: the restatement (tests/beamform_design_restatement.py) against itself,
against numpy.linalg.solve and against closed forms, the sanity table of the README, and the options, merges and
refusals of native.py, latent.py, files.py and the command line.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ditsep_amd import files, native, separate
from ditsep_amd.latent import LatentDiffSep
from tests import beamform_design_restatement as bd
from tests import beamform_restatement as br

E32, R32 = float(np.float32(1e-10)), float(np.float32(1e-3))
KINDS = ("rank1", "gev")
SMALL = dict(n_fft=64, hop=16)
# the cases of tests/test_gpu_beamform_design.py and one of every kind besides
CASES = [((3, "generic", 2, 2, 700), SMALL, 1), ((3, "generic", 3, 3, 700), SMALL, 2), ((3, "generic", 4, 8, 6000), {}, 7),
         ((3, "generic", 1, 4, 700), SMALL, 1), ((1, "generic", 2, 2, 33), SMALL, 0), ((1, "dual", 2, 3, 700), SMALL, 0),
         ((1, "hard", 2, 4, 700), SMALL, 3), ((1, "silent_ch", 2, 4, 700), SMALL, 0),
         ((3, "silent_est", 1, 4, 700), SMALL, 0), ((2, "silent_est", 3, 3, 700), SMALL, 1)]


@pytest.fixture(scope="module")
def stats():
    """the float64 statistics of every case, formed once"""
    return [bd.item_statistics(*br.make_case(*case), **kw) for case, kw, _ in CASES]


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ------------------------------------------------------------------ 1. the restatement
def test_the_two_forms_agree(stats):
    """scipy.linalg.eigh on the generalised problem against the Cholesky whitening and the Jacobi iteration: 1e-11 of
    the largest weight (the silent estimates with n = 3 have three equal classes and no gap to speak of: both forms
    still take e_ref or the same filter only where the problem is well posed, so that case is left to the device's
    bit-for-bit test)"""
    worst = 0.0
    for (case, kw, ref), N in zip(CASES[:-1], stats):
        for kind in KINDS:
            a = bd.design_weights(N, case[2], ref, E32, R32, kind, form="jacobi")
            b = bd.design_weights(N, case[2], ref, E32, R32, kind, form="eigh")
            worst = max(worst, rel(a, b))
            assert rel(a, b) <= 1e-11, (case, kind, rel(a, b))
    for leak in (0.3, 0.6):
        mix, est, _ = br.sanity_case(leak=leak)
        N = bd.item_statistics(mix, est)
        for kind in KINDS:
            a, b = (bd.design_weights(N, 2, 0, E32, R32, kind, form=f) for f in ("jacobi", "eigh"))
            worst = max(worst, rel(a, b))
            assert rel(a, b) <= 1e-11, (leak, kind, rel(a, b))
    print(f"jacobi against eigh: at most {worst:.2e} of the largest weight")


def test_jacobi_converges_and_matches_eigh():
    """random Hermitian positive semidefinite 2 x 2 to 8 x 8 whose principal eigenvalue has a relative gap >= 1e-2, at
    the default ten sweeps: what is left off the diagonal is rounding (1e-14 ||G||: a few units in the last place per
    entry), and the phase-normalised principal eigenvector is numpy.linalg.eigh's within 1e-13 (rounding over the gap)"""
    g = np.random.default_rng(0)
    for C in range(2, 9):
        B = g.standard_normal((64, C, C + 2)) + 1j * g.standard_normal((64, C, C + 2))
        G = B @ np.swapaxes(B, 1, 2).conj()
        vals, vecs = np.linalg.eigh(G)
        keep = (vals[:, -1] - vals[:, -2]) / vals[:, -1] >= 1e-2
        mu, u, off = bd.jacobi(G[keep], bd.SWEEPS)
        assert off.max() <= 1e-14, (C, off.max())
        assert np.abs(mu / vals[keep, -1] - 1).max() <= 1e-14
        want = vecs[keep, :, -1]
        ph = np.einsum("fc,fc->f", want.conj(), u)
        assert np.abs(u * (ph.conj() / np.abs(ph))[:, None] - want).max() <= 1e-13, C
        assert np.abs(np.linalg.norm(u, axis=1) - 1).max() <= 1e-14
    tiny = np.array([[[1.0, 1e-300], [1e-300, 2.0]]], dtype=np.complex128)   # theta^2 overflows: t = 1 / (2 theta)
    mu, u, _ = bd.jacobi(tiny, 2)
    assert mu[0] == 2.0 and np.all(np.isfinite(u)) and abs(u[0, 1]) == 1.0
    skip = np.diag([3.0, 1.0, 0.0]).astype(np.complex128)[None]             # nothing to rotate: V stays I
    mu, u, _ = bd.jacobi(skip, 3)
    assert mu[0] == 3.0 and np.array_equal(u[0], [1.0, 0.0, 0.0])
    tie = np.eye(3, dtype=np.complex128)[None]                              # ties go to the lowest index
    assert np.array_equal(bd.jacobi(tie, 1)[1][0], [1.0, 0.0, 0.0])


def test_rank1_is_the_mvdr_filter_of_the_steering_estimate(stats):
    """w = A^-1 h / (h^H A^-1 h) conj(h_ref) by numpy.linalg.solve, with h = A v; v^H A v = 1"""
    for (case, kw, ref), N in zip(CASES[:4], stats):
        n = case[2]
        w = bd.design_weights(N, n, ref, E32, R32, "rank1")
        for i in range(n):
            A = bd.loaded(N, i, E32, R32)
            ok, v, h, mu = bd.principal(A, N[i])
            assert ok.all()
            assert np.abs(np.einsum("fc,fcd,fd->f", v.conj(), A, v) - 1).max() <= 1e-10
            assert rel(np.einsum("fcd,fd->fc", A, v), h) <= 1e-10
            z = np.linalg.solve(A, h[..., None])[..., 0]
            want = z / np.einsum("fc,fc->f", h.conj(), z)[:, None] * h[:, ref].conj()[:, None]
            assert rel(w[i], want) <= 1e-9, (case, i)
            # and the eigen-equation: N_i v = mu A v
            assert rel(np.einsum("fcd,fd->fc", N[i], v), mu[:, None] * h) <= 1e-9


def closed_forms(A, d, ref):
    z = np.linalg.solve(A, d[..., None])[..., 0]
    q = np.einsum("fc,fc->f", d.conj(), z).real
    rank1 = z / q[:, None] * d[:, ref].conj()[:, None]
    gev = z / q[:, None] * (d[:, ref].conj() / np.abs(d[:, ref]) * np.linalg.norm(d, axis=1)
                            / np.sqrt(d.shape[1]))[:, None]
    return {"rank1": rank1, "gev": gev}


def test_rank_one_statistics_give_the_closed_form(stats):
    """N_i = sigma d d^H: rank1 is A^-1 d / (d^H A^-1 d) conj(d_ref), gev the same vector with the BAN gain; d the
    all-ones vector ("dual": every channel carries the same signal), a unit vector ("hard": the source is in one
    channel) and a random one, and the "dual" mixtures of make_case themselves"""
    g = np.random.default_rng(1)
    bins, C = 9, 4
    B = g.standard_normal((bins, C, C)) + 1j * g.standard_normal((bins, C, C))
    Q = B @ np.swapaxes(B, 1, 2).conj()
    for d, ref in ((np.ones(C), 2), (np.eye(C)[1], 1), (g.standard_normal(C) + 1j * g.standard_normal(C), 0)):
        d = np.broadcast_to(d.astype(np.complex128), (bins, C))
        N = np.stack([3.0 * d[:, :, None] * d[:, None, :].conj(), Q])
        want = closed_forms(bd.loaded(N, 0, E32, R32), d, ref)
        for kind in KINDS:
            for form in ("jacobi", "eigh"):
                got = bd.design_weights(N, 1, ref, E32, R32, kind, form=form)[0]
                assert rel(got, want[kind]) <= 1e-10, (kind, form, ref)
    (case, kw, ref), N = CASES[5], stats[5]
    assert case[1] == "dual"
    for i in range(2):
        want = closed_forms(bd.loaded(N, i, E32, R32), np.ones((N.shape[1], 3), dtype=np.complex128), ref)
        for kind in KINDS:
            assert rel(bd.design_weights(N, 2, ref, E32, R32, kind)[i], want[kind]) <= 1e-9, (kind, i)


def test_the_phase_of_u_does_not_reach_the_weights(stats):
    g = np.random.default_rng(2)
    for (case, kw, ref), N in zip(CASES[:3], stats):
        phase = g.uniform(-np.pi, np.pi, N.shape[1])
        for kind in KINDS:
            a = bd.design_weights(N, case[2], ref, E32, R32, kind)
            b = bd.design_weights(N, case[2], ref, E32, R32, kind, phase=phase)
            assert rel(b, a) <= 1e-13, (case, kind)


def test_fallbacks(stats):
    N = stats[0].copy()
    w = bd.design_weights(N[:, :, :1, :1], 2, 0, E32, R32, "gev")
    assert np.all(w == 1.0)                                                  # one channel
    silent = np.stack([np.zeros_like(N[0]), N[1]])
    for kind in KINDS:
        for form in ("jacobi", "eigh"):
            w = bd.design_weights(silent, 2, 1, E32, R32, kind, form=form)
            assert np.array_equal(w[0], np.broadcast_to([0.0, 1.0], w[0].shape))   # mu = 0: e_ref
            assert np.all(np.isfinite(w[1]))
    bad = N.copy()
    bad[1, 3] = np.nan                                                       # a NaN class: its bin falls back in both
    with np.errstate(all="ignore"):
        w = bd.design_weights(bad, 2, 0, E32, R32, "rank1")
    assert np.array_equal(w[:, 3], np.broadcast_to([1.0, 0.0], (2, 2)))
    assert np.array_equal(np.delete(w, 3, axis=1), np.delete(bd.design_weights(N, 2, 0, E32, R32, "rank1"), 3, axis=1))


def test_no_design_and_souden_are_the_beamformer_restated():
    mix, est = br.make_case(4, "generic", 2, 3, 900)
    N = bd.item_statistics(mix, est, **SMALL)
    want = br.weights(N, 1, E32, R32)
    for kind in (None, "souden"):
        assert np.array_equal(bd.design_weights(N, 2, 1, E32, R32, kind), want)
        assert np.array_equal(bd.beamform(mix, est, design=kind, ref=1, **SMALL), br.beamform(mix, est, ref=1, **SMALL))
    assert br.weights is bd._souden                                          # the substitution is undone
    out = bd.beamform(mix, est, design="rank1", ref=1, **SMALL)
    assert not np.array_equal(out, br.beamform(mix, est, ref=1, **SMALL))
    assert br.weights is bd._souden
    # the yardstick run: float32 transforms, float64 design
    out32 = bd.beamform(mix, est, design="rank1", ref=1, dtype=np.float32, **SMALL)
    assert out32.dtype == np.float32 and 0 < br.rel_err(out32, out, mix) < 1e-4


# SI-SDR in dB against the images at channel 0, source 0 / source 1: the README's table
SANITY = {0.3: dict(souden=(19.15, 14.21), rank1=(25.01, 10.06), gev=(10.13, 8.02)),
          0.6: dict(souden=(11.89, 9.91), rank1=(21.94, 11.57), gev=(9.97, 8.67))}


@pytest.mark.parametrize("leak", sorted(SANITY))
def test_sanity_table(leak):
    """beamform_restatement.sanity_case (4 channels, 2 burst-noise sources, 512 / 128) within 0.05 dB, losses included;
    its smallest eigenvalue gap is what tests/test_gpu_beamform_design.py's condition was checked against"""
    mix, est, img0 = br.sanity_case(leak=leak)
    for kind, want in SANITY[leak].items():
        out = bd.beamform(mix, est, design=kind)
        got = [br.si_sdr(out[i], img0[i]) for i in range(2)]
        print(f"leak {leak} {kind}: {got[0]:.2f} / {got[1]:.2f} dB")
        assert max(abs(a - b) for a, b in zip(got, want)) <= 0.05, (leak, kind, got)
    gap = float(bd.gaps(bd.item_statistics(mix, est), 2, E32, R32).min())
    assert abs(gap - {0.3: 0.036, 0.6: 0.023}[leak]) < 1e-3


def test_pack_is_the_layout_of_the_solver():
    g = np.random.default_rng(3)
    B = g.standard_normal((2, 5, 3, 3)) + 1j * g.standard_normal((2, 5, 3, 3))
    N = B @ np.swapaxes(B, -1, -2).conj()
    P = bd.pack(N, 4)
    assert P.shape == (2, 20, 5)
    at = lambda c1, c2: 2 * (c1 * 4 - c1 * (c1 - 1) // 2 + (c2 - c1))
    assert np.array_equal(P[:, at(1, 2)], N[:, :, 1, 2].real) and np.array_equal(P[:, at(1, 2) + 1], N[:, :, 1, 2].imag)
    assert np.array_equal(P[:, at(2, 2)], N[:, :, 2, 2].real) and np.all(np.isnan(P[:, at(0, 3)]))
    assert np.all(np.isnan(P[:, at(3, 3)]))


# ------------------------------------------------------------------ 2. options, merges and refusals
def test_design_options():
    assert native.DESIGN_DEFAULTS == dict(kind="rank1", sweeps=10)
    assert native.BEAMFORM_DESIGNS == dict(souden=0, rank1=1, gev=2) and native.BEAMFORM_MAX_SWEEPS == 30
    assert native.design_options(None) is None and native.check_design(None) is None
    for kind, code in native.BEAMFORM_DESIGNS.items():
        assert native.design_options(kind) == dict(kind=kind, sweeps=10)
        assert native.check_design(kind) == (code, 10)
    assert native.design_options({}) == native.DESIGN_DEFAULTS
    assert native.design_options(dict(sweeps=3)) == dict(kind="rank1", sweeps=3)
    assert native.check_design(dict(kind="gev", sweeps=30)) == (2, 30)
    opts = native.design_options("gev")
    opts["sweeps"] = 1
    assert native.DESIGN_DEFAULTS["sweeps"] == 10                            # a copy
    for bad, msg in ((True, "design must be None, 'rank1', 'gev', 'souden' or a dict"), (False, "design must be"),
                     ("mvdr", "design must be"), (1, "design must be"), (dict(kind="mpdr"), "design: kind must be one of"),
                     (dict(kind=1), "design: kind must be one of"), (dict(rank=1), r"design: unknown keys \['rank'\]"),
                     (dict(sweeps=0), r"design: sweeps = 0 outside \[1, 30\]"),
                     (dict(sweeps=31), r"design: sweeps = 31 outside \[1, 30\]"),
                     (dict(sweeps=2.0), r"design: sweeps = 2.0 outside"), (dict(sweeps=True), "design: sweeps = True")):
        with pytest.raises(ValueError, match=msg):
            native.design_options(bad)


def test_the_merge_and_the_existing_helpers():
    """design_beamform_keywords adds one key; what the existing helpers return without it is what it was"""
    assert native.BEAMFORM_DEFAULTS == dict(ref=0, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, postfilter=None)
    beam, spat, trk = native.beamform_options(2), native.spatial_options(True), native.track_options(True)
    assert beam == dict(native.BEAMFORM_DEFAULTS, ref=2)
    assert native.design_beamform_keywords(beam, None) is beam and native.design_beamform_keywords(None, None) is None
    with pytest.raises(ValueError, match="design= picks the filter of the beamformer: it needs beamform="):
        native.design_beamform_keywords(None, native.design_options("gev"))
    des = native.design_options(dict(kind="gev", sweeps=4))
    merged = native.design_beamform_keywords(beam, des)
    assert merged == dict(beam, design=des) and "design" not in beam and merged["design"] is not des
    plain_s, plain_t = native.spatial_beamform_keywords(beam, spat), native.track_beamform_keywords(beam, trk, 16000)
    assert "design" not in plain_s and "design" not in plain_t
    assert plain_s == dict(ref=2, n_fft=512, hop=128, power=2, eps=1e-10, reg=1e-3, iterations=1, noise=0.1, floor=0.1,
                           mask_reg=1e-3, mask_eps=1e-10)
    assert plain_t == dict(beam, block_frames=100, context=1, interpolate=True)
    assert native.spatial_beamform_keywords(merged, spat) == dict(plain_s, design=des)
    assert native.track_beamform_keywords(merged, trk, 16000) == dict(plain_t, design=des)
    assert native.spatial_beamform_keywords(merged, None) == merged
    # every key of the merged dicts is a keyword of the engine call it goes to
    for fn, kw in ((native.Engine.beamform, merged), (native.Engine.beamform_spatial, dict(plain_s, design=des)),
                   (native.Engine.beamform_track, dict(plain_t, design=des))):
        params = inspect.signature(fn).parameters
        assert set(kw) <= set(params) and params["design"].default is None
    assert native.check_beamform((1, 3, 600), (1, 2, 600))[3] == 0           # (untouched: no design in its signature)
    assert "design" not in inspect.signature(native.check_beamform).parameters


def test_keyword_refusals(tmp_path):
    m = object.__new__(LatentDiffSep)           # no engine to touch: the refusals come first
    m.engine = None
    mix, clips = torch.zeros(1, 3, 4000), [torch.zeros(3, 4000)]
    calls = (lambda **kw: m.separate(mix, **kw), lambda **kw: m.separate_batch(clips, **kw),
             lambda **kw: m.separate_long(clips, 2048, **kw), lambda **kw: m.separate_long(clips, 2048, mode="score", **kw))
    for call in calls:
        with pytest.raises(ValueError, match="design= picks the filter of the beamformer: it needs beamform="):
            call(design="gev")
        with pytest.raises(ValueError, match="design= picks the filter of the beamformer: it needs beamform="):
            call(design="rank1", stems="mask")
        with pytest.raises(ValueError, match="beamform= does not go with stems="):
            call(design="rank1", beamform=True, stems="mask")
        with pytest.raises(ValueError, match="beamform= does not go with intermediate"):
            call(design="rank1", beamform=True, intermediate=True)
        with pytest.raises(ValueError, match="design must be None, 'rank1', 'gev', 'souden' or a dict"):
            call(design=True, beamform=True)
        with pytest.raises(ValueError, match=r"design: sweeps = 40 outside \[1, 30\]"):
            call(design=dict(sweeps=40), beamform=True)
        with pytest.raises(ValueError, match="track= does not go with spatial="):
            call(design="gev", beamform=True, spatial=True, track=True)
    with pytest.raises(ValueError, match="beamform= filters waveforms: with latent=True"):
        m.separate(mix, design="gev", beamform=True, latent=True)

    class NoDevice:
        engine, hop_length, n_src = None, 8, 2

        def _model_rate(self, what):
            return 16000

    for kw, msg in ((dict(design="gev"), "design= picks the filter of the beamformer: it needs beamform="),
                    (dict(design="gev", beamform=True, stems="mask"), "beamform= does not go with stems="),
                    (dict(design="best", beamform=True), "design must be"),
                    (dict(design=dict(kind="gev", sweeps=0), beamform=True), r"design: sweeps = 0 outside \[1, 30\]")):
        with pytest.raises(ValueError, match=msg):
            files.separate_files(NoDevice(), [tmp_path / "a.wav"], tmp_path / "never", **kw)
    assert not (tmp_path / "never").exists()
    # a call that is in order passes every check made before the device is touched (the beamformer's stand-in check
    # among them, which takes no design) and ends at the missing engine
    from ditsep_amd import wavio
    wavio.write_wav(tmp_path / "a.wav", (0.3 * np.random.default_rng(0).standard_normal(4 * 900) * 2 ** 15)
                    .astype("<i2").tobytes(), 16000, 4, "s16")
    for extra in (dict(), dict(track=True), dict(spatial=True)):
        with pytest.raises((AttributeError, RuntimeError)):
            files.separate_files(NoDevice(), [tmp_path / "a.wav"], tmp_path / "never",
                                 beamform=dict(ref=1, n_fft=128, hop=32), design="gev", **extra)
    for fn in (LatentDiffSep.separate, LatentDiffSep.separate_batch, LatentDiffSep.separate_long,
               LatentDiffSep.separate_files, files.separate_files, native.Engine.beamform,
               native.Engine.beamform_spatial, native.Engine.beamform_track):
        assert inspect.signature(fn).parameters["design"].default is None


def test_symbols_declared_exported_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ditsep_hip.h")).read()
    assert "enum { DSN_BEAMFORM_DESIGN_SOUDEN = 0, DSN_BEAMFORM_DESIGN_RANK1 = 1, DSN_BEAMFORM_DESIGN_GEV = 2 };" in hdr
    flat = re.sub(r"\s+", " ", hdr)
    for name, count in (("dsn_beamform_design", 22), ("dsn_beamform_spatial_design", 28),
                        ("dsn_beamform_track_design", 25)):
        old = re.search(r"\bint %s\(([^;]*)\);" % name[:-len("_design")], flat).group(1)
        new = re.search(r"\bint %s\(([^;]*)\);" % name, flat).group(1)
        assert new == old.replace("float reg,", "float reg, int design, int sweeps,"), name
        assert len(new.split(",")) == count
    assert ("int dsn_beamform_solve(dsn_ctx* ctx, const double* N, const int32_t* channels, int ref, int items, int C, "
            "int n, int classes, int bins, float reg, float eps, int design, int sweeps, double* w, void* stream);") in flat
    lib = native.load_library()
    for name, count in (("dsn_beamform_design", 22), ("dsn_beamform_spatial_design", 28),
                        ("dsn_beamform_track_design", 25), ("dsn_beamform_solve", 15)):
        assert name in native.EXPORTS and hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == count
    for name in ("dsn_beamform", "dsn_beamform_spatial", "dsn_beamform_track"):   # the old ones are what they were
        assert len(getattr(lib, name).argtypes) == len(getattr(lib, name + "_design").argtypes) - 2
    src = open(os.path.join(root, "ditsep_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bbeamform_design\.hip\b", src, flags=re.M)
    assert os.path.exists(os.path.join(root, "ditsep_amd", "csrc", "beamform_design.hip"))


def test_command_line_flags():
    p = separate.build_parser()
    base = ["in", "out", "--config", "c.json"]
    a = p.parse_args(base + ["--beamform"])
    assert a.beamform_design is None and separate.design_of(a) is None
    assert separate.beamform_of(a) == dict(ref=0, n_fft=512, hop=128, reg=1e-3, postfilter=None)
    a = p.parse_args(base + ["--beamform", "--beamform-design", "rank1"])
    assert separate.design_of(a) == native.DESIGN_DEFAULTS == native.design_options(separate.design_of(a))
    a = p.parse_args(base + ["--beamform", "--beamform-design", "gev", "--beamform-sweeps", "4"])
    assert separate.design_of(a) == dict(kind="gev", sweeps=4)
    a = p.parse_args(base + ["--beamform-sweeps", "4"])                      # sweeps alone ask for nothing
    assert separate.design_of(a) is None
    for bad in (["--beamform-design", "souden"], ["--beamform-design", "mvdr"], ["--beamform-sweeps", "1.5"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)
