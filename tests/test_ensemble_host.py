"""The host side of the ensemble combine (no GPU): the float64 restatement's two alignments against each other and
against the constructed truth, native.ensemble_checks, the `samples` / `combine` keywords, the command line and the
file plan."""
import inspect
import math

import numpy as np
import pytest
import torch

from ditsep_amd import LatentDiffSep, files, native, wavio
from ditsep_amd import separate as cli
from tests import ensemble_restatement as er

CASES = [(K, n, L) for K in (1, 2, 3, 8, 16) for n in (1, 2, 3, 4) for L in (1, 3, 257, 600) if n <= L or L >= 257]


@pytest.mark.parametrize("K,n,L", CASES)
def test_the_two_alignments_agree_and_recover_the_truth(K, n, L):
    cands, mix, perms, _ = er.make_case(1000 * K + 10 * n + L, K, n, L)
    res = er.restate_item(cands, mix)
    assert er.margins_clear(res), (K, n, L, res["margins"])
    assert np.array_equal(res["perm"], res["perm_lsa"]) and res["anchor"] == res["anchor_lsa"]
    a = res["anchor"]
    for k in range(K):
        assert sorted(res["perm"][k]) == list(range(n))
        assert all(perms[k][res["perm"][k][i]] == perms[a][i] for i in range(n)), (k, res["perm"][k], perms[k], perms[a])
    assert np.array_equal(res["perm"][a], np.arange(n))
    # the figures lie in their own intervals, the anchor agrees with itself
    assert np.all(res["resid_db_lo"] <= res["resid_db"]) and np.all(res["resid_db"] <= res["resid_db_hi"])
    assert np.all(res["agree_db_lo"] <= res["agree_db"]) and np.all(res["agree_db"] <= res["agree_db_hi"])
    assert np.all(np.isposinf(res["agree_db"][a]))
    if K > 1 and L >= 257:
        others = np.delete(res["agree_db"], a, axis=0)
        assert np.all(others > 3.0) and np.all(others < 12.0)      # two rows with noise 10 dB below the source: ~7 dB
        assert np.all(np.abs(res["resid_db"] + 10.0) < 2.0)        # n noises 10 dB below n sources
    # the exact Gram and the float64 dot agree within the bound
    G2, _ = er.gram(np.concatenate([cands.reshape(K * n, L), mix[None]]), exact=False)
    assert np.all(np.abs(G2 - res["gram"]) <= res["bound"])


def test_restated_combine():
    c = np.array([[[1, 5, -0.0, 3]], [[3, 1, 0.0, 3]], [[2, 9, 7, 3]], [[8, 2, 1, 4]]], dtype=np.float32)
    assert np.array_equal(er.combine_rows(c, "mean"), np.array([[3.5, 4.25, 2, 3.25]], dtype=np.float32))
    assert np.array_equal(er.combine_rows(c, "median"), np.array([[2.5, 3.5, 0.5, 3]], dtype=np.float32))
    assert np.array_equal(er.combine_rows(c[:3], "median"), np.array([[2, 5, 0, 3]], dtype=np.float32))
    assert np.array_equal(er.combine_rows(c, "best", 2), c[2]) and np.array_equal(er.combine_rows(c[:1], "mean"), c[0])
    # ties go to the first permutation and the lowest index
    res = er.restate_item(np.ones((3, 2, 5), dtype=np.float32), np.ones(5, dtype=np.float32))
    assert res["perm"].tolist() == [[0, 1]] * 3 and res["anchor"] == 0 and res["best"] == 0
    assert not er.margins_clear(res)
    # a candidate that sums exactly to the mixture: no residual
    s = (np.arange(12, dtype=np.float32).reshape(2, 6) - 5) / 8
    res = er.restate_item(np.stack([s, s[::-1] + np.float32(0.25)]), s.sum(axis=0))
    assert res["best"] == 0 and res["resid_db"][0] == -math.inf and res["perm"].tolist() == [[0, 1], [1, 0]]
    # silent rows have no agreement figure, and no mixture no residual
    res = er.restate_item(np.zeros((2, 1, 4), dtype=np.float32))
    assert np.all(np.isnan(res["agree_db"])) and np.all(np.isnan(res["resid_db"])) and res["best"] == -1
    assert "best" not in res["out"]


def test_restated_mean_of_copies_is_the_copy():
    """K = 2, 4, 8, 16 copies of x: the two-sum gives the rounding errors back exactly and K x / K is x to the bit,
    subnormals and -0 included; the bare sequential float32 sum is not, from K = 8"""
    g = np.random.default_rng(3)
    x = np.concatenate([s * g.standard_normal(4000) for s in (0.3, 1e-38, 1e-44, 1e30)] + [[-0.0, 0.0]])
    x = x.astype(np.float32).reshape(1, -1)
    for K in (2, 4, 8, 16):
        out = er.combine_rows(np.stack([x] * K), "mean")
        assert np.array_equal(out.view(np.int32), x.view(np.int32)), K
    bare = x.copy()
    for _ in range(7):
        bare = bare + x
    assert not np.array_equal(bare / np.float32(8), x)
    # any data: one rounding of the sum and one of the division, plus the compensated sum's own second-order term
    # (15 2^-24)^2 sum |c_k| < 2^-40 sum |c_k| (Ogita, Rump and Oishi's bound for this summation)
    c = (0.3 * g.standard_normal((16, 2, 5000))).astype(np.float32)
    exact = c.astype(np.float64).sum(axis=0) / 16
    allow = 2.0 ** -23 * np.abs(exact) + 2.0 ** -40 * np.abs(c.astype(np.float64)).sum(axis=0)
    assert np.all(np.abs(er.combine_rows(c, "mean") - exact) <= allow)


def test_ensemble_checks_refuse_by_name():
    c = torch.zeros((2, 4, 2, 50))
    m = torch.zeros((2, 50))
    assert native.ensemble_checks(c, m, None, "median") == ((2, 4, 2, 50), None, native.ENSEMBLE_MODES["median"])
    assert native.ensemble_checks(c, m[:, None], [50, 1], "best") == ((2, 4, 2, 50), [50, 1], 2)
    assert native.ensemble_checks(c, None, None, "medoid")[2] == 3
    for kw, msg in ((dict(cands=torch.zeros((2, 17, 2, 50))), r"K = 17 outside \[1, 16\]"),
                    (dict(cands=torch.zeros((2, 0, 2, 50))), r"K = 0 outside \[1, 16\]"),
                    (dict(cands=torch.zeros((2, 4, 5, 50))), r"n = 5 outside \[1, 4\]"),
                    (dict(cands=torch.zeros((2, 4, 0, 50))), r"n = 0 outside \[1, 4\]"),
                    (dict(cands=torch.zeros((2, 4, 50))), r"cands must be float32 \[B, K, n, L\]"),
                    (dict(cands=c.double()), r"cands must be float32 \[B, K, n, L\]"),
                    (dict(mix=torch.zeros((2, 49))), r"mix must be \[B, L\] or \[B, 1, L\] with B = 2, L = 50"),
                    (dict(mix=torch.zeros((1, 50))), r"mix must be \[B, L\] or \[B, 1, L\]"),
                    (dict(mix=torch.zeros((2, 2, 50))), r"mix must be \[B, L\] or \[B, 1, L\]"),
                    (dict(mix=m.double()), r"mix must be float32 \(got torch.float64\)"),
                    (dict(mix=None, mode="best"), r"mode 'best' ranks the candidates by their residual.*mix is None"),
                    (dict(lens=[50, 0]), r"lens\[1\] = 0 outside \[1, Lmax = 50\]"),
                    (dict(lens=[51, 50]), r"lens\[0\] = 51 outside \[1, Lmax = 50\]"),
                    (dict(lens=[50]), r"one sample count per item \(B = 2\), got 1"),
                    (dict(mode="mode"), r"mode must be one of \['best', 'mean', 'median', 'medoid'\] \(got 'mode'\)")):
        with pytest.raises(ValueError, match=msg):
            native.ensemble_checks(**dict(dict(cands=c, mix=m, lens=None, mode="mean"), **kw))
    assert native.check_samples(4, "median") == 4 and native.check_samples(16) == 16
    for bad, msg in (((0,), "samples = 0 is not an int"), ((17,), "samples = 17 is not an int"),
                     ((2.5,), "samples = 2.5 is not an int"), ((True,), "samples = True is not an int"),
                     ((2, "mode"), "combine must be one of")):
        with pytest.raises(ValueError, match=msg):
            native.check_samples(*bad)
    assert "dsn_ensemble_combine" in native.EXPORTS


def test_keywords_and_their_defaults():
    for fn in (LatentDiffSep.separate, LatentDiffSep.separate_batch, LatentDiffSep.separate_files):
        p = inspect.signature(fn).parameters
        assert p["samples"].default is None and p["combine"].default == "mean", fn.__name__
    assert inspect.signature(files.separate_files).parameters["samples"].default is None
    assert "samples" not in inspect.signature(LatentDiffSep.separate_long).parameters
    p = inspect.signature(native.Engine.ensemble_combine).parameters
    assert [p[k].default for k in ("mix", "lens", "mode", "return_info")] == [None, None, "mean", False]


def test_command_line():
    p = cli.build_parser()
    a = p.parse_args(["in", "out", "--config", "c.json"])
    assert a.samples is None and a.combine == "mean"
    a = p.parse_args(["in", "out", "--config", "c.json", "--samples", "4", "--combine", "median"])
    assert a.samples == 4 and a.combine == "median"
    with pytest.raises(SystemExit):
        p.parse_args(["in", "out", "--config", "c.json", "--combine", "foo"])


def test_file_plan_with_samples(tmp_path):
    hs = [wavio.WavHeader(16000, 1, 1000 + 10 * i, "s16", 44, 2 * (1000 + 10 * i)) for i in range(10)]
    assert files.files_per_batch(8) == 8 and files.files_per_batch(8, 1) == 8
    for K, per in ((2, 4), (3, 2), (8, 1)):
        assert files.files_per_batch(8, K) == per == 8 // K
        plan = files.plan_files(hs, 16000, 8, batch=files.files_per_batch(8, K))
        assert max(len(b) for b in plan["batches"]) == per
        assert sorted(i for b in plan["batches"] for i in b) == list(range(10))
    with pytest.raises(ValueError, match="batch = 3 < samples = 4"):
        files.files_per_batch(3, 4)

    # separate_files refuses before any device work: the model below has no engine to touch
    class NoDevice:
        engine, hop_length, n_src = None, 8, 2

        def _model_rate(self, what):
            return 16000

    g = np.random.default_rng(3)
    for name, frames in (("a", 400), ("b", 16000 + 80)):
        wavio.write_wav(tmp_path / f"{name}.wav", (0.1 * g.standard_normal(frames) * 2 ** 15).astype("<i2").tobytes(),
                        16000, 1, "s16")
    paths = sorted(tmp_path.glob("*.wav"))
    with pytest.raises(ValueError, match=r"b\.wav is longer than long_after = 1.0 s .* samples= has no separate_long form"):
        files.separate_files(NoDevice(), paths, tmp_path / "never", samples=2, long_after=1.0)
    with pytest.raises(ValueError, match="batch = 3 < samples = 4"):
        files.separate_files(NoDevice(), paths, tmp_path / "never", samples=4, batch=3)
    with pytest.raises(ValueError, match="samples = 17 is not an int in"):
        files.separate_files(NoDevice(), paths, tmp_path / "never", samples=17)
    with pytest.raises(ValueError, match="combine must be one of"):
        files.separate_files(NoDevice(), paths, tmp_path / "never", samples=2, combine="vote")
    assert not (tmp_path / "never").exists()
