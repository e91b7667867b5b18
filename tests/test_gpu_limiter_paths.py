"""The `limit` keyword: Engine.loudness_normalize(limit=) on the burst input of tests/limiter_restatement.py against the
float64 restatement and against the public calls done by hand, and LatentDiffSep.separate / separate_batch /
separate_long / separate_files with the tiny model of tests/test_gpu_separate_files.py (hop 8, fs = 16000, bf16x3):
None is the call without the keyword to the bit and to the byte, True is the calls by hand.

The input: two sources of burst noise, 4 s at 16 kHz, peak 0.3 each; target -12 LUFS under a ceiling of -1 dBTP.  A
single gain falls short of that target by more than 3 LU (the restatement says so first); the limiter reaches it
within the +-0.1 LU meter tolerance of EBU Tech 3341 in three evaluations, with about 4 dB of reduction at the peaks."""
import math

import numpy as np
import pytest
import torch

from ditsep_amd import native, wavio
from tests import limiter_restatement as lim
from tests import pcm_restatement as pr
from tests.util import make_engine

pytestmark = pytest.mark.gpu

FS = 16000
N_STEPS = 4
TARGET, PEAK = -12.0, -1.0
CEIL = float(np.float32(10.0 ** (PEAK / 20.0)))


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def burst():
    """-> (stems [2, L] float32, mixture [1, L], the restatement of the keyword on them)"""
    s = lim.burst_sources(fs=FS)
    mix = s.sum(0, keepdims=True)
    res = lim.normalize(s[:, None, :], mix, FS, TARGET, PEAK, limit={})
    return torch.from_numpy(s), torch.from_numpy(mix), res


def lin(db):
    return float(np.float32(10.0 ** (db / 20.0)))


def by_hand(eng, mix, est, rate, target=-23.0, peak=-1.0, link="mixture", limit=True):
    """the two keywords' step for one item from the public calls: mix [C', L] (or None), est [n, L] or [n, C, L] ->
    (tensor shaped like est, a dict of per-stem lists)"""
    opt = native.limit_options(limit)
    kw = dict(drive_db=opt["drive_db"], iterations=opt["iterations"], tol=opt["tol"])
    n, L = int(est.shape[0]), int(est.shape[-1])
    rows = est.reshape(n, -1, L).cuda().float()
    st = eng.loudness(rows, [rate] * n)
    if target is None:
        I = st["loudness"].tolist()
        g = {"gain_db": [0.0] * n, "gain": [1.0] * n, "limited": [True] * n}
        groups = [list(range(n))] if link == "mixture" else [[i] for i in range(n)]
    elif link == "mixture":
        I = eng.loudness(mix.reshape(-1, mix.shape[-1]), rate, true_peak=False)["loudness"].tolist() * n
        g = native.loudness_gain(I, st["true_peak"].tolist(), [0] * n, target, peak)
        groups = [list(range(n))]
    else:
        I = st["loudness"].tolist()
        g = native.loudness_gain(I, st["true_peak"].tolist(), None, target, peak)
        groups = [[i] for i in range(n)]
    out = rows.clone() if target is None else eng.apply_gain(rows, g["gain"])
    info = {"gain_db": list(g["gain_db"]), "loudness_out": [a + b for a, b in zip(I, g["gain_db"])],
            "reached": [True] * n, "evaluations": [0] * n, "reduction_db": [0.0] * n, "limited_samples": [0] * n}
    c_db = opt["ceiling"] if opt["ceiling"] is not None else (peak if peak is not None else -1.0)
    c = lin(c_db)
    for q in groups:
        if not g["limited"][q[0]]:
            continue
        xs, grp = rows[q].contiguous(), [0] * len(q)
        hist, cur = [], 0.0
        if target is not None:
            if link == "mixture":
                prog = torch.zeros((1, mix.reshape(-1, mix.shape[-1]).shape[0], L), device="cuda")
                v = min(L, int(mix.shape[-1]))
                prog[0, :, :v] = mix.reshape(-1, mix.shape[-1])[:, :v]
            else:
                prog = xs
            G = native.limiter_drive(g["gain_db"][q[0]], I[q[0]], target, [], **kw)
            while G is not None:
                curve, _ = eng.limiter_curve(xs, rate, grp, [lin(G)], c, opt["lookahead_ms"])
                y = eng.apply_curve(prog, [0], [lin(G)], curve)
                hist.append((G, float(eng.loudness(y, rate, true_peak=False)["loudness"][0])))
                G = native.limiter_drive(g["gain_db"][q[0]], I[q[0]], target, hist, **kw)
            cur, loud = hist[native.limiter_best(hist, target)]
        curve, cs = eng.limiter_curve(xs, rate, grp, [lin(cur)], c, opt["lookahead_ms"])
        y = eng.apply_curve(xs, grp, [lin(cur)], curve)
        m = eng.loudness(y, [rate] * len(q))
        if target is None:
            loud = float(m["loudness"][0])
        trim, final, tp = 1.0, y, m["true_peak"].tolist()
        for _ in range(3):
            if max(tp) <= c:
                break
            trim = float(np.float32(trim * (c / max(tp))))
            final = eng.apply_gain(y, [trim] * len(q))
            tp = eng.loudness(final, [rate] * len(q))["true_peak"].tolist()
        out[q] = final
        for k, r in enumerate(q):
            info["gain_db"][r] = cur + 20.0 * math.log10(trim)
            info["loudness_out"][r] = loud + 20.0 * math.log10(trim)
            info["reached"][r] = True if target is None else abs(target - info["loudness_out"][r]) <= opt["tol"]
            info["evaluations"][r] = max(len(hist), 1)
            info["reduction_db"][r] = 20.0 * math.log10(float(cs["min_gain"][0]))
            info["limited_samples"][r] = int(cs["limited_samples"][0])
    info["limited"] = list(g["limited"])
    return out.reshape(est.shape), info


NEW_KEYS = ("reached", "evaluations", "reduction_db", "limited_samples")


# ---------------------------------------------------------------------------------------------- the Engine's step
def test_a_single_gain_cannot_reach_the_target(burst):
    _, _, res = burst
    assert res["limited"] and TARGET - res["single"]["loudness_out"] > 1.0
    # .. and the restated limiter gets there within the default number of evaluations
    assert len(res["history"]) <= lim.DEFAULTS["iterations"] and abs(res["loudness_out"] - TARGET) <= lim.DEFAULTS["tol"]
    print(f"restatement: single gain reaches {res['single']['loudness_out']:.3f} LUFS; limiter history {res['history']}, "
          f"deepest g {20 * math.log10(res['min_gain']):.2f} dB, overshoot before the trim {res['overshoot']:.3e}")


def test_the_limiter_reaches_it(eng, burst):
    stems, mix, res = burst
    old, old_info = eng.loudness_normalize([mix], [stems], FS, target=TARGET, peak=PEAK)
    assert old_info["limited"] == [[True, True]] and TARGET - old_info["loudness_out"][0][0] > 1.0
    assert not any(k in old_info for k in NEW_KEYS)
    outs, info = eng.loudness_normalize([mix], [stems], FS, target=TARGET, peak=PEAK, limit=True)
    out = outs[0]
    print({k: info[k] for k in ("loudness_in", "loudness_out", "gain_db", "true_peak_db") + NEW_KEYS})
    assert info["reached"] == [[True, True]]
    assert abs(info["loudness_out"][0][0] - TARGET) <= native.LIMIT_DEFAULTS["tol"]
    assert info["evaluations"][0][0] == len(res["history"]) <= native.LIMIT_DEFAULTS["iterations"]
    assert info["gain_db"][0][0] == info["gain_db"][0][1] and info["loudness_out"][0][0] == info["loudness_out"][0][1]
    assert -6.0 < info["reduction_db"][0][0] < -1.0 and info["limited_samples"][0][0] > 0
    # the restatement's figures: the device's loudness is within 1e-6 LU of float64's, the curves within their bound
    assert abs(info["gain_db"][0][0] - (res["history"][res["kept"]][0] + 20 * math.log10(res["trim"]))) <= 1e-3
    assert abs(info["loudness_out"][0][0] - res["loudness_out"]) <= 1e-3
    assert abs(info["reduction_db"][0][0] - 20 * math.log10(res["min_gain"])) <= 1e-3
    assert float((out.cpu().double() - torch.from_numpy(res["out"][:, 0])).abs().max()) <= 1e-5
    # measured again: the ceiling holds after the trim, and the limited mixture is at the target
    again = eng.loudness(out[:, None], [FS] * 2)
    tp = float(again["true_peak"].max())
    print(f"true peak after the trim {tp:.9f}, ceiling {CEIL:.9f}, ratio - 1 = {tp / CEIL - 1.0:.3e}")
    assert tp <= CEIL * (1.0 + 2.0 ** -23)
    assert max(info["true_peak_db"][0]) == 20.0 * math.log10(tp)
    whole = eng.loudness(out.sum(0)[None, None], FS, true_peak=False)
    assert abs(float(whole["loudness"][0]) - info["loudness_out"][0][0]) <= 1e-4
    assert abs(float(whole["loudness"][0]) - TARGET) <= native.LIMIT_DEFAULTS["tol"]
    # .. and it is the public calls done by hand
    want, winfo = by_hand(eng, mix, stems, FS, TARGET, PEAK)
    assert torch.equal(out, want)
    for k in ("gain_db", "loudness_out") + NEW_KEYS:
        assert info[k][0] == winfo[k], k


def test_a_reachable_target_returns_the_bits_without_the_keyword(eng, burst):
    stems, mix, _ = burst
    a, ia = eng.loudness_normalize([mix], [stems], FS, target=-23.0, peak=PEAK)
    b, ib = eng.loudness_normalize([mix], [stems], FS, target=-23.0, peak=PEAK, limit=True)
    assert ia["limited"] == [[False, False]] and torch.equal(a[0], b[0])
    for k in ia:
        assert ia[k] == ib[k], k
    assert ib["reached"] == [[True, True]] and ib["evaluations"] == [[0, 0]] and ib["reduction_db"] == [[0.0, 0.0]]
    assert ib["limited_samples"] == [[0, 0]]


def test_stem_link_and_a_batch_of_items(eng, burst):
    """two items in one call -- one that the single gain serves, one stereo at another rate that it does not -- and
    link "stem": every stem its own curve.  Each item is what it is alone, by hand."""
    stems, mix, _ = burst
    t = torch.arange(30000, dtype=torch.float64) / 44100.0
    quiet = torch.stack([0.05 * torch.sin(2 * math.pi * f * t) for f in (440.0, 587.0, 659.0, 880.0)]).float()
    quiet = quiet.reshape(2, 2, -1)                                     # sines: 15 dB of gain leaves their peaks at 0.3
    loud = torch.from_numpy(lim.burst_sources(fs=8000, seconds=2.0, seed=3))[:, None, :].repeat(1, 2, 1)
    loud[:, 1] *= -0.5
    items, mixes, rates = [quiet, loud, stems], [quiet.sum(0), loud.sum(0), mix], [44100, 8000, FS]
    for link, target in (("mixture", -14.0), ("stem", -17.0)):
        outs, info = eng.loudness_normalize(mixes, items, rates, target=target, peak=PEAK, link=link, limit=True)
        assert any(any(v) for v in info["limited"]) and not all(all(v) for v in info["limited"])
        for b in range(3):
            want, winfo = by_hand(eng, mixes[b], items[b], rates[b], target, PEAK, link)
            assert torch.equal(outs[b], want), (link, b)
            for k in ("gain_db", "loudness_out", "limited") + NEW_KEYS:
                assert info[k][b] == winfo[k], (link, b, k)
            tp = eng.loudness(outs[b].reshape(2, -1, outs[b].shape[-1]), [rates[b]] * 2)["true_peak"]
            assert float(tp.max()) <= CEIL * (1.0 + 2.0 ** -23)
        print(link, {k: info[k] for k in ("loudness_out", "limited") + NEW_KEYS})


def test_limit_without_loudness_is_one_evaluation_at_0_db(eng, burst):
    stems, mix, _ = burst
    opts = dict(ceiling=-14.0)
    outs, info = eng.loudness_normalize(None, [stems], FS, target=None, peak=None, limit=opts)
    c = lin(-14.0)
    curve, st = eng.limiter_curve(stems[:, None], FS, [0, 0], [1.0], c, 5.0)
    y = eng.apply_curve(stems[:, None], [0, 0], [1.0], curve)[:, 0]
    tp = eng.loudness(outs[0][:, None], [FS] * 2)["true_peak"]
    assert float(tp.max()) <= c * (1.0 + 2.0 ** -23)
    trim = 10.0 ** (info["gain_db"][0][0] / 20.0)
    assert 1.0 - 1e-5 < trim <= 1.0 and info["evaluations"] == [[1, 1]] and info["reached"] == [[True, True]]
    assert torch.equal(outs[0], y if trim == 1.0 else eng.apply_gain(y[:, None], [float(np.float32(trim))] * 2)[:, 0])
    assert info["limited_samples"][0][0] == int(st["limited_samples"][0]) > 0
    want, winfo = by_hand(eng, None, stems, FS, None, None, limit=opts)
    assert torch.equal(outs[0], want)
    with pytest.raises(ValueError, match="needs limit="):
        eng.loudness_normalize(None, [stems], FS, target=None)
    with pytest.raises(ValueError, match="unknown keys"):
        eng.loudness_normalize([mix], [stems], FS, limit={"target": -14.0})


# ---------------------------------------------------------------------------------------------- the entry points
@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    import json

    from ditsep_amd import LatentDiffSep
    from oracle import dit as odit
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights

    tmp = tmp_path_factory.mktemp("limit")
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


@pytest.fixture(scope="module")
def mix():
    return 0.2 * torch.randn((2, 1, 8000), generator=torch.Generator().manual_seed(7))


def clip_of(path, h):
    return torch.from_numpy(pr.decode(wavio.read_payload(path, h), h.frames, h.channels, h.encoding))


def floats_of(path):
    h = wavio.read_header(path)
    assert h.encoding == "f32"
    x = np.frombuffer(wavio.read_payload(path, h), dtype="<f4").reshape(h.frames, h.channels).T
    return h, torch.from_numpy(np.array(x, dtype=np.float32, order="C"))


LOUD = dict(target=-6.0, peak=-1.0)          # white noise has a crest factor no single gain takes to -6 LUFS


def test_none_returns_the_bits_of_the_call_without_the_keyword(setup, mix):
    m = setup["model"]
    a, nfe = m.separate(mix, seed=3, loudness=LOUD)
    b, _ = m.separate(mix, seed=3, loudness=LOUD, limit=None)
    assert torch.equal(a, b) and nfe == 2 * N_STEPS
    a, _ = m.separate(mix, seed=3)
    b, _ = m.separate(mix, seed=3, limit=None)
    assert torch.equal(a, b)
    clips = [mix[0], mix[1, :, :7001]]
    a, _ = m.separate_batch(clips, codec="padded", seed=4)
    b, _ = m.separate_batch(clips, codec="padded", seed=4, limit=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a, _ = m.separate_long(mix[0], 4096, seed=5)
    b, _ = m.separate_long(mix[0], 4096, seed=5, limit=None)
    assert torch.equal(a, b)


def test_separate_with_limit_is_the_calls_by_hand(setup, mix):
    m = setup["model"]
    eng = m.engine
    est, _ = m.separate(mix, seed=3)
    got, _, info = m.separate(mix, seed=3, loudness=LOUD, limit=True, return_info=True)
    assert info["limited"] == [[True, True], [True, True]]
    plain = m.separate(mix, seed=3, loudness=LOUD, return_info=True)[2]
    for b in range(2):
        want, winfo = by_hand(eng, mix[b], est[b], FS, **LOUD)
        assert torch.equal(got[b], want)
        for k in ("gain_db", "loudness_out") + NEW_KEYS:
            assert info[k][b] == winfo[k], k
        assert info["evaluations"][b][0] >= 1 and info["reduction_db"][b][0] < 0.0
        # closer to the target than the single gain gets (how much closer is the material's business: noise-like
        # estimates have peaks everywhere, and the drive stops at 6 dB)
        assert LOUD["target"] > info["loudness_out"][b][0] > plain["loudness_out"][b][0]
    # without loudness=: one pass at 0 dB against the limiter's own ceiling
    got, _, info = m.separate(mix, seed=3, limit=dict(ceiling=-30.0), return_info=True)
    for b in range(2):
        want, _ = by_hand(eng, None, est[b], FS, None, None, limit=dict(ceiling=-30.0))
        assert torch.equal(got[b], want) and info["limited_samples"][b][0] > 0


def test_separate_batch_and_long_with_limit(setup, mix):
    m = setup["model"]
    eng = m.engine
    clips = [mix[0], mix[1, :, :7001]]
    est, _ = m.separate_batch(clips, codec="padded", seed=4)
    got, _, info = m.separate_batch(clips, codec="padded", seed=4, loudness=dict(LOUD, link="stem"), limit=True,
                                    return_info=True)
    for b in range(2):
        want, winfo = by_hand(eng, clips[b], est[b], FS, link="stem", **LOUD)
        assert torch.equal(got[b], want) and info["reached"][b] == winfo["reached"]
    est, _ = m.separate_long(mix[0], 4096, seed=5)
    got, _ = m.separate_long(mix[0], 4096, seed=5, loudness=LOUD, limit=dict(iterations=2))
    want, winfo = by_hand(eng, mix[0], est, FS, limit=dict(iterations=2), **LOUD)
    assert torch.equal(got, want) and winfo["evaluations"][0] <= 2


def test_separate_files_with_limit(setup):
    """f32 outputs hold the very floats: the files written with limit= are the calls by hand on the files written
    without; with s16 the bytes are the quantiser's of those"""
    m, paths, hs = setup["model"], setup["paths"], setup["headers"]
    eng = m.engine
    o1, o2, o3, o4 = (setup["tmp"] / d for d in ("plain", "limit", "limit16", "loud"))
    r1 = m.separate_files(paths, o1, batch=2, seed=5, encoding="f32")
    r2 = m.separate_files(paths, o2, batch=2, seed=5, encoding="f32", loudness=LOUD, limit=True)
    r3 = m.separate_files(paths, o3, batch=2, seed=5, loudness=LOUD, limit=True)
    r4 = m.separate_files(paths, o4, batch=2, seed=5, encoding="f32", loudness=LOUD)
    for i, (a, b, c, d) in enumerate(zip(r1, r2, r3, r4)):
        stems = torch.stack([floats_of(p)[1][0] for p in a["outputs"]])               # [n, frames]
        want, winfo = by_hand(eng, clip_of(paths[i], hs[i]), stems, hs[i].rate, **LOUD)
        got = torch.stack([floats_of(p)[1][0] for p in b["outputs"]])
        assert torch.equal(got, want.cpu())
        assert set(b) - set(d) == set(NEW_KEYS) and set(d) - set(a) == {"loudness_in", "loudness_out", "gain_db",
                                                                         "true_peak_db"}
        for k in ("gain_db", "loudness_out") + NEW_KEYS:
            assert b[k] == winfo[k] == c[k], k
        assert b["evaluations"][0] >= 1 and b["limited_samples"][0] > 0
        payloads, clipped = eng.pcm_encode(want, [hs[i].frames] * 2, "s16")
        for s, p in enumerate(c["outputs"]):
            h = wavio.read_header(p)
            assert wavio.read_payload(p, h) == bytes(payloads[s]) and h.rate == hs[i].rate
        assert c["clipped"] == list(clipped)


def test_refusals(setup, mix):
    m = setup["model"]
    with pytest.raises(ValueError, match="latent=True"):
        m.separate(mix, latent=True, limit=True)
    with pytest.raises(ValueError, match="intermediate"):
        m.separate_batch([mix[0]], limit=True, intermediate=2)
    with pytest.raises(ValueError, match="limit must be"):
        m.separate(mix, limit=False)
    with pytest.raises(ValueError, match="unknown keys"):
        m.separate_files(setup["paths"], setup["tmp"] / "never", limit={"target": -14})
    assert not (setup["tmp"] / "never").exists()
