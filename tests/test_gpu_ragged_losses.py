"""GPU: the two losses on mixed-length batches -- dsn_mrstft_loss_ragged (Engine.mrstft_loss with lens=) and
dsn_score_loss_ragged (Engine.score_loss with frames=) -- and the list forms above them (LDM.losses_gen,
evaluate_batches).  The yardstick is per item: what the float64 restatements give the item alone
(tests/ragged_losses_restatement.py, whose padded formulation tests/test_ragged_losses_host.py ties to it).

MR-STFT.  (a) against the restatement of each item alone, TOL_RESTATEMENT = 1e-6 of tests/test_gpu_mrstft.py;
(b) against the dense call on the item alone, 2 N 2^-53 relative with N the number of summed terms (bins * frames_b for
the spectral tables, lens[b] for l1 / l2): the terms are identical and non-negative and only their order may differ, so
each of the two sums is within N 2^-53 of the exact one (the spectral convergence, a ratio of two square roots of such
sums, stays inside the same bound); (c) bit for bit under more padding, another batch order, as a batch of one and on a
rerun.  The padding holds NaN throughout.

Score loss.  Isolation tier as tests/test_gpu_score_loss.py (TOL = 1e-6 against the restatement fed the device's own
ragged score), x_t bit for bit the dense call's on the item alone.  End to end against oracle.dit.DiTScore (fp32) per
item: the ragged call's worst per-item distance may not exceed 4x the worst distance of the dense calls on the items
alone measured in the same test (floor 1e-6), the convention of E2E_BOUND there.  Every value is printed as a
"loss-margin {json}" line.
Measured on an MI355X (tiny DiT, bf16x3, frames (12, 7, 9, 1, 5), worst relative distance per item from the oracle-driven
restatement; the ragged call and the dense calls on the items alone gave the same figures to every printed digit):
  seed 0: DSM 2.19e-7, PIT 7.05e-7   seed 1: DSM 8.41e-8, PIT 7.69e-7   seed 2: DSM 1.73e-7, PIT 5.43e-7
  worst 7.69e-7 for both routes -> bound max(4 x 7.69e-7, 1e-6) = 3.08e-6.
MR-STFT against the restatement: log_mag up to 7.4e-7 (seven resolutions, A-weighted, n = 2), sc and lin_mag below 1e-8,
l1 / l2 exact to 2.3e-16; against the dense call on the item alone every entry was bit-identical (0.000 of the bound)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from oracle import dit as odit
from tests import mrstft_restatement as M
from tests import ragged_losses_restatement as RL
from tests import score_loss_restatement as S
from tests.test_gpu_score_loss import E2E_BOUND, SDE, T_EPS, TOL, _model, _tiny_dit, rel_each
from tests.util import make_engine

pytestmark = pytest.mark.gpu

TOL_RESTATEMENT = 1e-6
KEYS = RL.KEYS
SPECTRAL = ("sc", "log_mag", "lin_mag")
FS = 8000
# name: (fft sizes, hop sizes, lens, the two padded lengths)
MR_CASES = {"seven": (M.FFT_SIZES, M.HOP_SIZES, (1025, 1031, 2047, 2048, 3001, 4101), (4101, 5000)),
            "fft64": ((64,), (16,), (33, 40, 1024, 1025, 2049), (2049, 2500))}
MR_PARAMS = [("seven", n, w) for n in (1, 2, 3) for w in (False, True)] + [("fft64", 2, False), ("fft64", 2, True)]


@pytest.fixture(scope="module")
def eng():
    e = make_engine(precision=2)
    yield e
    e.close()


def _taps(weighted):
    if not weighted:
        return None
    from ditsep_amd import aweight
    return aweight.taps(FS)


@functools.lru_cache(maxsize=None)
def mr_case(name, n, weighted):
    """signals [B,n,max len] (float32, valid everywhere: the tests cut and pad them) and the float64 tables of every
    item alone, computed once"""
    ffts, hops, lens, _ = MR_CASES[name]
    reals, decoded = M.make_signals(FS, len(lens), n, max(lens), 300 + 10 * n + len(lens))
    want = RL.mrstft_items(reals, decoded, lens, ffts, hops, taps=_taps(weighted))
    assert all(np.isfinite(want[k]).all() for k in KEYS)
    return reals, decoded, want


def padded(x, lens, L, order=None):
    """x [B,n,max len] -> [B,n,L] on the device in `order`, NaN at and past each item's end"""
    order = range(len(lens)) if order is None else order
    out = torch.full((len(lens), x.shape[1], L), float("nan"))
    for k, b in enumerate(order):
        out[k, :, :lens[b]] = torch.from_numpy(x[b, :, :lens[b]])
    return out.cuda()


def call(eng, name, n, weighted, L, order=None, **kw):
    ffts, hops, lens, _ = MR_CASES[name]
    reals, decoded, _ = mr_case(name, n, weighted)
    order = list(range(len(lens))) if order is None else order
    return eng.mrstft_loss(padded(reals, lens, L, order), padded(decoded, lens, L, order), FS, fft_sizes=ffts,
                           hop_sizes=hops, perceptual_weighting=weighted, w_lin_mag=1.0, l1_weight=1.0, l2_weight=1.0,
                           lens=[lens[b] for b in order], **kw)


def alone(eng, name, n, weighted, b, ragged=False, **kw):
    """the item alone: the dense call on its own samples, or the ragged call on a batch of one"""
    ffts, hops, lens, _ = MR_CASES[name]
    reals, decoded, _ = mr_case(name, n, weighted)
    r, d = (torch.from_numpy(np.ascontiguousarray(a[b:b + 1, :, :lens[b]])) for a in (reals, decoded))
    return eng.mrstft_loss(r, d, FS, fft_sizes=ffts, hop_sizes=hops, perceptual_weighting=weighted, w_lin_mag=1.0,
                           l1_weight=1.0, l2_weight=1.0, lens=[lens[b]] if ragged else None, **kw)


def item_rows(tab, k, b):
    return tab[k][:, b] if k in SPECTRAL else tab[k][b]


@pytest.mark.parametrize("name,n,weighted", MR_PARAMS)
def test_mrstft_items_get_what_they_get_alone(eng, name, n, weighted):
    ffts, hops, lens, (L0, L1) = MR_CASES[name]
    _, _, want = mr_case(name, n, weighted)
    got = call(eng, name, n, weighted, L0)
    # 1. finite although the padding is NaN; 2. the float64 restatement of each item alone
    for k in KEYS:
        g = got[k].numpy()
        assert g.shape == want[k].shape and np.isfinite(g).all(), k
        err = float(np.abs(g / want[k] - 1.0).max())
        print(f"{name} n{n} w{int(weighted)}: {k} max |device / restatement - 1| = {err:.3e} (bound {TOL_RESTATEMENT:.0e})")
        assert err <= TOL_RESTATEMENT, (k, err)
    # 3. the dense call on the item alone: the summation-order bound; 4. the ragged call on a batch of one: the bits
    worst = 0.0
    for b, v in enumerate(lens):
        dense, one = alone(eng, name, n, weighted, b), alone(eng, name, n, weighted, b, ragged=True)
        for k in KEYS:
            a, d = item_rows(got, k, b).double(), item_rows(dense, k, 0).double()
            assert torch.equal(item_rows(got, k, b), item_rows(one, k, 0)), (k, b)
            for r in range(len(ffts) if k in SPECTRAL else 1):
                bound = 2.0 * RL.sum_terms(k, ffts[r], hops[r], v) * 2.0 ** -53
                ar, dr = (a[r], d[r]) if k in SPECTRAL else (a, d)
                ratio = float(((ar - dr).abs() / dr).max()) / bound
                worst = max(worst, ratio)
                assert ratio <= 1.0, (k, b, r, ratio)
    print(f"{name} n{n} w{int(weighted)}: worst distance from the dense call on the item alone = {worst:.3f} of the "
          f"bound 2 N 2^-53")
    # 4. bit for bit under more padding, in another batch order and on a rerun
    order = [3, 0, len(lens) - 1, 1, 2] + list(range(4, len(lens) - 1))
    more, perm, again = call(eng, name, n, weighted, L1), call(eng, name, n, weighted, L0, order), call(eng, name, n, weighted, L0)
    for k in KEYS:
        assert torch.equal(got[k], more[k]) and torch.equal(got[k], again[k]), k
        for pos, b in enumerate(order):
            assert torch.equal(item_rows(perm, k, pos), item_rows(got, k, b)), (k, b)


@pytest.mark.parametrize("pit", ["item", "batch"])
def test_mrstft_pit_results_are_the_combine_of_the_per_item_tables(eng, pit):
    from ditsep_amd import native

    name, n, weighted = "seven", 3, True
    lens, L = MR_CASES[name][2], MR_CASES[name][3][1]
    got = call(eng, name, n, weighted, L, pit=pit)
    per = [alone(eng, name, n, weighted, b, ragged=True) for b in range(len(lens))]
    stacked = {k: torch.cat([p[k] for p in per], dim=1 if k in SPECTRAL else 0) for k in KEYS}
    want = native.mrstft_combine(stacked, w_lin_mag=1.0, l1_weight=1.0, l2_weight=1.0, pit=pit)
    for k, v in want.items():
        if k == "perms":
            assert got[k] == v
        else:
            assert torch.equal(torch.as_tensor(got[k]), torch.as_tensor(v)), k
    assert len({tuple(r) for r in got["pit_mrstft_perm"].tolist()}) == (2 if pit == "item" else 1)


def test_mrstft_refusals_happen_before_any_launch(eng):
    from ditsep_amd import native

    x = torch.zeros((3, 2, 3000), device="cuda")
    tabs = np.zeros(4096)

    def raw(lens, fft=(2048, 64), hop=(512, 16), L=3000):
        R_ = len(fft)
        cfg = native.DsnMrstftConfig(n_res=R_, fft=(C.c_int * R_)(*fft), hop=(C.c_int * R_)(*hop),
                                     win=(C.c_int * R_)(*fft), w_sc=1.0, w_log_mag=1.0, w_lin_mag=0.0, taps=None, n_taps=0)
        out = native.DsnMrstftOut(sc=tabs.ctypes.data_as(C.POINTER(C.c_double)))
        return eng.lib.dsn_mrstft_loss_ragged(eng.ctx, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr()),
                                              (C.c_int32 * 3)(*lens), 3, 2, L, C.byref(cfg), C.byref(out), None)

    for lens, what in (((3000, 1024, 2000), r"lens\[1\] = 1024 needs reflect padding"),
                       ((0, 3000, 3000), r"sample count lens\[0\] = 0 outside"),
                       ((3000, 3000, 3001), r"sample count lens\[2\] = 3001 outside")):
        assert raw(lens) == -1, what
        with pytest.raises(RuntimeError, match="dsn_mrstft_loss_ragged: " + what):
            eng._check(-1, "dsn_mrstft_loss_ragged")
    assert raw((3000, 1025, 2000), fft=(4096,), hop=(1024,)) == -1            # the dense call's refusals apply unchanged
    assert not np.any(tabs)
    assert raw((3000, 1025, 2000)) == 0 and np.isfinite(tabs).all()           # the engine goes on
    for lens in ((3000, 1024, 2000), (0, 3000, 3000), (3000, 3000, 3001), (3000, 3000)):
        with pytest.raises(ValueError):
            eng.mrstft_loss(x, x, FS, lens=lens)
    assert eng.mrstft_loss(x, x, FS, fft_sizes=(64,), hop_sizes=(16,), lens=(33, 3000, 40))["l1"].shape == (3, 2, 2)


# ------------------------------------------------------------------ score loss
FRAMES = (40, 32, 33, 1, 17)        # D frames = 2560, 2048, 2112, 64, 1088 elements against the 2048-element chunk


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(n_src):
        if n_src not in made:
            cfg, sd = _tiny_dit(n_src)
            made[n_src] = (cfg, sd, make_engine(cfg, sd, precision=2))
        return made[n_src]

    yield get
    for _, _, e in made.values():
        e.close()


def _ragged_inputs(frames, n, T, seed, D=64, order=None):
    """per-item draws that do not depend on T or on the batch order; x0 and z are NaN past each item's end, the
    mixture's padding is finite (it goes to the score call)"""
    B = len(frames)
    order = list(range(B)) if order is None else order
    mix, target, z = torch.zeros((B, 1, D, T)), torch.full((B, n, D, T), float("nan")), torch.full((B, n, D, T), float("nan"))
    t, perm = torch.zeros(B), torch.zeros((B, n), dtype=torch.long)
    for k, b in enumerate(order):
        g = torch.Generator().manual_seed(1000 * seed + b)
        f = frames[b]
        mix[k, ..., :f] = torch.randn((1, D, f), generator=g)
        target[k, ..., :f] = 0.7 * torch.randn((n, D, f), generator=g)
        z[k, ..., :f] = torch.randn((n, D, f), generator=g)
        t[k] = T_EPS + (1 - T_EPS) * float(torch.rand((), generator=g))
        perm[k] = torch.argsort(torch.rand(n, generator=g))
    return mix, target, t, z, perm, [frames[b] for b in order]


def _check_isolation(eng, n, T, order=None):
    mix, target, t, z, perm, frames = _ragged_inputs(FRAMES, n, T, 7, order=order)
    B = len(frames)
    cut = lambda a, b: a[b:b + 1, ..., :frames[b]].contiguous()
    for p in (None, perm):
        tgt = target if p is None else S.shuffle_sources(target, p)
        for red in ("none", "mean"):
            loss, aux = eng.score_loss(mix, target, reduction=red, time=t, noise=z, perm=p, frames=frames, return_aux=True)
            assert torch.equal(aux["t"].cpu(), t)
            assert rel_each(aux["sigma"], SDE.std(t.double())) <= TOL
            for b, f in enumerate(frames):
                # 1. x_t: the dense call on the item alone, bit for bit, and zero past the end
                _, one = eng.score_loss(cut(mix, b), cut(target, b), time=t[b:b + 1], noise=cut(z, b),
                                        perm=None if p is None else p[b:b + 1], loss=False, return_aux=True)
                assert torch.equal(aux["x_t"][b:b + 1, ..., :f], one["x_t"]) and not aux["x_t"][b, ..., f:].any(), b
                assert torch.equal(aux["sigma"][b:b + 1], one["sigma"])
            # 3. the restatement fed the device's own ragged score, restricted to each item's frames
            dev = eng.score(aux["x_t"], aux["t"], mix, frames=frames).cpu().double()
            rows = RL.score_loss_items(SDE, lambda b: (lambda *a: dev[b:b + 1, ..., :frames[b]]), mix, tgt, t, z, frames,
                                       x_t=aux["x_t"].cpu())
            want = rows if red == "none" else RL.reduce_mean(rows)
            assert loss.shape == want.shape == ((B, n) if red == "none" else ()) and torch.isfinite(loss).all()
            assert rel_each(loss, want) <= TOL, (red, p is not None)
    loss, aux = eng.score_loss(mix, target, mode="init_pit", noise=z, frames=frames, return_aux=True)
    for b, f in enumerate(frames):
        _, one = eng.score_loss(cut(mix, b), cut(target, b), mode="init_pit", noise=cut(z, b), loss=False, return_aux=True)
        assert torch.equal(aux["x_t"][b:b + 1, ..., :f], one["x_t"]) and not aux["x_t"][b, ..., f:].any(), b
    dev = eng.score(aux["x_t"], aux["t"], mix, frames=frames).cpu().double()
    want = RL.score_loss_items(SDE, lambda b: (lambda *a: dev[b:b + 1, ..., :frames[b]]), mix, target, None, z, frames,
                               mode="init_pit", x_t=aux["x_t"].cpu())
    assert loss.shape == (B, n) and rel_each(loss, want) <= TOL
    mean = eng.score_loss(mix, target, mode="init_pit", reduction="mean", noise=z, frames=frames)
    assert mean.shape == () and rel_each(mean, want.mean()) <= TOL


@pytest.mark.parametrize("n", [2, 3])
def test_score_loss_perturb_and_reduce_in_isolation(engines, n):
    _, _, eng = engines(n)
    _check_isolation(eng, n, 40)
    # 4. the same items under more padding and in another batch order pass the same check
    _check_isolation(eng, n, 48)
    _check_isolation(eng, n, 40, [2, 4, 0, 3, 1])


def test_score_loss_pit_variant_makes_one_ragged_score_call(engines):
    _, _, eng = engines(3)
    mix, target, _, z, _, frames = _ragged_inputs(FRAMES, 3, 40, 9)
    eng.profile_begin()
    eng.score(torch.zeros_like(target), torch.ones(len(frames)), mix, frames=frames)
    one = eng.profile_end()["gemm_launches"]
    eng.profile_begin()
    eng.score_loss(mix, target, mode="init_pit", noise=z, frames=frames)
    got = eng.profile_end()["gemm_launches"]
    assert one > 0 and got == one


def test_score_loss_reruns_are_bit_identical_eager_and_graph_replayed(engines):
    _, _, eng = engines(2)
    mix, target, t, z, perm, frames = _ragged_inputs(FRAMES, 2, 40, 11)
    other = [40, 3, 33, 7, 17]                         # other lengths through the same captured graph
    clean = lambda a: torch.nan_to_num(a)             # (valid everywhere, so that any lengths may be asked of it)
    for kw in (dict(seed=11), dict(seed=11, mode="init_pit"), dict(seed=11, reduction="mean"),
               dict(time=t, noise=clean(z), perm=perm)):
        eng.enable_graphs(False)
        a, aux_a = eng.score_loss(mix, clean(target), frames=frames, return_aux=True, **kw)
        assert torch.equal(a, eng.score_loss(mix, clean(target), frames=frames, **kw))
        want_other = eng.score_loss(mix, clean(target), frames=other, **kw)
        eng.enable_graphs(True)
        for _ in range(3):                             # eager warm-up, capture, replay
            c, aux_c = eng.score_loss(mix, clean(target), frames=frames, return_aux=True, **kw)
            assert torch.equal(a, c) and all(torch.equal(aux_a[k], aux_c[k]) for k in aux_a)
        assert torch.equal(want_other, eng.score_loss(mix, clean(target), frames=other, **kw))
        eng.enable_graphs(False)


def test_score_loss_refusals(engines):
    _, _, eng = engines(2)
    mix, target, t, z, _, frames = _ragged_inputs(FRAMES, 2, 40, 13)
    from ditsep_amd import native

    fr = (C.c_int32 * 5)(40, 32, 41, 1, 17)
    o = native.DsnLossOpts(0, 0, 0.03)
    p = lambda a: C.c_void_p(a.data_ptr())
    m, x = mix.cuda(), torch.nan_to_num(target).cuda()
    out = torch.zeros((5, 2), device="cuda")
    rc = eng.lib.dsn_score_loss_ragged(eng.ctx, p(m), p(x), fr, None, None, None, 1, p(out), None, None, None, None, 5,
                                       40, C.byref(o), None)
    assert rc == -1 and not out.any()
    with pytest.raises(RuntimeError, match=r"dsn_score_loss_ragged: frame count frames\[2\] = 41 outside"):
        eng._check(-1, "dsn_score_loss_ragged")
    with pytest.raises(ValueError, match="outside"):
        eng.score_loss(mix, target, frames=(40, 32, 0, 1, 17))
    assert torch.isfinite(eng.score_loss(mix, target, time=t, noise=z, frames=frames)).all()


def test_score_loss_e2e_against_the_oracle_per_item(engines):
    """ragged worst <= 4 x dense-alone worst (floor 1e-6), both against oracle.dit.DiTScore (fp32) on the item alone"""
    torch.set_num_threads(16)
    cfg, sd, eng = engines(2)
    net = odit.DiTScore(sd, cfg)
    frames0 = (12, 7, 9, 1, 5)
    worst = {"ragged": 0.0, "dense": 0.0}
    for seed in (0, 1, 2):
        mix, target, t, z, _, frames = _ragged_inputs(frames0, 2, 12, 50 + seed)
        cut = lambda a, b: a[b:b + 1, ..., :frames[b]].contiguous()
        with torch.no_grad():
            ref = RL.score_loss_items(SDE, lambda b: net, mix, target, t, z, frames, score_dtype=torch.float32)
            ref_pit = RL.score_loss_items(SDE, lambda b: net, mix, target, None, z, frames, mode="init_pit",
                                          score_dtype=torch.float32)
        rag = eng.score_loss(mix, target, time=t, noise=z, frames=frames).cpu().double()
        rag_pit = eng.score_loss(mix, target, mode="init_pit", noise=z, frames=frames).cpu().double()
        den = torch.cat([eng.score_loss(cut(mix, b), cut(target, b), time=t[b:b + 1], noise=cut(z, b))
                         for b in range(len(frames))]).cpu().double()
        den_pit = torch.cat([eng.score_loss(cut(mix, b), cut(target, b), mode="init_pit", noise=cut(z, b))
                             for b in range(len(frames))]).cpu().double()
        d = {"ragged_dsm": rel_each(rag, ref), "ragged_pit": rel_each(rag_pit, ref_pit),
             "dense_dsm": rel_each(den, ref), "dense_pit": rel_each(den_pit, ref_pit)}
        worst["ragged"] = max(worst["ragged"], d["ragged_dsm"], d["ragged_pit"])
        worst["dense"] = max(worst["dense"], d["dense_dsm"], d["dense_pit"])
        print("loss-margin " + json.dumps({"case": "tiny_dit/bf16x3 ragged", "frames": frames, "seed": seed, **d}))
    bound = max(4.0 * worst["dense"], 1e-6)
    print("loss-margin " + json.dumps({"case": "tiny_dit/bf16x3 ragged", **worst, "bound": bound}))
    assert worst["ragged"] <= bound


# ------------------------------------------------------------------ the harness and the LDM list form
def test_evaluate_batches_list_batch_with_both_losses(tmp_path):
    from ditsep_amd import evaluate

    model = _model(tmp_path)
    eng = model.engine
    g = torch.Generator().manual_seed(31)
    lens = (4000, 5000, 6100, 4500)
    batch = ([0.3 * torch.randn((1, L), generator=g) for L in lens], [0.3 * torch.randn((2, L), generator=g) for L in lens])
    seen = {}
    score_loss, decode_ragged = eng.score_loss, eng.decode_ragged

    def spy_loss(y, x0, **kw):
        seen["loss"] = (y.clone(), x0.clone(), dict(kw))
        return score_loss(y, x0, **kw)

    def spy_decode(*a, **k):
        seen["est"] = [e.clone() for e in decode_ragged(*a, **k)]
        return seen["est"]

    eng.score_loss, eng.decode_ragged = spy_loss, spy_decode
    res = evaluate.evaluate_batches(model, [batch], FS, N=2, seed=4, score_loss=True, mrstft=True, ragged_losses=True)
    eng.score_loss, eng.decode_ragged = score_loss, decode_ragged
    keys = ["batch_idx", "si_sdr", "si_sir", "si_sar", "pesq", "stoi", "nfe", "runtime", "len_s", "perm"]
    y, x0, kw = seen["loss"]
    assert kw["seed"] == 4 and kw["reduction"] == "none"
    frames = kw["frames"]
    _, aux = score_loss(y, x0, return_aux=True, **kw)                   # the t and z the harness call drew
    for b in range(4):
        rec, f = res[b], frames[b]
        assert list(rec) == keys + ["score_loss", "mrstft", "l1"] and rec["len_s"] == lens[b] / FS
        cut = lambda a: a[b:b + 1, ..., :f].contiguous()
        one = score_loss(cut(y), cut(x0), time=aux["t"][b:b + 1], noise=cut(aux["z"])).cpu().double()[0]
        got = torch.tensor(rec["score_loss"], dtype=torch.float64)
        print("loss-margin " + json.dumps({"case": "harness", "item": b, "rel": rel_each(got, one)}))
        assert rel_each(got, one) <= E2E_BOUND["tiny_dit/bf16x3"]
        tabs = eng.mrstft_loss(batch[1][b][None], seen["est"][b][None], FS, pit=None)
        bound = 2.0 * max(RL.sum_terms("sc", ff, hh, lens[b]) for ff, hh in zip(M.FFT_SIZES, M.HOP_SIZES)) * 2.0 ** -53
        for i in range(2):
            j = rec["perm"][i]
            want = float((tabs["sc"] + tabs["log_mag"]).mean(0)[0, i, j])
            assert abs(rec["mrstft"][i] - want) <= bound * want
            assert abs(rec["l1"][i] - float(tabs["l1"][0, i, j])) <= 2.0 * lens[b] * 2.0 ** -53 * float(tabs["l1"][0, i, j])
    model.close()


def test_ldm_losses_gen_on_lists_equals_the_padded_call(tmp_path):
    from ditsep_amd import LDM
    from oracle import oobleck as ovae
    from oracle.make_golden import tiny_vae_weights
    from tests.test_gpu_kernels import _tiny_config

    cfg = dict(_tiny_config(tmp_path))
    cfg["training"] = {"loss": {"spectral": {"type": "mrstft", "decay": 1.0, "weights": {"mrstft": 1.0},
                                             "config": {"sample_rate": FS, "fft_sizes": [1024, 256, 64],
                                                        "hop_sizes": [256, 64, 16], "win_lengths": [1024, 256, 64],
                                                        "perceptual_weighting": True}},
                                "time": {"type": "l1", "weights": {"l1": 15.0}}}}
    model = LDM(cfg, precision="fp16")
    _, dsd = _tiny_dit()
    sd = {"score_model." + k: v for k, v in dsd.items()}
    sd.update({"vae." + k: v for k, v in tiny_vae_weights(ovae.OobleckConfig(channels=32), 31).items()})
    model.load_state_dict(sd)
    lens = (2100, 1500, 1800)
    reals, decoded = M.make_signals(FS, 3, 2, 2100, 17)
    rl = [torch.from_numpy(reals[b, :, :v].copy()) for b, v in enumerate(lens)]
    dl = [torch.from_numpy(decoded[b, :, :v].copy()) for b, v in enumerate(lens)]
    loss, losses = model.losses_gen(dl, rl)
    tabs = model.last_loss_tables
    loss2, losses2 = model.losses_gen(padded(decoded, lens, 2100), padded(reals, lens, 2100), lens=lens)
    assert list(losses) == ["pit_mrstft_loss", "pit_l1_loss"] == list(losses2)
    assert float(loss) == float(loss2) and np.isfinite(float(loss))
    for k in KEYS:
        assert torch.equal(tabs[k], model.last_loss_tables[k]), k
    want = RL.mrstft_items(reals, decoded, lens, (1024, 256, 64), (256, 64, 16), taps=_taps(True))
    obj = M.objective(want, 2, l1_weight=15.0)
    assert abs(float(loss) / obj["loss"] - 1.0) <= TOL_RESTATEMENT
    model.close()


def test_latentdiffsep_list_forms_make_one_ragged_call(tmp_path):
    lens = (4000, 6143, 9000)
    g = torch.Generator().manual_seed(41)
    mixes = [0.3 * torch.randn((1, L), generator=g) for L in lens]
    targets = [0.3 * torch.randn((2, L), generator=g) for L in lens]
    model = _model(tmp_path, loss={"_target_": "torch.nn.MSELoss"})
    eng = model.engine
    y, x, frames = model.encode_lists(mixes, targets, seed=5)
    assert frames == [eng.latent_frames(L) for L in lens] and x.shape == (3, 2, 64, max(frames))
    want = eng.score_loss(y, x, reduction="mean", t_eps=T_EPS, seed=5, frames=frames)
    assert torch.equal(model.compute_score_loss(mixes, targets, seed=5), want)
    out = model.validation_step((mixes, targets), 0, seed=5)
    assert out["val/score_loss"].shape == () and torch.equal(out["val/score_loss"], want)
    assert np.isfinite(float(out["val/si_sdr"])) and abs(float(out["val/si_sdr"])) <= 30.0
    assert set(model.validation_step((mixes, targets), 1, seed=5)) == {"val/score_loss"}
    with pytest.raises(ValueError, match="minibatch"):
        model.compute_score_loss(mixes, targets, seed=5, minibatch=2)
    model.close()
    model = _model(tmp_path, loss={"_target_": "torch.nn.MSELoss"}, init_hack=5, init_hack_p=0.5)
    eng = model.engine
    mask, perm, t = torch.tensor([True, False, False]), torch.tensor([[1, 0], [0, 1]]), torch.tensor([0.2, 0.9])
    got = model.train_step_init_5(mixes, targets, pit_mask=mask, perm=perm, time=t, seed=3)
    y, x, frames = model.encode_lists(mixes, targets, seed=3)
    a = eng.score_loss(y[:1], x[:1], mode="init_pit", t_eps=T_EPS, seed=3, frames=frames[:1])
    b = eng.score_loss(y[1:], x[1:], time=t, perm=perm, t_eps=T_EPS, seed=3 + 7919, frames=frames[1:])
    assert got.shape == () and torch.equal(got, torch.cat([a, b]).mean())
    assert model.compute_score_loss_init_hack_pit(mixes, targets, seed=1).shape == (3, 2)
    assert torch.isfinite(model.validation_step((mixes, targets), 0, seed=2)["val/score_loss"])
    model.close()
