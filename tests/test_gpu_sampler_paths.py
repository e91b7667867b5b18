"""The latent samplers' shared host path (engine.hip: run_sampler, upload_step_times, TimeEmbedPass, StreamScope).

Every sampler entry point stages its tensors into the same workspace buffers ("pc_y", "pc_noise", "pc_t") and shares
the uploaded step-time table's signature, so three things are pinned here on the tiny DiT (bf16x3, B=2, T=8, injected
noise): a graph-replayed call equals the eager call bit for bit, for the Mix / PriorMix / Schroedinger-bridge samplers
and the pc_sample variants the other test files leave out; calls of different samplers interleaved on one engine
do not disturb each other; and a context whose weights are not finalized is refused on the host.  A fourth (fp16, width
256): a captured graph follows a kernel-choice switch that changes between two calls."""
import pytest
import torch

from ditsep_amd import native
from oracle import dit as odit
from tests.util import make_engine

pytestmark = pytest.mark.gpu

X3 = 2
B, T, N = 2, 8, 3
PC_DRAWS = 1 + N * 2          # prior + N x (one corrector step + predictor)

# name -> (Engine method, noise draws (0: the sampler takes none), keyword arguments)
CALLS = {
    "mix": ("pc_sample_mix", PC_DRAWS, dict(N=N, prior_mix=False)),
    "prior_mix": ("pc_sample_mix", PC_DRAWS, dict(N=N, prior_mix=True)),
    "sb_sde": ("sb_sample", N, dict(N=N, sampler_type="sde")),
    "sb_ode": ("sb_sample", 0, dict(N=N, sampler_type="ode")),
    "pc": ("pc_sample", PC_DRAWS, dict(N=N)),
    "pc_timesteps": ("pc_sample", PC_DRAWS, dict(N=N, timesteps=[1.0, 0.55, 0.2, 0.03])),
    "pc_langevin": ("pc_sample", PC_DRAWS, dict(N=N, corrector="langevin")),
}


def _tiny_dit():
    cfg = odit.DiTConfig(n_src=2, embed_dim=128, depth=2, num_heads=2)
    return cfg, odit.random_dit_weights(cfg, 34, out_gain=0.005)


@pytest.fixture(scope="module")
def tiny():
    cfg, sd = _tiny_dit()
    eng = make_engine(cfg, sd, precision=X3)
    yield cfg, sd, eng
    eng.close()


def _inputs(cfg, seed=5):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((B, 1, cfg.latent_dim, T), generator=g)
    noise = torch.randn((PC_DRAWS, B, cfg.n_src, cfg.latent_dim, T), generator=g)
    return y, noise


def _run(eng, name, y, noise):
    method, draws, kw = CALLS[name]
    out = getattr(eng, method)(y, noise[:draws].contiguous() if draws else None, **kw)
    return (out[0] if isinstance(out, tuple) else out).clone()


@pytest.mark.parametrize("name", ["mix", "prior_mix", "sb_sde", "sb_ode", "pc_timesteps", "pc_langevin"])
def test_eager_equals_graph_replayed(tiny, name):
    cfg, _, eng = tiny
    y, noise = _inputs(cfg)
    eng.enable_graphs(False)
    eager = _run(eng, name, y, noise)
    eager_half = _run(eng, name, y * 0.5, noise)
    assert not torch.equal(eager, eager_half)
    eng.enable_graphs(True)
    try:
        for _ in range(4):                    # eager warm-up, capture, two replays
            assert torch.equal(_run(eng, name, y, noise), eager)
        assert torch.equal(_run(eng, name, y * 0.5, noise), eager_half)   # another input through the captured graph
    finally:
        eng.enable_graphs(False)


def test_interleaved_samplers_keep_their_own_step_times(tiny):
    """SB, PC, Mix, SB on one engine with graphs on: all stage into "pc_y" / "pc_noise" / "pc_t", and SB and PC
    upload different step-time tables of the same [N][B] shape.  Three rounds: every graph is warmed up, captured and
    replayed with the other samplers' calls in between."""
    cfg, _, eng = tiny
    y, noise = _inputs(cfg, seed=6)
    order = ["sb_sde", "pc", "mix", "sb_sde"]
    eng.enable_graphs(False)
    eager = {name: _run(eng, name, y, noise) for name in set(order)}
    eng.enable_graphs(True)
    try:
        for rnd in range(3):
            for name in order:
                assert torch.equal(_run(eng, name, y, noise), eager[name]), (rnd, name)
    finally:
        eng.enable_graphs(False)


def test_unfinalized_context_is_refused_before_any_launch():
    """No weights loaded, no finalize(): the three samplers fail on the host with the state error; the same engine
    then loads, finalizes and samples exactly what a freshly built engine does."""
    cfg, sd = _tiny_dit()
    y, noise = _inputs(cfg, seed=7)
    eng = native.Engine(precision=X3, score_kind=native.SCORE_DIT, n_src=cfg.n_src, latent_dim=cfg.latent_dim,
                        dit_embed_dim=cfg.embed_dim, dit_depth=cfg.depth, dit_heads=cfg.num_heads,
                        vae_has_encoder=False, vae_has_decoder=False)
    fresh = None
    try:
        eng.enable_graphs(True)
        ws = eng.workspace_bytes()
        for name in ("pc", "mix", "sb_sde"):
            with pytest.raises(RuntimeError, match="weights not finalized"):
                _run(eng, name, y, noise)
        assert eng.workspace_bytes() == ws    # refused before the first workspace buffer
        eng.load_state_dict(sd, prefix="score_model.")
        eng.finalize()
        got = _run(eng, "pc", y, noise)
        fresh = make_engine(cfg, sd, precision=X3)
        assert torch.equal(got, _run(fresh, "pc", y, noise))
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()


def test_captured_graph_follows_a_switch_changed_between_calls(monkeypatch):
    """A graph remembers the switches it was built under (engine.hip: run_graphed, Switches).  DiT of width 256 (4 heads,
    depth 2), fp16, B = 2, T = 8: M = 18 token rows, inside the skinny window by default and on the row-panel kernels
    under DSN_SKINNY_MAX=0 -- another summation order, so the two eager results differ.  With graphs on, four calls under
    the default switches (warm-up, capture, two replays), then DSN_SKINNY_MAX=0: the call must give the eager
    DSN_SKINNY_MAX=0 result, not a replay of the graph captured under the old choice."""
    monkeypatch.delenv("DSN_SKINNY_MAX", raising=False)
    cfg = odit.DiTConfig(n_src=2, embed_dim=256, depth=2, num_heads=4)
    sd = odit.random_dit_weights(cfg, 35, out_gain=0.005)
    n = 2
    g = torch.Generator().manual_seed(8)
    y = torch.randn((B, 1, cfg.latent_dim, T), generator=g)
    noise = torch.randn((1 + n * 2, B, cfg.n_src, cfg.latent_dim, T), generator=g)
    eng = make_engine(cfg, sd, precision=native.PREC_FP16)

    def run():
        out = eng.pc_sample(y, noise, N=n)
        return (out[0] if isinstance(out, tuple) else out).clone()

    try:
        eager_skinny = run()
        monkeypatch.setenv("DSN_SKINNY_MAX", "0")
        eager_panel = run()
        assert not torch.equal(eager_skinny, eager_panel)    # else the last assertion below would be vacuous
        monkeypatch.delenv("DSN_SKINNY_MAX")
        eng.enable_graphs(True)
        for _ in range(4):
            assert torch.equal(run(), eager_skinny)
        monkeypatch.setenv("DSN_SKINNY_MAX", "0")
        assert torch.equal(run(), eager_panel)
    finally:
        eng.close()
