"""The masking argument behind the padded codec pass (include/ditsep_hip.h), no GPU: if every layer's output
rows past an item's end are zero before the next layer reads them, the valid rows of an item inside a padded batch are
the rows of the item run alone.  Checked in float64 on oracle/oobleck.py's own layers, driven in sequence with the
zeroing the engine adds between them (the same places: the latent, conv_in, every transposed / strided conv, every
ResidualUnit, conv_out), with the tiny fixtures' weights, ELU and Snake.  A control run without the zeroing must miss
the same bound by far.  Also the host-side rules around it: the level-length helpers, the Python refusals and the
`codec=` keyword."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from ditsep_amd import native
from oracle import oobleck as ovae
from oracle.make_golden import tiny_vae_weights

N_SRC = 2
FRAMES = [1, 3, 2]          # 1 frame: shorter than the dilation-9 reach at the coarse levels; 3 = T: a full-length item
T = max(FRAMES)
BOUND = 1e-12               # float64 round-off of a handful of convolutions; the control misses it by many orders


def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


@pytest.fixture(scope="module", params=["elu", "snake"])
def vae(request):
    cfg = ovae.OobleckConfig(channels=8, use_snake=request.param == "snake")
    return cfg, _f64(tiny_vae_weights(cfg, 21))          # the weights of tests/golden/vae_tiny_{elu,snake}.npz


def _tail(frames, rep, zero):
    """-> f(x [S,C,L], mul): rows [frames[s // rep] * mul, L) of every item written as zero (zero=False: identity)"""
    def f(x, mul):
        if not zero:
            return x
        x = x.clone()
        for s, r in enumerate(native.codec_valid_rows(frames, rep, mul, x.shape[0])):
            x[s, :, r:] = 0.0
        return x
    return f


def decoder_layers(sd, cfg, z, tail, prefix="decoder."):
    """ovae.decoder_forward, layer by layer, with tail(x, rows per frame) after each engine launch"""
    muls = native.codec_level_rows(cfg.strides, "decoder")
    m, snake = cfg.mults, cfg.use_snake
    x = tail(z, muls[0])
    x = tail(ovae._conv(sd, prefix + "layers.0.", x, padding=3), muls[0])
    li = 1
    for i in range(len(m) - 1, 0, -1):
        p, s = f"{prefix}layers.{li}.", cfg.strides[i - 1]
        x = ovae._act(sd, p + "layers.0.", x, snake)
        x = F.conv_transpose1d(x, ovae.fold_weight_norm(sd, p + "layers.1."), sd.get(p + "layers.1.bias"), stride=s,
                               padding=math.ceil(s / 2))
        x = tail(x, muls[li])
        for j, d in enumerate((1, 3, 9)):
            x = tail(ovae._res_unit(sd, f"{p}layers.{2 + j}.", x, d, snake), muls[li])
        li += 1
    x = ovae._act(sd, f"{prefix}layers.{li}.", x, snake)
    x = ovae._conv(sd, f"{prefix}layers.{li + 1}.", x, padding=3)
    return tail(torch.tanh(x) if cfg.final_tanh else x, muls[-1])


def encoder_layers(sd, cfg, wav, tail, prefix="encoder."):
    """ovae.encoder_forward, layer by layer, with tail(x, rows per frame) after each engine launch"""
    muls = native.codec_level_rows(cfg.strides, "encoder")
    m, snake = cfg.mults, cfg.use_snake
    x = tail(ovae._conv(sd, prefix + "layers.0.", wav, padding=3), muls[0])
    li = 1
    for i in range(len(m) - 1):
        p, s = f"{prefix}layers.{li}.", cfg.strides[i]
        for j, d in enumerate((1, 3, 9)):
            x = tail(ovae._res_unit(sd, f"{p}layers.{j}.", x, d, snake), muls[li - 1])
        x = ovae._act(sd, p + "layers.3.", x, snake)
        x = tail(ovae._conv(sd, p + "layers.4.", x, stride=s, padding=math.ceil(s / 2)), muls[li])
        li += 1
    x = ovae._act(sd, f"{prefix}layers.{li}.", x, snake)
    return tail(ovae._conv(sd, f"{prefix}layers.{li + 1}.", x, padding=1), muls[-1])


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_layer_drivers_are_the_oracle(vae):
    """without zeroing, the layer-by-layer drivers are oracle.decoder_forward / encoder_forward bit for bit"""
    cfg, sd = vae
    g = torch.Generator().manual_seed(3)
    z = torch.randn((2, cfg.latent_dim, 2), generator=g, dtype=torch.float64)
    ident = _tail(None, 1, False)
    assert torch.equal(decoder_layers(sd, cfg, z, ident), ovae.decoder_forward(sd, cfg, z, "decoder."))
    wav = torch.randn((2, 1, cfg.hop), generator=g, dtype=torch.float64)
    assert torch.equal(encoder_layers(sd, cfg, wav, ident), ovae.encoder_forward(sd, cfg, wav, "encoder."))


def test_decoder_masking_argument(vae):
    cfg, sd = vae
    g = torch.Generator().manual_seed(11)
    B, hop = len(FRAMES), cfg.hop
    est = torch.randn((B, N_SRC, cfg.latent_dim, T), generator=g, dtype=torch.float64)
    alone = [ovae.decoder_forward(sd, cfg, est[b, :, :, :f], "decoder.") for b, f in enumerate(FRAMES)]
    dirty = est.clone()
    clean = est.clone()
    for b, f in enumerate(FRAMES):
        dirty[b, ..., f:] *= 7.0                       # finite garbage in the padded region
        clean[b, ..., f:] = 0.0
    S = B * N_SRC
    out = decoder_layers(sd, cfg, dirty.reshape(S, cfg.latent_dim, T), _tail(FRAMES, N_SRC, True)).reshape(B, N_SRC, -1)
    # control: a zero latent tail, but no zeroing between the layers -- biases fill the tail and leak into valid rows
    ctl = decoder_layers(sd, cfg, clean.reshape(S, cfg.latent_dim, T), _tail(FRAMES, N_SRC, False)).reshape(B, N_SRC, -1)
    saw_defect = False
    for b, f in enumerate(FRAMES):
        err = _rel(out[b, :, :f * hop], alone[b][:, 0])
        cerr = _rel(ctl[b, :, :f * hop], alone[b][:, 0])
        print(f"decoder item {b} ({f} frames): masked rel {err:.3e}, control rel {cerr:.3e}")
        assert err <= BOUND, f"item {b}: masked padded run differs from the item alone by {err:.3e}"
        assert (out[b, :, f * hop:] == 0).all()
        if f < T:
            assert cerr > 1e3 * BOUND, f"item {b}: the control run cannot see the defect ({cerr:.3e})"
            saw_defect = True
        else:
            assert cerr <= BOUND               # a full-length item has no tail to leak
    assert saw_defect


def test_encoder_masking_argument(vae):
    cfg, sd = vae
    g = torch.Generator().manual_seed(12)
    B, hop = len(FRAMES), cfg.hop
    lens = [f * hop - 1 - 37 * b for b, f in enumerate(FRAMES)]           # sample counts with these frame counts
    assert [native.latent_frames_of(L, hop) for L in lens] == FRAMES
    wav = torch.zeros((B, 1, hop * T), dtype=torch.float64)
    for b, L in enumerate(lens):
        wav[b, 0, :L] = 0.3 * torch.randn(L, generator=g, dtype=torch.float64)
    noise = torch.randn((B, cfg.latent_dim, T), generator=g, dtype=torch.float64)
    alone = [ovae.encoder_forward(sd, cfg, wav[b:b + 1, :, :f * hop], "encoder.") for b, f in enumerate(FRAMES)]
    out = encoder_layers(sd, cfg, wav, _tail(FRAMES, 1, True))
    ctl = encoder_layers(sd, cfg, wav, _tail(FRAMES, 1, False))
    for b, f in enumerate(FRAMES):
        err, cerr = _rel(out[b:b + 1, :, :f], alone[b]), _rel(ctl[b:b + 1, :, :f], alone[b])
        print(f"encoder item {b} ({f} frames): masked rel {err:.3e}, control rel {cerr:.3e}")
        assert err <= BOUND, f"item {b}: masked padded run differs from the item alone by {err:.3e}"
        assert (out[b, :, f:] == 0).all()
        if f < T:
            assert cerr > 1e3 * BOUND, f"item {b}: the control run cannot see the defect ({cerr:.3e})"
        # the bottleneck acts per frame: the item's latent is the sample of its own encoder output
        y = ovae.vae_sample(out[b:b + 1, :, :f], noise[b:b + 1, :, :f])
        assert _rel(y, ovae.vae_sample(alone[b], noise[b:b + 1, :, :f])) <= BOUND


# ------------------------------------------------------------------ level-length helpers
def test_codec_level_rows_and_valid_rows():
    strides = (2, 4, 4, 8, 8)
    dec = native.codec_level_rows(strides, "decoder")
    assert dec == [1, 8, 64, 256, 1024, 2048]            # the decoder up-samples by the reversed strides
    enc = native.codec_level_rows(strides, "encoder")
    assert enc == [2048, 1024, 256, 64, 8, 1]
    assert dec[-1] == enc[0] == math.prod(strides)
    assert native.codec_level_rows((3, 5), "decoder") == [1, 5, 15]
    with pytest.raises(ValueError):
        native.codec_level_rows(strides, "both")
    # decoder: S = B * n_src items, the sources of a mixture share its length; encoder: one item per mixture
    assert native.codec_valid_rows([1, 6], 2, 4, 4) == [4, 4, 24, 24]
    assert native.codec_valid_rows([1, 5, 2], 1, 2048, 3) == [2048, 10240, 4096]
    with pytest.raises(ValueError):
        native.codec_valid_rows([1, 6], 2, 4, 5)
    with pytest.raises(ValueError):
        native.codec_valid_rows([1, 6], 0, 4, 0)


# ------------------------------------------------------------------ Python-side refusals and the keyword
class _Untouchable:
    """stands in for the loaded library: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the refusal")


def _engine(score_kind):
    e = object.__new__(native.Engine)
    e.cfg = native.DsnConfig()
    e.cfg.score_kind = score_kind
    e.lib, e.ctx, e.n_src, e.latent_dim, e.device = _Untouchable(), None, 2, 64, torch.device("cpu")
    return e


def test_padded_codec_refusals_before_the_library():
    x = torch.zeros(3, 2, 64, 5)
    for kind in (native.SCORE_DIT, native.SCORE_NCSNPP, native.SCORE_NONE):     # the codec needs no score network
        e = _engine(kind)
        for bad, msg in (((5, 0, 3), r"frames\[1\] = 0 outside \[1, T = 5\]"),
                         ((5, 2, 6), r"frames\[2\] = 6 outside \[1, T = 5\]"),
                         ((5, 2), r"one frame count per item \(B = 3\)")):
            with pytest.raises(ValueError, match=msg):
                e.decode_ragged(x, bad, [100] * 3, codec="padded")
        with pytest.raises(ValueError, match="x must be"):
            e.decode_ragged(torch.zeros(3, 1, 64, 5), (5, 2, 3), [100] * 3, codec="padded")
        for call in (lambda: e.decode_ragged(x, (5, 2, 3), [100] * 3, codec="fused"),
                     lambda: e.encode_ragged([torch.zeros(1, 4000)], codec="fused"),
                     lambda: e.separate_ragged([torch.zeros(1, 4000)], N=4, codec="fused")):
            with pytest.raises(ValueError, match="codec must be one of"):
                call()
    with pytest.raises(ValueError, match="need the DiT score network"):
        _engine(native.SCORE_NCSNPP).separate_ragged([torch.zeros(1, 4000), torch.zeros(1, 9000)], N=4, codec="padded")
    assert native.check_ragged(native.SCORE_NCSNPP, (5, 2, 3), 3, 5, need_dit=False) == [5, 2, 3]


def test_codec_keyword_defaults_to_grouped():
    from ditsep_amd.evaluate import evaluate_batches
    from ditsep_amd.latent import LatentDiffSep

    for fn in (native.Engine.encode_ragged, native.Engine.decode_ragged, native.Engine.separate_ragged,
               LatentDiffSep.separate_batch, evaluate_batches):
        assert inspect.signature(fn).parameters["codec"].default == "grouped", fn
    assert native.CODEC_MODES == ("grouped", "padded")
    for name in ("dsn_decode_ragged", "dsn_encode_ragged", "dsn_separate_ragged"):
        assert name in native.EXPORTS
    assert native.TEST_KERNEL_KINDS["codec_tail_zero"] == 23
    # the default still decodes once per group of equal frame count
    e = _engine(native.SCORE_DIT)
    calls = []

    def decode(x, target_len):
        calls.append(tuple(x.shape))
        return torch.zeros(x.shape[0], 2, 2048 * x.shape[-1])

    e.decode = decode
    out = e.decode_ragged(torch.zeros(3, 2, 64, 3), [2, 3, 2], [3000, 5000, 4000])
    assert calls == [(2, 2, 64, 2), (1, 2, 64, 3)]
    assert [tuple(o.shape) for o in out] == [(2, 3000), (2, 5000), (2, 4000)]
