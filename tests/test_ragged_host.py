"""Host-side rules of the ragged (mixed-length) batches, no GPU: how a data set is cut into batches
(evaluate.length_batches), how an item is grouped and zero-extended before its group is encoded (native.latent_frames_of,
ragged_extended_length, frame_groups) and the refusals the Python entry points raise before the library is touched."""
import pytest
import torch

from ditsep_amd import native
from ditsep_amd.evaluate import length_batches
from oracle import sampler

HOP = 2048


def test_length_batches_partition_sorted():
    g = torch.Generator().manual_seed(5)
    lengths = torch.randint(32000, 64000, (23,), generator=g).tolist()
    lengths[7] = lengths[3]                                        # a tie
    batches = length_batches(lengths, 4)
    flat = [i for b in batches for i in b]
    assert sorted(flat) == list(range(23)), "every index exactly once"
    assert [len(b) for b in batches] == [4] * 5 + [3]
    assert [lengths[i] for i in flat] == sorted(lengths), "sorted by length across and within the cuts"
    assert length_batches([], 4) == []
    assert length_batches([9, 1], 5) == [[1, 0]]
    with pytest.raises(ValueError):
        length_batches([1, 2], 0)


@pytest.mark.parametrize("L", [4000, 4095, 4096, 4097, 6143])
def test_zero_extension_rule(L):
    """An item zero-extended to T_b hop - 1 samples pads (by the reference's rule, oracle sampler.pad_to_hop) to the same
    signal as the item itself: same frame count, same samples, zeros after."""
    T = native.latent_frames_of(L, HOP)
    x = torch.arange(1, L + 1, dtype=torch.float32).reshape(1, 1, L)
    own = sampler.pad_to_hop(x, HOP)
    assert own.shape[-1] == T * HOP
    Lx = native.ragged_extended_length(L, HOP)
    assert Lx == T * HOP - 1 and L <= Lx
    ext = torch.zeros(1, 1, Lx)
    ext[..., :L] = x
    assert torch.equal(sampler.pad_to_hop(ext, HOP), own)


def test_frame_groups():
    frames = [native.latent_frames_of(L, HOP) for L in (4000, 6143, 9000, 4095, 4096)]
    assert frames == [2, 3, 5, 2, 3]
    assert native.frame_groups(frames) == {2: [0, 3], 3: [1, 4], 5: [2]}


class _Untouchable:
    """stands in for the loaded library: any use fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name}) before the refusal")


def _engine(score_kind):
    e = object.__new__(native.Engine)
    e.cfg = native.DsnConfig()
    e.cfg.score_kind = score_kind
    e.lib, e.ctx, e.n_src, e.latent_dim = _Untouchable(), None, 2, 64
    return e


def test_ragged_refusals_before_the_library():
    B, n, D, T = 3, 2, 64, 20
    xt, t, y = torch.zeros(B, n, D, T), torch.ones(B), torch.zeros(B, 1, D, T)
    dit, ncsn = _engine(native.SCORE_DIT), _engine(native.SCORE_NCSNPP)
    with pytest.raises(ValueError, match="need the DiT score network"):
        ncsn.score(xt, t, y, frames=(20, 15, 3))
    with pytest.raises(ValueError, match="need the DiT score network"):
        ncsn.pc_sample(y, None, N=4, frames=(20, 15, 3))
    with pytest.raises(ValueError, match="need the DiT score network"):
        ncsn.separate_ragged([torch.zeros(1, 4000), torch.zeros(1, 9000)], N=4)
    for bad, msg in (((20, 0, 3), r"frames\[1\] = 0 outside \[1, T = 20\]"),
                     ((20, 15, 21), r"frames\[2\] = 21 outside \[1, T = 20\]"),
                     ((20, 15), r"one frame count per item \(B = 3\)")):
        with pytest.raises(ValueError, match=msg):
            dit.score(xt, t, y, frames=bad)
        with pytest.raises(ValueError, match=msg):
            dit.pc_sample(y, None, N=4, frames=bad)
    with pytest.raises(ValueError, match="langevin corrector has no ragged form"):
        dit.pc_sample(y, None, N=4, corrector="langevin", frames=(20, 15, 3))
    # and the rule itself hands back the counts it accepted
    assert native.check_ragged(native.SCORE_DIT, (20, 15, 3), B, T) == [20, 15, 3]
