"""Record the reference's own multi-resolution STFT and waveform losses into tests/golden/mrstft.npz.

    python scripts/make_golden_mrstft.py /path/to/reference

Loads stable_audio_tools/training/losses/auraloss.py and losses.py of the reference checkout by file path (the
package __init__ pulls in torchaudio) and runs MultiResolutionSTFTLoss / AuralossLoss / L1Loss / MSELoss / PITLoss on
the inputs of tests/mrstft_restatement.py::CASES, in float32 (as the reference runs) and in float64 (module.double(),
window cast).  Per case it stores the inputs, the reference's A-weighting taps, every permutation's MR-STFT value,
the output="full" terms of the identity permutation per resolution, and the PITLoss values of the MR-STFT (weight 1),
L1 (weight 15) and L2 (weight 1) terms."""
import importlib.util
import os
import sys
from itertools import permutations

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import mrstft_restatement as R  # noqa: E402

L1_WEIGHT = 15.0


def load(ref_root, name):
    path = os.path.join(ref_root, "src", "stable_audio_tools", "training", "losses", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mrstft(aura, fs, dtype, **kw):
    m = aura.MultiResolutionSTFTLoss(sample_rate=fs, fft_sizes=list(R.FFT_SIZES), hop_sizes=list(R.HOP_SIZES),
                                     win_lengths=list(R.FFT_SIZES), perceptual_weighting=True, **kw)
    if dtype == torch.float64:
        m = m.double()
        for f in m.stft_losses:
            f.window = f.window.double()
    return m


def main(ref_root):
    aura, losses = load(ref_root, "auraloss"), load(ref_root, "losses")
    torch.set_num_threads(16)
    out = {}
    for name, (fs, B, n, L, _) in R.CASES.items():
        reals, decoded = R.make_case(name)
        out[f"{name}_reals"], out[f"{name}_decoded"] = reals, decoded
        out[f"{name}_taps"] = aura.FIRFilter("aw", fs=fs).fir.weight.data.reshape(-1).numpy()
        perms = list(permutations(range(n)))
        out[f"{name}_perms"] = np.array(perms)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            x, y = torch.from_numpy(reals).to(dtype), torch.from_numpy(decoded).to(dtype)
            info = {"reals": x, "decoded": y}
            base = losses.AuralossLoss(mrstft(aura, fs, dtype), input_key="decoded", target_key="reals", name="m")
            vals = [float(base({"reals": x, "decoded": y[:, p]})) for p in perms]
            out[f"{name}_perm_values_{tag}"] = np.array(vals)
            full = losses.AuralossLoss(mrstft(aura, fs, dtype, output="full"), input_key="decoded",
                                       target_key="reals", name="m")
            total, sc, lg, _, _ = full.loss_module(x, y)
            assert abs(float(total) - vals[0]) <= 1e-6 * abs(vals[0])
            out[f"{name}_sc_{tag}"] = np.array([s.reshape(B, n).double().numpy() for s in sc])       # [R,B,n]
            out[f"{name}_log_mag_{tag}"] = np.array([float(v) for v in lg])                          # [R]
            mods = {"mrstft": base,
                    "l1": losses.L1Loss(key_a="reals", key_b="decoded", weight=L1_WEIGHT, name="l1"),
                    "l2": losses.MSELoss(key_a="reals", key_b="decoded", weight=1.0, name="l2")}
            for key, mod in mods.items():
                mod = mod.to(dtype)
                p = losses.PITLoss(mod, input_key="decoded", target_key="reals", name="pit_" + key)
                out[f"{name}_pit_{key}_{tag}"] = np.array(float(p(info)))
        print(name, "fp32 vs fp64, relative:",
              float(np.abs(out[f"{name}_perm_values_f32"] / out[f"{name}_perm_values_f64"] - 1).max()))
    path = os.path.join(ROOT, "tests", "golden", "mrstft.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
