"""Cases of tests/golden/ppl_*.npz (written by tests/make_golden_ppl.py from the reference's ppl.py), shared by the
fixture writer and the tests: every draw is a pure function of integer keys (synth.det_*), so the GPU machine rebuilds
the reference's inputs without any RNG agreement."""
import numpy as np
import torch

from stylerenderer_amd import synth

STYLE_DIM, N_MLP, SALT = 512, 8, 71
N_SAMPLE, BATCH = 5, 3                          # batches of 3 and 2 pairs: the trailing partial batch is exercised

# name -> (size, space, crop, eps, sampling, key)
PATH_CASES = {}
for _size, _crops in ((32, (False,)), (64, (False, True))):
    for _space in ("z", "w"):
        for _crop in _crops:
            for _eps in (1e-2, 1e-4):
                _name = "s%d_%s%s_e%d" % (_size, _space, "_crop" if _crop else "", int(round(-np.log10(_eps))))
                PATH_CASES[_name] = (_size, _space, _crop, _eps, "full" if _size == 32 else "end",
                                     9000 + 100 * len(PATH_CASES))

# nominal relative bars of the per-pair distances (max |err| / max |value|), before any widening from the reference's own
# float32 error (see tests/test_ppl_cpu.py)
NOMINAL_BAR = {1e-2: 2e-4, 1e-4: 2e-2}

# lerp / slerp fixtures: B = 16 pairs of D = 512 at t = 0, random t in [0, 1) and t near 1
INTERP_B, INTERP_D = 16, 512


def interp_inputs():
    a = synth.det_normal((INTERP_B, INTERP_D), 8101)
    b = synth.det_normal((INTERP_B, INTERP_D), 8102)
    ts = {"t0": np.zeros((INTERP_B, 1), np.float32),
          "trand": ((synth.det_uniform((INTERP_B, 1), 8103) + 1) / 2).astype(np.float32),
          "tnear1": (1 - np.abs(synth.det_uniform((INTERP_B, 1), 8104)) * 1e-3).astype(np.float32)}
    return a, b, ts


def make_generator(cls, size):
    """cls(size, 512, 8) (the product's or the reference's Generator) with the deterministic fill of `size`."""
    g = cls(size, STYLE_DIM, N_MLP)
    synth.fill_state_dict(g.state_dict(), salt=SALT + size)
    return g.eval()


def det_draw(key):
    """A draw(g, batch, sampling, device) for ppl.path_lengths: batch j of case `key` -> (noise, inputs, t)."""
    count = [0]

    def draw(g, batch, sampling, device):
        k = key + 10 * count[0]
        count[0] += 1
        noise = [torch.from_numpy(synth.det_normal(tuple(n.shape), 100 * k + i))
                 for i, n in enumerate(g.make_noise())]
        inputs = torch.from_numpy(synth.det_normal((2 * batch, g.style_dim), 100 * k + 50))
        if sampling == "full":
            t = torch.from_numpy(((synth.det_uniform((batch,), 100 * k + 60) + 1) / 2).astype(np.float32))
        else:
            t = torch.zeros(batch)
        return ([n.to(device) for n in noise], inputs.to(device), t.to(device))

    return draw


def batch_sizes(n_sample, batch):
    """The reference's batch split (ppl.py:136-138) without its empty trailing batch."""
    n_batch = n_sample // batch
    resid = n_sample - n_batch * batch
    return [batch] * n_batch + ([resid] if resid else [])
