"""CPU: perceptual path length (stylerenderer_amd/ppl.py) against the reference's ppl.py — tests/golden/ppl_*.npz,
written by tests/make_golden_ppl.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppl_cases
from stylerenderer_amd import lpips, model, ppl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def path_bar(gold, name, eps):
    """Nominal bar, widened to twice the reference's own float32 error (float64 run), at most 10x."""
    d32, d64 = gold[name + "_f32"].astype(np.float64), gold[name + "_f64"]
    ref_err = float(np.abs(d32 - d64).max() / np.abs(d64).max())
    nominal = ppl_cases.NOMINAL_BAR[eps]
    return min(max(nominal, 2 * ref_err), 10 * nominal)


def check_paths(gold, name, got):
    size, space, crop, eps, sampling, key = ppl_cases.PATH_CASES[name]
    want = gold[name + "_f64"]
    assert got.shape == want.shape
    err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
    bar = path_bar(gold, name, eps)
    assert err <= bar, "%s: distance error %.3e of scale (bar %.1e)" % (name, err, bar)
    return err


@pytest.mark.parametrize("tag", ["t0", "trand", "tnear1"])
def test_lerp_slerp_match_reference(golden, tag):
    z = golden("ppl_interp")
    a, b, ts = ppl_cases.interp_inputs()
    t, a, b = torch.from_numpy(ts[tag]), torch.from_numpy(a), torch.from_numpy(b)
    assert np.array_equal(ppl.lerp(t, a, b).numpy(), z["lerp_" + tag])
    got = ppl.slerp(t, a, b).numpy()
    assert np.abs(got - z["slerp_" + tag]).max() <= 1e-6


def test_lerp_l1_form():
    a, b = torch.randn(4, 8), torch.randn(4, 8)
    w = torch.rand(4, 2) + 0.1
    want = a * (w[:, :1] / w.sum(-1, keepdim=True)) + b * (w[:, 1:] / w.sum(-1, keepdim=True))
    assert torch.allclose(ppl.lerp(w, a, b), want, rtol=1e-6, atol=1e-6)


def test_slerp_three_inputs_raises():
    x = torch.randn(2, 8)
    with pytest.raises(NotImplementedError, match="SLerp"):
        ppl.slerp(torch.rand(2, 2), x, x, x)


def test_filtered_mean_matches_reference_expression():
    d = np.abs(np.random.default_rng(5).standard_cauchy(1000)).astype(np.float32)
    lo = np.percentile(d, 1, method="lower")
    hi = np.percentile(d, 99, method="higher")
    want = np.extract(np.logical_and(lo <= d, d <= hi), d).mean()
    assert ppl.filtered_mean(d) == want
    assert ppl.filtered_mean(d) < d.mean()


@pytest.mark.parametrize("name", sorted(ppl_cases.PATH_CASES))
def test_path_lengths_match_reference(golden, name):
    size, space, crop, eps, sampling, key = ppl_cases.PATH_CASES[name]
    g = ppl_cases.make_generator(model.Generator, size)
    got = ppl.path_lengths(g, lpips.PNetLin(), ppl_cases.N_SAMPLE, ppl_cases.BATCH, space, eps, crop, sampling,
                           device="cpu", draw=ppl_cases.det_draw(key))
    check_paths(golden("ppl_paths"), name, got)


def test_batch_split_skips_empty_trailing_batch():
    assert ppl.batch_sizes(8, 4) == [4, 4]
    assert ppl.batch_sizes(10, 4) == [4, 4, 2]


def test_cli_end_to_end(tmp_path):
    g = model.Generator(32, 512, 8)
    torch.save({"g_ema": g.state_dict()}, str(tmp_path / "g.pt"))
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-m", "stylerenderer_amd.ppl", "--space", "w", "--size", "32", "--n_sample",
                        "4", "--batch", "2", "--seed", "3", "--sampling", "full", str(tmp_path / "g.pt")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ppl:")]
    assert len(line) == 1, r.stdout
    assert np.isfinite(float(line[0].split()[1]))
    assert "synthetic" in r.stderr
