"""CPU: the FID Inception trunk (stylerenderer_amd/inception.py), calc_fid and the two CLIs (fid.py,
calc_inception.py) against the reference's inception.py / fid.py — tests/golden/fid_*.npz, written by
tests/make_golden_fid.py."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import fid_cases
from stylerenderer_amd import dataset, fid, inception, model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_error(gold, key):
    f32, f64 = gold[key + "_f32"].astype(np.float64), gold[key + "_f64"]
    return float(np.abs(f32 - f64).max() / np.abs(f64).max())


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def net():
    return inception.InceptionV3FID()


@pytest.mark.parametrize("name", sorted(fid_cases.NET_CASES))
def test_network_matches_reference(golden, net, name):
    gold = golden("fid_net")
    x = torch.from_numpy(fid_cases.images(name))
    with torch.no_grad():
        feat, blocks = net(x, return_blocks=True)
    for k, blk in enumerate(blocks):
        key = "%s_blk%d" % (name, k)
        err = rel_err(blk.mean((2, 3)).numpy(), gold[key + "_f64"])
        assert err <= max(1e-5, 10 * ref_error(gold, key)), "%s: %.3e" % (key, err)
    key = name + "_feat"
    err = rel_err(feat.numpy(), gold[key + "_f64"])
    # same composite form as the reference: within a few times the reference's own float32 error
    assert err <= max(1e-5, 10 * ref_error(gold, key)), "%s: %.3e" % (key, err)
    assert feat.shape == (fid_cases.NET_CASES[name][0], 2048)


def test_float64_network_matches_reference_float64(golden):
    gold = golden("fid_net")
    net64 = inception.InceptionV3FID().double()
    x = torch.from_numpy(fid_cases.images("s64")).double()
    with torch.no_grad():
        feat = net64(x)
    assert rel_err(feat.numpy(), gold["s64_feat_f64"]) <= 1e-12


def test_synthetic_features_neither_zero_nor_exploding(net):
    x = torch.from_numpy(fid_cases.images("s64"))
    with torch.no_grad():
        f = net(x)
    assert torch.isfinite(f).all()
    assert (f > 0).float().mean() > 0.5          # most of the 2048 pooled ReLU features are live
    assert 0.01 < f.abs().mean() < 10 and f.abs().max() < 100
    assert (f[0] - f[1]).abs().max() > 1e-3      # and they depend on the image


def test_state_dict_keys_are_torchvision_names(net):
    keys = inception.trunk_keys(net)
    assert "Conv2d_1a_3x3.conv.weight" in keys
    assert "Mixed_5b.branch1x1.bn.running_var" in keys
    assert "Mixed_7c.branch3x3dbl_3b.conv.weight" in keys
    assert not any(k.endswith("num_batches_tracked") for k in keys)
    assert set(keys) == set(inception.synthetic_state(net))


def test_load_ignores_fc_and_aux_and_requires_every_trunk_key():
    net = inception.InceptionV3FID()
    state = {k: v * 0.5 for k, v in inception.synthetic_state(net).items()}
    extra = dict(state)
    extra["fc.weight"] = torch.zeros(1008, 2048)
    extra["fc.bias"] = torch.zeros(1008)
    extra["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    extra["Mixed_5b.branch1x1.bn.num_batches_tracked"] = torch.tensor(0)
    inception.load_inception_state(net, extra)
    assert torch.equal(net.Mixed_6a.branch3x3.conv.weight, state["Mixed_6a.branch3x3.conv.weight"])
    missing = dict(state)
    del missing["Mixed_7b.branch_pool.bn.running_mean"]
    with pytest.raises(KeyError, match="Mixed_7b.branch_pool.bn.running_mean"):
        inception.load_inception_state(net, missing)


def test_weights_file_names_trunk_by_sha256(tmp_path):
    net = inception.InceptionV3FID()
    assert net.trunk_name == "synthetic"
    path = str(tmp_path / "w.pth")
    torch.save(inception.synthetic_state(net), path)
    net.load_weights_file(path)
    assert len(net.trunk_name) == 64 and net.trunk_name == inception.file_sha256(path)


@pytest.mark.parametrize("name", sorted(fid_cases.FID_CASES))
def test_calc_fid_matches_reference(golden, name):
    gold = golden("fid_calc")
    s, r = fid_cases.fid_inputs(name)
    (ms, cs), (mr, cr) = fid_cases.stats(s), fid_cases.stats(r)
    got = fid.calc_fid(ms, cs, mr, cr)
    assert abs(got - gold[name]) <= 1e-8 * abs(gold[name])


def test_calc_fid_closed_form_for_diagonal_covariances():
    rng = np.random.default_rng(1)
    a, b = rng.uniform(0.1, 2, 64), rng.uniform(0.1, 2, 64)
    m1, m2 = rng.normal(size=64), rng.normal(size=64)
    want = ((m1 - m2) ** 2).sum() + (a + b - 2 * np.sqrt(a * b)).sum()
    assert abs(fid.calc_fid(m1, np.diag(a), m2, np.diag(b)) - want) <= 1e-10 * want


def test_calc_fid_singular_retry_adds_eps(monkeypatch, capsys):
    """The retry branch: a non-finite square root of the product is recomputed on (S1 + eps I)(S2 + eps I)."""
    real = fid.linalg.sqrtm
    calls = []

    def sqrtm(m, disp=True):
        calls.append(m.copy())
        if len(calls) == 1:
            return np.full_like(m, np.nan), 0.0
        return real(m, disp=disp)

    monkeypatch.setattr(fid.linalg, "sqrtm", sqrtm)
    a, b = np.diag([1.0, 0.0, 2.0]), np.diag([0.0, 3.0, 2.0])
    got = fid.calc_fid(np.zeros(3), a, np.zeros(3), b, eps=1e-6)
    assert "singular" in capsys.readouterr().out
    assert np.allclose(calls[1], (a + 1e-6 * np.eye(3)) @ (b + 1e-6 * np.eye(3)))
    e = 1e-6
    want = np.trace(a) + np.trace(b) - 2 * (np.sqrt((1 + e) * e) + np.sqrt(e * (3 + e)) + (2 + e))
    assert abs(got - want) < 1e-9


def test_calc_fid_imaginary_component_raises(monkeypatch):
    monkeypatch.setattr(fid.linalg, "sqrtm", lambda m, disp=True: (np.eye(2) * (1 + 1j), 0.0))
    with pytest.raises(ValueError, match="Imaginary component"):
        fid.calc_fid(np.zeros(2), np.eye(2), np.zeros(2), np.eye(2))


def test_feature_stats_cpu_matches_np_cov():
    f = fid_cases.features(157, 96, 77, offset=3.0)
    st = inception.FeatureStats()
    for lo, hi in ((0, 5), (5, 64), (64, 65), (65, 157)):
        st.update(torch.from_numpy(f[lo:hi]))
    mean, cov = st.finalize()
    want_m, want_c = fid_cases.stats(f)
    assert mean.dtype == np.float64 and cov.dtype == np.float64
    assert rel_err(mean, want_m) <= 1e-12 and rel_err(cov, want_c) <= 1e-10


def test_batch_split_skips_empty_trailing_batch():
    assert fid.batch_sizes(8, 4) == [4, 4]
    assert fid.batch_sizes(10, 4) == [4, 4, 2]


def _env():
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def make_store(path, n=5, res=32):
    rng = np.random.default_rng(3)
    imgs = [{res: rng.integers(0, 256, (res, res, 3), dtype=np.uint8)} for _ in range(n)]
    dataset.write_store(str(path), imgs, [res], fmt="PNG")


def test_cli_calc_inception_then_fid(tmp_path):
    make_store(tmp_path / "store")
    stats = str(tmp_path / "stats.pkl")
    r = subprocess.run([sys.executable, "-m", "stylerenderer_amd.calc_inception", "--size", "32", "--batch", "2",
                        "--n_sample", "4", "--out", stats, str(tmp_path / "store")],
                       cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "synthetic" in r.stderr
    with open(stats, "rb") as f:
        data = pickle.load(f)
    assert set(data) == {"mean", "cov", "size", "path", "inception"}
    assert data["mean"].dtype == np.float64 and data["mean"].shape == (2048,)
    assert data["cov"].dtype == np.float64 and data["cov"].shape == (2048, 2048)
    assert data["size"] == 32 and data["inception"] == "synthetic"
    assert np.allclose(data["cov"], data["cov"].T)

    g = model.Generator(32, 512, 8)
    torch.save({"g_ema": g.state_dict()}, str(tmp_path / "g.pt"))
    r = subprocess.run([sys.executable, "-m", "stylerenderer_amd.fid", "--inception", stats, "--size", "32",
                        "--n_sample", "4", "--batch", "2", "--seed", "3", "--truncation", "0.7",
                        "--truncation_mean", "16", str(tmp_path / "g.pt")],
                       cwd=str(tmp_path), env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("fid:")]
    assert len(line) == 1, r.stdout
    assert np.isfinite(float(line[0].split()[1]))
    assert "synthetic" in r.stderr
    assert "different feature spaces" not in r.stderr


def test_fid_warns_on_trunk_mismatch(capsys):
    fid.warn_trunk("synthetic", False, {"inception": "ab" * 32})
    err = capsys.readouterr().err
    assert "not comparable with published FID" in err and "different feature spaces" in err
    fid.warn_trunk("ab" * 32, True, {"inception": "ab" * 32})
    assert capsys.readouterr().err == ""
