"""CPU: adaptive discriminator augmentation (ADA).  The composite utils_3d form split into draw / apply halves, the ADA p
controller against the eager trainer's host recurrence, graph_train.GraphedTrainer with augment=True (one rank and two
gloo ranks), the C-ABI argument checks of sr_ada_*, and `train --augment --data`."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from stylerenderer_amd import checkpoint, dataset, graph_train, synth, train
from stylerenderer_amd import distributed as sr_dist
from stylerenderer_amd import utils_3d as u
from stylerenderer_amd.op import augment as ada

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, LATENT, NMLP, BATCH = 8, 32, 2, 4


def images(b=5, h=20, w=24, seed=5):
    return torch.from_numpy(synth.det_uniform((b, 3, h, w), seed))


# ---- composite refactor --------------------------------------------------------------------------------------------
def test_draw_apply_halves_reproduce_the_public_functions():
    img = images()
    p6, p5 = [.3, .2, .4, .3, .1, .5], [.3, .3, .5, .4, .5]
    for seed in (1, 2):
        torch.manual_seed(seed)
        want = u.random_apply_pose2D_img(p=p6, img=img)
        torch.manual_seed(seed)
        ps = u._pose2d_sigmas(p6)
        assert torch.equal(want, u._pose2d_from_draws(img, u._pose2d_draws(5, ps), ps))
        torch.manual_seed(seed)
        want = u.random_apply_color(p=p5, img=img)
        torch.manual_seed(seed)
        cs = u._color_sigmas(p5)
        assert torch.equal(want, u._color_from_draws(img, u._color_draws(5, cs), cs))
        torch.manual_seed(seed)
        want = u.augment(img, 0.6)
        torch.manual_seed(seed)
        zp = u._pose2d_draws(5, u._pose2d_sigmas([.1, .1, .05, .15, 0, .5]))
        zc = u._color_draws(5, u._color_sigmas([.2, .3, 0, .15, .5]))
        pick = torch.rand(5, 1, 1, 1)
        assert torch.equal(want, u._augment_from_draws(img, zp, zc, pick, 0.6))


def test_augment_takes_a_tensor_probability_and_keeps_unselected_samples():
    img = images(8)
    torch.manual_seed(3)
    out = u.augment(img, torch.tensor(0.5, dtype=torch.float64))
    kept = [bool(torch.equal(out[i], img[i])) for i in range(8)]
    assert 0 < sum(kept) < 8
    torch.manual_seed(3)
    assert torch.equal(u.augment(img, torch.tensor(0.0, dtype=torch.float64)), img)


def test_composite_of_native_draws_identity_and_flip():
    """The oracle the GPU tests use: zero sigmas are the identity; a flip probability above one mirrors the image."""
    img = images(3, 16, 12).double()
    raw = torch.randn(3, ada.NDRAW)
    out = ada.composite_from_draws(img, raw, 1.0, pose_p=[0] * 6, color_p=[0] * 5)
    assert float((out - img).abs().max()) < 1e-12
    out = ada.composite_from_draws(img, raw, 1.0, pose_p=[0, 0, 0, 0, 0, 1.1], color_p=[0] * 5)
    assert float((out - img.flip(3)).abs().max()) < 1e-12
    assert torch.equal(ada.composite_from_draws(img, raw, 0.0), img)


# ---- the p controller ----------------------------------------------------------------------------------------------
def host_recurrence(stats, target, length, p0=0.0):
    """train.Trainer.step's ADA update (float32 accumulator, Python floats), over a sequence of (sign sum, count)."""
    acc = torch.zeros(2)
    p, rt, out = p0, 0.0, []
    for s in stats:
        acc += torch.tensor(s, dtype=torch.float32)
        if float(acc[1]) > 255:
            pred_signs, n_pred = acc.tolist()
            rt = pred_signs / n_pred
            sign = 1 if rt > target else -1
            p = min(1.0, max(0.0, p + sign * target / length * n_pred))
            acc.mul_(0)
        out.append((p, rt))
    return out


def scripted_stats():
    rng = np.random.RandomState(0)
    stats = []
    for phase in range(6):                      # mostly-positive, then mostly-negative D(real): p climbs, then falls
        bias = 0.9 if phase % 2 == 0 else -0.9
        for _ in range(80):
            signs = np.sign(rng.rand(8) - 0.5 + bias * 0.5)
            stats.append((float(signs.sum()), 8.0))
    return stats


def test_composite_controller_equals_the_host_recurrence_exactly():
    stats = scripted_stats()
    target, length = 0.6, 200.0                 # each crossing moves p by 0.6 / 200 * 256 = 0.77: clamps at both ends
    want = host_recurrence(stats, target, length)
    state = torch.zeros(4, dtype=torch.float64)
    got = []
    for s in stats:
        ada.update(state, torch.tensor(s, dtype=torch.float32), target, length)
        got.append((float(state[2]), float(state[3])))
    assert got == want
    ps = [p for p, _ in want]
    crossings = sum(1 for a, b in zip(ps, ps[1:]) if a != b)
    assert crossings >= 8 and ps.count(1.0) > 1 and 0.0 in ps[ps.index(1.0):]
    assert any(0.0 < p < 1.0 for p in ps)


# ---- graphed trainer with augment=True -----------------------------------------------------------------------------
def make_trainer(**kw):
    v0, _ = synth.uv_ellipsoid(16, 14)
    return graph_train.GraphedTrainer(size=SIZE, latent=LATENT, n_mlp=NMLP, device="cpu", seed=3, use_mesh=True,
                                      batch=BATCH, mesh_vertices=v0.shape[0], capture=False, n_buckets=2, augment=True,
                                      **kw)


def test_graphed_trainer_trains_with_augment_and_checkpoints_p(tmp_path):
    tr = make_trainer(ada_length=1000)
    assert tr.ada_adaptive and tr.ada_aug_p == 0.0
    mesh = train.synthetic_mesh(BATCH, "cpu", seed=1, face_sized=False)
    data = train.SyntheticImages(8, SIZE, "cpu")
    for _ in range(66):                         # 64 x 4 > 255: one update of p, then 2 more iterations
        log = tr.step(data.batch(BATCH), mesh=mesh, log=False)
    assert all(torch.isfinite(v).all() for v in log.values())
    assert float(tr.s_ada[1]) == 2 * BATCH and tr.ada_aug_p in (0.0, 0.6 / 1000 * 256)
    tr.ada_aug_p = 0.375
    path = checkpoint.save_checkpoint(str(tmp_path / "000066.pt"), tr)
    assert torch.load(path, weights_only=False)["ada_aug_p"] == 0.375
    other = make_trainer()
    checkpoint.load_checkpoint(path, other)
    assert other.ada_aug_p == 0.375 and float(other.s_ada[2]) == 0.375
    fixed = make_trainer(augment_p=0.25)
    assert not fixed.ada_adaptive
    fixed.step(data.batch(BATCH), mesh=mesh)
    assert fixed.ada_aug_p == 0.25 and float(fixed.s_ada[1]) == 0.0


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    torch.cuda.is_available = lambda: False
    sr_dist.initialize(backend="gloo")
    tr = make_trainer(ada_length=500)
    mesh = train.synthetic_mesh(BATCH, "cpu", seed=1 + rank, face_sized=False)
    data = train.SyntheticImages(8, SIZE, "cpu")
    ps, stats = [], []
    for _ in range(100):                        # 100 x 4 x 2 ranks = 800 samples: three crossings of 255
        tr.step(data.batch(BATCH), mesh=mesh, log=False)
        stats.append(tuple(tr.s_ada_stat.tolist()))
        ps.append(tr.ada_aug_p)
    torch.save({"ps": ps, "stats": stats, "flat": tr.g_optim.flat_p.clone(), "rt": tr.r_t_stat},
               os.path.join(outdir, "r%d.pt" % rank))
    sr_dist.synchronize()
    torch.distributed.destroy_process_group()


def test_two_ranks_share_p_through_threshold_crossings(tmp_path):
    mp.spawn(worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = [torch.load(str(tmp_path / ("r%d.pt" % r)), weights_only=False) for r in range(2)]
    assert r0["ps"] == r1["ps"] and r0["stats"] == r1["stats"]
    assert all(s[1] == 2 * BATCH for s in r0["stats"])                    # the statistic is summed over both ranks
    want = host_recurrence(r0["stats"], 0.6, 500)
    assert [p for p, _ in want] == r0["ps"] and want[-1][1] == r0["rt"] == r1["rt"]
    assert len({rt for _, rt in want}) >= 4                                 # three updates (r_t starts at 0)
    assert torch.equal(r0["flat"], r1["flat"])


# ---- C ABI ---------------------------------------------------------------------------------------------------------
def test_ada_entry_points_reject_bad_arguments_before_any_launch():
    import ctypes

    from stylerenderer_amd import _lib

    L = _lib.lib()
    sig = (ctypes.c_float * 6)(*ada.POSE_P)
    col = (ctypes.c_float * 5)(*ada.COLOR_P)
    assert L.sr_abi_version() == 12
    assert L.sr_ada_params(None, None, 4, sig, col, None, 0.5, 8, 8, None) == -1       # NULL record / draws
    assert L.sr_ada_params(None, None, 0, sig, col, None, 0.5, 8, 8, None) == 0        # nothing to do
    assert L.sr_ada_params(None, None, 4, sig, col, None, 0.5, 0, 8, None) == -1       # empty image
    assert L.sr_ada_params(None, None, -1, sig, col, None, 0.5, 8, 8, None) == -1
    assert L.sr_ada_params(None, None, 4, None, None, None, 0.5, 8, 8, None) == -1
    assert L.sr_ada_apply(None, None, None, 2, 8, 8, 1, None) == -1
    assert L.sr_ada_apply(None, None, None, 2, 8, 8, 2, None) == -1                    # with_bias is 0 or 1
    assert L.sr_ada_apply(None, None, None, 0, 8, 8, 1, None) == 0
    assert L.sr_ada_apply(None, None, None, 2, 8, -3, 1, None) == -1
    assert L.sr_ada_apply_grad(None, None, None, 2, 8, 8, None) == -1
    assert L.sr_ada_apply_grad(None, None, None, 0, 8, 8, None) == 0
    assert L.sr_ada_update(None, None, 0.6, 500.0, None) == -1
    buf = ctypes.create_string_buffer(64)
    assert L.sr_ada_update(buf, buf, 0.6, 0.0, None) == -1                             # length must be positive
    big = ctypes.create_string_buffer(64)
    assert L.sr_ada_apply(big, buf, buf, 70000, 8, 8, 1, None) == -2                   # batch beyond the grid's y range


# ---- CLI -----------------------------------------------------------------------------------------------------------
def test_train_cli_augment_on_a_store(tmp_path):
    store = str(tmp_path / "store")
    rng = np.random.RandomState(0)
    imgs = [{16: rng.randint(0, 256, (16, 16, 3), dtype=np.uint8)} for _ in range(16)]
    dataset.write_store(store, imgs, [16], fmt="NPY")
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    cmd = [sys.executable, "-m", "stylerenderer_amd.train", "--size", "16", "--latent", "32", "--n_mlp", "2",
           "--batch", "4", "--iter", "2", "--augment", "--data", store, "--save", str(tmp_path / "out.pt")]
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.count("iter ") == 2
    ck = torch.load(str(tmp_path / "out.pt"), weights_only=False)
    assert ck["args"]["augment"] and 0.0 <= ck["ada_aug_p"] <= 1.0


def test_store_images_follow_the_training_transform(tmp_path):
    store = {}
    imgs = [{8: np.full((8, 8, 3), 10 * i, dtype=np.uint8)} for i in range(6)]
    dataset.write_store(store, imgs, [8], fmt="NPY")
    data = train.StoreImages(store, 8, 3, "cpu")
    seen = set()
    for _ in range(4):
        b = data.batch(3)
        assert tuple(b.shape) == (3, 3, 8, 8) and b.dtype == torch.float32
        seen.update(round(float(x), 4) for x in b[:, 0, 0, 0])
    want = {round((10 * i / 255.0 - 0.5) / 0.5, 4) for i in range(6)}
    assert seen <= want and len(seen) >= 4
    with pytest.raises(ValueError):
        train.StoreImages(store, 8, 7, "cpu")
