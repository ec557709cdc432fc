"""bench.py's plain run, --full and --dump-outputs: the plain line carries the headline and none of
the secondary measurements, --full carries them, and --dump-outputs writes the last timed step's
images, radii and gradients as float32 .npy files within 64 MB, the same elements on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus")
SECONDARY = ("kernels", "roofline", "cpu_baseline", "sustained", "serial_one_stream", "render_mpix_s", "single_view",
             "graph", "train_step", "view_parallel_train", "init_knn", "num_rendered")


def _fake_step(P, M, H, W, K):
    # expanded scalars: C3-sized outputs without their memory
    z = torch.zeros(())
    params = [z.expand(P, 3), z.expand(P, M, 3), z.expand(P, 1), z.expand(P, 3), z.expand(P, 4)]
    for p in params:
        p.grad = torch.ones(()).expand(p.shape)
    views = {k: (torch.full((), float(k)).expand(3, H, W), torch.ones((), dtype=torch.int32).expand(P)) for k in range(K)}
    return views, params


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path):
    import bench

    P, M, H, W, K = 1_000_000, 16, 1080, 1920, 4  # C3: 236 MB of gradients, 100 MB of images
    views, params = _fake_step(P, M, H, W, K)
    s1 = bench.dump_outputs(str(tmp_path / "a"), views, params)
    s2 = bench.dump_outputs(str(tmp_path / "b"), views, params)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) == s1["bytes"] <= 64 * 10**6
    assert s1["bytes"] > 48 * 10**6  # the budget is used, not a token sample
    assert sorted(a) == sorted(b) == sorted(
        ["gaussian_rows", "pixels"] + [f"image_view{k}" for k in range(K)] + [f"radii_view{k}" for k in range(K)]
        + ["grad_means3D", "grad_shs", "grad_opacities", "grad_scales", "grad_rotations"])
    for name in a:
        assert a[name].dtype in (np.float32, np.float64)
        assert np.array_equal(a[name], b[name]), name
    rows, pix = a["gaussian_rows"], a["pixels"]
    assert s1["gaussian_rows"] == s2["gaussian_rows"] == [len(rows), P] and s1["pixels"] == [len(pix), H * W]
    assert np.all(np.diff(rows) > 0) and 0 <= rows[0] and rows[-1] < P and np.all(rows == np.floor(rows))
    assert np.all(np.diff(pix) > 0) and 0 <= pix[0] and pix[-1] < H * W
    assert a["grad_shs"].shape == (len(rows), M, 3) and a["radii_view0"].shape == (len(rows),)
    for k in range(K):
        assert a[f"image_view{k}"].shape == (3, len(pix)) and np.all(a[f"image_view{k}"] == k)


def test_dump_outputs_small_workload_is_written_whole(tmp_path):
    import bench

    P, M, H, W, K = 1000, 1, 40, 56, 2
    views, params = _fake_step(P, M, H, W, K)
    s = bench.dump_outputs(str(tmp_path / "d"), views, params)
    a = _load(tmp_path / "d")
    assert s["gaussian_rows"] == [P, P] and s["pixels"] == [H * W, H * W]
    assert np.array_equal(a["gaussian_rows"], np.arange(P)) and np.array_equal(a["pixels"], np.arange(H * W))
    assert a["image_view1"].shape == (3, H * W) and a["grad_rotations"].shape == (P, 4)


def _bench(*args):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *args], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
@pytest.mark.spawn_first
def test_plain_bench_reports_the_headline_only_and_dumps_its_last_step(tmp_path):
    d = tmp_path / "out"
    line = _bench("--workload", "c1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d))
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert len(line["regions_iters_s"]) == 1  # --steps is the number of timed steps
    vps = line["config"]["views_per_step"]
    assert line["value"] == pytest.approx(vps * 1e3 / line["ms_per_step"], rel=1e-3)
    assert not [k for k in SECONDARY if k in line]
    a = _load(d)
    P, npix = 10_000, 256 * 256  # C1 fits the budget whole
    assert line["dumped_outputs"]["gaussian_rows"] == [P, P] and line["dumped_outputs"]["pixels"] == [npix, npix]
    for k in range(vps):
        img = a[f"image_view{k}"]
        assert img.dtype == np.float32 and img.shape == (3, npix) and np.isfinite(img).all() and img.max() > 0
        assert (a[f"radii_view{k}"] > 0).any()
    for name in ("means3D", "shs", "opacities", "scales", "rotations"):
        g = a[f"grad_{name}"]
        assert g.dtype == np.float32 and g.shape[0] == P and np.isfinite(g).all() and np.abs(g).max() > 0


@pytest.mark.gpu
@pytest.mark.spawn_first
def test_full_bench_reports_the_secondary_measurements():
    line = _bench("--workload", "c1", "--steps", "3", "--warmup", "2", "--full", "--train-steps", "2",
                  "--vp-train-steps", "2", "--single-view-steps", "3", "--sustain-s", "0.05", "--cpu-runs", "1")
    for k in HEADLINE + SECONDARY:
        assert line.get(k) is not None, k
    assert line["full"] is True and len(line["regions_iters_s"]) == 5
    assert "error" not in line["view_parallel_train"]
