"""bench.py's plain line and `--dump-outputs`: the headline fields only (everything else is `--full`), and the arrays the
timed path computed in its last step, within the 64 MB budget (a seeded sample of larger arrays)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import benchlib  # noqa: E402


def test_dump_outputs_writes_small_sets_whole(tmp_path):
    a = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    b = torch.linspace(0, 1, 5)[1:]           # a view
    names = benchlib.dump_outputs(str(tmp_path / "d"), {"a": a, "b": b})
    assert names == ["a.npy", "b.npy"]
    got_a, got_b = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert got_a.dtype == np.float32 and got_a.shape == (4, 3) and np.array_equal(got_a, a.numpy())
    assert got_b.dtype == np.float32 and np.array_equal(got_b, b.numpy())


def test_dump_outputs_samples_large_sets_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(benchlib, "DUMP_BYTES", 4096)
    big = torch.arange(3000, dtype=torch.float32).reshape(1000, 3)
    small = torch.ones(10)
    runs = []
    for d in ("d1", "d2"):
        names = benchlib.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
        assert names == ["big_sample.npy", "small.npy"]
        runs.append(np.load(tmp_path / d / "big_sample.npy"))
        assert np.array_equal(np.load(tmp_path / d / "small.npy"), small.numpy())
    s = runs[0]
    assert s.dtype == np.float32 and s.size == 4096 // 4 // 2
    assert sum(os.path.getsize(tmp_path / "d1" / n) - 128 for n in names) <= 4096     # (.npy header: 128 bytes)
    assert np.all(np.diff(s) >= 0) and s.min() >= 0 and s.max() < 3000     # ascending flat indices of `big` = its values here
    assert np.array_equal(runs[0], runs[1])                                 # the same sample on every run


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "config"} <= set(d)
    assert not {"roofline", "kernels", "cpu_baseline", "exact", "dropin", "configs"} & set(d), sorted(d)
    H, W = d["config"]["H"], d["config"]["W"]
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(H * W / (d["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)

    n = d["config"]["gaussians"]
    want = {"image": (H, W, 3), "grad_sigmas": (n, 3), "grad_coords": (n, 2), "grad_colors": (n, 3)}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    arrs = {k: np.load(out / (k + ".npy")) for k in want}
    for k, shape in want.items():
        assert arrs[k].dtype == np.float32 and arrs[k].shape == shape and np.isfinite(arrs[k]).all(), k
        assert np.abs(arrs[k]).max() > 0, k
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    # the image is the render of the bench's own seeded inputs: a band of it against the double-precision oracle
    from gsasr_amd import synthetic
    from oracle import gs_oracle
    h_lr, w_lr, scale, _ = benchlib.CONFIGS["c2"]
    sig, xy, col, _, _ = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=0, device="cpu")
    rows = (H // 2, H // 2 + 8)
    ref = gs_oracle.forward_f64(sig.numpy(), xy.numpy(), col.numpy(), H, W, d["config"]["dmax"], rows=rows)
    assert np.abs(arrs["image"][rows[0]:rows[1]] - ref).max() <= 1e-4
