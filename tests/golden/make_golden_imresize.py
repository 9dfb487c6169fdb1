"""Writes tests/golden/imresize_<case>.npz: the reference's `imresize` / `imresize_new` on the cases of tests/test_imresize.py.

    python tests/golden/make_golden_imresize.py /path/to/GSASR/TrainTestGSASR/basicsr/utils/matlab_functions.py

Runs on the CPU.  The reference module is loaded by path, here and nowhere else; the files hold numbers only: the case's
parameters, the NumPy seed its input is regenerated from (`default_rng(seed).random(shape, dtype=float32)`), the reference's
float32 output, and `ref_dist` = the reference's own largest distance from the test's float64 restatement on that case.
Also prints the reference's CPU time per sample for the two shapes profiles/imresize.txt quotes, and checks that the
reference fails on 26 pixels at scale 1/16.
"""
import importlib.util
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_imresize import CASES, case_input, case_scales, resize_f64      # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_matlab_functions", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    for name, case in CASES.items():
        x = case_input(case)
        fn = getattr(ref, case["fn"])
        out = fn(x if case["kind"] == "hw" else torch.from_numpy(x), *case["scales"], antialiasing=case["aa"])
        out = np.ascontiguousarray(out if case["kind"] == "hw" else out.numpy(), dtype=np.float32)
        want = resize_f64(x, case["out"], case_scales(case), case["aa"])
        assert out.shape == want.shape, (name, out.shape, want.shape)
        dist = float(np.abs(out - want).max())
        path = os.path.join(HERE, f"imresize_{name}.npz")
        np.savez_compressed(path, fn=np.str_(case["fn"]), seed=np.int64(case["seed"]), in_hw=np.array([case["h"], case["w"]], np.int64),
                            channels=np.int64(case["c"]), scales=np.array(case_scales(case), np.float64),
                            antialiasing=np.bool_(case["aa"]), out=out, ref_dist=np.float64(dist))
        print(f"{name}: out {out.shape}, reference's distance from float64 {dist:.3e}, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 256 * 1024
    try:
        ref.imresize(torch.rand(1, 26, 26), 1 / 16)
    except Exception as e:      # noqa: BLE001
        print(f"26 pixels at 1/16: the reference raises {type(e).__name__}: {str(e).splitlines()[0][:100]}")
    else:
        raise SystemExit("the reference accepted 26 pixels at scale 1/16")
    for (h, out) in ((1024, 64), (192, 48)):
        x = torch.rand(3, h, h)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            ref.imresize_new(x, out / h, out / h)
            ts.append(time.perf_counter() - t0)
        print(f"reference on the CPU, 3x{h}x{h} -> {out}x{out}: {1e3 * sorted(ts)[2]:.2f} ms per sample (median of 5)")


if __name__ == "__main__":
    main()
