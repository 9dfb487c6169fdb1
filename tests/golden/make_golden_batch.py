"""Writes tests/golden/batch_<case>.npz: the reference's training samples on the cases of tests/test_make_batch.py.

    python tests/golden/make_golden_batch.py /path/to/GSASR/TrainTestGSASR/basicsr

Runs on the CPU.  Two reference modules are loaded by path, here and nowhere else: utils/matlab_functions.py (`imresize_new`)
and data/transforms.py (`augment`).  transforms.py imports `cv2`, which this script replaces for that import by a NumPy stand-in
for `cv2.flip` (flipCode 1: columns reversed, 0: rows reversed, written to `dst`), and `basicsr.utils.matlab_functions`, which it
gets as the module loaded by path.  `augment` draws its three booleans from `random`; the script gives its module a `random`
that answers 0.0 or 1.0 so that each case's flags come out, and checks them through `return_status`.  The two lines of
utils/img_util.py `img2tensor` (BGR -> RGB, HWC -> CHW, float) are restated here: that module needs torchvision.  Each sample
follows data/continuous_bicubic_downsample_dataset.py:49-98: `astype(float32) / 255.`, the crop, `imresize_new(crop,
1 / scale_modify_h, 1 / scale_modify_w)`, `augment([gt, lq])`, img2tensor, `F.pad` to the case's gt_pad.

The files hold arrays only: the source bytes `src` (regenerated from the case's seed and compared by the test), `crops` [B,4],
`flags` [B,3] = (hflip, vflip, rot90), `lr` [2], `gt_pad` [2], and the reference's `gt` [B,3,Gh,Gw] and `lq` [B,3,lh,lw].
Before anything is recorded, `axis_taps` checks the resize's reflection condition on every sample.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_make_batch import CASES, case_pad, case_source      # noqa: E402

from gsasr_amd.resize import axis_taps      # noqa: E402


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def numpy_flip(src, flipCode, dst=None):
    out = np.ascontiguousarray(src[:, ::-1] if flipCode == 1 else src[::-1] if flipCode == 0 else src[::-1, ::-1])
    if dst is None:
        return out
    dst[...] = out
    return dst


class Answers:
    """`random` for augment: random() < 0.5 exactly where the flag is wanted"""

    def __init__(self, flags):
        self.values = [0.0 if f else 1.0 for f in flags]

    def random(self):
        return self.values.pop(0)


def load_reference(basicsr):
    matlab = load("reference_matlab_functions", os.path.join(basicsr, "utils", "matlab_functions.py"))
    saved = {k: sys.modules.get(k) for k in ("cv2", "basicsr", "basicsr.utils", "basicsr.utils.matlab_functions")}
    sys.modules["cv2"] = types.SimpleNamespace(flip=numpy_flip)
    sys.modules["basicsr"] = types.ModuleType("basicsr")
    sys.modules["basicsr.utils"] = types.ModuleType("basicsr.utils")
    sys.modules["basicsr.utils.matlab_functions"] = matlab
    try:
        transforms = load("reference_transforms", os.path.join(basicsr, "data", "transforms.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return matlab, transforms


def img2tensor(img):
    """utils/img_util.py:29-37 with bgr2rgb=True, float32=True, restated"""
    return torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1]).transpose(2, 0, 1).copy()).float()


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    matlab, transforms = load_reference(sys.argv[1])
    for name, case in CASES.items():
        src = case_source(case)
        lh, lw = case["lr"]
        Gh, Gw = case_pad(case)
        gts, lqs = [], []
        for (y0, x0, gh, gw), flags in zip(case["crops"], case["flags"]):
            axis_taps(gh, lh, lh / gh)
            axis_taps(gw, lw, lw / gw)
            img_gt = src.astype(np.float32) / 255.
            crop_gt = img_gt[y0:y0 + gh, x0:x0 + gw, :]
            scale_modify_h, scale_modify_w = float(crop_gt.shape[0] / lh), float(crop_gt.shape[1] / lw)
            crop_lr = np.ascontiguousarray(matlab.imresize_new(img=crop_gt, scale_h=1 / scale_modify_h, scale_w=1 / scale_modify_w, antialiasing=True))
            assert crop_lr.shape == (lh, lw, 3), crop_lr.shape
            transforms.random = Answers(flags)
            (a_gt, a_lq), status = transforms.augment([crop_gt, crop_lr], True, True, return_status=True)
            assert tuple(int(bool(s)) for s in status) == tuple(flags) and not transforms.random.values
            t_gt, t_lq = img2tensor(a_gt), img2tensor(a_lq)
            gts.append(F.pad(t_gt, (0, Gw - t_gt.shape[2], 0, Gh - t_gt.shape[1]), "constant", 0))
            lqs.append(t_lq)
        gt, lq = torch.stack(gts).numpy(), torch.stack(lqs).numpy()
        path = os.path.join(HERE, f"batch_{name}.npz")
        np.savez_compressed(path, src=src, crops=np.array(case["crops"], np.int64), flags=np.array(case["flags"], np.int64),
                            lr=np.array(case["lr"], np.int64), gt_pad=np.array([Gh, Gw], np.int64), gt=gt.astype(np.float32), lq=lq.astype(np.float32))
        print(f"{name}: gt {gt.shape}, lq {lq.shape}, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
