"""Writes tests/golden/attention_<self|cross>_<12|16>.npz: the reference's `GSSelfAttn` and `WindowCrossAttn` on the cases of
tests/test_window_attention.py.

    python tests/golden/make_golden_attention.py /path/to/GSASR/utils/fea2gs.py

Runs on the CPU in well under a second.  The reference module is loaded by path, here and nowhere else; the files hold numbers
only: the modules' weights (seeded `randn / sqrt(dim)`), `relative_position_index`, the bias table the module initialised
perturbed by 0.5 randn, the reference's fp32 output on the case's inputs and the gradients of sum(weights o out) in the inputs,
the q / k / v Linears and the table.  The inputs and the loss weights are regenerated from the NumPy seed the file records
(`attention_inputs` of the test module), not stored.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_window_attention import GOLDEN_CASES, attention_inputs      # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_fea2gs", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    for name, case in GOLDEN_CASES.items():
        dim, heads, side, seed = case["dim"], case["heads"], case["side"], case["seed"]
        torch.manual_seed(seed)
        if case["kind"] == "self":
            m = ref.GSSelfAttn(dim=dim, num_heads=heads, num_gs_seed_sqrt=side)
        else:
            m = ref.WindowCrossAttn(dim=dim, num_heads=heads, window_size=side, num_gs_seed=side * side)
        rng = np.random.default_rng(seed)
        with torch.no_grad():
            for lin in (m.qhead, m.khead, m.vhead, m.proj):
                lin.weight.copy_(torch.from_numpy((rng.standard_normal((dim, dim)) / np.sqrt(dim)).astype(np.float32)))
                lin.bias.copy_(torch.from_numpy((0.1 * rng.standard_normal(dim)).astype(np.float32)))
            m.relative_position_bias_table.add_(torch.from_numpy((0.5 * rng.standard_normal(tuple(m.relative_position_bias_table.shape))).astype(np.float32)))
        gs, feat, wgt = (torch.from_numpy(a) for a in attention_inputs(case))
        gs.requires_grad_(True)
        feat.requires_grad_(True)
        out = m(gs) if case["kind"] == "self" else m(gs, feat)
        params = [m.qhead.weight, m.qhead.bias, m.khead.weight, m.khead.bias, m.vhead.weight, m.vhead.bias, m.relative_position_bias_table]
        ins = [gs] if case["kind"] == "self" else [gs, feat]
        grads = torch.autograd.grad((out * wgt).sum(), ins + params)
        index = m.relative_position_index.numpy()
        assert index.min() >= 0 and index.max() < m.relative_position_bias_table.shape[0]
        f32 = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)      # noqa: E731
        data = dict(seed=np.int64(seed), index=index.astype(np.int32), table=f32(m.relative_position_bias_table), scale=np.float64(m.scale), out=f32(out))
        for lin_name in ("qhead", "khead", "vhead", "proj"):
            data[lin_name + "_weight"], data[lin_name + "_bias"] = f32(getattr(m, lin_name).weight), f32(getattr(m, lin_name).bias)
        names = (["g_gs"] if case["kind"] == "self" else ["g_gs", "g_feat"]) + \
            ["g_qhead_weight", "g_qhead_bias", "g_khead_weight", "g_khead_bias", "g_vhead_weight", "g_vhead_bias", "g_table"]
        for n, g in zip(names, grads):
            data[n] = f32(g)
        path = os.path.join(HERE, f"attention_{name}.npz")
        np.savez_compressed(path, **data)
        used = len(np.unique(index))
        print(f"{name}: out {tuple(out.shape)}, index uses {used} of {data['table'].shape[0]} table rows (max {index.max()}), {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
