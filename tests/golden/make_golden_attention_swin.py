"""Writes tests/golden/attention_swin_8_shift.npz and attention_swin_8_plain.npz: the reference's SwinIR `WindowAttention` inside a
shifted and a plain `SwinTransformerBlock`, on the cases of tests/test_window_attention_masked.py.

    python tests/golden/make_golden_attention_swin.py /path/to/GSASR/utils/swinir.py

Runs on the CPU in well under a second.  The reference module is loaded by path, here and nowhere else (its `import torchvision`
is served by an empty stand-in module when torchvision is not installed: nothing of it is used); the files hold numbers only: the
attention's weights (seeded `randn / sqrt(dim)`), `relative_position_index`, the bias table the module initialised perturbed by
0.5 randn, the block's own `attn_mask` (shifted block: [4, 64, 64] of 0 / -100), the reference's fp32 `attn(x, mask)` on the case's
input and the gradients of sum(weights o out) in the input, the packed Linear and the table.  The input and the loss weights are
regenerated from the NumPy seed the file records (`swin_inputs` of the test module), not stored.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_window_attention_masked import SWIN_CASES, swin_inputs      # noqa: E402


def load_reference(path):
    try:
        import torchvision      # noqa: F401
    except ImportError:
        stand_in = types.ModuleType("torchvision")
        stand_in.__version__ = "0.0.0"
        sys.modules["torchvision"] = stand_in
    spec = importlib.util.spec_from_file_location("reference_swinir", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    for name, case in SWIN_CASES.items():
        dim, heads, seed = case["dim"], case["heads"], case["seed"]
        torch.manual_seed(seed)
        block = ref.SwinTransformerBlock(dim=dim, input_resolution=(16, 16), num_heads=heads, window_size=case["window"], shift_size=case["shift"])
        m, mask = block.attn, block.attn_mask
        rng = np.random.default_rng(seed)
        with torch.no_grad():
            for lin in (m.qkv, m.proj):
                rows = lin.weight.shape[0]
                lin.weight.copy_(torch.from_numpy((rng.standard_normal((rows, dim)) / np.sqrt(dim)).astype(np.float32)))
                lin.bias.copy_(torch.from_numpy((0.1 * rng.standard_normal(rows)).astype(np.float32)))
            m.relative_position_bias_table.add_(torch.from_numpy((0.5 * rng.standard_normal(tuple(m.relative_position_bias_table.shape))).astype(np.float32)))
        x, wgt = (torch.from_numpy(a) for a in swin_inputs(case))
        x.requires_grad_(True)
        out = m(x, mask=mask)
        grads = torch.autograd.grad((out * wgt).sum(), [x, m.qkv.weight, m.qkv.bias, m.relative_position_bias_table])
        index = m.relative_position_index.numpy()
        assert index.min() >= 0 and index.max() < m.relative_position_bias_table.shape[0]
        f32 = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)      # noqa: E731
        data = dict(seed=np.int64(seed), index=index.astype(np.int32), table=f32(m.relative_position_bias_table), scale=np.float64(m.scale), out=f32(out))
        if mask is not None:
            assert tuple(mask.shape) == (4, 64, 64) and set(mask.unique().tolist()) == {0.0, -100.0} and bool((mask.max(-1).values == 0).all())
            data["mask"] = f32(mask)
        for lin_name in ("qkv", "proj"):
            data[lin_name + "_weight"], data[lin_name + "_bias"] = f32(getattr(m, lin_name).weight), f32(getattr(m, lin_name).bias)
        for n, g in zip(("g_x", "g_qkv_weight", "g_qkv_bias", "g_table"), grads):
            data[n] = f32(g)
        path = os.path.join(HERE, f"attention_{name}.npz")
        np.savez_compressed(path, **data)
        print(f"{name}: out {tuple(out.shape)}, mask {None if mask is None else tuple(mask.shape)}, table {data['table'].shape}, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
