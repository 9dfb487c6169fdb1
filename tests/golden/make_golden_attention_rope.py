"""Writes tests/golden/attention_rope_<self|cross>_<12|16>.npz: the RoPE decoder's `GSSelfAttn` and `WindowCrossAttn` (the
reference's utils/fea2gsropeamp.py, rope_mixed) on the cases of tests/test_window_attention_rope.py.

    python tests/golden/make_golden_attention_rope.py /path/to/GSASR/utils/fea2gsropeamp.py

Runs on the CPU in well under a second.  The reference module is loaded by path, here and nowhere else; the files hold arrays
only: the modules' Linear weights (seeded `randn / sqrt(dim)`), `rope_freqs` as the module initialised it under the case's torch
seed, the buffers `rope_t_x` / `rope_t_y`, the reference's fp32 output on the case's inputs and the gradients of
sum(weights o out) in the inputs, the q / k / v Linears and `rope_freqs`.  The inputs and the loss weights are regenerated from
the case's NumPy seed (`attention_inputs` of the test module), not stored.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
from test_window_attention_rope import GOLDEN_CASES, PARAMS, attention_inputs      # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_fea2gsropeamp", path)
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
        gs, feat, wgt = (torch.from_numpy(a) for a in attention_inputs(case))
        gs.requires_grad_(True)
        feat.requires_grad_(True)
        out = m(gs) if case["kind"] == "self" else m(gs, feat)
        params = [m.qhead.weight, m.qhead.bias, m.khead.weight, m.khead.bias, m.vhead.weight, m.vhead.bias, m.rope_freqs]
        ins = [gs] if case["kind"] == "self" else [gs, feat]
        grads = torch.autograd.grad((out * wgt).sum(), ins + params)
        f32 = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)      # noqa: E731
        data = dict(seed=np.int64(seed), rope_freqs=f32(m.rope_freqs), rope_t_x=f32(m.rope_t_x), rope_t_y=f32(m.rope_t_y), out=f32(out))
        for lin_name in ("qhead", "khead", "vhead", "proj"):
            data[lin_name + "_weight"], data[lin_name + "_bias"] = f32(getattr(m, lin_name).weight), f32(getattr(m, lin_name).bias)
        names = (["g_gs"] if case["kind"] == "self" else ["g_gs", "g_feat"]) + ["g_" + p for p in PARAMS]
        for n, g in zip(names, grads):
            data[n] = f32(g)
        path = os.path.join(HERE, f"attention_rope_{name}.npz")
        np.savez_compressed(path, **data)
        fr = m.rope_freqs.detach()
        angle = float((m.rope_t_x[:, None, None] * fr[0][None] + m.rope_t_y[:, None, None] * fr[1][None]).abs().max())
        print(f"{name}: out {tuple(out.shape)}, angles up to {angle:.1f} rad, |g_rope_freqs| up to {float(grads[-1].abs().max()):.2f}, {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1024 * 1024


if __name__ == "__main__":
    main()
