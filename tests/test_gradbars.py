"""The per-column gradient bars of tests/gradbars.py, tested on the CPU with the oracle alone.

(a) The reference's own fp32 arithmetic stays far inside them: backward_f32 (with and without contracted multiply-adds)
    against backward_f64 on kernel-frame inputs, and torch fp32 autograd through host_ref.prologue fed with backward_f32 against
    float64 autograd fed with backward_f64 on raw parameters.  Asserted: worst error / element bar <= 0.25 and the column bar.
    Measured (error / element bar, error / column bar):
      kernel frame  24x24 x4 dmax 0.3   0.043 / 0.010        64x64 x4 dmax 0.1   0.063 / 0.010
                    12x12 x4 gpp 16     0.036 / 0.006        20x16 x12           0.148 / 0.031   (the d/dy column)
                    37x29 x3            0.031 / 0.004
      raw           24x32 x4 dmax 0.2   0.043 / 0.008        24x32 x4 unbounded  0.023 / 0.006
                    12x12 x4 dmax 0.2   0.022 / 0.003        20x28 x3 unbounded  0.022 / 0.003
                    9x7 x7.5 unbounded  0.038 / 0.008
    (the same with and without contracted multiply-adds, to the digits shown)
    Rows under the element bar (kappa = 1 - rho^2 >= 0.1): all of them in every case but 64x64 (4095 of 4096, smallest kappa
    0.061), 12x12 gpp 16 and 37x29 (one row each short); gradbars.SYNTHETIC_SHARE is asserted.

(b) The bars discriminate: five mutants of the float64 truth fail them.  The first four PASS the tensor-level bar of 2e-4 the
    suite had alone before (error / tensor max-abs): rho-logit column x 1.005 of the 24x32 raw case 1.50e-4, sx-logit column
    x 1.005 1.19e-4, a colour-logit column x 1.01 1.01e-4, the d/d rho column of g_sigmas x 1.005 on 64x64 1.06e-4 -- and are 9.7,
    9.7 and 19.3 times over the element bar (first three).
"""
import functools

import numpy as np
import pytest
import torch

import gradbars
from gsasr_amd import synthetic
from oracle import gs_oracle, host_ref

KERNEL_CASES = [(24, 24, 4.0, 3, 1, 0.3), (64, 64, 4.0, 3, 1, 0.1), (12, 12, 4.0, 3, 16, None), (20, 16, 12.0, 3, 1, None),
                (37, 29, 3.0, 3, 1, None)]
RAW_CASES = [(24, 32, 60, 4.0, 0.2), (24, 32, 60, 4.0, None), (12, 12, 5, 4.0, 0.2), (20, 28, 65, 3.0, None), (9, 7, 11, 7.5, None)]
REFERENCE_SHARE_OF_BAR = 0.25


@functools.lru_cache(maxsize=None)
def kernel_truth(case):
    h_lr, w_lr, scale, seed, gpp, dmax = case
    sig, xy, col, H, W = synthetic.kernel_inputs(h_lr, w_lr, scale, seed=seed, gpp=gpp)
    wgt = synthetic.grad_image(H, W, 4).numpy()
    a, b, c = sig.numpy(), xy.numpy(), col.numpy()
    return a, b, c, wgt, dmax, gs_oracle.backward_f64(a, b, c, wgt, dmax)


@functools.lru_cache(maxsize=None)
def raw_truth(case):
    h_lr, w_lr, seed, scale, dmax = case
    H, W = int(round(h_lr * scale)), int(round(w_lr * scale))
    p = synthetic.gs_parameters(h_lr, w_lr, seed=seed)
    sm = torch.tensor([scale, scale])
    sig, xy, col, _ = host_ref.prologue(p, (H, W), sm)
    a, b, c = sig.numpy(), xy.numpy(), col.numpy()
    wgt = synthetic.grad_image(H, W, seed + 1).numpy()
    pr = p.clone().double().requires_grad_(True)
    torch.autograd.backward(list(host_ref.prologue(pr, (H, W), sm.double())[:3]),
                            [torch.from_numpy(g) for g in gs_oracle.backward_f64(a, b, c, wgt, dmax)])
    return p, (H, W), sm, (a, b, c), wgt, dmax, pr.grad.numpy()


@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "lr%dx%d_s%g_seed%d_gpp%d_dmax%s" % c)
def test_reference_fp32_backward_stays_inside_the_bars(case):
    a, b, c, wgt, dmax, want = kernel_truth(case)
    for fma in (False, True):
        got = gs_oracle.backward_f32(a, b, c, wgt, dmax, use_fma=fma)
        elem, col = gradbars.check_kernel(got, want, a, gradbars.SYNTHETIC_SHARE, f"backward_f32 fma={fma} {case}")
        print(f"{case} fma={fma}: worst error / element bar {elem:.4f}, error / column bar {col:.4f}")
        assert elem <= REFERENCE_SHARE_OF_BAR and col <= 1.0


@pytest.mark.parametrize("case", RAW_CASES, ids=lambda c: "lr%dx%d_seed%d_s%g_dmax%s" % c)
def test_reference_fp32_autograd_to_raw_parameters_stays_inside_the_bars(case):
    p, (H, W), sm, (a, b, c), wgt, dmax, want = raw_truth(case)
    assert float(gradbars.kappa_of(gradbars.raw_rho(p)).min()) >= 0.12      # every row of the raw cases is in scope
    p32 = p.clone().requires_grad_(True)
    g32 = gs_oracle.backward_f32(a, b, c, wgt, dmax, use_fma=True)
    torch.autograd.backward(list(host_ref.prologue(p32, (H, W), sm)[:3]), [torch.from_numpy(np.asarray(g, np.float32)) for g in g32])
    elem, col = gradbars.check_raw(p32.grad, want, p, 1.0, f"fp32 autograd {case}")
    print(f"{case}: worst error / element bar {elem:.4f}, error / column bar {col:.4f}")
    assert elem <= REFERENCE_SHARE_OF_BAR and col <= 1.0


def _tensor_level(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("column,factor", [(2, 1.005), (0, 1.005), (5, 1.01)], ids=["rho-logit", "sx-logit", "colour-logit"])
def test_a_raw_column_slightly_off_fails_the_bars_and_passed_the_tensor_bar(column, factor):
    p, _, _, _, _, _, want = raw_truth(RAW_CASES[0])
    assert gradbars.check_raw(want.copy(), want, p, 1.0)[0] == 0.0
    mutant = want.copy()
    mutant[:, column] *= factor
    assert _tensor_level(mutant, want) <= 2e-4          # what the suite asked before: passes
    with pytest.raises(AssertionError, match="column " + gradbars.RAW_NAMES[column]):
        gradbars.check_raw(mutant, want, p, 1.0, "mutant")
    elem, _, _, _, _ = gradbars.ratios(mutant, want, gradbars.raw_rho(p), gradbars.RAW_GROUPS)
    print(f"column {column} x {factor}: tensor level {_tensor_level(mutant, want):.3e}, {elem[column]:.1f} times over the element bar")
    assert elem[column] > 5.0 and np.delete(elem, column).max() == 0.0


def test_the_rho_column_of_g_sigmas_slightly_off_fails_the_bars_and_passed_the_tensor_bar():
    a, _, _, _, _, want = kernel_truth(KERNEL_CASES[1])
    mutant = [w.copy() for w in want]
    mutant[0][:, 2] *= 1.005
    assert _tensor_level(mutant[0], want[0]) <= 2e-4
    with pytest.raises(AssertionError, match="column sigmas2"):
        gradbars.check_kernel(mutant, want, a, gradbars.SYNTHETIC_SHARE, "mutant")


def test_one_element_two_percent_off_fails_the_bars():
    p, _, _, _, _, _, want = raw_truth(RAW_CASES[0])
    for k in range(9):
        big = np.flatnonzero(np.abs(want[:, k]) >= 1e-2 * np.abs(want[:, k]).max())
        i = int(big[np.argmin(np.abs(want[big, k]))])       # the smallest such element: the hardest to see
        mutant = want.copy()
        mutant[i, k] *= 1.02
        with pytest.raises(AssertionError, match=f"column {gradbars.RAW_NAMES[k]} row {i}:"):
            gradbars.check_raw(mutant, want, p, 1.0, "mutant")


def test_rows_below_the_conditioning_scope_are_left_to_the_row_bar_and_min_share_is_asserted():
    p, _, _, _, _, _, want = raw_truth(RAW_CASES[0])
    q = p.clone()
    q[5, 2] = 3.0                                            # kappa = 1 - tanh(3)^2 ~ 0.01
    mutant = want.copy()
    mutant[5] *= 1.5
    assert gradbars.check_raw(mutant, want, q, 0.0) == (0.0, 0.0)
    with pytest.raises(AssertionError, match="of the rows have kappa"):
        gradbars.check_raw(mutant, want, q, 1.0)
    with pytest.raises(AssertionError, match="row 5"):
        gradbars.check_raw(mutant, want, p, 1.0)


def test_record_file(tmp_path, monkeypatch):
    p, _, _, _, _, _, want = raw_truth(RAW_CASES[0])
    out = tmp_path / "bars.txt"
    monkeypatch.setenv(gradbars.RECORD_ENV, str(out))
    gradbars.check_raw(want * (1 + 1e-5), want, p, 1.0, "route/kernel")
    line = out.read_text()
    assert line.startswith("route/kernel: sx ") and "muy" in line
