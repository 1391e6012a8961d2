"""Host statements shared by the tests of the backward at another input size (tests/test_any_size_grad_cpu.py, tests/test_any_size_grad_gpu.py):
the adjoint of the rel-pos table resize in float64, torch's own autograd of the reference's resize, and the length pairs both files use."""
import torch
import torch.nn.functional as F

# the length pairs of tests/test_any_size_gpu.py: test_relpos_resize_vs_float64 and test_relpos_resize_dyadic_cases_are_exact
RESIZE_PAIRS = [(15, 7, 19, 9), (15, 7, 11, 5), (111, 55, 139, 69)]
DYADIC_PAIRS = [(8, 16), (16, 8), (8, 32), (32, 8), (12, 48), (45, 15), (27, 9), (3, 6), (6, 3), (4, 1), (1, 4)]


def resize_adjoint_statement(g, n_src):
    """d t [n_src, hd] for d out = g [n_dst, hd] through F.interpolate(mode="linear", align_corners=False) along dim 0, in float64:
    d t[i] = sum_j w(j, i) g[j] with the forward statement's i0, i1, lambda per j (tests/test_any_size_gpu.py: resize_statement)."""
    g = g.double()
    n_dst = g.shape[0]
    j = torch.arange(n_dst, dtype=torch.float64)
    s = (n_src / n_dst * (j + 0.5) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_src - 1)
    i1 = (i0 + 1).clamp_max(n_src - 1)
    l1 = (s - i0)[:, None]
    dt = torch.zeros((n_src, g.shape[1]), dtype=torch.float64)
    dt.index_add_(0, i0, (1 - l1) * g)
    dt.index_add_(0, i1, l1 * g)
    return dt


def torch_resize_grad(g, n_src, dtype):
    """torch's own autograd of what the reference's get_rel_pos runs (util/vitdet_utils.py:79-85), on the CPU in `dtype`."""
    t = torch.zeros((n_src, g.shape[1]), dtype=dtype, requires_grad=True)
    n_dst = g.shape[0]
    out = F.interpolate(t.reshape(1, n_src, -1).permute(0, 2, 1), size=n_dst, mode="linear").reshape(-1, n_dst).permute(1, 0)
    out.backward(g.to(dtype))
    return t.grad
