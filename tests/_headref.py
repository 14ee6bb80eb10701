"""The classifier head (csrc/head_ops.hip) restated for the tests: which kernel csrc/head_select.h picks for a call (held to the
compiled header by tests/test_head_select_host.py, used by tests/test_head_gpu.py to predict the name the launcher notes), and
the float64 forward / backward the GPU results are held to."""
import torch

GROUP = 4          # channels a workgroup owns = channels of one 16-byte access
TPB = 1024
NAMES = ("head_fwd_kernel<1>", "head_fwd_kernel<4>", "head_bwd_kernel<1>", "head_bwd_kernel<4>")


def vec_ok(C, x_ptr, ldx, dx_ptr=0, lddx=0):
    return C % GROUP == 0 and ldx % GROUP == 0 and x_ptr % 16 == 0 and (dx_ptr == 0 or (lddx % GROUP == 0 and dx_ptr % 16 == 0))


def predict(backward, C, x_ptr, ldx, dx_ptr=0, lddx=0):
    """(kernel name, channels per access, workgroups) of a call; dx_ptr = 0 for the forward or a backward without dx."""
    vec = vec_ok(C, x_ptr, ldx, dx_ptr if backward else 0, lddx)
    return NAMES[(2 if backward else 0) + (1 if vec else 0)], GROUP if vec else 1, -(-C // GROUP)


def head_ref(x, gamma, beta, mean, invstd, gpooled, training):
    """float64 evaluation of the entry points' formulas on the operands as stored.  x (N,H,W,C), gpooled (N,C); returns
    (pooled, dx, dgamma, dbeta, y): y the pre-ReLU activation, for the tests' conditioning checks."""
    x, gamma, beta, mean, invstd, gpooled = (t.double().cpu() for t in (x, gamma, beta, mean, invstd, gpooled))
    N, H, W, C = x.shape
    HW, M = H * W, N * H * W
    xhat = (x - mean) * invstd
    y = xhat * gamma + beta
    pooled = y.clamp_min(0).sum(dim=(1, 2)) / HW
    g = torch.where(y > 0, (gpooled / HW).view(N, 1, 1, C).expand_as(y), torch.zeros_like(y))
    dbeta, dgamma = g.sum(dim=(0, 1, 2)), (g * xhat).sum(dim=(0, 1, 2))
    dx = gamma * invstd * ((g - dbeta / M - xhat * dgamma / M) if training else g)
    return pooled, dx, dgamma, dbeta, y
