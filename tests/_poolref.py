"""The fused BatchNorm -> ReLU -> MaxPool2d(2, 2) (csrc/pool_ops.hip) restated for the tests: which kernel csrc/pool_select.h picks
for a call, its grids and its workspace bytes (held to the compiled header by tests/test_pool_select_host.py, used by
tests/test_pool_gpu.py to predict the name the launcher notes), the workspace csrc/bn_select.h grants (kd_bn_nhwc_workspace), and the
float64 forward / backward the GPU results are held to: stock torch -- max_pool2d of relu of the affine map -- under float64
autograd, plus the BatchNorm backward's mean terms in closed form."""
import torch
import torch.nn.functional as F

VEC = 4            # channels of one 16-byte access
TPB = 256
CBLOCK = 64        # channels of a stage-1 workgroup
WINS = 48          # windows of a stage-1 workgroup
FINISH_CH = 64
CAP = 8192
BN_ROWS = 128      # csrc/bn_select.h: pixels per stage-1 workgroup of the BatchNorm kernels, whose workspace the backward borrows
NAMES = ("pool_fwd_kernel<1>", "pool_fwd_kernel<4>", "pool_bwd_kernel<1>", "pool_bwd_kernel<4>")


def shape_ok(N, H, W, C, ldx, ldo=0):
    return N >= 1 and H >= 2 and W >= 2 and C >= 1 and ldx >= C and (ldo == 0 or ldo >= C)


def view_ok(ptr, ld):
    return ptr == 0 or (ptr % 16 == 0 and ld % VEC == 0)


def vec_ok(C, *views):
    """views: (pointer value, pixel stride) of every activation view of the call; pointer 0 = absent."""
    return C % VEC == 0 and all(view_ok(p, ld) for p, ld in views)


def bn_workspace(M, C):
    """kd_bn_nhwc_workspace(M, C) restated (csrc/bn_select.h: bn_workspace)."""
    return 0 if M <= 0 or C <= 0 else (-(-M // BN_ROWS) * 3 * C + 2 * C) * 4


def grid(items):
    return min(max(-(-items // TPB), 1), CAP)


def predict(backward, bn, N, H, W, C, views):
    """dict(name, vec, grid, nwb, part, finish, sums_offset, ws) of a call.  views: x and y (forward) or x, gpooled and dx (backward;
    pointer 0 for a dx that is not wanted)."""
    vec = vec_ok(C, *views)
    v = VEC if vec else 1
    windows, cells = N * (H // 2) * (W // 2), N * -(-H // 2) * -(-W // 2)
    out = dict(name=NAMES[(2 if backward else 0) + (1 if vec else 0)], vec=v, windows=windows, cells=cells,
               grid=grid((cells if backward else windows) * (C // v)), nwb=0, part=(0, 0), finish=0, sums_offset=0, ws=0)
    if backward and bn:
        nwb = -(-windows // WINS)
        out.update(nwb=nwb, part=(nwb, -(-C // CBLOCK)), finish=-(-C // FINISH_CH), sums_offset=nwb * 2 * C, ws=(nwb * 2 * C + 2 * C) * 4)
    return out


def pool_ref(x, gamma, beta, mean, invstd, gpooled, training):
    """float64 evaluation on the operands as stored.  x (N,H,W,C), gpooled (N,H//2,W//2,C); gamma = None: no BatchNorm.  Returns
    (pooled, dx, dgamma, dbeta, y, gq): y the pre-ReLU activation and gq the routed gradient g' at full resolution (zero at
    non-maximal pixels and in a dropped odd row / column), for the tests' conditioning checks and bounds.  The routing is
    torch's: max_pool2d of relu under autograd."""
    x, gpooled = x.double().cpu(), gpooled.double().cpu()
    N, H, W, C = x.shape
    M = N * H * W
    if gamma is None:
        xhat, y = x, x.clone().requires_grad_(True)
    else:
        gamma, beta, mean, invstd = (t.double().cpu() for t in (gamma, beta, mean, invstd))
        xhat = (x - mean) * invstd
        y = (xhat * gamma + beta).requires_grad_(True)
    pooled = F.max_pool2d(F.relu(y.permute(0, 3, 1, 2)), 2, 2).permute(0, 2, 3, 1)
    (gq,) = torch.autograd.grad(pooled, y, gpooled)
    y = y.detach()
    if gamma is None:
        return pooled.detach(), gq, None, None, y, gq
    dbeta, dgamma = gq.sum(dim=(0, 1, 2)), (gq * xhat).sum(dim=(0, 1, 2))
    dx = gamma * invstd * ((gq - dbeta / M - xhat * dgamma / M) if training else gq)
    return pooled.detach(), dx, dgamma, dbeta, y, gq
