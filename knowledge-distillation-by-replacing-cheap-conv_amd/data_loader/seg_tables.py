"""The parameter table of the Cityscapes loader and the host-tensor path of its three stages.

One int32 row of HDR words per sample holds every random draw of the reference's chain (data_loader/joint_transforms.py:346-373,
75-123; data_loader/transforms.py:238-304, 101-110).  `expand` turns the rows of one batch into what the kernels read: the header
followed by the per-output-pixel resampling tables, all computed here in double so that no double-precision rounding question
reaches the device.  `host_crop`, `host_jitter`, `host_blur` and `host_normalise` are the torch compositions the kernels of csrc/seg_data_ops.hip
restate; they run on host tensors and give the same bits.

Row (int32 words):
   0 index   1 w   2 h   (the scaled size int(W*s), int(H*s))   3 pad_w   4 pad_h   5 x1   6 y1   7 flip
   8..11  the order of the four colour operations (BRIGHTNESS, CONTRAST, SATURATION, HUE), a permutation
  12 13 14  the brightness, contrast and saturation factors, fp32 bits (PIL's blend takes a C float)
  15  the hue shift byte np.uint8(hue_factor * 255)          16 blur radius int(4 sigma + 0.5), 0: no blur
  17  1 when the colour jitter runs                          18 19  sigma, the bits of a double
  20..31  the Gaussian weights of offsets 0..5 (scipy's, normalised in double), the bits of six doubles, 0 beyond the radius
Expanded row (HDR + 24 S words, S the crop size): the header, then
  HT (S,11) [xmin, taps, k0..k8]: the horizontal pass of PIL's bicubic resize for crop column j BEFORE the flip, 22-bit fixed
      point; xmin = -1: column j is padding          VT (S,11): the same for crop row i
  MX (S), MY (S): the nearest-neighbour source column / row of the mask, -1: padding."""
import numpy as np
import torch

HDR = 32
TAPS = 9                      # the widest bicubic window: support 2 widened by a down-scale of 2
ENTRY = 2 + TAPS
PRECISION_BITS = 22           # PIL's 8-bit resampling: 32 - 8 - 2
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
MAX_RADIUS = 5
(I_INDEX, I_W, I_H, I_PADW, I_PADH, I_X1, I_Y1, I_FLIP, I_ORDER, I_FB, I_FC, I_FS, I_HUE, I_RADIUS, I_JITTER, I_SIGMA,
 I_WEIGHTS) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14, 15, 16, 17, 18, 20
_PERMS = None


def expanded_len(S):
    return HDR + 2 * ENTRY * S + 2 * S


def _f32_bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


def _f64_words(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int32)


def gaussian_weights(sigma):
    """(radius, the weights of offsets 0..radius) of scipy.ndimage.gaussian_filter1d(sigma, truncate=4.0), in its arithmetic."""
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5)
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    phi = phi / phi.sum()
    return radius, phi[radius:]


def identity_row(index, W, H):
    """The row that leaves image `index` as it is (validation, test): full size, no pad, no flip, no jitter, no blur."""
    r = np.zeros(HDR, dtype=np.int32)
    r[I_INDEX], r[I_W], r[I_H] = index, W, H
    r[I_ORDER:I_ORDER + 4] = (0, 1, 2, 3)
    r[I_FB:I_FB + 3] = _f32_bits([1.0, 1.0, 1.0])
    return r


def make_row(index, W, H, S, w, h, x1, y1, flip, order=(0, 1, 2, 3), factors=None, hue=0.0, sigma=None):
    """One row from explicit draws.  factors: (brightness, contrast, saturation) or None for no jitter; hue the hue factor in
    [-0.5, 0.5]; sigma None for no blur.  The pad is the reference's rule, (S - h) // 2 + 1 where S > h."""
    r = identity_row(index, W, H)
    r[I_W], r[I_H] = w, h
    r[I_PADW] = (S - w) // 2 + 1 if S > w else 0
    r[I_PADH] = (S - h) // 2 + 1 if S > h else 0
    r[I_X1], r[I_Y1], r[I_FLIP] = x1, y1, int(bool(flip))
    r[I_ORDER:I_ORDER + 4] = order
    if factors is not None:
        r[I_JITTER] = 1
        r[I_FB:I_FB + 3] = _f32_bits(factors)
        r[I_HUE] = int(float(hue) * 255) & 255            # np.uint8(hue_factor * 255): truncation, then wrap-around
    if sigma is not None:
        radius, wts = gaussian_weights(sigma)
        r[I_RADIUS] = radius
        r[I_SIGMA:I_SIGMA + 2] = _f64_words([sigma])
        r[I_WEIGHTS:I_WEIGHTS + 2 * len(wts)] = _f64_words(wts)
    return r


def max_offsets(r, S):
    """(largest x1, largest y1) the reference's RandomCrop may draw for the scaled and padded size of row r."""
    return int(r[I_W] + 2 * r[I_PADW] - S), int(r[I_H] + 2 * r[I_PADH] - S)


def draw_rows(order, W, H, spec, g, centroids=None):
    """int32 (n, HDR): one epoch's draws for the sample indices `order` from the torch generator g, with the reference's
    distributions.  spec: the loader's reading of the transform lists (crop, scale_min, scale_max, flip, color_aug, blur) or None
    for no augmentation.  centroids: None, or int (n, 3) rows [has_centroid, cx, cy] in source pixels; a row that has one takes its
    crop offsets as RandomCrop does for a centroid (reference data_loader/joint_transforms.py:104-113, 368-369) from the same two
    uniforms: cx' = int(cx * s) in double, x1 = randint(cx' - S, cx') clamped to [0, mx], and likewise y1.  Two quirks of the
    reference stay: the centroid is not shifted by the pad, and x1 = cx' - S leaves it one pixel outside the crop.  The uniforms
    consumed and their order do not depend on `centroids`."""
    global _PERMS
    n = len(order)
    rows = np.zeros((n, HDR), dtype=np.int32)
    rows[:, I_INDEX] = np.asarray(order)
    rows[:, I_W], rows[:, I_H] = W, H
    rows[:, I_ORDER:I_ORDER + 4] = (0, 1, 2, 3)
    rows[:, I_FB:I_FB + 3] = _f32_bits([1.0, 1.0, 1.0])
    if spec is None:
        return torch.from_numpy(rows)
    S = spec["crop"]
    u = torch.rand((n, 9), generator=g, dtype=torch.float64).numpy()
    s = spec["scale_min"] + (spec["scale_max"] - spec["scale_min"]) * u[:, 0]          # random.uniform(a, b) = a + (b - a) * U
    w, h = (W * s).astype(np.int64), (H * s).astype(np.int64)                           # int(i * scale_amt)
    pw, ph = np.where(S > w, (S - w) // 2 + 1, 0), np.where(S > h, (S - h) // 2 + 1, 0)
    mx, my = w + 2 * pw - S, h + 2 * ph - S
    rows[:, I_W], rows[:, I_H], rows[:, I_PADW], rows[:, I_PADH] = w, h, pw, ph
    rows[:, I_X1] = np.minimum((u[:, 1] * (mx + 1)).astype(np.int64), mx)               # randint(0, mx), both ends included
    rows[:, I_Y1] = np.minimum((u[:, 2] * (my + 1)).astype(np.int64), my)
    if centroids is not None:
        cen = np.asarray(centroids, dtype=np.int64).reshape(n, 3)
        for col, c, uc, top in ((I_X1, cen[:, 1], u[:, 1], mx), (I_Y1, cen[:, 2], u[:, 2], my)):
            hi = (c * s).astype(np.int64)                                               # int(c * scale_amt)
            at = np.minimum(hi - S + (uc * (S + 1)).astype(np.int64), hi)               # randint(c' - S, c'), both ends included
            rows[:, col] = np.where(cen[:, 0] != 0, np.minimum(top, np.maximum(0, at)), rows[:, col])
    rows[:, I_FLIP] = (u[:, 3] < 0.5) if spec["flip"] else 0
    a = float(spec["color_aug"])
    if a > 0:
        if _PERMS is None:
            import itertools
            _PERMS = np.array(list(itertools.permutations(range(4))), dtype=np.int32)
        lo = max(0.0, 1.0 - a)
        rows[:, I_JITTER] = 1
        rows[:, I_FB:I_FB + 3] = _f32_bits(lo + (1.0 + a - lo) * u[:, 4:7])
        hue = -a + 2 * a * u[:, 7]
        rows[:, I_HUE] = np.trunc(hue * 255).astype(np.int64) & 255                     # np.uint8(hue_factor * 255)
        rows[:, I_ORDER:I_ORDER + 4] = _PERMS[torch.randint(0, 24, (n,), generator=g).numpy()]
    if spec["blur"]:
        sigma = 0.15 + u[:, 8] * 1.15
        for i in range(n):
            radius, wts = gaussian_weights(sigma[i])
            rows[i, I_RADIUS] = radius
            rows[i, I_WEIGHTS:I_WEIGHTS + 2 * len(wts)] = _f64_words(wts)
        rows[:, I_SIGMA:I_SIGMA + 2] = _f64_words(sigma).reshape(n, 2)
    return torch.from_numpy(rows)


# ---------------------------------------------------------------------------------------------- PIL's resampling, restated
def _bicubic(x):
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def bicubic_coeffs(in_size, out_size, first=0, last=None):
    """(xmin (m,), taps (m,), k (m,TAPS) int32) for output pixels first..last-1 (all by default): the coefficients of one pass of
    Image.resize(..., Image.BICUBIC) from in_size to out_size pixels, PIL's precompute_coeffs and normalize_coeffs_8bpc in the same
    double arithmetic."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    last = out_size if last is None else last
    center = 0.0 + (np.arange(first, last) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size)
    taps = xmax - xmin
    if taps.max() > TAPS:
        raise ValueError(f"resize {in_size} -> {out_size}: a window of {taps.max()} taps, {TAPS} at most (scale below 0.5)")
    k = np.zeros((len(center), max(ksize, TAPS)))
    ww = np.zeros(len(center))
    for x in range(ksize):
        wgt = np.where(x < taps, _bicubic((x + xmin - center + 0.5) * ss), 0.0)
        k[:, x] = wgt
        ww = ww + wgt
    k = np.where(ww[:, None] != 0.0, k / np.where(ww == 0.0, 1.0, ww)[:, None], k)
    fixed = np.trunc(np.where(k < 0, -0.5, 0.5) + k * (1 << PRECISION_BITS)).astype(np.int32)
    return xmin.astype(np.int32), taps.astype(np.int32), fixed[:, :TAPS]


def nearest_indices(in_size, out_size):
    """The source index of every output pixel of Image.resize(..., Image.NEAREST): PIL's running sum of the step, in double."""
    a = float(in_size) / out_size
    steps = np.full(out_size, a)
    steps[0] = 0.0 + a * 0.5
    return np.minimum(np.cumsum(steps).astype(np.int64), in_size - 1).astype(np.int32)


def expand(rows, W, H, S):
    """int32 (B, expanded_len(S)) from header rows (B, HDR): the tables the crop kernel reads (see the module docstring)."""
    rows = np.asarray(rows, dtype=np.int32)
    B = rows.shape[0]
    out = np.zeros((B, expanded_len(S)), dtype=np.int32)
    out[:, :HDR] = rows
    j = np.arange(S)
    for b in range(B):
        r = rows[b]
        for axis, (src, dst, pad, off) in enumerate(((W, int(r[I_W]), int(r[I_PADW]), int(r[I_X1])),
                                                     (H, int(r[I_H]), int(r[I_PADH]), int(r[I_Y1])))):
            u = off + j - pad
            ok = (u >= 0) & (u < dst)
            first = int(np.clip(u[0], 0, dst - 1))
            last = int(np.clip(u[-1], first, dst - 1)) + 1                  # only the crop's part of the scaled image
            xmin, taps, k = bicubic_coeffs(src, dst, first, last)
            near = nearest_indices(src, dst)[first:last]
            uc = np.clip(u, first, last - 1) - first
            ent = np.zeros((S, ENTRY), dtype=np.int32)
            ent[:, 0] = np.where(ok, xmin[uc], -1)
            ent[:, 1] = np.where(ok, taps[uc], 0)
            ent[:, 2:] = np.where(ok[:, None], k[uc], 0)
            base = HDR + axis * ENTRY * S
            out[b, base:base + ENTRY * S] = ent.reshape(-1)
            base = HDR + 2 * ENTRY * S + axis * S
            out[b, base:base + S] = np.where(ok, near[uc], -1)
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------- the host-tensor path
def _tables(row, S):
    ht = row[HDR:HDR + ENTRY * S].view(S, ENTRY).long()
    vt = row[HDR + ENTRY * S:HDR + 2 * ENTRY * S].view(S, ENTRY).long()
    mx = row[HDR + 2 * ENTRY * S:HDR + 2 * ENTRY * S + S].long()
    my = row[HDR + 2 * ENTRY * S + S:HDR + 2 * ENTRY * S + 2 * S].long()
    return ht, vt, mx, my


def _clip8_shift(acc):
    return ((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS).clamp_(0, 255)


def host_crop(data, targets, table, S):
    """Resample + pad + crop + flip: (B,S,S,3) and (B,S,S) uint8 from the resident bytes and an expanded table."""
    B = table.shape[0]
    H, W = data.shape[1:3]
    img = torch.zeros((B, S, S, 3), dtype=torch.uint8)
    msk = torch.full((B, S, S), 255, dtype=torch.uint8)
    t9 = torch.arange(TAPS)
    for b in range(B):
        row = table[b]
        idx, flip = int(row[I_INDEX]), int(row[I_FLIP])
        ht, vt, mx, my = _tables(row, S)
        okx, oky = ht[:, 0] >= 0, vt[:, 0] >= 0
        if bool(okx.any()) and bool(oky.any()):
            lo = int(vt[oky, 0].min())
            hi = int((vt[oky, 0] + vt[oky, 1]).max())
            src = data[idx, lo:hi].long()                                                   # (R,W,3)
            gx = (ht[:, :1].clamp(min=0) + t9[None, :]).clamp(max=W - 1)                      # (S,TAPS); taps beyond the window weigh 0
            T = _clip8_shift((src[:, gx] * ht[None, :, 2:, None]).sum(2))                   # (R,S,3): the horizontal pass, a byte again
            gy = (vt[:, :1].clamp(min=0) + t9[None, :] - lo).clamp(max=hi - lo - 1)
            out = _clip8_shift((T[gy] * vt[:, 2:, None, None]).sum(1))                      # (S,S,3)
            inside = (oky[:, None] & okx[None, :])
            out = torch.where(inside[:, :, None], out, torch.zeros_like(out))
            m = targets[idx][my.clamp(min=0)][:, mx.clamp(min=0)]
            m = torch.where(inside, m, torch.full_like(m, 255))
            if flip:
                out, m = out.flip(1), m.flip(1)
            img[b], msk[b] = out.to(torch.uint8), m
    return img, msk


def _grey(p):
    """PIL's convert("L") of int64 (...,3) RGB."""
    return (p[..., 0] * 19595 + p[..., 1] * 38470 + p[..., 2] * 7471 + 0x8000) >> 16


def _blend(lo, p, alpha):
    """Image.blend(lo, p, alpha) in its C float arithmetic: (UINT8)(lo + alpha * (p - lo)), clipped when it extrapolates."""
    t = lo.to(torch.float32) + alpha * (p - lo).to(torch.float32)
    return t.clamp_(0.0, 255.0).to(torch.int64)


def _hue(p, shift):
    """PIL's RGB -> HSV, H += shift (mod 256), HSV -> RGB, in the float / double mixture of its Convert.c."""
    f32, f64 = torch.float32, torch.float64
    r, g, b = p.unbind(-1)
    maxc, minc = p.amax(-1), p.amin(-1)
    grey = maxc == minc
    cr = (maxc - minc).to(f32)
    cr = torch.where(grey, torch.ones_like(cr), cr)
    s = cr / torch.where(grey, torch.ones_like(cr), maxc.to(f32))
    rc, gc, bc = ((maxc - c).to(f32) / cr for c in (r, g, b))
    h = torch.where(r == maxc, (bc - gc).to(f64),
                    torch.where(g == maxc, (2.0 + rc.to(f64)) - bc.to(f64), (4.0 + gc.to(f64)) - rc.to(f64))).to(f32)
    h = (h.to(f64) / 6.0 + 1.0)
    h = (h - h.floor()).to(f32)                                                             # fmod(x, 1.0), x > 0: exact
    uh = (h.to(f64) * 255.0).to(torch.int64).clamp_(0, 255)
    us = (s.to(f64) * 255.0).to(torch.int64).clamp_(0, 255)
    uh, us = torch.where(grey, torch.zeros_like(uh), uh), torch.where(grey, torch.zeros_like(us), us)
    uh = (uh + shift) & 255
    h6 = uh.to(f32).to(f64) * 6.0 / 255.0
    i = h6.floor()
    f = (h6 - i.to(f32).to(f64)).to(f32)
    fs = (us.to(f32).to(f64) / 255.0).to(f32)
    v = maxc.to(f32).to(f64)
    rnd = lambda x: (x + 0.5).floor().to(torch.int64).clamp_(0, 255)
    pp = rnd(v * (1.0 - fs.to(f64)))
    q = rnd(v * (1.0 - (fs * f).to(f64)))
    t = rnd(v * (1.0 - fs.to(f64) * (1.0 - f.to(f64))))
    i6 = i.to(torch.int64) % 6
    vv = maxc
    pick = lambda c0, c1, c2, c3, c4, c5: torch.where(i6 == 0, c0, torch.where(i6 == 1, c1, torch.where(i6 == 2, c2, torch.where(
        i6 == 3, c3, torch.where(i6 == 4, c4, c5)))))
    out = torch.stack((pick(vv, q, pp, pp, t, vv), pick(t, vv, vv, q, pp, pp), pick(pp, pp, t, vv, vv, q)), -1)
    return torch.where((us == 0)[..., None], vv[..., None].expand_as(out), out)


def host_jitter(img, table):
    """The colour jitter of every sample whose row asks for it, on (B,S,S,3) uint8, in the row's order."""
    out = img.clone()
    for b in range(img.shape[0]):
        row = table[b]
        if not int(row[I_JITTER]):
            continue
        fb, fc, fs = row[I_FB:I_FB + 3].clone().view(torch.float32).tolist()
        p = img[b].long()
        for op in row[I_ORDER:I_ORDER + 4].tolist():
            if op == BRIGHTNESS:
                p = _blend(torch.zeros_like(p), p, fb)
            elif op == CONTRAST:
                total, count = int(_grey(p).sum()), p.shape[0] * p.shape[1]
                mean = (2 * total + count) // (2 * count)                                  # int(sum / N + 0.5), exactly
                p = _blend(torch.full_like(p, mean), p, fc)
            elif op == SATURATION:
                p = _blend(_grey(p)[..., None].expand_as(p), p, fs)
            else:
                p = _hue(p, int(row[I_HUE]))
        out[b] = p.to(torch.uint8)
    return out


def host_blur(img, table):
    """RandomGaussianBlur on (B,h,w,3) uint8: scipy's symmetric correlate1d along the rows then the columns of img / 255. in double,
    edge replicated, then * 255 truncated to a byte."""
    out = img.clone()
    h, w = img.shape[1:3]
    for b in range(img.shape[0]):
        row = table[b]
        radius = int(row[I_RADIUS])
        if radius == 0:
            continue
        wts = row[I_WEIGHTS:I_WEIGHTS + 12].clone().view(torch.float64)
        x = img[b].to(torch.float64) / 255.0
        for dim, size in ((0, h), (1, w)):
            ar = torch.arange(size)
            acc = x * wts[0]
            for j in range(radius, 0, -1):
                acc = acc + (x.index_select(dim, (ar - j).clamp(min=0)) + x.index_select(dim, (ar + j).clamp(max=size - 1))) * wts[j]
            x = acc
        out[b] = (x * 255.0).clamp_(0.0, 255.0).to(torch.uint8)
    return out


def host_normalise(img, norm_table, out):
    """table[c][byte] of (B,h,w,3) uint8 into the (B,3,h,w)-logical `out`."""
    val = norm_table.t()[img.long(), torch.arange(3)]
    out.copy_(val.permute(0, 3, 1, 2))
    return out
