"""GPU: the layer-compressibility analysis.  The masked engine site (frozen conv on the kept filters only -> compact tensor ->
trainable 1x1) and AnalysisTrainer against the reference's own run (tests/golden/analysis.npz, tools/make_golden_analysis.py), and
kd_logit_metrics_up against a float64 restatement and against the ops it replaces."""
import functools
import signal

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _netutil import trainer_config  # noqa: E402
from _seeded import sample_idx, seeded_fill_, seeded_input  # noqa: E402

U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def limit(seconds):
    """Per-test time limit (SIGALRM in the main thread): a test that overruns fails instead of holding the device."""
    def deco(fn):
        @functools.wraps(fn)
        def run(*a, **k):
            def on_alarm(signum, frame):
                raise TimeoutError(f"{fn.__name__} exceeded its {seconds}-s limit")
            old = signal.signal(signal.SIGALRM, on_alarm)
            signal.alarm(seconds)
            try:
                return fn(*a, **k)
            finally:
                signal.alarm(0)
                signal.signal(signal.SIGALRM, old)
        return run
    return deco


def _check(t, g, key, tol, what, allow_kinks=False):
    """tests/test_modeb_gpu.py's comparison against a stored subsample + sum of squares."""
    f = t.detach().float().contiguous().reshape(-1).cpu()
    assert list(t.shape) == [int(v) for v in g[f"{key}.shape"]], what
    ref = g[f"{key}.sample"].astype(np.float64)
    got = f[sample_idx(f.numel())].numpy().astype(np.float64)
    l2 = np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)
    scale = max(np.abs(ref).max(), 1e-30)
    frac_bad = float((np.abs(got - ref) > tol * scale).mean())
    ssq, rs = float((f.double() ** 2).sum()), float(g[f"{key}.sumsq"][0])
    print(f"{what}: relative L2 {l2:.3e}, samples off {frac_bad:.3%}, sumsq {ssq:.6e} vs {rs:.6e}")
    assert l2 < tol, f"{what}: relative L2 err {l2:.3e} (tol {tol})"
    assert frac_bad <= (0.004 if allow_kinks else 0.0), f"{what}: {frac_bad:.3%} of samples off by more than {tol} of range"
    assert abs(ssq - rs) <= 4 * tol * rs + 1e-30, f"{what}: sumsq {ssq} vs {rs}"


def _teacher():
    from kdcc_amd.models import DeepWV3Plus
    t = DeepWV3Plus(num_classes=19)
    seeded_fill_(t, "teacher.")
    return t.eval()


def _probe(model, name, seed):
    """What tools/make_golden_analysis.py did on the reference: seed numpy (the mask) and torch, replace, seed the new 1x1."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    model.replace([name], droprate=0.85)
    blk = model.get_block(name, model.student)
    seeded_fill_(blk[2], f"student.{name}.2.")
    model.register_hint_layers([name])
    return blk


def _student(name, seed, dtype, teacher=None):
    from kdcc_amd.models.students import AnalysisStudent
    model = AnalysisStudent(teacher if teacher is not None else _teacher(), None, dtype=dtype)
    blk = _probe(model, name, seed)
    return model.cuda(), model.get_block(name, model.student)


def _step(model):
    from kdcc_amd import losses
    x = seeded_input("analysis.x0", (2, 3, 64, 128)).cuda()
    st, tc = model(x)
    crit = losses.MSELoss(num_classes=1000)
    hint = sum(crit(a, b) for a, b in zip(model.student_hidden_outputs, model.teacher_hidden_outputs))
    hint.backward()
    torch.cuda.synchronize()
    return st, tc, hint


# ================================================================================== masked site
@pytest.mark.parametrize("i", [0, 1])
@limit(420)
def test_masked_site_matches_reference_fp32(golden, i):
    from kdcc_amd import losses
    g = golden("analysis")
    name, seed = str(g["layers"][i]), int(g["seed"]) + i
    model, blk = _student(name, seed, torch.float32)
    assert np.array_equal(blk[1].mask.reshape(-1).cpu().numpy().astype(np.uint8), g[f"step{i}.mask"])     # the reference's draw
    from kdcc_amd import ops
    ops.PROFILER = []
    try:
        st, tc, hint = _step(model)
        prof = list(ops.PROFILER)
    finally:
        ops.PROFILER = None
    assert st.pending and tc.pending
    # the launch log: the frozen conv ran with Cout == Kp (fp32 granule 32: 96 for 77 kept filters, 64 for 39), never dense
    C, kk = blk[2].weight.shape[0], int(blk[1].keep.numel())
    kp = (kk + 31) // 32 * 32
    cin, k, dil = blk[0].in_channels, blk[0].kernel_size[0], blk[0].dilation[0]
    labels = [p[4] for p in prof if p[0] == "conv_igemm"]
    print("kept", kk, "Kp", kp, [l for l in labels if f" {cin}->{kp} " in l or f" {kp}->{C} " in l])
    assert kp == {77: 96, 39: 64}[kk] and kp < C
    assert len([l for l in labels if l.startswith(f"{k}x{k} s1 d{dil} ") and f" {cin}->{kp} " in l]) == 1, labels
    assert len([l for l in labels if l.startswith("1x1 ") and f" {kp}->{C} " in l]) == 1, labels
    # dense launches of this signature: one per teacher conv and per untouched student conv -- none for the probed layer's copy
    sig = lambda m_: isinstance(m_, torch.nn.Conv2d) and (m_.in_channels, m_.out_channels, m_.kernel_size[0], m_.dilation[0],
                                                         m_.stride[0]) == (cin, C, k, dil, 1)
    dense = sum(sig(m_) for _, m_ in model.teacher.named_modules()) + \
        sum(sig(m_) for n_, m_ in model.student.named_modules() if n_ != name + ".0")
    assert len([l for l in labels if l.startswith(f"{k}x{k} s1 d{dil} ") and f" {cin}->{C} " in l]) == dense, (dense, labels)
    assert any(p[0] == "pw_wgrad" and f"{kp}->{C}" in p[4] for p in prof), [p[4] for p in prof if p[0] == "pw_wgrad"]
    key = f"step{i}"
    _check(model.student_hidden_outputs[0], g, key + ".block_out", 1e-3, f"{name} block output")
    _check(model.teacher_hidden_outputs[0], g, key + ".teacher_hint", 1e-3, f"{name} teacher hint")
    print("hint loss", hint.item(), float(g[key + ".hint_loss"]))
    np.testing.assert_allclose(hint.item(), float(g[key + ".hint_loss"]), rtol=1e-3)
    w = blk[2].weight
    assert w.grad is not None and tuple(w.grad.shape) == tuple(w.shape)
    _check(w.grad, g, key + ".grad", 1e-3, f"{name} 1x1 gradient", allow_kinks=True)
    dropped = (blk[1].mask.reshape(-1) == 0).cpu()
    gd = w.grad.detach().cpu().reshape(w.shape[0], -1)[:, dropped]
    assert gd.numel() == w.shape[0] * int(w.shape[1] * 0.85)
    assert bool((gd.view(torch.int32) == 0).all()), "dropped columns of the gradient must be +0.0 bit for bit"
    assert float(g[key + ".grad_dropped_absmax"]) == 0.0
    tgt = torch.from_numpy(g["target0"].astype(np.int64)).cuda()
    ce, kd = losses.CrossEntropyLoss2d(ignore_index=255), losses.MSELoss("mean", 1)
    np.testing.assert_allclose(ce(st, tgt).item(), float(g[key + ".supervised_loss"]), rtol=1e-3)
    np.testing.assert_allclose(ce(tc, tgt).item(), float(g[key + ".teacher_loss"]), rtol=1e-3)
    np.testing.assert_allclose(kd(st, tc).item(), float(g[key + ".kd_loss"]), rtol=1e-3)
    _check(st, g, key + ".student_logits", 1e-3, f"{name} student logits")
    _check(tc, g, key + ".teacher_logits", 1e-3, f"{name} teacher logits")


def _site_io(model, name):
    """(engine, site, its input, the shortcut its epilogue adds or None) of the masked site `name`, from one forward's tape."""
    eng = model._student_engine()
    eng.hint_names = [name]
    with torch.no_grad():
        eng.forward(seeded_input("analysis.x0", (2, 3, 64, 128)).cuda())
    tape, eng._tape = eng._tape, None
    if name.startswith("aspp"):
        site = [b["site"] for b in tape["aspp"]["branches"] if b["site"].name == name][0]
        return eng, site, tape["aspp"]["x7"], None
    rec = [r for r in tape["blocks"] if r is not None and r["name"] == name.split(".convs.")[0]][0]
    si = [st.name for st in rec["sites"]].index(name)
    assert si == len(rec["sites"]) - 1 and not rec["proj"]           # last conv of an identity-shortcut block
    return eng, rec["sites"][si], rec["a_in"][si], rec["x_raw"]


@pytest.mark.parametrize("i", [0, 1])
@limit(420)
def test_masked_site_bf16_against_fp32(golden, i):
    """The measured dtype.  (a) One bf16 analysis step: the ops-level launch log shows the frozen conv launched with Cout == Kp, the
    1x1 with Cin == Kp and the weight gradient against the compact tensor; dropped gradient columns are bitwise zero.  (b) The
    masked site in bf16 against the same site in fp32 ON THE SAME INPUTS (the bf16 activations the network hands it, as
    tests/test_ops_gpu.py rounds an operator's inputs to the storage dtype before its oracle sees them), forward and weight
    gradient, at that file's bf16 operator bars: 1.5e-2 of range, 5e-3 relative L2.  (c) The two whole networks' block outputs
    differ by what the bf16 layers upstream of the site have accumulated; that figure is printed, not held to an operator bar."""
    from kdcc_amd import ops
    g = golden("analysis")
    name, seed = str(g["layers"][i]), int(g["seed"]) + i
    teacher = _teacher()
    m16, b16 = _student(name, seed, torch.bfloat16, teacher)
    ops.PROFILER = []
    try:
        _step(m16)
        prof = list(ops.PROFILER)
    finally:
        ops.PROFILER = None
    C = b16[2].weight.shape[0]
    kk = int(b16[1].keep.numel())
    kp = (kk + 63) // 64 * 64
    cin, k = b16[0].in_channels, b16[0].kernel_size[0]
    labels = [p[4] for p in prof if p[0] == "conv_igemm"]
    frozen = [l for l in labels if l.startswith(f"{k}x{k} ") and f" {cin}->{kp} " in l]
    print("kept", kk, "Kp", kp, "frozen-conv launches", frozen)
    assert len(frozen) == 1 and kp < C, labels
    assert len([l for l in labels if l.startswith("1x1 ") and f" {kp}->{C} " in l]) == 1, labels
    assert any(p[0] == "pw_wgrad" and f"{kp}->{C}" in p[4] for p in prof), [p[4] for p in prof if p[0] == "pw_wgrad"]
    dropped = (b16[1].mask.reshape(-1) == 0).cpu()
    assert bool((b16[2].weight.grad.cpu().reshape(C, -1)[:, dropped].view(torch.int32) == 0).all())
    # (b) the site alone, both dtypes on identical inputs
    m32, b32 = _student(name, seed, torch.float32, teacher)
    assert torch.equal(b16[1].mask, b32[1].mask) and torch.equal(b16[2].weight, b32[2].weight)
    eng16, site16, a_in, short = _site_io(m16, name)
    eng32, site32, _, _ = _site_io(m32, name)
    assert site16.masked and site32.masked and a_in.dtype == torch.bfloat16
    h16 = m16.student_hidden_outputs[0].detach().float().cpu().numpy().astype(np.float64)
    _step(m32)
    h32 = m32.student_hidden_outputs[0].detach().float().cpu().numpy().astype(np.float64)
    print(f"bf16 network vs fp32 network, {name} block output: max err {np.abs(h16 - h32).max() / np.abs(h32).max():.3e} of range, "
          f"relative L2 {np.sqrt(((h16 - h32) ** 2).sum() / (h32 ** 2).sum()):.3e}")
    N, H, W, _ = a_in.shape
    res = {}
    for tag, eng, site, dt in (("bf16", eng16, site16, torch.bfloat16), ("fp32", eng32, site32, torch.float32)):
        out = torch.empty((N, H, W, C), dtype=dt, device="cuda")
        kw = {} if short is None else {"res_pre": short.to(dt)}
        mid = eng._masked_fwd(site, a_in.to(dt).contiguous(), out_raw=out, **kw)
        if tag == "bf16":
            gy = (out.float() - out.float().mean()).to(torch.bfloat16)       # one upstream gradient for both: bf16-representable
        grads = {}
        eng._masked_bwd(site, mid, gy.to(dt), grads, False)
        torch.cuda.synchronize()
        res[tag] = (out.float().cpu().numpy().astype(np.float64), grads[site.mod[2].weight].cpu().numpy().astype(np.float64))
    for j, what in enumerate(("site output", "1x1 gradient")):
        got, ref = res["bf16"][j], res["fp32"][j]
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
        l2 = np.sqrt(((got - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-30))
        print(f"bf16 {name} {what}: max err {err:.3e} of range, relative L2 {l2:.3e}")
        assert err < 1.5e-2 and l2 < 5e-3, what


@pytest.mark.parametrize("name", ["mod7.block1.convs.conv3", "mod5.block1.convs.conv2"])
@limit(420)
def test_masked_projection_block_sites_match_the_uncompacted_composition(name):
    """The last conv of a projection block: a masked conv3 takes the two-launch form (no K-concatenated conv3 + proj_conv launch).
    Reference: the same site run uncompacted from existing ops -- full frozen conv, mask multiply, full 1x1 (+ the shortcut the
    site's epilogue adds) -- on the site's own input, taken from the engine's tape."""
    from kdcc_amd import ops
    from kdcc_amd._lib import KD_PACK_FWD
    for dtype, tol, tol2 in ((torch.float32, 1e-3, 2e-4), (torch.bfloat16, 1.5e-2, 5e-3)):
        model, blk = _student(name, 11, dtype)
        eng = model._student_engine()
        eng.hint_names = [name]
        x = seeded_input("analysis.x0", (2, 3, 64, 128)).cuda()
        ops.PROFILER = []
        try:
            with torch.no_grad():
                _, hints = eng.forward(x)
            prof = list(ops.PROFILER)
        finally:
            ops.PROFILER = None
        rec = [r for r in eng._tape["blocks"] if r is not None and r["name"] == name.split(".convs.")[0]][0]
        si = [s.name for s in rec["sites"]].index(name)
        assert rec["sites"][si].masked and rec["dual"] is False and si == len(rec["sites"]) - 1
        assert not [p[4] for p in prof if p[0] == "conv_igemm" and "+" in p[4].split("->")[0]], "a K-concatenated launch ran"
        a = rec["a_in"][si]
        conv, pw = blk[0], blk[2]
        N, H, W, _ = a.shape
        full = torch.empty((N, H, W, conv.out_channels), dtype=dtype, device="cuda")
        ops.conv2d(a, ops.pack_conv_weight(conv.weight, dtype, KD_PACK_FWD), conv.stride[0], conv.padding[0], conv.dilation[0], out_raw=full)
        masked = (full * blk[1].mask.reshape(1, 1, 1, -1).to(dtype)).contiguous()
        pcv = rec["blk"].proj_conv
        short = torch.empty((N, H, W, pw.out_channels), dtype=dtype, device="cuda")
        ops.conv2d(rec["a_in"][0], ops.pack_conv_weight(pcv.weight, dtype, KD_PACK_FWD), pcv.stride[0], 0, 1, out_raw=short)
        ref = torch.empty((N, H, W, pw.out_channels), dtype=dtype, device="cuda")
        ops.conv2d(masked, ops.pack_conv_weight(pw.weight, dtype, KD_PACK_FWD), res_pre=short, out_raw=ref)
        torch.cuda.synchronize()
        got, ref = hints[0].float().cpu().numpy().astype(np.float64), ref.float().cpu().numpy().astype(np.float64)
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
        l2 = np.sqrt(((got - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-30))
        print(f"{name} {dtype}: max err {err:.3e} of range, relative L2 {l2:.3e}")
        assert err < tol and l2 < tol2
        eng._tape = None


@limit(300)
def test_masked_site_refuses_an_input_gradient():
    from kdcc_amd.engine import EngineError
    name = "mod4.block2.convs.conv2"
    model, blk = _student(name, 5, torch.float32)
    model.student.mod4.block2.convs.conv1.weight.requires_grad = True       # something upstream of the masked site trains
    with pytest.raises(EngineError, match="input gradient"):
        _step(model)


# ================================================================================== kd_logit_metrics_up
def _ref_metrics(s_lo, t_lo, tgt, size, ignore_index, align_corners):
    """float64 restatement on the host: F.interpolate, log-softmax cross entropy over the valid pixels, the mean squared difference."""
    import torch.nn.functional as F
    up = lambda a: F.interpolate(a.double().cpu().permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=align_corners)
    S, T = up(s_lo), up(t_lo)
    Cc = S.shape[1]
    y = tgt.cpu().clone()
    valid = (y >= 0) & (y < Cc) & (y != ignore_index)
    ysafe = torch.where(valid, y, torch.zeros_like(y))
    out = {}
    for nm, A in (("s", S), ("t", T)):
        nll = -torch.log_softmax(A, 1).gather(1, ysafe.unsqueeze(1)).squeeze(1)
        out["ce_" + nm] = float(nll[valid].mean()) if bool(valid.any()) else 0.0
        out["ce_abs_" + nm] = float(nll[valid].abs().mean()) if bool(valid.any()) else 0.0
    d = S - T
    out["mse"], out["absd"] = float((d * d).mean()), float(d.abs().mean())
    out["X"] = float(max(s_lo.abs().max(), t_lo.abs().max()))
    return out


METRIC_CASES = [
    # N, h, w, C, H, W, align_corners
    (2, 32, 64, 19, 64, 128, True),       # the goldens' crop, DeepWV3Plus
    (2, 32, 64, 19, 64, 128, False),      # GSCNN's last upsample
    (1, 17, 23, 19, 67, 301, True),       # ragged: two 256-pixel chunks per row, the second partial
    (2, 9, 40, 7, 33, 157, False),        # any class count (re-interpolating instantiation)
    (1, 8, 24, 48, 16, 48, True),         # the largest class count: 138 KiB of LDS
]


@pytest.mark.parametrize("case", METRIC_CASES, ids=[f"{c[3]}cls-{c[1]}x{c[2]}-{c[4]}x{c[5]}-ac{int(c[6])}" for c in METRIC_CASES])
@limit(180)
def test_logit_metrics_up(case):
    from kdcc_amd import ops
    N, h, w, Cc, H, W, ac = case
    gen = torch.Generator().manual_seed(h * 1000 + W)
    s_lo = (torch.randn((N, h, w, Cc), generator=gen) * 2.5).cuda()
    t_lo = (s_lo.cpu() + torch.randn((N, h, w, Cc), generator=gen)).cuda()
    tgt = torch.randint(0, Cc, (N, H, W), generator=gen)
    tgt[:, :3] = 255                                    # ignored rows
    tgt[:, 5, ::7] = -1                                 # labels outside [0, C) ...
    tgt[:, 6, ::5] = Cc + 2
    tgt = tgt.cuda()
    # sentinels around every output
    obuf = torch.full((3 + 16,), 777.0, device="cuda")
    cbuf = torch.full((2 * Cc * Cc + 64,), -5, dtype=torch.int64, device="cuda")
    out_ref, cs, ct = ops.logit_metrics_up(s_lo, t_lo, tgt, (H, W), 255, ac)
    conf_s, conf_t = cbuf[16:16 + Cc * Cc].view(Cc, Cc), cbuf[32 + Cc * Cc:32 + 2 * Cc * Cc].view(Cc, Cc)
    conf_s.zero_(); conf_t.zero_()
    _, a, b = ops.logit_metrics_up(s_lo, t_lo, tgt, (H, W), 255, ac, conf_s=conf_s, conf_t=conf_t, accumulate=True)
    assert a.data_ptr() == conf_s.data_ptr() and b.data_ptr() == conf_t.data_ptr()
    # the second accumulating call goes to the library directly, its three floats into the middle of a sentinel-filled buffer
    from kdcc_amd import _lib
    ws, need = ops.loss_workspace(N, Cc, H * W, s_lo.device)
    out2 = obuf[8:11]
    _lib.check(_lib.lib().kd_logit_metrics_up(s_lo.data_ptr(), t_lo.data_ptr(), tgt.data_ptr(), 255, N, h, w, Cc, H, W, int(ac),
                                              out2.data_ptr(), conf_s.data_ptr(), conf_t.data_ptr(), 1, ws.data_ptr(), need,
                                              ops.stream_ptr()), "kd_logit_metrics_up")
    torch.cuda.synchronize()
    assert bool((obuf[:8] == 777.0).all()) and bool((obuf[11:] == 777.0).all()), "written outside the three outputs"
    keep = torch.ones_like(cbuf, dtype=torch.bool)
    keep[16:16 + Cc * Cc] = False; keep[32 + Cc * Cc:32 + 2 * Cc * Cc] = False
    assert bool((cbuf[keep] == -5).all()), "a confusion matrix was written out of bounds"
    assert out_ref.view(torch.int32).tolist() == out2.view(torch.int32).tolist(), "two runs differ bitwise"
    # integer-equal to kd_confusion on the materialised tensors; accumulate adds, the plain call overwrites
    S = ops.upsample_bilinear_ac(s_lo, (H, W), out_dtype=torch.float32, align_corners=ac).permute(0, 3, 1, 2)
    T = ops.upsample_bilinear_ac(t_lo, (H, W), out_dtype=torch.float32, align_corners=ac).permute(0, 3, 1, 2)
    want_s, want_t = ops.confusion(S, tgt), ops.confusion(T, tgt)
    assert torch.equal(cs, want_s) and torch.equal(ct, want_t)
    assert torch.equal(conf_s, 2 * want_s) and torch.equal(conf_t, 2 * want_t)
    assert int(want_s.sum()) == int(((tgt >= 0) & (tgt < Cc)).sum())
    # float outputs against float64.  Bounds (fp32 unit roundoff U): an interpolated logit is three two-term blends, |error| <=
    # gamma(6) X with X = max |logit|; log-sum-exp is 1-Lipschitz in the max norm, so a pixel's cross entropy moves by at most
    # 2 gamma(6) X from its inputs, plus the fast exp / log intrinsics (a few ulp on z and on its logarithm: 2^-18 covers 32 ulp
    # of a sum of <= 48 terms and the logarithm's absolute error), plus gamma(C + 4) of its own magnitude for the C-term sums;
    # the mean over pixels is taken in fp64.  MSE: d = s - t carries 2 gamma(6) X + U |d|, so sum d^2 moves by <= 4 gamma(7) X
    # mean|d| + gamma(C + 3) mse.
    r = _ref_metrics(s_lo, t_lo, tgt, (H, W), 255, ac)
    got = out_ref.cpu().double().tolist()
    b_mse = 4 * gamma(7) * r["X"] * r["absd"] + gamma(Cc + 3) * r["mse"] + U * r["mse"]
    for nm, gv in (("s", got[0]), ("t", got[1])):
        b_ce = 2 * gamma(6) * r["X"] + 2.0 ** -18 + gamma(Cc + 4) * r["ce_abs_" + nm] + U * r["ce_" + nm]
        print(f"CE({nm}) {gv!r} ref {r['ce_' + nm]!r} |err| {abs(gv - r['ce_' + nm]):.3e} bound {b_ce:.3e}")
        assert abs(gv - r["ce_" + nm]) <= b_ce
    print(f"MSE {got[2]!r} ref {r['mse']!r} |err| {abs(got[2] - r['mse']):.3e} bound {b_mse:.3e}")
    assert abs(got[2] - r["mse"]) <= b_mse
    # and the ops it replaces agree at their own precision
    assert abs(got[0] - ops.ce2d_up(s_lo, tgt, (H, W), 255, ac).item()) <= 2 * U * abs(got[0])
    np.testing.assert_allclose(got[2], ops.hint_mse(S, T, 1.0, want_grad=False)[0].item(), rtol=1e-5)


@limit(120)
def test_logit_metrics_up_all_ignored_and_limits():
    from kdcc_amd import ops
    s_lo, t_lo = torch.randn(1, 8, 16, 19).cuda(), torch.randn(1, 8, 16, 19).cuda()
    tgt = torch.full((1, 16, 32), 255, dtype=torch.int64).cuda()
    out, cs, ct = ops.logit_metrics_up(s_lo, t_lo, tgt, (16, 32))
    assert out[0].item() == 0.0 and out[1].item() == 0.0 and out[2].item() > 0 and int(cs.sum()) == 0 and int(ct.sum()) == 0
    # beyond the resampling-ratio limit (more than 160 source columns under 256 output pixels): refused, nothing launched
    s2, t2 = torch.randn(1, 8, 400, 19).cuda(), torch.randn(1, 8, 400, 19).cuda()
    with pytest.raises(ops.MetricsUnsupported):
        ops.logit_metrics_up(s2, t2, torch.zeros((1, 16, 512), dtype=torch.int64).cuda(), (16, 512))
    with pytest.raises(ops.MetricsUnsupported):
        ops.logit_metrics_up(torch.randn(1, 4, 8, 49).cuda(), torch.randn(1, 4, 8, 49).cuda(), torch.zeros((1, 8, 16), dtype=torch.int64).cuda(), (8, 16))


# ================================================================================== trainer
def _trainer(tmp_path, layers, epochs=2, len_epoch=2, lr=1e-3, batches=(), fused=True):
    from kdcc_amd import ConfigParser, losses, models
    from kdcc_amd.models.students import AnalysisStudent
    from kdcc_amd.trainer import AnalysisTrainer
    from kdcc_amd.utils import WeightScheduler
    from kdcc_amd.utils import optim as optim_module
    cfg = trainer_config([], lr=lr, len_epoch=len_epoch, save_dir=str(tmp_path))
    cfg["trainer"].update(name="AnalysisTrainer", epochs=epochs, fused_metrics=fused)
    cfg["layer_compressible"] = layers
    config = ConfigParser(cfg, run_id="a")
    teacher = config.init_obj("teacher", models)
    seeded_fill_(teacher, "teacher.")
    teacher.eval()
    model = AnalysisStudent(teacher, config)
    assert model.dtype == torch.float32
    crit = [config.init_obj(k, losses) for k in ("supervised_loss", "kd_loss", "hint_loss")]
    opt = config.init_obj("optimizer", optim_module, model.student.parameters())
    sched = config.init_obj("lr_scheduler", optim_module.lr_scheduler, opt)
    tr = AnalysisTrainer(model, crit, [], opt, config, list(batches), None, sched, WeightScheduler(config["weight_scheduler"]))
    return tr, model


@pytest.mark.parametrize("fused", [True, False])
@limit(600)
def test_analysis_trainer_epoch_matches_reference(golden, tmp_path, fused):
    """One 3-step AnalysisTrainer._train_epoch against the reference's log dict and final 1x1 weight (bars of
    tests/test_trainer_gpu.py); with the fused metrics neither logits tensor is ever materialised."""
    from kdcc_amd.lazy import LazyLogits
    g = golden("analysis")
    name, lr = str(g["epoch.layer"]), float(g["lr"])
    batches = [(seeded_input(f"analysis.x{10 + i}", (2, 3, 64, 128)), torch.from_numpy(g["epoch.targets"][i].astype(np.int64)))
               for i in range(3)]
    tr, model = _trainer(tmp_path, [{"layer_name": name, "lrs": [lr], "args": {"droprate": 0.85}}], lr=lr, batches=batches, fused=fused)
    blk = _probe(model, name, int(g["seed"]) + 7)
    assert np.array_equal(blk[1].mask.reshape(-1).cpu().numpy().astype(np.uint8), g["epoch.mask"])
    tr.reset_scheduler()
    tr.create_new_optimizer()
    for group in tr.optimizer.param_groups:
        group["lr"] = lr
    seen, held, ends = [], [], []
    orig = tr._logged_metrics

    def spy(st, tc, target):
        res = orig(st, tc, target)
        seen.append((isinstance(st, LazyLogits) and st.pending, isinstance(tc, LazyLogits) and tc.pending))
        held.append((st, tc))
        return res
    tr._logged_metrics = spy
    fwd = model.forward

    def forward_spy(x):
        # a step ends where the next one calls the model: hint loss, backward, optimizer and metric updates are behind it
        ends.extend((isinstance(a, LazyLogits) and a.pending, isinstance(b, LazyLogits) and b.pending) for a, b in held[len(ends):])
        return fwd(x)
    model.forward = forward_spy
    try:
        log = tr._train_epoch(1, lr=lr, layer_name=name)
    finally:
        del model.forward
    ends.extend((isinstance(a, LazyLogits) and a.pending, isinstance(b, LazyLogits) and b.pending) for a, b in held[len(ends):])
    print({k: (log[k], float(g["epoch.log:" + k])) for k in log})
    assert len(seen) == 3 and len(ends) == 3 and tr.fused_metric_steps == (3 if fused else 0)
    if fused:
        assert all(a and b for a, b in seen), "a logits tensor was materialised by the step's logged metrics"
        assert all(a and b for a, b in ends), "a logits tensor was materialised before its step ended"
    for k in ("loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss"):
        np.testing.assert_allclose(log[k], float(g["epoch.log:" + k]), rtol=1e-3, err_msg=k)
    for k in ("train_teacher_mIoU", "train_student_mIoU"):
        np.testing.assert_allclose(log[k], float(g["epoch.log:" + k]), rtol=2e-2, atol=1e-4, err_msg=k)   # argmax ties on random nets
    assert set(log) == {"loss", "supervised_loss", "kd_loss", "hint_loss", "teacher_loss", "train_teacher_mIoU", "train_student_mIoU"}
    f = blk[2].weight.detach().float().contiguous().reshape(-1).cpu()
    ref = g["epoch.weight.sample"].astype(np.float64)
    got = f[sample_idx(f.numel())].numpy().astype(np.float64)
    rel = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print("final 1x1 weight: relative L2", rel)
    assert rel < 1e-3


@limit(300)
def test_trainer_falls_back_beyond_the_ratio_limit(tmp_path):
    """LazyLogits whose resampling ratio kd_logit_metrics_up refuses: the trainer composes the criteria and kd_confusion and logs
    the same numbers as on a supported shape it is told not to fuse."""
    from kdcc_amd.lazy import LazyLogits
    gen = torch.Generator().manual_seed(9)
    tr, _ = _trainer(tmp_path, [])
    for (h, w, H, W), supported in (((8, 400, 16, 512), False), ((8, 64, 16, 128), True)):
        s_lo, t_lo = torch.randn((1, h, w, 19), generator=gen).cuda(), torch.randn((1, h, w, 19), generator=gen).cuda()
        tgt = torch.randint(0, 19, (1, H, W), generator=gen)
        tgt[:, :2] = 255                                   # ignored rows ...
        tgt[:, 3, ::9] = -1                                # ... and labels outside [0, C): skipped by both paths alike
        tgt[:, 4, ::7] = 23
        tgt = tgt.cuda()
        res = {}
        for fused in (True, False):
            tr.fused_metrics, tr.fused_metric_steps = fused, 0
            tr.train_iou_metrics.reset(); tr.train_teacher_iou_metrics.reset()
            vals = tr._logged_metrics(LazyLogits(s_lo, (H, W)), LazyLogits(t_lo, (H, W)), tgt)
            res[fused] = ([float(v) for v in vals], tr.train_iou_metrics.conf.clone(), tr.train_teacher_iou_metrics.conf.clone(),
                          tr.fused_metric_steps)
        print(h, w, H, W, res[True][0], res[False][0])
        assert res[True][3] == (1 if supported else 0) and res[False][3] == 0
        np.testing.assert_allclose(res[True][0], res[False][0], rtol=1e-5)
        assert torch.equal(res[True][1], res[False][1]) and torch.equal(res[True][2], res[False][2])


@limit(900)
def test_analysis_train_leaves_the_student_equal_to_the_teacher(tmp_path):
    """train() over two layers x two learning rates (epochs = 2 -> one epoch each): every probe trains, and after the last reset()
    the student is the teacher again, key for key and bit for bit."""
    batches = [(seeded_input(f"analysis.x{20 + i}", (1, 3, 64, 64)),
                torch.randint(0, 19, (1, 64, 64), generator=torch.Generator().manual_seed(i))) for i in range(2)]
    layers = [{"layer_name": "mod4.block2.convs.conv1", "lrs": [0.01, 0.001], "args": {"droprate": 0.85}},
              {"layer_name": "aspp.features.2.0", "lrs": [0.005, 0.0005], "args": {"droprate": 0.85}}]
    tr, model = _trainer(tmp_path, layers, epochs=2, len_epoch=1, batches=batches)
    epochs = []
    orig = tr._train_epoch

    def spy(epoch, **kw):
        blk = model.get_block(kw["layer_name"], model.student)
        before = blk[2].weight.detach().clone()
        assert all(gr["lr"] == kw["lr"] for gr in tr.optimizer.param_groups)
        log = orig(epoch, **kw)
        assert not torch.equal(before, blk[2].weight.detach()), "the probe's 1x1 did not train"
        epochs.append((kw["layer_name"], kw["lr"], log["hint_loss"]))
        return log
    tr._train_epoch = spy
    tr.train()
    assert [(a, b) for a, b, _ in epochs] == [(l["layer_name"], lr) for l in layers for lr in l["lrs"]]
    assert all(np.isfinite(h) and h > 0 for _, _, h in epochs)
    sd_s, sd_t = model.student.state_dict(), model.teacher.state_dict()
    assert list(sd_s) == list(sd_t)
    assert all(torch.equal(sd_s[k].float().cpu(), sd_t[k].float().cpu()) for k in sd_s)
    assert model.replaced_block_names == [] and model.hint_block_names == []
