"""The engine's fused epilogues on both sides of their shape gates, against oracle/net_ref.py (fp32 CPU) and against the same engine with
that one fusion switched off:

  * the decoder classifier in the epilogue of final[3] (cls_epilogue, engine._decoder_fwd) with a logit loss back-propagated on a
    model whose logits_need_grad was never set -- the backward must rebuild the activation the forward did not store;
  * the ASPP image-pool channel sums in the epilogue of the trunk's last conv (out_sums_epilogue): aspp_image_pool(sums=) takes rows
    of 128 pixels inside one image, so a crop whose trunk output is not whole 128-pixel rows per image must pool the map instead;
  * the K-concatenated conv3 + proj_conv (the "dual" 1x1) refused by the real call after the engine chose it: the two-launch fallback
    must not leave the never-written sums buffer behind for the image pooling.

Each test first asserts, through the kernel log or the selection query, that its shape does (or does not) open the gate it is about,
so a later dispatch change fails here instead of turning the test into a no-op.  test_bf16_path_gpu.py covers the bench's own step."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from _netutil import P92, build_student, check_step, oracle_threads, rel_l2, seeded_cheap_weights, seeded_teacher_sd  # noqa: E402
from _seeded import seeded_input  # noqa: E402

BF = torch.bfloat16
_SD = {}
_REF = {}


def _oracle(key, shape, backprop):
    """net_ref.kd_step on the seeded P92 student, memoised per input (two tests share the 2 x 256 x 512 one)."""
    from oracle import net_ref
    if "t" not in _SD:
        _SD["t"] = seeded_teacher_sd()
        _SD["s"] = net_ref.make_student_sd(_SD["t"], P92, seeded_cheap_weights(_SD["t"], P92))
    if (key, backprop) not in _REF:
        oracle_threads()
        _REF[(key, backprop)] = net_ref.kd_step(_SD["t"], _SD["s"], seeded_input(key, shape), None, P92, backprop=backprop)
    return _REF[(key, backprop)]


def _step(x, backprop="hint"):
    """One step of a fresh bf16 P92 model: loss = hint MSE, or KLDiv(student, teacher logits) + hint MSE.  Returns the model (for
    check_step) and a dict: the kernel-log counts, the student's ASPP image-pool branch as the forward left it, whether that branch
    was fed the conv epilogue's sums, and CPU copies of the logits / hints / loss / gradients for the engine-to-engine comparisons."""
    from kdcc_amd import _lib, losses
    model = build_student(P92, BF)
    with _lib.kernel_log() as log:
        out_st, out_tc = model(x)
        tape = model._engine._tape
        red = model.student.aspp.img_conv[0].out_channels
        pool = tape["aspp"]["cat"][..., :red].float().cpu()
        fed_sums = tape.get("x7_sums") is not None
        crit = losses.MSELoss(num_classes=1000)
        hint = 0
        for s, t in zip(model.student_hidden_outputs, model.teacher_hidden_outputs):
            hint = hint + crit(s, t)
        kd = losses.KLDivergenceLoss(1)(out_st, out_tc)
        loss = hint if backprop == "hint" else kd + hint
        loss.backward()
        torch.cuda.synchronize()
    res = dict(counts=log.counts, pool=pool, fed_sums=fed_sums, out_st=out_st, out_tc=out_tc, hint=hint, kd=kd, loss=loss.item(),
               st=out_st.detach().float().cpu(), tc=out_tc.detach().float().cpu(),
               hints=[h.detach().float().cpu() for h in model.student_hidden_outputs],
               grads={n: p.grad.detach().cpu() for n, p in model.student.named_parameters() if p.requires_grad})
    return model, res


def _vs_engine(a, b, what):
    """Relative L2 of run a against run b: ({logits and student hints}, {gradient name: ...})."""
    errs = {"student logits": rel_l2(a["st"], b["st"]), "teacher logits": rel_l2(a["tc"], b["tc"])}
    for i, (h, g) in enumerate(zip(a["hints"], b["hints"])):
        errs[f"hint {i}"] = rel_l2(h, g)
    grads = {n: rel_l2(a["grads"][n], b["grads"][n]) for n in b["grads"]}
    assert a["grads"].keys() == b["grads"].keys()
    print(what, {k: f"{v:.2e}" for k, v in errs.items()}, "worst gradients", sorted(grads.items(), key=lambda t: -t[1])[:3],
          "loss", a["loss"], b["loss"])
    return errs, grads


def _sums_rows(N, H, W, cin, cout):
    """kd_conv2d_bn_sums_rows for the trunk's last 1x1 as ops.conv2d(out_raw=, out_sums=) asks it: > 0 when the selected kernel would
    take the output sums in its epilogue."""
    from kdcc_amd import _lib
    d = _lib.ConvDesc(_lib.KD_BF16, N, H, W, cin, H, W, cout, 1, 1, 1, 0, 1, cin)
    ep = _lib.ConvEpilogue()
    ep.out_raw, ep.ld_raw = C.c_void_p(256), cout
    return int(_lib.lib().kd_conv2d_bn_sums_rows(C.byref(d), C.byref(ep)))


# ----------------------------------------------------------------------------------------- classifier epilogue + a logit loss
def test_classifier_epilogue_with_a_back_propagated_logit_loss(monkeypatch):
    """P92, bf16, 1 x 512 x 2048 (the decoder's 128 x 512 final[3] fills the row kernel: cls_epilogue selected), the default frozen
    head and logits_need_grad left False -- yet loss = KLDiv + hints is back-propagated, eagerly and through LazyLogits.  The forward
    ran the classifier in the epilogue and stored no final[3] activation; the backward rebuilds it from d1.  Loss and all 12
    gradients against net_ref.kd_step(backprop="kd+hint") and against the engine with the fusion off (KDCC_FUSE_CLS=0)."""
    shape = (1, 3, 512, 2048)
    x = seeded_input("gates.cls.x", shape).cuda()
    r = _oracle("gates.cls.x", shape, "kd+hint")
    runs = {}
    for fuse, lazy in (("1", "0"), ("1", "1"), ("0", "0")):
        monkeypatch.setenv("KDCC_FUSE_CLS", fuse)
        monkeypatch.setenv("KDCC_LAZY_LOGITS", lazy)
        model, res = _step(x, "kd+hint")
        # premise: the classifier epilogue carries the head exactly when the switch is on (teacher and student forwards)
        assert (res["counts"].get("cls_epilogue", 0) >= 2) == (fuse == "1"), res["counts"]
        assert abs(res["loss"] - r["loss"].item()) <= 5e-3 * abs(r["loss"].item()), (res["loss"], r["loss"].item())
        check_step(model, r, res["hint"], res["kd"], res["out_st"], res["out_tc"], 12, f"cls fuse={fuse} lazy={lazy} vs net_ref:")
        runs[fuse, lazy] = res
        del model, res
        torch.cuda.empty_cache()
    eager, lazy, off = runs["1", "0"], runs["1", "1"], runs["0", "0"]
    # the lazily materialised logits feed the same backward as the eager ones (the logged KL takes the half-resolution path: fp32 order)
    assert abs(eager["loss"] - lazy["loss"]) <= 1e-5 * abs(eager["loss"])
    for n in eager["grads"]:
        assert torch.equal(eager["grads"][n], lazy["grads"][n]), n
    # the same head either way, its classes summed in another fp32 order; measured: logits 5.6e-8 relative L2, hints bit-identical,
    # gradients <= 3.7e-5, loss equal
    errs, grads = _vs_engine(eager, off, "cls epilogue vs KDCC_FUSE_CLS=0:")
    assert all(torch.equal(h, g) for h, g in zip(eager["hints"], off["hints"]))
    assert max(errs.values()) < 2e-7 and max(grads.values()) < 1e-4, (errs, grads)
    assert abs(eager["loss"] - off["loss"]) <= 1e-6 * abs(off["loss"])


# ------------------------------------------------------------------------------------------- image-pool sums at odd crops
def test_image_pool_sums_at_a_crop_of_partial_128_pixel_rows(monkeypatch):
    """P92, bf16, 4 x 192 x 320: the trunk output is 24 x 40 = 960 = 7.5 x 128 pixels per image while its last 1x1 (M = 3840, 240 wide
    tiles) is on the ping-pong kernel that would take output sums.  Those rows straddle images, so the engine must not ask for
    them: the image pooling reads the map, forward and hint backward run, and the result is the _FUSE_GAP=False engine's bit for bit
    and net_ref's within the bf16 bars."""
    from kdcc_amd import engine
    shape = (4, 3, 192, 320)
    x = seeded_input("gates.gap.odd.x", shape).cuda()
    h8, w8 = shape[2] // 8, shape[3] // 8
    assert (h8 * w8) % 128 == 64 and _sums_rows(shape[0], h8, w8, 2048, 4096) > 0        # premise: the kernel would hand sums out
    r = _oracle("gates.gap.odd.x", shape, "hint")
    runs = {}
    for fuse in (True, False):
        monkeypatch.setattr(engine, "_FUSE_GAP", fuse)
        model, res = _step(x)
        assert not res["fed_sums"] and res["counts"].get("out_sums_epilogue", 0) == 0, res["counts"]
        check_step(model, r, res["hint"], res["kd"], res["out_st"], res["out_tc"], 12, f"4x192x320 _FUSE_GAP={fuse} vs net_ref:")
        runs[fuse] = res
        del model, res
    on, off = runs[True], runs[False]
    assert torch.equal(on["pool"], off["pool"]) and torch.equal(on["st"], off["st"]) and torch.equal(on["tc"], off["tc"])
    for n in off["grads"]:
        assert torch.equal(on["grads"][n], off["grads"][n]), n


def test_image_pool_sums_where_they_fit(monkeypatch):
    """The companion shape, 2 x 256 x 512: 32 x 64 = 2048 trunk pixels per image, whole 128-pixel rows -- the image pooling takes the
    sums of the (dual) conv3 + proj_conv epilogue.  Against net_ref and against the _FUSE_GAP=False engine, which pools the map."""
    from kdcc_amd import engine
    shape = (2, 3, 256, 512)
    x = seeded_input("gates.gap.x", shape).cuda()
    r = _oracle("gates.gap.x", shape, "hint")
    runs = {}
    for fuse in (True, False):
        monkeypatch.setattr(engine, "_FUSE_GAP", fuse)
        model, res = _step(x)
        assert res["fed_sums"] == fuse and (res["counts"].get("out_sums_epilogue", 0) >= 2) == fuse, res["counts"]   # teacher + student
        check_step(model, r, res["hint"], res["kd"], res["out_st"], res["out_tc"], 12, f"2x256x512 _FUSE_GAP={fuse} vs net_ref:")
        runs[fuse] = res
        del model, res
    on, off = runs[True], runs[False]
    pool = rel_l2(on["pool"], off["pool"])
    errs, grads = _vs_engine(on, off, f"2x256x512 sums vs read-back pooling (image pool {pool:.2e}):")
    # measured: bit-identical (the epilogue sums the stored bf16 values per 128-pixel block, as the pooling pass does); the bar
    # leaves room for an fp32 summation order, a wrong or unwritten block of sums is off by O(1)
    assert pool < 1e-6 and max(errs.values()) < 1e-6 and max(grads.values()) < 1e-6, (pool, errs, grads)


# ------------------------------------------------------------------------------------- the dual 1x1 refused after the engine chose it
def test_dual_conv_refused_by_the_real_call_falls_back_cleanly(monkeypatch):
    """At 2 x 256 x 512 the engine runs mod7.block1's conv3 + proj_conv as one K-concatenated 1x1 launch with the image-pool sums in
    its epilogue, and chooses the same for its conv1 + proj_conv input gradients in the backward.  Here the size check says yes
    (ops.conv1x1_dual_ok_dims) and the real call says no (kd_conv1x1_dual_supported = 0), as a view or epilogue the size check cannot
    see would: both fallbacks run, the forward one after the sums buffer was requested.  The image-pool branch, logits, hints and
    gradients must equal the normal run's within bf16 noise and net_ref's within the bf16 bars."""
    from kdcc_amd import _lib, ops
    shape = (2, 3, 256, 512)
    x = seeded_input("gates.gap.x", shape).cuda()
    r = _oracle("gates.gap.x", shape, "hint")
    lib = _lib.lib()
    real = lib.kd_conv1x1_dual_supported
    seen = []

    def record(answer):
        def f(d, cin2, ldx2, ep):
            d, e = d._obj, ep._obj
            ok = real(C.byref(d), cin2, ldx2, C.byref(e)) if answer is None else answer
            seen.append(dict(cin=d.Cin, cin2=cin2, cout=d.Cout, sums=bool(e.bn_sums), ok=bool(ok)))
            return ok
        return f

    monkeypatch.setattr(lib, "kd_conv1x1_dual_supported", record(None))
    model, normal = _step(x)
    del model
    # premise: the normal step takes the dual launch for mod7's conv3 + proj_conv with the sums in its epilogue, and the engine
    # chooses it for conv1 + proj_conv's input gradients (there the real call already refuses this shape's epilogue: measured)
    fwd = [s for s in seen if s["cout"] == 4096 and s["cin2"] == 2048]
    bwd = [s for s in seen if s["cin"] == 1024 and s["cin2"] == 4096]
    assert fwd and bwd and all(s["ok"] for s in fwd) and any(s["sums"] for s in fwd), seen
    assert normal["fed_sums"]

    seen.clear()
    monkeypatch.setattr(ops, "conv1x1_dual_ok_dims", lambda *a, **k: True)
    monkeypatch.setattr(lib, "kd_conv1x1_dual_supported", record(0))
    model, refused = _step(x)
    fwd = [s for s in seen if s["cout"] == 4096 and s["cin2"] == 2048]
    bwd = [s for s in seen if s["cin"] == 1024 and s["cin2"] == 4096]
    assert fwd and bwd and any(s["sums"] for s in fwd), seen          # both fallbacks ran, the forward one with the sums requested
    assert not refused["fed_sums"]                                    # ... and the image pooling read the map
    check_step(model, r, refused["hint"], refused["kd"], refused["out_st"], refused["out_tc"], 12, "2x256x512 dual refused vs net_ref:")
    del model
    pool = rel_l2(refused["pool"], normal["pool"])
    errs, grads = _vs_engine(refused, normal, f"2x256x512 dual refused vs dual (image pool {pool:.2e}):")
    # the two-launch form rounds the shortcut to bf16 before the add; measured: image pool 3.6e-4, logits 1.7e-3, the hints upstream
    # of mod7 bit-identical and the ASPP ones 4.2e-3, gradients <= 1.6e-4.  (A never-written sums buffer may hold an earlier step's
    # values and pass these bars: the fed_sums check above is the one that catches it.)
    assert pool < 1e-3 and errs["student logits"] < 5e-3 and errs["teacher logits"] < 5e-3 and max(errs.values()) < 1e-2, (pool, errs)
    assert max(grads.values()) < 5e-4, grads
