"""CPU: the reference's criteria names resolve in kdcc_amd.losses with the reference's constructor signatures
(tests/golden/criteria_names.json), and the reference's recorded values (tests/golden/criteria.npz) agree with the float64
restatement of their formulas (tests/_criteria_ref.py) that the GPU tests hold the kernels to."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import _criteria_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def crit():
    return np.load(os.path.join(GOLDEN, "criteria.npz"), allow_pickle=False)


def test_every_reference_criterion_resolves_with_its_signature():
    import kdcc_amd.losses as losses
    with open(os.path.join(GOLDEN, "criteria_names.json")) as f:
        names = json.load(f)
    assert {"JSDivergenceLoss", "EnsembleKLDivergenceLoss", "FocalLoss", "TopkHintMSELoss"} <= set(names)
    for name, params in names.items():
        cls = getattr(losses, name)            # AttributeError: a config naming it would fail at start-up
        sig = [(pn, p.default) for pn, p in inspect.signature(cls.__init__).parameters.items() if pn != "self"]
        assert [pn for pn, _ in sig] == [p["name"] for p in params], name
        for (pn, default), p in zip(sig, params):
            if p["required"]:
                assert default is inspect.Parameter.empty, (name, pn)
            else:
                assert default == p["default"] and type(default) is type(p["default"]), (name, pn, default, p["default"])


def test_focal_keeps_the_cross_entropy_weight_buffer():
    import kdcc_amd.losses as losses
    f = losses.FocalLoss(2, alpha=torch.arange(1.0, 4.0), ignore_index=255, reduction="mean")
    assert isinstance(f, torch.nn.CrossEntropyLoss)
    assert "weight" in dict(f.named_buffers()) and f.reduction == "mean" and f.gamma == 2 and f.ignore_index == 255
    assert losses.FocalLoss(0.5).reduction == "none"


def test_topk_refuses_what_the_reference_gets_wrong():
    import kdcc_amd.losses as losses
    with pytest.raises(ValueError, match="no channel"):
        losses.TopkHintMSELoss(topk=0.01)(torch.zeros(1, 8, 2, 2), torch.zeros(1, 8, 2, 2))
    with pytest.raises(ValueError, match="N,C,H,W"):
        losses.TopkHintMSELoss()(torch.zeros(2, 8), torch.zeros(2, 8))


def _close(loss, grad, g, tag):
    np.testing.assert_allclose(np.asarray(loss), g[f"{tag}.loss"], rtol=1e-4, atol=1e-7, err_msg=tag)
    np.testing.assert_allclose(grad, g[f"{tag}.grad"], rtol=1e-3, atol=1e-7, err_msg=tag)


def test_golden_jsd_and_ensemble_kl_match_the_formulas(crit):
    g = crit
    for T in (1, 4):
        for tag in (f"jsd_T{T}", f"jsd2d_T{T}"):
            loss, grad = R.jsd(torch.from_numpy(g[f"{tag}.s"]), torch.from_numpy(g[f"{tag}.t"]), T)
            _close(loss.item(), grad.numpy(), g, tag)
    loss, grad = R.ensemble_kl(torch.from_numpy(g["ekl.s"]), torch.from_numpy(g["ekl.t"]))
    _close(loss.item(), grad.numpy(), g, "ekl")


def focal_cases():
    for ign in (-100, 255):
        for gamma in (0, 2, 0.5):
            for red in ("none", "mean", "sum"):
                for an in ("noalpha", "alpha"):
                    yield ign, gamma, red, an


def focal_tag(ign, gamma, red, an):
    return f"focal_g{gamma}_{red}_{an}_{'m100' if ign < 0 else ign}"


def test_golden_focal_matches_the_formulas(crit):
    g = crit
    x = torch.from_numpy(g["focal.x"])
    for ign, gamma, red, an in focal_cases():
        tag = focal_tag(ign, gamma, red, an)
        tgt = torch.from_numpy(g[f"focal.target_{'m100' if ign < 0 else ign}"])
        assert (tgt == ign).any()
        alpha = torch.from_numpy(g["focal.alpha"]) if an == "alpha" else None
        up = torch.from_numpy(g[f"{tag}.up"]) if red == "none" else None
        loss, grad = R.focal(x, tgt, gamma, alpha, ign, red, up)
        _close(loss.numpy(), grad.numpy(), g, tag)


def test_golden_topk_matches_the_formulas(crit):
    g = crit
    for Cc in (24, 64):
        for k in (0.5, 0.25):
            tag = f"topk_{Cc}_{k}"
            t = torch.from_numpy(g[f"{tag}.t"])
            norm = np.sort(t.double().norm(dim=(-1, -2)).numpy(), axis=1)[:, ::-1]
            K = int(k * Cc)
            assert (norm[:, K - 1] - norm[:, K] > 1e-3 * norm[:, K]).all()     # a pivot far above rounding
            loss, grad = R.topk_hint(torch.from_numpy(g[f"{tag}.s"]), t, k)
            _close(loss.item(), grad.numpy(), g, tag)
