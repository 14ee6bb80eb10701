"""bench.py's stdout contract (CPU): the ONE JSON line must stay well inside the driver's stdout window (round 3's 21-KB line
was cut and the headline went unparsed), carry every contract key plus `roofline` and `cpu_baseline`, and pick the PMC traffic
summary that matches the configuration."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cls(ms, frac, hbm=False):
    return {"bound": "hbm" if hbm else "mfma", "launches_per_step": 67.0, "ms_per_step": ms, "achieved": 1234.56789, "unit": "TFLOP/s",
            "peak": 2500.0, "frac": frac, "algorithmic_tflop_per_step": 123.456789}


def _roofline():
    names = ["conv3x3_row_persistent_256x256", "conv1x1_persistent_256x256", "conv3x3_row_512x128", "conv_other_tiles", "dense_wgrad",
             "pointwise_wgrad", "depthwise_wgrad", "depthwise_fwd_fanout", "depthwise_dgrad_sum", "depthwise_dgrad_epilogue",
             "depthwise_fwd", "bn_param_sums", "losses"]
    return {"bound": "mfma", "kernel": "k" * 200, "achieved": 1262.123456, "peak": 2500.0, "unit": "TFLOP/s", "frac": 0.50484938,
            "traffic": 2911308624.124031, "traffic_note": "n" * 300, "launches_per_step": 129.0, "ms_per_step_in_kernel": 160.39123,
            "algorithmic_tflop_per_step": 202.4912345, "classes": {n: _cls(100.123456 / (i + 1), 0.5441234) for i, n in enumerate(names)}}


def _full_record():
    sub = {"metric": "m" * 60, "value": 38.351234, "unit": "images/sec", "steps": 8, "warmup": 2, "ms_per_step": 208.612345, "dtype": "bf16",
           "roofline": _roofline(), "dense_wgrad": {"frac": 0.41234, "achieved": 1030.0}, "losses": {"hint": 1.0}, "what": "w" * 120,
           "config": {"plan": "P86", "mode": "A", "arch": "gscnn", "hint_loss": "mse", "per_gpu_batch": 8}}
    return {"metric": "images/sec KD train step, DeepLabV3+(WRN38) student 1024x2048", "value": 41.7123456, "unit": "images/sec", "n_gpus": 1,
            "steps": 20, "warmup": 5, "ms_per_step": 191.7891234, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic", "_hw": "1024x2048",
            "profiler": {"events_in_timed_region": True, "ms_per_step_without_events": 190.123456, "ab_steps": 8},
            "config": {"workload": "w" * 400, "plan": "P92", "mode": "A", "arch": "deeplab", "hint_loss": "mse", "per_gpu_batch": 8,
                       "global_batch": 8, "parallelism": "dp1", "ranks_seen": 1, "backend": None,
                       "rank_devices": [{"rank": 0, "device": 0, "name": "AMD Instinct MI355X", "pci_bus_id": 5}], "replicas_identical_after_run": None, "teacher_overlap": False,
                       "teacher_backend": "hip", "per_step_host_syncs": False, "share_frozen_prefix": False,
                       "per_gpu_batch_sweep": {str(n): {"images_per_sec": 40.123456, "ms_per_step": 24.9, "steps": 8} for n in (1, 2, 4)}},
            "roofline": _roofline(), "dense_wgrad": None,
            "losses": {"hint": 123.456789012, "supervised": 3.0123456, "kd": 1e-6, "teacher": 3.0123456},
            "cpu_baseline": {"unit": "images/sec", "cores": 16, "host_cpu_count": 256, "kind": "port", "value": 0.01761234,
                             "step_1024x2048_s": 56.7812, "step_512x1024_s": 13.651234, "sample": "s" * 300},
            "sub_records": {n: sub for n in ("P79", "modeB", "gscnn_P86", "weighted_hint", "share_prefix", "ref_logging", "f32_parity")}}


def test_compact_line_is_short_and_complete():
    import bench
    full = _full_record()
    assert len(json.dumps(full)) > 15000            # the full record is the size that broke round 3's driver parse
    line = json.dumps(bench.compact_record(full, "gpurun_out/bench_full.json"))
    assert len(line) < 4096, len(line)
    rec = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in rec, k
    assert rec["config"]["workload"] and "model" not in rec["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rec["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in rec["cpu_baseline"], k
    assert abs(rec["value"] - full["value"]) < 1e-2 and abs(rec["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-3
    assert set(rec["sub_records"]) == {"P79", "modeB", "gscnn_P86", "weighted_hint", "share_prefix", "ref_logging", "f32_parity"}
    assert rec["sub_records"]["modeB"]["wgrad_frac"] == 0.412
    assert rec["batch_sweep"] == {"1": 40.12, "2": 40.12, "4": 40.12}
    assert len(rec["roofline"]["classes"]) == 13 and rec["roofline"]["classes"]["losses"][1] == 0.544


def test_traffic_summary_follows_the_configuration():
    import bench
    for mode, arch, plan, suffix in (("A", "deeplab", "P92", "traffic_pmc.json"), ("B", "deeplab", "P92", "traffic_modeB_pmc.json")):
        t, src = bench.conv_traffic(plan, 8, 1024, 2048, "bf16", mode, arch)
        assert t and t > 1e9 and src.endswith(suffix), (mode, t, src)
    assert bench.conv_traffic("P79", 8, 1024, 2048, "bf16", "A", "deeplab") == (None, None)
    assert bench.conv_traffic("P92", 8, 512, 1024, "bf16", "A", "deeplab") == (None, None)


def test_plain_record_carries_the_headline_only():
    """A run without --full measures no kernel figures: its line has the contract keys and no roofline / cpu_baseline."""
    import bench
    full = _full_record()
    plain = {k: v for k, v in full.items() if k not in ("roofline", "dense_wgrad", "cpu_baseline", "sub_records")}
    plain["profiler"] = {"events_in_timed_region": False, "ms_per_step_without_events": None, "ab_steps": 0}
    plain["config"] = dict(full["config"], per_gpu_batch_sweep={})
    rec = json.loads(json.dumps(bench.compact_record(plain)))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "losses"):
        assert k in rec, k
    assert "roofline" not in rec and "cpu_baseline" not in rec and "sub_records" not in rec and "batch_sweep" not in rec
    assert rec["ms_per_step"] == 191.8 and rec["profiler"]["events_in_timed_region"] is False


def test_dump_outputs_files_size_and_seeded_samples(tmp_path):
    """--dump-outputs on the CPU with stand-in tensors: float32 / float64 .npy files, the trainable parameters whole while they fit the
    budget and sampled (in proportion, seeded) beyond it, logits sampled at the same seeded (N, C, H, W) positions on every call."""
    import numpy as np
    import torch
    import bench

    class Net(torch.nn.Module):
        def __init__(self, big):
            super().__init__()
            self.a = torch.nn.Parameter(torch.randn(big))
            self.b = torch.nn.Parameter(torch.randn(4, 3, 3, 3))
            self.frozen = torch.nn.Parameter(torch.randn(10), requires_grad=False)

    model = type("M", (), {})()
    logits = torch.randn(2, 19, 64, 48).permute(0, 1, 3, 2)          # non-contiguous, as the engine's channels-last logits
    keep = {"student_logits": logits, "teacher_logits": logits * 2}
    losses = (torch.tensor(1.5), torch.tensor(2.0), torch.tensor(0.25), 3.0)

    model.student = Net(1000)
    bench.dump_outputs(str(tmp_path / "small"), model, keep, losses)
    d = tmp_path / "small"
    assert sorted(p.name for p in d.iterdir()) == sorted(["loss.npy", "supervised.npy", "kd.npy", "teacher.npy", "param.a.npy", "param.b.npy",
                                                         "student_logits.npy", "teacher_logits.npy"])
    assert np.load(d / "loss.npy").dtype == np.float64 and float(np.load(d / "kd.npy")) == 0.25
    np.testing.assert_array_equal(np.load(d / "param.b.npy"), model.student.b.detach().numpy())
    assert np.load(d / "param.b.npy").dtype == np.float32
    np.testing.assert_array_equal(np.load(d / "student_logits.npy"), logits.numpy())       # small: whole, logical (N, C, H, W)

    old = bench.DUMP_SAMPLE, bench.DUMP_PARAM_BUDGET
    try:
        bench.DUMP_SAMPLE, bench.DUMP_PARAM_BUDGET = 500, 2000
        model.student = Net(100000)
        for run in ("x", "y"):
            bench.dump_outputs(str(tmp_path / run), model, keep, losses)
        x, y = tmp_path / "x", tmp_path / "y"
        s = np.load(x / "student_logits.npy")
        idx = bench._sample_index(logits.shape, 500, 5).numpy()
        np.testing.assert_array_equal(s, logits.contiguous().reshape(-1).numpy()[idx])
        np.testing.assert_array_equal(np.load(x / "teacher_logits.npy"), 2 * logits.contiguous().reshape(-1).numpy()[bench._sample_index(logits.shape, 500, 6).numpy()])
        pa = np.load(x / "param.a.npy")
        assert pa.dtype == np.float32 and 1990 <= pa.size <= 2000 and np.isin(pa, model.student.a.detach().numpy()).all()
        assert sum(np.load(x / f).size for f in ("param.a.npy", "param.b.npy")) <= 2002
        for f in x.iterdir():
            np.testing.assert_array_equal(np.load(f), np.load(y / f.name))
    finally:
        bench.DUMP_SAMPLE, bench.DUMP_PARAM_BUDGET = old
