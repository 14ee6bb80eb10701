"""kd_gated_conv on a row of tests/_shape_stream_cases.py, shared by tests/test_shape_stream_gpu.py and by the child process it
starts for the bf16 VALU kernel: KDCC_GATED_MFMA is read once per process, so `python tests/_shape_stream_child.py` (with
KDCC_GATED_MFMA=0 in its environment) is the only way to reach gated_conv_kernel<bf16_t, C>.  The child runs the three C values
at 546 pixels against the same float64 reference under the project's bf16 bars and asserts the kernel log and the plumbing slot
(the name csrc/gscnn_select.h, compiled for the host, gives with the switch off)."""
import os
import sys

import numpy as np
import torch

GC_FEAT_LD, GC_OUT_PAD, GC_OUT_OFF = 64, 16, 8     # features: the first C channels of 64; output: a slice at element 8 of C + 16


def run_gated_conv(ops, c, inp):
    """-> (output as float64, kernel log counts); asserts that nothing outside the output slice was written."""
    import _shape_stream_cases as S
    from kdcc_amd import _lib
    C, dt = c["C"], S.DT[c["dt"]]
    shape = S.GC_NPIX[c["npix"]]
    buf = torch.full(shape + (GC_FEAT_LD,), 7.0, dtype=dt, device="cuda")
    buf[..., :C] = torch.from_numpy(inp["feat"]).to(dt).cuda()
    gate = torch.from_numpy(inp["gate"]).to(dt).cuda()
    ob = torch.full(shape + (C + GC_OUT_PAD,), 7.0, dtype=dt, device="cuda")
    out = ob[..., GC_OUT_OFF:GC_OUT_OFF + C]
    with _lib.kernel_log() as log:
        ops.gated_conv(buf, gate, torch.from_numpy(inp["params"]).cuda(), C, out=out)
    torch.cuda.synchronize()
    assert bool((ob[..., :GC_OUT_OFF] == 7.0).all()) and bool((ob[..., GC_OUT_OFF + C:] == 7.0).all()), f"{c['id']}: wrote outside the slice"
    return out.float().cpu().numpy().astype(np.float64), log.counts


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import kdcc_amd  # noqa: F401
    from kdcc_amd import ops
    import _shape_stream_cases as S
    from kdcc_amd import _lib
    from test_gscnn_select_host import load, select
    from test_ops_gpu import assert_close
    assert os.environ.get("KDCC_GATED_MFMA") == "0"
    sel_lib = load()
    for c in S.GC_VALU_BF16:
        inp, ref = S.build(c)
        got, counts = run_gated_conv(ops, c, inp)
        assert counts.get("gated_conv_kernel", 0) == 1 and "gated_conv_mfma_kernel" not in counts, counts
        slot = _lib.last_plumbing_kernel()
        assert slot == select(sel_lib, c, mfma=False)["name"] == S.slot_name(c, mfma=False), slot
        assert_close(got, ref["y"], "bf16", c["id"] + " (VALU)")
        print("ok", c["id"], counts)


if __name__ == "__main__":
    main()
