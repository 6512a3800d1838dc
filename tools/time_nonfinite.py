#!/usr/bin/env python3
"""ON THE GPU BOX: what the non-finite check costs.  For every kind and dtype, mdc_forward against mdc_forward_checked under
REPORT and PROPAGATE, interleaved in one process (one of each per round, HIP events around each call, median of the rounds):
2^20 frames per call for VT-CNN2, 2^24 for the deployed nets and cnn.py's net.  Clean frames (the check's cost does not
depend on what it finds).
usage: time_nonfinite.py [out.json = profiles/r06_nonfinite_cost.json] [rounds = 7]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from modulationdetectioncnn_amd import VTCNN2, Topology, _cabi, synthetic_frames  # noqa: E402

CASES = [("deployed3", "f32"), ("deployed3", "bf16"), ("deployed3", "f16"), ("deployed3", "fp8"),
         ("deployed10", "f32"), ("deployed10", "bf16"), ("deployed10", "f16"), ("deployed10", "fp8"),
         ("vtcnn2", "f32"), ("vtcnn2", "bf16"), ("vtcnn2", "fp8"), ("vtcnn2", "fp8_bf16"), ("cnnpy", "f32")]


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r06_nonfinite_cost.json")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    L = _cabi.lib()
    x_all = synthetic_frames(1 << 24, seed=2016, device="cuda:0")
    rows = []
    for topo, dtype in CASES:
        t = Topology.vtcnn2(11) if topo == "vtcnn2" else topo
        kw = {"dtype": "fp8", "fp8_bf16_features": True} if dtype == "fp8_bf16" else {"dtype": dtype}
        m = VTCNN2.synthetic(t, seed=2016, device=0, **kw)
        n = 1 << (20 if topo == "vtcnn2" else 24)
        x = x_all[:n]
        C = m.topology.classes
        probs = torch.empty((n, C), dtype=torch.float32, device="cuda:0")
        labels = torch.empty((n,), dtype=torch.int32, device="cuda:0")
        flags = torch.empty((n,), dtype=torch.uint8, device="cuda:0")
        count = torch.zeros((1,), dtype=torch.int64, device="cuda:0")
        ws, ws_bytes = m._workspace(n)
        h, s = m._engine(), torch.cuda.current_stream().cuda_stream
        wsp = ws.data_ptr() if ws is not None else None

        def plain():
            _cabi.check(L.mdc_forward(h, x.data_ptr(), n, probs.data_ptr(), labels.data_ptr(), None, 0, wsp, ws_bytes, s))

        def checked(policy):
            _cabi.check(L.mdc_forward_checked(h, x.data_ptr(), n, probs.data_ptr(), labels.data_ptr(), wsp, ws_bytes, flags.data_ptr(),
                                              count.data_ptr(), policy, s))

        calls = {"forward": plain, "report": lambda: checked(_cabi.NONFINITE_REPORT),
                 "propagate": lambda: checked(_cabi.NONFINITE_PROPAGATE)}
        for f in calls.values():      # warm
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for k, f in calls.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                times[k].append(a.elapsed_time(b))
        med = {k: float(np.median(v)) for k, v in times.items()}
        row = {"kind": topo, "dtype": dtype, "frames": n, "rounds": rounds,
               "ms_median": {k: round(v, 4) for k, v in med.items()},
               "report_vs_forward": round(med["report"] / med["forward"] - 1, 4),
               "propagate_vs_forward": round(med["propagate"] / med["forward"] - 1, 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del m, ws, probs, labels, flags
        torch.cuda.empty_cache()
    dev = torch.cuda.get_device_properties(0)
    with open(out, "w") as f:
        json.dump({"what": "mdc_forward vs mdc_forward_checked (REPORT, PROPAGATE): device time per call, median of interleaved rounds",
                   "device": dev.name, "rows": rows}, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
