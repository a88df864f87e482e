"""How deep the start-up records of the headline frame are, rule by rule, read back from the device:
python3 scripts/dev/prefix_depth_hist.py [out.json] [rules: rim,wide,deep]

For each rule a fresh DeviceFrame (1024 x 1024 x 5, the bench camera and parameters) records by that rule from its first trace
(BHGEO_RIM_PREFIX=1 / BHGEO_WIDE_PREFIX=1 / neither), replays twice, and the last plane of its records -- (ray, attempted,
accepted, rejected bit) -- is tabulated against the attempts the trace counted: kept, executed, the shares at the caps, and the
factor by which a replaying run's counted attempts overstate the executed ones."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from blackhole_geodesic_calculator_amd import _ffi  # noqa: E402
from blackhole_geodesic_calculator_amd.device_frame import DeviceFrame  # noqa: E402

RULES = {"rim": {"BHGEO_RIM_PREFIX": "1"}, "wide": {"BHGEO_RIM_PREFIX": "0", "BHGEO_WIDE_PREFIX": "1"},
         "deep": {"BHGEO_RIM_PREFIX": "0", "BHGEO_WIDE_PREFIX": "0"}}
CAPS = {"rim": (_ffi.PREFIX_RIM_ACCEPTED, _ffi.PREFIX_RIM_ATTEMPTS), "wide": (_ffi.PREFIX_WIDE_ACCEPTED, _ffi.PREFIX_DEEP_ATTEMPTS),
        "deep": (_ffi.PREFIX_DEEP_ACCEPTED, _ffi.PREFIX_DEEP_ATTEMPTS)}


def one(ctx, rule):
    for k in ("BHGEO_RIM_PREFIX", "BHGEO_WIDE_PREFIX"):
        os.environ.pop(k, None)
    os.environ.update(RULES[rule])
    fr = DeviceFrame(ctx, 1024, 1024, 5, fov_x=0.6, fov_y=0.6)
    p = _ffi.make_params(r_s=1.0, lambda_end=50.0)
    fr.generate_rays()
    ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fr.trace(p)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ss = fr.start_steps
    w = ss.d_rec[96 * fr.n:].view(torch.int32).view(fr.n, 4).cpu().numpy()
    att, acc, bit = w[:, 1].astype(np.int64), w[:, 2].astype(np.int64), w[:, 3]
    steps = fr.d_steps.cpu().numpy().astype(np.int64)
    acc_max, att_max = CAPS[rule]
    out = {"n": int(fr.n), "rule": rule, "rho": float(ss.rho), "prefix_recorded": int(ss.prefix_recorded),
           "prefix_replayed": int(ss.prefix_replayed), "attempted_hist": np.bincount(att, minlength=att_max + 1).tolist(),
           "accepted_hist": np.bincount(acc, minlength=acc_max + 1).tolist(), "share_with_rejection": float((att > acc).mean()),
           "share_rejected_bit": float((bit != 0).mean()), "share_at_accepted_cap": float((acc >= acc_max).mean()),
           "share_at_attempt_cap": float((att >= att_max).mean()), "attempted_per_ray": float(steps.mean()),
           "kept_per_ray": float(att.mean()), "executed_per_ray": float((steps - att).mean()),
           "attempted_over_executed": float(steps.sum() / (steps - att).sum()), "recording_call_ms": ms[0], "replaying_call_ms": ms[1:]}
    print(rule, "rho %.6f" % out["rho"], "kept %.3f of %.3f, executed %.3f, attempted/executed %.3f, at a cap %.3f %% / %.3f %%" %
          (out["kept_per_ray"], out["attempted_per_ray"], out["executed_per_ray"], out["attempted_over_executed"],
           100 * out["share_at_accepted_cap"], 100 * out["share_at_attempt_cap"]), "ms", ["%.3f" % m for m in ms])
    return out


def main():
    rules = (sys.argv[2] if len(sys.argv) > 2 else "rim,wide,deep").split(",")
    ctx = _ffi.Context(0)
    res = {"frame": [one(ctx, r) for r in rules]}
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
