"""The start-up records' rule restated on scipy's RK45, without a GPU:
how many of a headline ray's step attempts a record keeps, by the radius of its ball and by its caps.

python3 scripts/dev/prefix_rule_restate.py [rays] [seed]

The rule (record_prefix_kernel<RHS, true>): rejected attempts are kept; the record stops in front of an accepted attempt that ends
outside the ball of radius rho about the camera (rejections in front of it are kept), in front of the attempt that ends the ray,
after acc_max accepted steps and after att_max attempts.  scipy's RK45 object is stepped by hand: each attempt costs six
evaluations of the right-hand side, so the attempts behind an accepted step are the growth of nfev over six."""
import json
import os
import sys

import numpy as np
from scipy.integrate import RK45

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from oracle.scipy_reference import make_rhs  # noqa: E402

CAM = np.array([1e-4, 0.0, 30.0])
R_S, LAMBDA_END, RTOL, ATOL, FOV = 1.0, 50.0, 1e-3, 1e-6, 0.6
FRACTIONS = [("1/4", 0.25), ("3/4", 0.75), ("15/16", 15 / 16), ("31/32", 31 / 32), ("63/64", 63 / 64), ("127/128", 127 / 128),
             ("1-2^-10", 1 - 2.0 ** -10)]
CAPS = [(6, 12), (8, 12), (8, 16), (10, 16), (12, 16), (12, 20), (16, 24)]


def ray_steps(k0):
    """[(attempts of this accepted step, distance of its end from the camera, ends the ray)] of one ray's whole solve."""
    y0 = np.array([k0[0], CAM[0], k0[1], CAM[1], k0[2], CAM[2]])
    s = RK45(make_rhs(R_S, "christoffel"), 0.0, y0, LAMBDA_END, rtol=RTOL, atol=ATOL)
    out, nfev = [], s.nfev
    while s.status == "running":
        s.step()
        if s.status == "failed":
            break
        x = np.array([s.y[1], s.y[3], s.y[5]])
        ends = s.status == "finished" or np.linalg.norm(x) <= R_S
        out.append(((s.nfev - nfev) // 6, float(np.linalg.norm(x - CAM)), ends))
        nfev = s.nfev
        if ends:
            break
    return out


def kept(steps, rho, acc_max, att_max):
    """(attempts kept, accepted steps kept) of a record by the rule."""
    att = acc = 0
    for tries, dist, ends in steps:
        if acc >= acc_max:
            break
        rejected = tries - 1
        if att + rejected >= att_max:          # the attempt cap falls among this step's rejections (or right behind them)
            return att_max, acc
        att += rejected
        if ends or dist > rho:
            break
        att, acc = att + 1, acc + 1
    return att, acc


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 11
    rng = np.random.default_rng(seed)
    k = np.stack([rng.uniform(-FOV / 2, FOV / 2, n), rng.uniform(-FOV / 2, FOV / 2, n), -np.ones(n)], 1)
    k /= np.linalg.norm(k, axis=1)[:, None]
    rays = [ray_steps(ki) for ki in k]
    total = float(np.mean([sum(t for t, _, _ in r) for r in rays]))
    ball = min(np.linalg.norm(CAM) - R_S, np.linalg.norm(CAM))
    table = {"rays": n, "seed": seed, "attempts_per_ray": total, "rows": []}
    print(f"{n} uniform rays of the headline window, {total:.2f} attempts per ray")
    print("fraction      rho     reaches r   " + "   ".join(f"<={a:2d}acc/<={t:2d}att" for a, t in CAPS))
    for name, frac in FRACTIONS:
        rho = frac * ball
        cells = []
        for acc_max, att_max in CAPS:
            ka = np.array([kept(r, rho, acc_max, att_max) for r in rays])
            at_cap = float(np.mean((ka[:, 0] >= att_max) | (ka[:, 1] >= acc_max)))
            cells.append({"acc_max": acc_max, "att_max": att_max, "kept_per_ray": float(ka[:, 0].mean()), "share_at_a_cap": at_cap,
                          "max_attempts": int(ka[:, 0].max()), "max_accepted": int(ka[:, 1].max())})
        table["rows"].append({"fraction": name, "rho": rho, "cells": cells})
        print(f"{name:9s} {rho:9.5f}  {np.linalg.norm(CAM) - rho:7.4f}    " +
              "   ".join(f"{c['kept_per_ray']:5.2f} ({100 * c['share_at_a_cap']:4.1f} %)" for c in cells))
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
