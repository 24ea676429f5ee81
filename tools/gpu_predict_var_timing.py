"""The conditional variance on batched plans (clr_batch_predict_var): what it costs against the host route.

At B = 64, N = 20000, M = 256, width 8 (2 real + 3 complex), lean layout:
  * new: ``plan.predict(xs, return_var=True)`` less ``plan.predict(xs)`` is not separable in one call, so the variance
    alone is timed through the C entry (``clr_batch_predict_var``): only xs goes up, only var comes down;
  * old: the only route without it -- the (B, M, N) cross-covariances built on the host in NumPy, ``plan.solve(b)``
    (upload, both sweeps, download) and the host reduction ``k(0) - sum b o x``.
Both warmed up, 10 repetitions each, alternating; wall time (median) and the device time of ``solve_device_ms``.
Then the headline shape 1024 x 1e5 x width 8 at M = 64 on the new route only: automatic tile and a tile of 4 points.
Per (problem, point): device time, and the HBM bytes it implies at 5.3 TB/s against the factor's size.  Usage:
    python tools/gpu_predict_var_timing.py [--reps K] [--skip-headline]
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import make_inputs
from celerite_amd import batch

HBM_BYTES_PER_S = 5.3e12  # achievable copy bandwidth of an MI355X (8 TB/s peak)


def kernel_value(coeffs, tau):
    """k_p(tau) for tau (B, M, N), a term at a time: no temporary larger than the result."""
    ar, cr, ac, bc, cc, dc = (np.asarray(c) for c in coeffs)
    tau = np.abs(tau)
    k = np.zeros_like(tau)
    for j in range(ar.shape[1]):
        k += ar[:, j, None, None] * np.exp(-cr[:, j, None, None] * tau)
    for j in range(ac.shape[1]):
        ph = dc[:, j, None, None] * tau
        k += np.exp(-cc[:, j, None, None] * tau) * (ac[:, j, None, None] * np.cos(ph) + bc[:, j, None, None] * np.sin(ph))
    return k


def predict_var(plan, xs):
    lib = batch._load()
    lib.clr_batch_predict_var.argtypes = [C.c_void_p, C.c_int, batch._dp, C.c_long, batch._dp]
    var = np.empty((plan.B, xs.shape[-1]))
    batch._check(lib.clr_batch_predict_var(plan._h, xs.shape[-1], batch._ptr(xs), 0 if xs.ndim == 1 else xs.shape[1], batch._ptr(var)))
    return var


def host_route(plan, coeffs, t, xs):
    b = kernel_value(coeffs, xs[None, :, None] - t[:, None, :])  # (B, M, N)
    x = plan.solve(b)
    k0 = np.sum(coeffs[0], axis=1) + np.sum(coeffs[2], axis=1)
    return k0[:, None] - np.sum(b * x, axis=2)


def report(name, plan, B, N, M, wall_ms, dev_ms):
    per = dev_ms * 1e-3 / (B * M)
    factor = plan.factor_bytes()
    print("%s: wall %.2f ms, device %.3f ms; per (problem, point) %.3f us = %.2f MB of HBM traffic at %.1f TB/s against a "
          "factor of %.2f MB per problem (%.2fx)" % (name, wall_ms, dev_ms, per * 1e6, per * HBM_BYTES_PER_S / 1e6,
                                                     HBM_BYTES_PER_S / 1e12, factor / 1e6, per * HBM_BYTES_PER_S / factor), flush=True)


def make_plan(B, N, JR, JC):
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, 42)
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_factor_layout("lean")
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    assert (plan.log_likelihood(materialize=True)[3] == 0).all()
    return plan, coeffs[:6], t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-headline", action="store_true")
    args = ap.parse_args()
    print("device:", batch.device_info(), flush=True)
    B, N, M, JR, JC = 64, 20000, 256, 2, 3
    plan, coeffs, t = make_plan(B, N, JR, JC)
    xs = np.sort(np.random.RandomState(1).uniform(t.min(), t.max(), M))
    new, old = predict_var(plan, xs), host_route(plan, coeffs, t, xs)   # (warm-up of both)
    k0 = np.sum(coeffs[0], axis=1) + np.sum(coeffs[2], axis=1)
    print("B = %d, N = %d, M = %d, width %d, lean: new vs host route max |dvar| / k(0) = %.2e"
          % (B, N, M, JR + 2 * JC, np.max(np.abs(new - old) / k0[:, None])), flush=True)
    walls, devs = {"new": [], "old": []}, {"new": [], "old": []}
    for _ in range(args.reps):
        for key, fn in (("new", lambda: predict_var(plan, xs)), ("old", lambda: host_route(plan, coeffs, t, xs))):
            t0 = time.perf_counter()
            fn()
            walls[key].append((time.perf_counter() - t0) * 1e3)
            devs[key].append(plan.solve_device_ms())
            print("  repetition %d, %s route: wall %.2f ms, device %.3f ms" % (len(walls[key]), key, walls[key][-1], devs[key][-1]), flush=True)
    report("new route (clr_batch_predict_var)", plan, B, N, M, np.median(walls["new"]), np.median(devs["new"]))
    report("old route (host cross-covariances + solve + host reduction)", plan, B, N, M, np.median(walls["old"]), np.median(devs["old"]))
    print("new / old: wall %.3fx, device %.3fx" % (np.median(walls["new"]) / np.median(walls["old"]),
                                                   np.median(devs["new"]) / np.median(devs["old"])), flush=True)
    plan.close()
    if args.skip_headline:
        return
    B, N, M = 1024, 100000, 64
    plan, coeffs, t = make_plan(B, N, JR, JC)
    xs = np.sort(np.random.RandomState(2).uniform(t.min(), t.max(), M))
    for tile in (0, 4):
        plan.set_predict_tile(tile)
        predict_var(plan, xs[:8])
        t0 = time.perf_counter()
        predict_var(plan, xs)
        wall = (time.perf_counter() - t0) * 1e3
        report("headline 1024 x 1e5 x width 8, M = 64, tile %s" % (tile or "automatic"), plan, B, N, M, wall, plan.solve_device_ms())
    plan.close()


if __name__ == "__main__":
    main()
