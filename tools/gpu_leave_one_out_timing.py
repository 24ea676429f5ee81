"""diag(K^-1) and the leave-one-out predictive distribution on batched plans (clr_batch_leave_one_out): what they cost.

At the headline shape (1024 x 1e5 x width 8, lean factor), at BASELINE configs[1] (256 x 1e4 x width 4) and at configs[4]
(256 x 1e5 x width 32):
  * ``inverse_diagonal()`` -- kinv_diag only -- and ``leave_one_out()`` -- everything: host wall time (median) and the device
    time of the three parts (``clr_batch_get_leave_one_out_ms``: the diagonal, the solve, the reduction), beside
    ``plan.solve()`` of the same plan (wall, and ``solve_device_ms``);
  * ``leave_one_out(arrays=False)``: the step of a leave-one-out cross-validation comparison (logpdf and status down only).
At configs[1] only, also the one route to the same numbers without it: ``predict(t_b, return_var=True)`` at the plan's own N
points per problem, converted with ``c = (s - var) / s^2``, ``s = diag + jitter`` -- O(N^2 J) per problem.
Writes profiles/leave_one_out_timing.txt.  Usage:
    python tools/gpu_leave_one_out_timing.py [--reps K] [--skip-headline] [--skip-wide]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from bench import make_inputs
from celerite_amd import batch

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def make_plan(B, N, JR, JC, seed, lean, d_spread=False):
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed, d_spread=d_spread)
    plan = batch.BatchedGP(B, N, JR, JC)
    if lean:
        plan.set_factor_layout("lean")
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    assert (plan.log_likelihood(materialize=True)[3] == 0).all()
    return plan, t, diag


def timed(fn, reps):
    """Median wall time in ms of ``fn`` and what it last returned; ``fn`` returns the device parts it wants recorded."""
    walls, parts = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        p = fn()
        walls.append((time.perf_counter() - t0) * 1e3)
        parts.append(p)
    return float(np.median(walls)), np.median(np.array(parts, dtype=float), axis=0)


def shape(label, B, N, JR, JC, seed, lean, reps, d_spread=False, old_route=False):
    plan, t, diag = make_plan(B, N, JR, JC, seed, lean, d_spread)
    try:
        say("%s: B = %d, N = %d, width %d (%d real + %d complex), %s factor, chunks %s"
            % (label, B, N, JR + 2 * JC, JR, JC, "lean" if lean else "reference", plan.chunks))
        c = plan.inverse_diagonal()          # (warm-up: buffers, the chunk maps)
        plan.solve()
        loo = plan.leave_one_out()
        say("  diag_n c_n in [%.3g, %.3g]; logpdf per sample %.4f" % (np.min(diag * c), np.max(diag * c), np.mean(loo.logpdf) / N))
        wall, dev = timed(lambda: (plan.solve(), plan.solve_device_ms())[1:], reps)
        say("  solve():                       wall %9.2f ms, device %8.3f ms" % (wall, dev[0]))
        solve_dev = dev[0]
        wall, dev = timed(lambda: (plan.inverse_diagonal(), plan.leave_one_out_ms())[1], reps)
        say("  inverse_diagonal():            wall %9.2f ms, device %8.3f ms (the diagonal) = %.2f x solve()'s device time"
            % (wall, dev[0], dev[0] / solve_dev))
        wall, dev = timed(lambda: (plan.leave_one_out(), plan.leave_one_out_ms())[1], reps)
        say("  leave_one_out():               wall %9.2f ms, device %8.3f ms = diagonal %.3f + solve %.3f + reduction %.3f"
            % (wall, dev.sum(), dev[0], dev[1], dev[2]))
        wall, dev = timed(lambda: (plan.leave_one_out(arrays=False), plan.leave_one_out_ms())[1], reps)
        say("  leave_one_out(arrays=False):   wall %9.2f ms, device %8.3f ms" % (wall, dev.sum()))
        if old_route:
            t0 = time.perf_counter()
            var = plan.predict(t, return_var=True)[1]
            wall = (time.perf_counter() - t0) * 1e3
            s = diag      # (jitter 0)
            c_old = (s - var) / (s * s)
            say("  predict(t_b, return_var=True): wall %9.2f ms (N points per problem, O(N^2 J)); c = (s - var) / s^2 against "
                "inverse_diagonal(): max |dc| / max c = %.2e" % (wall, np.max(np.abs(c_old - c) / np.max(c, axis=1, keepdims=True))))
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-headline", action="store_true")
    ap.add_argument("--skip-wide", action="store_true")
    args = ap.parse_args()
    say("# diag(K^-1) and leave-one-out on batched plans: tools/gpu_leave_one_out_timing.py --reps %d" % args.reps)
    say("# Wall: host time of the call, downloads included (median).  Device: HIP events around the kernels of each part.")
    say("device: %s" % (batch.device_info(),))
    shape("configs[1]", 256, 10000, 0, 2, 7, True, args.reps, old_route=True)
    if not args.skip_headline:
        shape("headline", 1024, 100000, 2, 3, 42, True, args.reps)
    if not args.skip_wide:
        shape("configs[4]", 256, 100000, 0, 16, 11, False, args.reps, d_spread=True)
    out = os.path.join(ROOT, "profiles", "leave_one_out_timing.txt")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
