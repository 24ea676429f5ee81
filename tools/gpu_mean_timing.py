"""A constant mean per problem on batched plans (clr_batch_set_mean): what it costs.

At the headline shape (B = 1024, N = 1e5, width 8 = 2 real + 3 complex) and at BASELINE configs[4] (256 x 1e5 x width 32):
  * the optimiser step with a FRESH per-problem mean every step (clr_batch_evaluate_mean: upload of B doubles, the
    residual pass y - mu, the interleaved copy of y where the route reads one) against the plain step (clr_batch_evaluate);
  * the gradient with the mean's partial (clr_batch_grad_mean) against the gradient (clr_batch_grad).
Host wall time per call (every call returns synchronised results), median of the timed calls.  Usage:
    python tools/gpu_mean_timing.py [--steps K]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import make_inputs
from celerite_amd import batch


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--grad-calls", type=int, default=3)
    args = ap.parse_args()
    print("device:", batch.device_info(), flush=True)
    shapes = [("headline 1024 x 1e5 x width 8, per-problem series", 1024, 100000, 2, 3, False, False),
              ("headline 1024 x 1e5 x width 8, one shared y", 1024, 100000, 2, 3, False, True),
              ("configs[4] 256 x 1e5 x width 32", 256, 100000, 0, 16, True, False)]
    rng = np.random.RandomState(5)
    for name, B, N, JR, JC, spread, shared_y in shapes:
        coeffs, t, diag, y = make_inputs(B, N, JR, JC, 42, d_spread=spread)
        if shared_y:
            y = y[0]
        plan = batch.BatchedGP(B, N, JR, JC)
        plan.set_series(t, diag, y)
        plan.set_coefficients(*coeffs)
        for _ in range(3):
            plan.evaluate(*coeffs)
        base = timed(lambda: plan.evaluate(*coeffs), args.steps)
        means = [rng.uniform(-0.1, 0.1, B) for _ in range(args.steps + 3)]
        it = iter(means)
        for _ in range(3):
            plan.evaluate(*coeffs, mean=next(it))
        fresh = timed(lambda: plan.evaluate(*coeffs, mean=next(it)), args.steps)
        same = timed(lambda: plan.evaluate(*coeffs, mean=means[-1]), args.steps)
        print("%s: step %.3f ms; fresh per-problem mean every step %.3f ms (%.2fx); same mean every step %.3f ms"
              % (name, base, fresh, fresh / base, same), flush=True)
        if shared_y:
            plan.close()
            continue
        plan.set_mean(None)
        plan.grad_log_likelihood()
        g = timed(lambda: plan.grad_log_likelihood(), args.grad_calls)
        plan.set_mean(means[-1])
        plan.grad_log_likelihood(mean_partial=True)
        gm = timed(lambda: plan.grad_log_likelihood(mean_partial=True), args.grad_calls)
        print("%s: clr_batch_grad %.2f ms; clr_batch_grad_mean %.2f ms (%.2fx; the partial alone %.2f ms)"
              % (name, g, gm, gm / g, gm - g), flush=True)
        plan.close()


if __name__ == "__main__":
    main()
