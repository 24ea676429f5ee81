"""Batched plans driven from `terms` kernel parameters (clr_batch_evaluate_params / _grad_params): what a step costs.

At the headline shape (B = 1024, N = 1e5, width 8: the bench kernel, 2 real + 3 complex terms) and at BASELINE
configs[1] (256 x 1e4 x width 4), median host wall time per step (every call returns synchronised results) of
  (a) evaluate with precomputed coefficient arrays -- the floor;
  (b) kernel_coefficient_table(compiled=False) + evaluate -- the Python loop over the draws, the only bridge from a
      `terms` kernel before the compiled program;
  (c) evaluate_parameters -- parameters in, the coefficients formed on the device;
and the same three for the gradient chained to the parameters: (a) evaluate + grad_log_likelihood + chain_gradient with
a precomputed Jacobian table, (b) the same with both Python tables built every step, (c) evaluate_parameters +
grad_parameters.  The three are timed alternately, `--repeats` rounds of `--steps` calls each; (a) and (c) swap places
from round to round and every timed window follows three untimed calls of its own kind, because the device idles
through the Python loop of (b) and the first steps after it run slower whatever they are.  The spread of (a) over the
rounds (max - min of the rounds' medians) is the noise (c) is held against.
Usage:
    python tools/gpu_kernel_params_timing.py [--steps K] [--repeats R]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from bench import make_inputs
from celerite_amd import batch, terms


def timed(fn, n):
    for _ in range(3):
        fn()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def kernel_of(JR, JC):
    k = None
    for _ in range(JR):
        t = terms.RealTerm(1.0, 0.1)
        k = t if k is None else k + t
    for _ in range(JC):
        t = terms.ComplexTerm(0.1, 2.0, 1.6)
        k = t if k is None else k + t
    return k


def report(name, rounds):
    a, b, c = (np.array(rounds[k]) for k in "abc")
    spread = float(a.max() - a.min())
    print("%s: (a) %.3f ms [rounds %.3f..%.3f, spread %.3f]  (b) %.3f ms  (c) %.3f ms  (c) - (a) = %+.3f ms (%s the spread of (a))"
          % (name, np.median(a), a.min(), a.max(), spread, np.median(b), np.median(c), np.median(c) - np.median(a),
             "within" if np.median(c) - np.median(a) <= spread else "beyond"), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=6)
    ap.add_argument("--grad-calls", type=int, default=3)
    args = ap.parse_args()
    print("device:", batch.device_info(), flush=True)
    shapes = [("headline 1024 x 1e5 x width 8", 1024, 100000, 2, 3, 42),
              ("configs[1] 256 x 1e4 x width 4", 256, 10000, 0, 2, 7)]
    for name, B, N, JR, JC, seed in shapes:
        coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed)
        kernel = kernel_of(JR, JC)
        # the bench draws as parameter vectors: log of the coefficient tables, in get_parameter_vector() order
        cols = [np.log(coeffs[0][:, j:j + 1]) if i == 0 else np.log(coeffs[1][:, j:j + 1]) for j in range(JR) for i in (0, 1)]
        for j in range(JC):
            cols += [np.log(coeffs[2][:, j:j + 1]), np.log(coeffs[4][:, j:j + 1]), np.log(coeffs[5][:, j:j + 1])]
        params = np.ascontiguousarray(np.concatenate(cols, axis=1))
        plan = batch.BatchedGP(B, N, JR, JC)
        plan.set_series(t, diag, y)
        plan.set_kernel(kernel)
        tab = batch.kernel_coefficient_table(kernel, params)
        step = {"a": lambda: plan.evaluate(*tab[:6], jitter=tab[6]),
                "b": lambda: plan.evaluate(*batch.kernel_coefficient_table(kernel, params)[:6]),
                "c": lambda: plan.evaluate_parameters(params)}
        for fn in step.values():
            for _ in range(3):
                fn()
        rounds = {k: [] for k in step}
        for r in range(args.repeats):
            for k in ("bac", "bca")[r % 2]:
                rounds[k].append(timed(step[k], args.steps))
        report(name + ", step", rounds)
        jac = batch.kernel_coefficient_jacobian_table(kernel, params)

        def grad_b():
            plan.evaluate(*batch.kernel_coefficient_table(kernel, params)[:6])
            v, g, st = plan.grad_log_likelihood()
            return batch.chain_gradient(g, *batch.kernel_coefficient_jacobian_table(kernel, params))

        def grad_a():
            plan.evaluate(*tab[:6], jitter=tab[6])
            v, g, st = plan.grad_log_likelihood()
            return batch.chain_gradient(g, *jac)

        def grad_c():
            plan.evaluate_parameters(params)
            return plan.grad_parameters()

        gstep = {"a": grad_a, "b": grad_b, "c": grad_c}
        for fn in gstep.values():
            fn()
        rounds = {k: [] for k in gstep}
        for r in range(args.repeats):
            for k in ("bac", "bca")[r % 2]:
                rounds[k].append(timed(gstep[k], args.grad_calls))
        report(name + ", step + gradient chained to the parameters ((a): precomputed tables and Jacobian)", rounds)
        plan.close()


if __name__ == "__main__":
    main()
