"""A linear mean model on batched plans (clr_batch_set_mean_basis / _set_mean_weights / _grad_mean_weights): what it costs.

At the headline shape (B = 1024, N = 1e5, width 8 = 2 real + 3 complex; K = 3 basis functions shared by all problems):
  * the optimiser step with FRESH weights every step (upload of B x K doubles, the residual pass, the copy of y the route
    reads) against the step with a fresh constant mean and the plain step;
  * grad_mean_weights() after a materialising run: host wall time, and the device time of its two halves -- the batched
    solve (clr_batch_get_solve_ms) and the projection (clr_batch_get_mean_project_ms).
Host wall time per call (every call returns synchronised results), median of the timed calls.  Each measurement runs in
a child process of its own under `timeout`; the first one that fails ends the run.  Usage:
    python tools/gpu_linear_mean_timing.py [--steps K] [--commit ID] [--out profiles/linear_mean_timing.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

B, N, JR, JC, K = 1024, 100000, 2, 3, 3
SHAPE = "headline 1024 x 1e5 x width 8, K = 3 shared basis"


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def make_plan():
    from bench import make_inputs
    from celerite_amd import batch

    coeffs, t, diag, y = make_inputs(B, N, JR, JC, 42)
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    tt = t[0]
    Phi = np.stack([np.ones(N), tt - tt.mean(), np.sin(0.3 * tt)])
    return plan, coeffs, Phi


def step_times(steps):
    from celerite_amd import batch

    print("device: %s" % (batch.device_info(),), flush=True)
    rng = np.random.RandomState(5)
    plan, coeffs, Phi = make_plan()
    for _ in range(3):
        plan.evaluate(*coeffs)
    base = timed(lambda: plan.evaluate(*coeffs), steps)
    means = iter([rng.uniform(-0.1, 0.1, B) for _ in range(steps + 3)])
    for _ in range(3):
        plan.evaluate(*coeffs, mean=next(means))
    const = timed(lambda: plan.evaluate(*coeffs, mean=next(means)), steps)
    plan.set_mean(None)
    plan.set_mean_basis(Phi)
    weights = iter([rng.uniform(-0.1, 0.1, (B, K)) for _ in range(steps + 3)])
    for _ in range(3):
        plan.evaluate(*coeffs, mean_weights=next(weights))
    fresh = timed(lambda: plan.evaluate(*coeffs, mean_weights=next(weights)), steps)
    plan.close()
    print("%s: step with no mean %.3f ms; fresh constant mean every step %.3f ms (%.2fx); fresh weights every step %.3f ms (%.2fx)"
          % (SHAPE, base, const, const / base, fresh, fresh / base), flush=True)


def grad_times(calls):
    rng = np.random.RandomState(6)
    plan, coeffs, Phi = make_plan()
    plan.set_mean_basis(Phi)
    plan.set_mean_weights(rng.uniform(-0.1, 0.1, (B, K)))
    st = plan.log_likelihood(True)[3]
    assert (st == 0).all()
    for _ in range(2):
        plan.grad_mean_weights()
    wall, solve, project = [], [], []
    for _ in range(calls):
        plan.set_mean_weights(rng.uniform(-0.1, 0.1, (B, K)))      # (an optimiser's call: new weights, the same factor)
        t0 = time.perf_counter()
        dw, gst = plan.grad_mean_weights()
        wall.append((time.perf_counter() - t0) * 1e3)
        solve.append(plan.solve_device_ms())
        project.append(plan.mean_project_ms())
    assert (gst == 0).all() and np.isfinite(dw).all()
    plan.close()
    print("%s: grad_mean_weights() %.3f ms of host wall time; on the device the solve %.3f ms + the projection %.3f ms"
          % (SHAPE, np.median(wall), np.median(solve), np.median(project)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--grad-calls", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_mean_timing.txt"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measurement")
    ap.add_argument("--only", choices=["steps", "grad"], help="(a child's measurement)")
    args = ap.parse_args()
    if args.only == "steps":
        return step_times(args.steps)
    if args.only == "grad":
        return grad_times(args.grad_calls)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = ["# tools/gpu_linear_mean_timing.py (MI355X, one GPU): a linear mean model on batched plans.",
             "# Host wall time per call, median of %d steps / %d gradient calls; every call returns synchronised results."
             % (args.steps, args.grad_calls),
             "# Device times: HIP events around the kernels of the batched solve and of the projection.",
             "commit: %s" % commit]
    for only in ("steps", "grad"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--only", only,
               "--steps", str(args.steps), "--grad-calls", str(args.grad_calls)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:       # nothing more is started on the device after a failure
            sys.exit("measurement '%s' ended with status %d" % (only, r.returncode))
        lines += [l for l in r.stdout.splitlines() if l.startswith((SHAPE, "device:"))]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
