"""The generalised-least-squares fit of a linear mean's weights on batched plans (clr_batch_fit_mean_weights): what it
costs, against the route the library offered before it for the same numbers.

At the headline shape (B = 1024, N = 1e5, width 8 = 2 real + 3 complex) and at BASELINE configs[1]'s (B = 256, N = 1e4,
width 4 = 2 complex), K = 3 basis functions shared by all problems, after a materialising run, in ONE process per shape:
  * fit_mean_weights(): host wall time, and the device time of its three parts (clr_batch_get_mean_fit_ms) -- the
    batched solves of the K + 1 right-hand sides formed on the device, the bordered Gram pass, the small solve;
  * the host route: solve(b = Phi) -- B x K x N doubles up and as many down -- plus solve() of the residual, the Gram
    matrix and the K x K solves in NumPy.
Both routes start from fresh weights every call (an optimiser's or sampler's call: the same factor).  Host wall time per
call, median of the timed calls; each shape runs in a child process of its own under `timeout`, and the first one that
fails ends the run.  Usage:
    python tools/gpu_linear_mean_fit_timing.py [--calls K] [--commit ID] [--out profiles/linear_mean_fit_timing.txt]
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

K = 3
SHAPES = {"headline": (1024, 100000, 2, 3, "headline 1024 x 1e5 x width 8, K = 3 shared basis"),
          "configs1": (256, 10000, 0, 2, "configs[1] 256 x 1e4 x width 4, K = 3 shared basis")}


def measure(name, calls):
    from bench import make_inputs
    from celerite_amd import batch

    B, N, JR, JC, label = SHAPES[name]
    print("device: %s" % (batch.device_info(),), flush=True)
    rng = np.random.RandomState(6)
    coeffs, t, diag, y = make_inputs(B, N, JR, JC, 42)
    u = (t[0] - t[0].min()) / (t[0].max() - t[0].min())
    Phi = np.stack([np.ones(N), 2.0 * u - 1.0, np.sin(6.0 * np.pi * u)])
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    plan.set_mean_basis(Phi)
    plan.set_mean_weights(rng.uniform(-0.1, 0.1, (B, K)))
    assert (plan.log_likelihood(True)[3] == 0).all()

    def host_route():
        """What the library offered before: the basis goes up as B x K right-hand sides, the solutions come down."""
        w0 = plan._mean_w
        Z = plan.solve(np.broadcast_to(Phi, (B, K, N)))              # K^-1 Phi_k
        z = plan.solve()                                             # K^-1 r
        G = np.einsum("jn,bkn->bjk", Phi, Z)
        d = np.einsum("jn,bn->bj", Phi, z)
        G = 0.5 * (G + G.transpose(0, 2, 1))
        return w0 + np.linalg.solve(G, d[:, :, None])[:, :, 0], np.linalg.inv(G)

    plan.fit_mean_weights()
    wall, parts = [], []
    for _ in range(calls):
        plan.set_mean_weights(rng.uniform(-0.1, 0.1, (B, K)))
        t0 = time.perf_counter()
        fit = plan.fit_mean_weights()
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(plan.mean_fit_ms())
    assert (fit.status == 0).all()
    w_host, cov_host = host_route()
    dev = float(np.max(np.abs(fit.weights - w_host) / (1 + np.abs(w_host))))
    host = []
    for _ in range(max(1, calls // 2)):
        plan.set_mean_weights(rng.uniform(-0.1, 0.1, (B, K)))
        t0 = time.perf_counter()
        host_route()
        host.append((time.perf_counter() - t0) * 1e3)
    plan.close()
    solve, gram, small = np.median(np.array(parts), axis=0)
    new, old = float(np.median(wall)), float(np.median(host))
    print("%s: fit_mean_weights() %.3f ms of host wall time; on the device the solves %.3f ms + the Gram pass %.3f ms + the small "
          "solve %.3f ms" % (label, new, solve, gram, small), flush=True)
    print("%s: the host route (solve(b = Phi) + solve() + NumPy Gram and solve) %.1f ms of host wall time: %.1fx the new call; "
          "the two routes' weights agree to %.1e (1 + |w|)" % (label, old, old / new, dev), flush=True)
    if not new <= old:
        sys.exit("fit_mean_weights() is slower than the host route at " + label)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_mean_fit_timing.txt"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per shape")
    ap.add_argument("--only", choices=sorted(SHAPES), help="(a child's measurement)")
    args = ap.parse_args()
    if args.only:
        return measure(args.only, args.calls)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = ["# tools/gpu_linear_mean_fit_timing.py (MI355X, one GPU): the GLS fit of a linear mean's weights on batched plans.",
             "# Host wall time per call, median of %d calls (the host route: %d); every call returns synchronised results."
             % (args.calls, max(1, args.calls // 2)),
             "# Device times: HIP events around the kernels of the three parts (clr_batch_get_mean_fit_ms).",
             "commit: %s" % commit]
    for only in ("configs1", "headline"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--only", only,
               "--calls", str(args.calls)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:       # nothing more is started on the device after a failure
            sys.exit("measurement '%s' ended with status %d" % (only, r.returncode))
        lines += [l for l in r.stdout.splitlines() if l.startswith((SHAPES[only][4], "device:")) and l not in lines]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
