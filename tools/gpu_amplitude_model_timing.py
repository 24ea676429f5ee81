"""The per-sample amplitude model on batched plans (clr_batch_set_amplitude_basis / _set_amplitudes / _grad_amplitudes): what
it costs, at the headline shape (B = 1024, N = 1e5, width 8 = 2 real + 3 complex) and at B = 256, N = 1e4, width 4 (2 real
+ 1 complex), K = 3 bands.

  (a) no regression: the step of a plan WITHOUT an amplitude basis, this build against another build of the library
      (--parent-lib: the parent commit's libcelerite_hip.so), alternately, --processes fresh processes each; both through
      the same C ABI calls, so that one script drives both.  DEVICE time per evaluation (clr_batch_run_timed over --steps
      evaluations, after --warmup evaluations).  Reported: each process' figure, the spread of the parent's over its
      processes, and whether this build's median lies inside it.
  (b) the step with FRESH amplitudes every step, Gamma shared and per problem, against the plain step and against the
      route without the amplitude model: y / s and diag / s^2 formed on the host and sent through clr_batch_set_series
      every step (formed before the clock starts: the upload and what set_series rebuilds are what is timed).
  (c) grad_amplitudes() after a materialising run: host wall time and the device time of its three parts (the diagonal's
      recurrence and the solve: clr_batch_get_leave_one_out_ms; the projection: clr_batch_get_amplitude_project_ms).
(b), (c): host wall time per call (every call returns synchronised results), median of the timed calls.  Each measurement
runs in a child process of its own under `timeout`; the first one that fails ends the run.  Usage:
    python tools/gpu_amplitude_model_timing.py [--parent-lib PATH] [--parts abc] [--out profiles/amplitude_model_timing.txt]
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

K = 3
SHAPES = {"headline": (1024, 100000, 2, 3), "small": (256, 10000, 2, 1)}
NAMES = {"headline": "headline 1024 x 1e5 x width 8", "small": "256 x 1e4 x width 4"}


def timed(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return np.array(out)


def inputs(shape):
    from bench import make_inputs

    B, N, JR, JC = SHAPES[shape]
    return (B, N, JR, JC) + make_inputs(B, N, JR, JC, 42)


def band_basis(B, N, per, rng):
    """The indicators of K bands, the samples assigned at random: (B, K, N) or (K, N)."""
    band = rng.randint(0, K, (B, N) if per else (N,))
    return np.ascontiguousarray((band[..., None, :] == np.arange(K)[:, None]).astype(np.float64))


def amplitudes(B, rng):
    """One sign per problem, magnitudes in [0.5, 2]."""
    return 0.5 * 4.0 ** rng.rand(B, K) * np.where(rng.rand(B, 1) < 0.5, -1.0, 1.0)


def plain_step(lib_path, shape, steps, warmup):
    """(a): the plain step through the C ABI of the library at lib_path (no entry the parent lacks is touched)."""
    B, N, JR, JC, coeffs, t, diag, y = inputs(shape)
    lib = C.CDLL(lib_path)
    dp = C.POINTER(C.c_double)
    lib.clr_batch_create.restype = C.c_void_p
    lib.clr_batch_create.argtypes = [C.c_int] * 5
    lib.clr_batch_destroy.argtypes = [C.c_void_p]
    lib.clr_batch_set_series.argtypes = [C.c_void_p, dp, C.c_long, dp, C.c_long, dp, C.c_long]
    lib.clr_batch_evaluate.argtypes = [C.c_void_p] * 12
    lib.clr_batch_run_timed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, dp, dp]
    h = C.c_void_p(lib.clr_batch_create(B, N, JR, JC, 0))
    assert h.value, "clr_batch_create failed"
    ptr = lambda a: a.ctypes.data_as(dp)
    assert lib.clr_batch_set_series(h, ptr(t), N, ptr(diag), N, ptr(y), N) == 0
    jit = np.zeros(B)
    out = [np.empty(B), np.empty(B), np.empty(B), np.empty(B, dtype=np.int32)]
    args = [jit.ctypes.data] + [a.ctypes.data for a in coeffs] + [a.ctypes.data for a in out]

    def step():
        assert lib.clr_batch_evaluate(h, *args) == 0

    for _ in range(warmup):
        step()
    assert (out[3] == 0).all()
    tot, parts = C.c_double(), (C.c_double * 6)()
    assert lib.clr_batch_run_timed(h, 0, steps, 0, C.byref(tot), parts) == 0
    lib.clr_batch_destroy(h)
    print("PLAIN %s %s median %.4f ms of device time per evaluation over %d steps" % (shape, os.path.abspath(lib_path),
                                                                                     tot.value / steps, steps), flush=True)


def step_times(shape, steps):
    from celerite_amd import batch

    B, N, JR, JC, coeffs, t, diag, y = inputs(shape)
    rng = np.random.RandomState(5)
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    med = lambda fn: float(np.median(timed(fn, steps)))
    for _ in range(3):
        plan.evaluate(*coeffs)
    base = med(lambda: plan.evaluate(*coeffs))
    # the route without the amplitude model: y / s and diag / s^2 through set_series every step (formed before the clock
    # starts)
    G = band_basis(B, N, True, rng)
    series = []
    for i in range(3):
        s = np.einsum("bk,bkn->bn", amplitudes(B, rng), G)
        series.append((y / s, diag / (s * s)))
    it = iter(range(10 ** 6))

    def series_step():
        yp, dp = series[next(it) % 3]
        plan.set_series(t, dp, yp)
        plan.evaluate(*coeffs)

    series_step()
    route = med(series_step)
    plan.set_series(t, diag, y)
    fresh = {}
    for per in (False, True):
        plan.set_amplitude_basis(G if per else G[0])
        amps = iter([amplitudes(B, rng) for _ in range(steps + 3)])

        def amp_step():
            plan.set_amplitudes(next(amps))
            plan.evaluate(*coeffs)

        for _ in range(3):
            amp_step()
        fresh[per] = med(amp_step)
        assert (plan.results()[3] == 0).all()
        plan.set_amplitude_basis(None)
    plan.close()
    print("STEPS %s: plain step %.3f ms; fresh amplitudes every step, Gamma shared %.3f ms (%.2fx), Gamma per problem %.3f ms "
          "(%.2fx); host-formed y / s and diag / s^2 through set_series every step %.3f ms (%.2fx; %.1fx the shared-Gamma step)"
          % (NAMES[shape], base, fresh[False], fresh[False] / base, fresh[True], fresh[True] / base, route, route / base,
             route / fresh[False]), flush=True)


def grad_times(shape, calls):
    from celerite_amd import batch

    B, N, JR, JC, coeffs, t, diag, y = inputs(shape)
    rng = np.random.RandomState(6)
    plan = batch.BatchedGP(B, N, JR, JC)
    plan.set_series(t, diag, y)
    plan.set_coefficients(*coeffs)
    plan.set_amplitude_basis(band_basis(B, N, False, rng))
    plan.set_amplitudes(amplitudes(B, rng))
    assert (plan.log_likelihood(True)[3] == 0).all()
    plan.grad_amplitudes()
    wall, parts = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        da, st = plan.grad_amplitudes()
        wall.append((time.perf_counter() - t0) * 1e3)
        parts.append(plan.leave_one_out_ms()[:2] + (plan.amplitude_project_ms(),))
    assert (st == 0).all() and np.isfinite(da).all()
    plan.close()
    d, s, p = np.median(np.array(parts), axis=0)
    print("GRAD %s: grad_amplitudes() %.3f ms of host wall time; on the device the diagonal %.3f ms + the solve %.3f ms + "
          "the projection %.3f ms" % (NAMES[shape], np.median(wall), d, s, p), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--grad-calls", type=int, default=5)
    ap.add_argument("--processes", type=int, default=5, help="fresh processes per build and shape in part (a)")
    ap.add_argument("--parent-lib", default="", help="the parent commit's libcelerite_hip.so (part (a) compares against it)")
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amplitude_model_timing.txt"))
    ap.add_argument("--timeout", type=int, default=300, help="seconds per measurement")
    ap.add_argument("--only", choices=["plain", "steps", "grad"], help="(a child's measurement)")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="headline")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.only == "plain":
        return plain_step(args.lib, args.shape, args.steps, args.warmup)
    if args.only == "steps":
        return step_times(args.shape, args.steps)
    if args.only == "grad":
        return grad_times(args.shape, args.grad_calls)
    from celerite_amd import batch

    commit = args.commit
    if not commit:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    lines = ["# tools/gpu_amplitude_model_timing.py (MI355X, one GPU): the per-sample amplitude model on batched plans.",
             "# (a): device time per evaluation (clr_batch_run_timed over %d evaluations after %d warm-up evaluations), fresh processes"
             " alternately, the parent commit's library first." % (args.steps, args.warmup),
             "# (b), (c): host wall time per call, median of %d steps / %d gradient calls; every call returns synchronised results."
             % (args.steps, args.grad_calls),
             "# Device times: HIP events around the kernels of the diagonal's recurrence, the solve and the projection.",
             "commit: %s" % commit]

    def child(extra):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--grad-calls", str(args.grad_calls)] + extra
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:       # nothing more is started on the device after a failure
            sys.exit("measurement %s ended with status %d" % (extra, r.returncode))
        return [l for l in r.stdout.splitlines() if l.startswith(("PLAIN", "STEPS", "GRAD"))]

    if "a" in args.parts:
        builds = [("this build", batch.LIB_PATH)] + ([("parent", args.parent_lib)] if args.parent_lib else [])
        for shape in ("headline", "small"):
            med = {name: [] for name, _ in builds}
            for _ in range(args.processes):
                for name, path in builds[::-1]:      # alternately, the parent first
                    out = child(["--only", "plain", "--shape", shape, "--lib", path])
                    med[name].append(float(out[0].split(" median ")[1].split()[0]))
            for name, _ in builds:
                m = med[name]
                lines.append("(a) %s, plan without an amplitude basis, %s: device ms per evaluation of %d fresh processes %s ms -> median %.4f, spread "
                             "%.4f .. %.4f" % (NAMES[shape], name, len(m), " ".join("%.4f" % v for v in m), np.median(m), min(m), max(m)))
            if args.parent_lib:
                mine, lo, hi = float(np.median(med["this build"])), min(med["parent"]), max(med["parent"])
                lines.append("(a) %s: this build's median %.4f ms is %s the parent's own run-to-run spread %.4f .. %.4f ms"
                             % (NAMES[shape], mine, "INSIDE" if lo <= mine <= hi else ("BELOW" if mine < lo else "ABOVE"), lo, hi))
    for part, only in (("b", "steps"), ("c", "grad")):
        if part in args.parts:
            for shape in ("headline", "small"):
                lines += ["(%s) %s" % (part, l.split(" ", 1)[1]) for l in child(["--only", only, "--shape", shape])]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
