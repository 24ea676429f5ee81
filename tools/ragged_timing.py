#!/usr/bin/env python
# -*- coding: utf-8 -*-
"""What per-problem series lengths cost (BatchedGP.set_series(..., lengths=)), on one MI355X.

Two questions, two shapes -- the headline shape (1024 x 1e5 x width 8) and BASELINE configs[1] (256 x 1e4 x width 4):

1. Uniform plans must not pay.  ``run_timed`` of the uniform plan with this tree's library and with a library built from
   the parent commit (``--parent-lib``), alternately, each run in a fresh process, ``--runs`` runs each.  Every process
   measures the uniform plan twice and the second measurement is the one compared (the first is recorded beside it).
   The change is acceptable if its median lies within the parent's own run-to-run spread (min .. max of its runs).
2. What a ragged batch costs: the same plan with lengths drawn uniformly from [N/2, N], and with half of the problems
   at N/10, against the uniform plan (this tree's library, the same processes).  Padded steps are still executed, so
   about the uniform time is expected; the ratio of the medians is reported.

    python tools/ragged_timing.py --parent-lib build_v/parent/libcelerite_hip.so --out profiles/ragged_timing.txt

Without ``--parent-lib`` only the second part is measured.  Device time per evaluation, HIP events around ``steps``
back-to-back evaluations (``clr_batch_run_timed``, the series resident, no relayout per step)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"headline 1024 x 1e5 x width 8": (1024, 100000, 2, 3, 20),
          "configs[1] 256 x 1e4 x width 4": (256, 10000, 0, 2, 100)}


def lengths_for(kind, B, N, seed=5):
    rng = np.random.RandomState(seed)
    if kind == "U[N/2, N]":
        return rng.randint(N // 2, N + 1, size=B).astype(np.int32)
    lens = np.full(B, N, dtype=np.int32)            # "half at N/10"
    lens[rng.permutation(B)[:B // 2]] = N // 10
    return lens


def child(args):
    """One process, one library: the uniform plan, and with this tree's library the two ragged batches."""
    from celerite_amd import batch
    if args.lib:
        batch.LIB_PATH = os.path.abspath(args.lib)
    B, N, JR, JC, steps = SHAPES[args.shape]
    d = np.load(args.inputs)
    coeffs = [d[k] for k in ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")]
    t, diag, y = d["t"], d["diag"], d["y"]
    out = {}
    plan = batch.BatchedGP(B, N, JR, JC)
    try:
        def measure(lengths):
            if lengths is None:
                plan.set_series(t, diag, y)
            else:
                plan.set_series(t, diag, y, lengths=lengths)
            plan.set_coefficients(*coeffs)
            ll, ld, q, st = plan.log_likelihood()
            assert (st == 0).all() and np.isfinite(ll).all()
            plan.run_timed(max(steps // 4, 2), relayout_each_step=False)      # warm-up
            ms, k = plan.run_timed(steps, relayout_each_step=False)
            kernels[len(kernels)] = {name: v / steps for name, v in k.items()}
            return ms / steps
        kernels = {}
        out["uniform_first"] = measure(None)     # (the first measurement of a process runs on a device that is still ramping)
        out["uniform"] = measure(None)
        out["uniform_kernels"] = kernels[1]
        out["summarize_kernel"] = plan.summarize_kernel()
        out["small_mode"] = bool(plan.small_mode_active())
        out["warm_start"] = bool(plan.warm_start()["active"])
        if args.ragged:
            for kind in ("U[N/2, N]", "half at N/10"):
                out[kind] = measure(lengths_for(kind, B, N))
                out[kind + " kernels"] = kernels[len(kernels) - 1]
            out["ragged_summarize_kernel"] = plan.summarize_kernel()
    finally:
        plan.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(shape, inputs, lib, ragged):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--shape", shape, "--inputs", inputs]
    if lib:
        cmd += ["--lib", lib]
    if ragged:
        cmd += ["--ragged"]
    text = subprocess.check_output(cmd, timeout=600).decode()
    for line in text.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError("no result from " + " ".join(cmd) + "\n" + text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libcelerite_hip.so built from the parent commit")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated substrings of the shape names")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--shape")
    ap.add_argument("--inputs")
    ap.add_argument("--lib")
    ap.add_argument("--ragged", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    from bench import make_inputs
    from celerite_amd import batch
    lines = ["per-problem series lengths: device ms per evaluation (clr_batch_run_timed), %d runs each, a fresh process per run"
             % args.runs, "device: %s" % (batch.device_info(),), ""]
    fmt = lambda v: " ".join("%.4f" % x for x in v)
    for shape, (B, N, JR, JC, steps) in SHAPES.items():
        if args.shapes and not any(s in shape for s in args.shapes.split(",")):
            continue
        coeffs, t, diag, y = make_inputs(B, N, JR, JC, seed=7)
        with tempfile.TemporaryDirectory() as tmp:
            inputs = os.path.join(tmp, "inputs.npz")
            np.savez(inputs, t=t, diag=diag, y=y, **dict(zip(("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp"), coeffs)))
            del t, diag, y
            parent, this = [], []
            for _ in range(args.runs):                       # alternately: parent, this tree, parent, ...
                if args.parent_lib:
                    parent.append(run_child(shape, inputs, args.parent_lib, False))
                this.append(run_child(shape, inputs, None, True))
        lines.append("%s (%d steps per run)" % (shape, steps))
        u = [r["uniform"] for r in this]
        lines.append("  uniform plan takes: one-launch small mode %s, warm start %s" % (this[0]["small_mode"], this[0]["warm_start"]))
        if parent:
            p = [r["uniform"] for r in parent]
            lines.append("  (first measurement of each process, not compared: parent %s | this change %s)"
                         % (fmt([r["uniform_first"] for r in parent]), fmt([r["uniform_first"] for r in this])))
            lines.append("  uniform, parent commit : %s   median %.4f  spread %.4f .. %.4f" % (fmt(p), np.median(p), min(p), max(p)))
            lines.append("  uniform, this change   : %s   median %.4f" % (fmt(u), np.median(u)))
            inside = min(p) <= np.median(u) <= max(p)
            lines.append("  this change's median is %s the parent's run-to-run spread (%+.2f %% of the parent's median)"
                         % ("WITHIN" if inside else ("BELOW" if np.median(u) < min(p) else "ABOVE"),
                            100.0 * (np.median(u) / np.median(p) - 1.0)))
        else:
            lines.append("  uniform, this change   : %s   median %.4f" % (fmt(u), np.median(u)))
        kfmt = lambda rows: "  ".join("%s %.4f" % (n, np.median([r[n] for r in rows])) for n in rows[0])
        lines.append("  per kernel (medians, ms), uniform: summarize kernel '%s'" % this[0]["summarize_kernel"])
        if parent:
            lines.append("    parent commit : " + kfmt([r["uniform_kernels"] for r in parent]))
        lines.append("    this change   : " + kfmt([r["uniform_kernels"] for r in this]))
        lines.append("  with lengths: summarize kernel '%s'" % this[0]["ragged_summarize_kernel"])
        for kind in ("U[N/2, N]", "half at N/10"):
            lines.append("    %-13s : %s" % (kind, kfmt([r[kind + " kernels"] for r in this])))
        for kind in ("U[N/2, N]", "half at N/10"):
            r = [x[kind] for x in this]
            lines.append("  lengths %-13s   : %s   median %.4f   = %.3f x the uniform plan" % (kind, fmt(r), np.median(r),
                                                                                        np.median(r) / np.median(u)))
        lines.append("")
        print("\n".join(lines[-15:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
