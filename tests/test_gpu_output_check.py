# -*- coding: utf-8 -*-
"""`-m gpu`: the output check of the chunked wide factorisation (widths 9..64; csrc/api_internal.h wide_flow,
BatchParams::head_check in csrc/clr_batch_kernels.h) on the adversarial families of tests/_cases.py, against the
sequential recurrence (the same problem with ``CLR_OUTPUT_CHECK_CAP=0``) and against the binary128 recurrence
(oracle.ref.quad_factor_solve).

The check settles a problem whose replayed end states missed the scanned start states by at most the cap (level 3)
once two consecutive replays WROTE the same W and D to ``CLR_OUTPUT_CHECK_TOL``.  That agreement bounds the replays'
difference from each other, not their distance from the sequential recurrence -- so every case is run both ways, and
what the default route wrote is compared with what the sequential route wrote: W per chunk (the rule's own
normalisation), W per row (each row against its own largest entry: F4's sine row, below 1e-6 of every chunk's
largest entry, is seen) and D."""
import numpy as np
import pytest

import celerite_amd
from celerite_amd import GP, batch, terms
from oracle import ref
from _cases import (OUTPUT_CHECK_SETTLED, coeffs_of, output_check_bucket, output_check_case, output_check_cases,
                    output_check_truth, synthetic, within)

pytestmark = pytest.mark.gpu
E_, E2_ = np.empty(0), np.empty((0, 0))
HEAD_TOL = 2e-11          # CLR_OUTPUT_CHECK_TOL's default (csrc/clr_options.h)
CASES = sorted(output_check_cases())

CALIBRATED = OUTPUT_CHECK_SETTLED


def _width(c):
    return len(c["a_real"]) + 2 * len(c["a_comp"])


def _options(opts):
    for k, v in opts.items():
        batch.set_option(k, v)


def _clear(opts):
    for k in opts:
        batch.set_option(k, None)


SEQUENTIAL = {"CLR_OUTPUT_CHECK_CAP": "0"}


def w_devs(W, D, Wr, Dr, L):
    """(W per chunk of L samples against the chunk's largest |W|, W per row against the row's largest |W|, D relative)."""
    N = Wr.shape[1]
    chunk = 0.0
    for n0 in range(0, N, L):
        m = np.max(np.abs(Wr[:, n0:n0 + L]))
        chunk = max(chunk, np.max(np.abs(W[:, n0:n0 + L] - Wr[:, n0:n0 + L])) / m if m > 0 else 0.0)
    rm = np.max(np.abs(Wr), axis=1)
    row = float(np.max(np.max(np.abs(W - Wr), axis=1) / np.where(rm > 0, rm, 1.0)))
    return float(chunk), row, float(np.max(np.abs(D - Dr) / np.abs(Dr)))


def solver_run(c, hint, opts=None):
    opts = opts or {}
    _options(opts)
    try:
        s = celerite_amd.CholeskySolver()
        if hint:
            s._hint_rhs(c["y"])
        s.compute(0.0, *coeffs_of(c), E_, E2_, E2_, c["t"], c["diag"])
        level, nchunk, _ = s._route()
    finally:
        _clear(opts)
    st = s.__getstate__()
    N, J = len(c["t"]), _width(c)
    # the solver's chunks (csrc/api_solver.hip: clr::chunking, all of length L but the last): L = ceil(N / want) and nchunk =
    # ceil(N / L), so ceil(N / nchunk) == L for every want (nchunk <= want < N / (L - 1)) -- the per-chunk W comparison
    # cuts at the solver's own boundaries
    L = -(-N // nchunk)
    assert -(-N // L) == nchunk and (nchunk - 1) * L < N <= nchunk * L
    return dict(level=level, nchunk=nchunk, L=L, ld=s.log_determinant(), q=s.dot_solve(c["y"]),
                x=s.solve(c["y"])[:, 0], W=np.asarray(st[6]).reshape(J, N), D=np.asarray(st[7]))


def plan_run(probs, opts=None):
    opts = opts or {}
    B, N = len(probs), len(probs[0]["t"])
    stack = lambda k: np.stack([p[k] for p in probs])
    _options(opts)
    try:
        plan = batch.BatchedGP(B, N, len(probs[0]["a_real"]), len(probs[0]["a_comp"]))
        try:
            plan.set_series(stack("t"), stack("diag"), stack("y"))
            plan.set_coefficients(*[stack(k) for k in ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")])
            ll, ld, q, st = plan.log_likelihood(materialize=True)
            levels = plan.exact_levels().copy()
            x = plan.solve()
            _, _, W, D = plan.factor(0)
            nchunk, L = plan.chunks
        finally:
            plan.close()
    finally:
        _clear(opts)
    return dict(level=int(levels[0]), levels=levels, nchunk=nchunk, L=L, ll=ll, ld=ld[0], q=q[0], st=st, x=x[0], W=W, D=D)


def verdict(name, run, seq):
    """``{check: (value, bar)}`` of the default route's run against the sequential route's and both against binary128.
    Default vs sequential: small multiples of the tolerance the check accepts with.  Against the truth: the default
    route may be no worse than 4x the sequential route's own distance, plus a floor (the rounding of double)."""
    Wq, Dq, xq, ldq, qq = output_check_truth(name)
    out = {}
    ch, row, dd = w_devs(run["W"], run["D"], seq["W"], seq["D"], seq["L"])
    out["default vs sequential: W per chunk (of the chunk's largest)"] = (ch, 2 * HEAD_TOL)
    out["default vs sequential: W per row (of the row's largest)"] = (row, HEAD_TOL)
    out["default vs sequential: D (relative)"] = (dd, HEAD_TOL)

    def truth(r):
        _, row_, d_ = w_devs(r["W"], r["D"], Wq, Dq, r["L"])
        return dict(row=row_, D=d_, ld=abs(r["ld"] - ldq) / abs(ldq), q=abs(r["q"] - qq) / abs(qq),
                    x=float(np.max(np.abs(r["x"] - xq)) / np.max(np.abs(xq))))

    td, ts = truth(run), truth(seq)
    floors = dict(row=1e-12, D=2e-13, ld=1e-14, q=1e-13, x=1e-13)
    labels = dict(row="W per row (of the row's largest)", D="D (relative)", ld="log det (relative)",
                  q="dot_solve (relative)", x="solve (of the largest)")
    for k in floors:
        out["vs binary128: %s, default route" % labels[k]] = (td[k], 4 * ts[k] + floors[k])
        out["vs binary128: %s, sequential route" % labels[k]] = (ts[k], ts[k])   # (recorded: the yardstick itself)
    return out


def check(entry, name, run, seq):
    tag = (name, entry, "levels %d / %d" % (run["level"], seq["level"]))
    for k, (v, bar) in verdict(name, run, seq).items():
        within("output check, %s: %s" % (entry, k), v, bar, tag)


def routes(entry, name, run, seq):
    """Record the route; the cap at 0 never leaves a problem at level 3, and the check only acts where the end states
    missed (a problem the sequential route settles at level 0 / 1 is settled the same way by default)."""
    # (in the session's measured summary: one line per case and entry point, the level by default against 2)
    within("output check route, %s, %s (%d chunks): level by default [level %d with the cap at 0]"
           % (entry, name, run["nchunk"], seq["level"]), run["level"], 2)
    assert run["nchunk"] > 1 and seq["nchunk"] == run["nchunk"]
    assert seq["level"] in (0, 1, 2) and run["level"] in (0, 1, 2)
    if seq["level"] < 2:
        assert run["level"] == seq["level"]
    if CALIBRATED.get((output_check_bucket(_width(output_check_case(name))), entry)) == name:
        assert (run["level"], seq["level"]) == (1, 2), (name, entry, run["level"], seq["level"])


@pytest.mark.parametrize("hint", [True, False], ids=["hint", "nohint"])
@pytest.mark.parametrize("name", CASES)
def test_solver_output_check_against_sequential_and_binary128(name, hint):
    """``CholeskySolver.compute`` with (``_hint_rhs``) and without a right-hand side (logdet_only: the quadratic form is
    not part of the end-state test), once by default and once with the sequential fallback forced."""
    c = output_check_case(name)
    run, seq = solver_run(c, hint), solver_run(c, hint, SEQUENTIAL)
    entry = "hint" if hint else "nohint"
    routes(entry, name, run, seq)
    check("CholeskySolver." + entry, name, run, seq)


@pytest.mark.parametrize("name", CASES)
def test_materialising_plan_output_check_decides_each_problem_on_its_own(name):
    """A materialising wide plan of B = 4: the case, the case again, a well-conditioned neighbour (summarised, level 0)
    and one that is not positive definite (status and -inf as the oracle's) -- each problem settled on its own."""
    c = output_check_case(name)
    N, JR, JC = len(c["t"]), len(c["a_real"]), len(c["a_comp"])
    nb = synthetic(1, N, JR, JC, "accuracy", seed=JR + JC)
    nb = {k: (v[0] if np.ndim(v) == 2 else v) for k, v in nb.items()}
    bad = dict(c, a_real=np.full(JR, -7.0), diag=np.zeros(N))
    probs = [c, c, nb, bad]
    run, seq = plan_run(probs), plan_run(probs, SEQUENTIAL)
    routes("plan", name, run, seq)
    check("materialising plan", name, run, seq)
    assert np.array_equal(run["levels"][:2], [run["level"]] * 2) and run["levels"][2] == 0
    l0, d0, q0, s0 = ref.batch_log_likelihood(0.0, *[np.stack([p[k] for p in probs]) for k in
                                                     ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")],
                                              np.stack([p["t"] for p in probs]), np.stack([p["diag"] for p in probs]),
                                              np.stack([p["y"] for p in probs]))
    assert np.array_equal(run["st"], s0) and np.array_equal(seq["st"], s0)
    assert np.isneginf(run["ll"][3]) and np.isneginf(l0[3])
    within("output check, materialising plan: neighbour's log-likelihood vs oracle", abs(run["ll"][2] - l0[2]) / abs(l0[2]), 1e-11, name)


def test_a_loosened_tolerance_is_caught_by_the_bars():
    """The power of the bars above: with ``CLR_OUTPUT_CHECK_TOL=1e-7`` the check accepts after one replay (attempt 1's
    output mismatch is about 3e-9, profiles/r06q_output_check_convergence.txt) and at least one calibrated case must then
    fail the default-vs-sequential or the truth bar."""
    failed = []
    for name in sorted(set(CALIBRATED.values())):
        c = output_check_case(name)
        seq = solver_run(c, True, SEQUENTIAL)
        loose = solver_run(c, True, {"CLR_OUTPUT_CHECK_TOL": "1e-7"})
        assert loose["level"] == 1, (name, loose["level"])
        for k, (v, bar) in verdict(name, loose, seq).items():
            if not v <= bar:
                failed.append((name, k, v, bar))
    for name, k, v, bar in failed:     # (in the session's measured summary: what the loosened route missed by)
        within("output check power test, CLR_OUTPUT_CHECK_TOL=1e-7, %s: %s (value / bar)" % (name, k), v / bar, np.inf)
    assert failed


def test_object_api_end_to_end_on_an_output_check_family():
    """``celerite.GP`` built from ``terms`` on F3 at width 25 (identical terms, uniform cadence): ``log_likelihood`` and
    ``predict`` with the output check on, against the same GP with the sequential fallback and against binary128."""
    name = "F3 w25"
    c = output_check_case(name)
    Wq, Dq, xq, ldq, qq = output_check_truth(name)
    kernel = None
    for a, cc in zip(c["a_real"], c["c_real"]):
        k = terms.RealTerm(np.log(a), np.log(cc))
        kernel = k if kernel is None else kernel + k
    for a, cc, d in zip(c["a_comp"], c["c_comp"], c["d_comp"]):
        kernel += terms.ComplexTerm(np.log(a), np.log(cc), np.log(d))
    N = len(c["t"])
    want_ll = -0.5 * (qq + ldq + N * np.log(2 * np.pi))
    x = np.linspace(c["t"][0], c["t"][-1], 7)
    r = ref.RefSolver()
    r.compute(0.0, *coeffs_of(c), E_, E2_, E2_, c["t"], c["diag"])
    want_mu = r.predict(c["y"], x)
    got = {}
    for tag, opts in (("default", {}), ("sequential", SEQUENTIAL)):
        _options(opts)
        try:
            gp = GP(kernel)
            gp.compute(c["t"], np.sqrt(c["diag"]))
            ll = gp.log_likelihood(c["y"])
            level = gp.solver._route()[0]
        finally:
            _clear(opts)
        mu = gp.predict(c["y"], x, return_cov=False)
        got[tag] = (ll, mu, level)
        within("output check, object API: log-likelihood vs binary128", abs(ll - want_ll) / abs(want_ll), 1e-13, (tag, level))
        within("output check, object API: predict vs oracle (of the largest)", np.max(np.abs(mu - want_mu)) / np.max(np.abs(want_mu)), 1e-10, (tag, level))
    print("object API routes: default %d, sequential %d" % (got["default"][2], got["sequential"][2]))
    assert (got["default"][2], got["sequential"][2]) == (1, 2)
    within("output check, object API: log-likelihood default vs sequential", abs(got["default"][0] - got["sequential"][0]) / abs(want_ll), 1e-13, name)
