# -*- coding: utf-8 -*-
"""Seeded inputs shared by the oracle-pinning tests and the GPU parity tests.

The first group regenerates, with ``np.random.seed(42)`` (legacy RandomState:
stable across NumPy versions), exactly the inputs the reference's own tests use
(tests/test_celerite.py, cited per case).  The second group is this repo's
synthetic families.
"""
import numpy as np

NO_GENERAL = (np.empty(0), np.empty((0, 0)), np.empty((0, 0)))

# coefficient sets of tests/test_celerite.py:66-84 / :132-150
COEFFS_W4 = (np.array([1.5, 0.1]), np.array([1.0, 0.3]), np.array([1.0]), np.array([0.1]),
             np.array([1.0]), np.array([1.0]))
COEFFS_W10 = (np.array([1.5, 0.1, 0.6, 0.3, 0.8, 0.7]), np.array([1.0, 0.3, 0.05, 0.01, 0.1, 0.2]),
              np.array([1.0, 2.0]), np.array([0.1, 0.5]), np.array([1.0, 1.0]), np.array([1.0, 1.0]))
# tests/test_celerite.py:160-165 (test_dot / test_dot_L)
COEFFS_DOT = (np.array([1.3, 0.2]), np.array([0.5, 0.8]), np.array([0.1]), np.array([0.0]),
              np.array([1.5]), np.array([0.1]))
# tests/test_celerite.py:256-261 (test_pickle)
COEFFS_PICKLE = (np.array([1.3, 1.5]), np.array([0.5, 0.2]), np.array([1.0]), np.array([0.1]),
                 np.array([1.0]), np.array([1.0]))
# cpp/src/test_solvers.cc:39-46
COEFFS_CC_REAL = (np.array([1.3, 1.5]), np.array([0.5, 0.2]))
COEFFS_CC_COMP = (np.array([1.0, 2.0]), np.array([0.1, 0.05]), np.array([1.0, 0.8]), np.array([1.0, 0.1]))


def general_terms(t, rng_rand):
    """U, V, A of tests/test_celerite.py:102-105."""
    U = np.vander(t - np.mean(t), 4).T
    V = U * rng_rand(4)[:, None]
    A = np.sum(U * V, axis=0) + 1e-8
    return A, U, V


def logdet_case(seed=42):
    """tests/test_celerite.py:49-52 (N = 5)."""
    np.random.seed(seed)
    t = np.sort(np.random.rand(5))
    diag = np.random.uniform(0.1, 0.5, len(t))
    return t, diag


def solve_case(with_general, seed=42):
    """tests/test_celerite.py:92-109 (N = 500)."""
    np.random.seed(seed)
    t = np.sort(np.random.rand(500))
    diag = np.random.uniform(0.1, 0.5, len(t))
    b = np.random.randn(len(t))
    gen = general_terms(t, np.random.rand) if with_general else NO_GENERAL
    return t, diag, b, gen


def first_tutorial_case():
    """docs/tutorials/first.rst:24-31,74-87: data + the two-SHO kernel; the printed
    log-likelihood at :101 is -6.756596382629468."""
    np.random.seed(42)
    t = np.sort(np.append(np.random.uniform(0, 3.8, 57), np.random.uniform(5.5, 10, 68)))
    yerr = np.random.uniform(0.08, 0.22, len(t))
    y = 0.2 * (t - 5) + np.sin(3 * t + 0.1 * (t - 5) ** 2) + yerr * np.random.randn(len(t))
    return t, yerr, y


FIRST_TUTORIAL_LOGLIKE = -6.756596382629468


def synthetic(B, N, J_real, J_comp, family, seed=0, b_frac=0.3):
    """The repo's synthetic families: 'bench' mirrors
    examples/benchmark/run.py:66-69,80-84; 'accuracy' mirrors
    paper/figures/error/error.py:24-25.  Per-draw log-parameter scatter 0.1."""
    rng = np.random.RandomState(seed)
    if family == "bench":
        t = np.sort(rng.rand(B, N), axis=1)
        sig = rng.uniform(0.1, 0.2, (B, N))
        y = np.sin(t)
    elif family == "accuracy":
        t = np.sort(rng.uniform(0, 0.8 * N, (B, N)), axis=1)
        sig = rng.uniform(1.0, 1.5, (B, N))
        y = rng.randn(B, N)
    else:
        raise ValueError(family)
    a_real = np.exp(1.0 + 0.1 * rng.randn(B, J_real))
    c_real = np.exp(0.1 + 0.1 * rng.randn(B, J_real))
    a_comp = np.exp(0.1 + 0.1 * rng.randn(B, J_comp))
    b_comp = b_frac * a_comp * rng.rand(B, J_comp)
    c_comp = np.exp(2.0 + 0.1 * rng.randn(B, J_comp))
    d_comp = np.exp(1.6 + 0.1 * rng.randn(B, J_comp))
    return dict(a_real=a_real, c_real=c_real, a_comp=a_comp, b_comp=b_comp, c_comp=c_comp,
                d_comp=d_comp, t=t, diag=sig ** 2, y=y)


def coeffs_of(case, p=None):
    keys = ("a_real", "c_real", "a_comp", "b_comp", "c_comp", "d_comp")
    if p is None:
        return tuple(case[k] for k in keys)
    return tuple(case[k][p] for k in keys)


def edge_points(case, rng, extra=6, own=10, L=32):
    """For a series cut into chunks of ``L`` samples (the consumer tests' 700 samples in 22 chunks of 32, the last one
    ragged).  Shared sorted points -- one before t_0, x = t_0 (m = 0), the chunk edges t[31], the midpoint of
    t[31] | t[32], t[32] and t[64], one inside the ragged last chunk, t[N-1] and 5 % past the end, a few random ones --,
    per-problem points, and an unsorted permutation of the shared ones.  The data times are problem 0's: exact there,
    interior elsewhere."""
    t = case["t"]
    B, N = t.shape
    lo, hi = t.min(), t.max()
    pad = 0.05 * (hi - lo)
    t0 = t[0]
    shared = np.sort(np.concatenate([[lo - pad, t0[0], t0[L - 1], 0.5 * (t0[L - 1] + t0[L]), t0[L], t0[2 * L],
                                      0.5 * (t0[21 * L + 9] + t0[21 * L + 10]), t0[N - 1], hi + pad],
                                     rng.uniform(lo - pad, hi + pad, extra)]))
    mine = np.stack([np.sort(np.concatenate([[t[p, 0] - pad, t[p, 0], t[p, L - 1], t[p, L], t[p, N - 1], t[p, N - 1] + pad],
                                             rng.uniform(lo - pad, hi + pad, own - 6)])) for p in range(B)])
    perm = rng.permutation(len(shared))
    assert np.any(np.diff(shared[perm]) < 0)
    return shared, mine, perm


ALL_WIDTH_SHAPES = [(jr, jc) for jc in range(5) for jr in range(9) if 1 <= jr + 2 * jc <= 8]

# one wide shape per summarize / prefix instantiation bucket of launch_wsweep_scan (csrc/wsweep_kernels.hip): the batched
# consumers of a wide plan at widths 12, 21, 31, 33, 45, 50, 61, 63, 64 (test_host_api.py keeps the list complete)
CONSUMER_WIDE_SHAPES = [(4, 4), (1, 10), (1, 15), (33, 0), (1, 22), (0, 25), (1, 30), (1, 31), (0, 32)]


def adversarial(B, N, J_real, J_comp, seed=0):
    """Near-singular and outright indefinite problems: white noise from exactly zero
    to 0.1, amplitudes over four decades with ~10 % negative ones, time spans from
    0.1 to 1000.  About a sixth of them make the reference throw linalg_exception
    (cholesky.h:176); most of the rest have condition numbers of 1e6 and beyond, where
    the reference's own recurrence is only accurate to cond * eps (checked against a
    60-digit dense factorisation during development)."""
    rng = np.random.RandomState(seed)
    span = 10 ** rng.uniform(-1, 3)
    t = np.sort(rng.uniform(0, span, (B, N)), axis=1)
    kind = rng.randint(0, 5)
    diag = {0: np.zeros((B, N)), 1: np.full((B, N), 1e-12), 2: 10 ** rng.uniform(-10, 0, (B, N)),
            3: np.full((B, N), 1e-6), 4: rng.uniform(0.01, 0.1, (B, N))}[kind]
    a_real = 10 ** rng.uniform(-2, 2, (B, J_real)) * np.where(rng.rand(B, J_real) < 0.15, -1, 1)
    c_real = 10 ** rng.uniform(-3, 2, (B, J_real))
    a_comp = 10 ** rng.uniform(-2, 2, (B, J_comp)) * np.where(rng.rand(B, J_comp) < 0.1, -1, 1)
    b_comp = a_comp * rng.uniform(-1.5, 1.5, (B, J_comp)) * (rng.rand(B, J_comp) < 0.5)
    c_comp = 10 ** rng.uniform(-3, 1, (B, J_comp))
    d_comp = 10 ** rng.uniform(-2, 2, (B, J_comp))
    return dict(a_real=a_real, c_real=c_real, a_comp=a_comp, b_comp=b_comp, c_comp=c_comp,
                d_comp=d_comp, t=t, diag=diag, y=rng.randn(B, N))


# ---- measured deviations: every tolerance assert that goes through `within` is also remembered, and the worst value
# per name is printed at the end of the session (tests/conftest.py) -- tolerances are set from these numbers, not guessed
MEASURED = {}


def within(name, dev, tol, context=None):
    dev = float(dev)
    rec = MEASURED.setdefault(name, [0.0, tol, 0])
    rec[0] = max(rec[0], dev) if dev == dev else float("nan")
    rec[1] = tol
    rec[2] += 1
    assert dev <= tol, (name, dev, tol, context)


# ---- adversarial families of the output check (csrc/api_internal.h wide_flow, BatchParams::head_check) ----------------
# Each returns ``dict(a_real, c_real, a_comp, b_comp, c_comp, d_comp, t, diag, y)`` for ONE problem (1-d coefficient
# arrays), from a fixed seed.  Widths J = J_real + 2 J_comp of 9..64 take the chunked wide kernels in
# ``CholeskySolver.compute``; the series are long enough for at least 8 chunks.

def _bench_series(rng, N, span=None):
    """The reference benchmark's sampling (examples/benchmark/run.py:66-69): the first N of 2^19 sorted uniform draws on
    [0, 1] -- so dense that no phase turns by more than a few hundredths of a radian over a chunk."""
    t = np.sort(rng.rand(2 ** 19))[:N]
    return t if span is None else t * (span / t[-1])


def _family(a_real, c_real, a_comp, b_comp, c_comp, d_comp, t, rng):
    N = len(t)
    f = lambda v: np.asarray(v, dtype=float).reshape(-1)
    return dict(a_real=f(a_real), c_real=f(c_real), a_comp=f(a_comp), b_comp=f(b_comp), c_comp=f(c_comp),
                d_comp=f(d_comp), t=np.asarray(t, dtype=float), diag=rng.uniform(0.1, 0.2, N) ** 2,
                y=np.sin(t) + 0.1 * rng.randn(N))


def family_near_identical_ladder(J_real, J_comp, N, eps, d=1.6, seed=0):
    """F1: complex terms ``d_k = d (1 + eps k)`` -- as good as identical over the first half, sampled at the benchmark's
    density -- beside ``J_real`` real terms, and ONE gap of ``1 / (eps d)`` mid-series.  Across the gap the phase
    differences of the terms jump by ``k`` radians, so directions of the state that no sample before it probed are probed
    after it.  ``c = 2 eps d``: ``exp(-c gap) = e^-2``, so the gap does not simply erase the state."""
    rng = np.random.RandomState(seed)
    gap = 1.0 / (eps * d)
    h = N // 2
    t0 = _bench_series(rng, N)
    t = np.concatenate([t0[:h], gap + t0[h:]])
    c = 2.0 * eps * d
    k = np.arange(J_comp)
    return _family(np.full(J_real, 1.0), np.full(J_real, 0.1), np.full(J_comp, 0.1), np.zeros(J_comp), np.full(J_comp, c),
                   d * (1.0 + eps * k), t, rng)


def family_harmonic_grid(J_real, J_comp, N, d0=1.0, c=1e-6, grid_frac=0.5, seed=0):
    """F2: harmonics ``d_k = k d0`` (k = 1 .. J_comp).  The first ``grid_frac`` of the series sits on multiples of
    ``pi / d0``, where every ``sin(d_k t)`` vanishes (to the rounding of the phase, which grows with t), so the sine
    directions of the state are as good as unprobed there; the rest is sampled at irregular times, where they are.
    ``c d0 / pi`` small: a chunk does not forget its start state."""
    rng = np.random.RandomState(seed)
    g = int(N * grid_frac)
    tg = np.arange(g) * (np.pi / d0)
    tr = tg[-1] + np.cumsum(rng.uniform(0.05, 2.0, N - g) * (np.pi / d0))
    k = np.arange(1, J_comp + 1)
    return _family(np.full(J_real, 1.0), np.full(J_real, 10 * c), np.full(J_comp, 0.1), np.zeros(J_comp), np.full(J_comp, c),
                   k * d0, np.concatenate([tg, tr]), rng)


def family_uniform_cadence(J_real, J_comp, N, gap=0.0, seed=0):
    """F3: IDENTICAL complex terms (a, c, d) = (0.1, 2.0, 1.6) at a uniform cadence (the benchmark's mean spacing,
    2^-19): every chunk has the same transfer map, so the rounding is systematic rather than random.  ``gap > 0``: one
    gap of that length mid-series."""
    rng = np.random.RandomState(seed)
    t = np.arange(N) * 2.0 ** -19
    if gap > 0:
        t[N // 2:] += gap
    return _family(np.full(J_real, 1.0), np.full(J_real, 0.1), np.full(J_comp, 0.1), np.zeros(J_comp), np.full(J_comp, 2.0),
                   np.full(J_comp, 1.6), t, rng)


def family_tiny_term(J_real, J_comp, N, seed=0, tiny=1e-8, d_tiny=1e-6):
    """F4: ``J_comp - 1`` identical terms (a, c, d) = (0.1, 2.0, 1.6) and ONE of amplitude ``tiny`` x 0.1 and frequency
    ``d_tiny``, at the benchmark's sampling (t <= 0.016).  The amplitude alone does not make a row of W small (the V
    rows, cos / sin of the phase, carry none; only u does), but the phase of that term never exceeds ``d_tiny t`` ~ 2e-8:
    its SINE row of W stays below 1e-6 of the largest |W| of every chunk, which is what the output check compares W
    against -- a wrong entry there is invisible to the check's normalisation and visible per row."""
    rng = np.random.RandomState(seed)
    a = np.full(J_comp, 0.1)
    d = np.full(J_comp, 1.6)
    a[-1] *= tiny
    d[-1] = d_tiny
    return _family(np.full(J_real, 1.0), np.full(J_real, 0.1), a, np.zeros(J_comp), np.full(J_comp, 2.0), d,
                   _bench_series(rng, N), rng)


def family_mixed(J_real, J_comp, N, seed=0):
    """F5: real terms (a, c) = (1.0, 0.1) and complex terms (a, c, d) = (0.1, 2.0, 1.6) -- the benchmark's parameter
    values taken as coefficients (it passes them as logs) -- with three complex terms perturbed by 1e-4 .. 1e-2 and
    ``b_comp = 0.05`` (positive definite: |b d| <= a c), at the benchmark's sampling."""
    rng = np.random.RandomState(seed)
    a = np.full(J_comp, 0.1)
    c = np.full(J_comp, 2.0)
    d = np.full(J_comp, 1.6)
    for i, s in zip(range(min(3, J_comp)), (1e-4, 1e-3, 1e-2)):
        a[i] *= 1 + s
        c[i] *= 1 - s
        d[i] *= 1 + 2 * s
    return _family(np.full(J_real, 1.0), np.full(J_real, 0.1), a, np.full(J_comp, 0.05), c, d, _bench_series(rng, N), rng)


def family_reference_benchmark(J_real, J_comp, N, seed=42):
    """F0, the control: the reference benchmark's own kernel, ``RealTerm(1.0, 0.1)`` and ``ComplexTerm(0.1, 2.0, 1.6)``
    in LOG parameters (examples/benchmark/run.py:80-84: a = e^0.1, c = e^2, d = e^1.6), its sampling and its data
    (:66-69: the first N of 2^19 sorted draws, yerr ~ U(0.1, 0.2), y = sin t) -- the family the output check was made
    for."""
    rng = np.random.RandomState(seed)
    t = np.sort(rng.rand(2 ** 19))[:N]
    yerr = rng.uniform(0.1, 0.2, 2 ** 19)[:N]
    e = np.exp
    return dict(a_real=np.full(J_real, e(1.0)), c_real=np.full(J_real, e(0.1)), a_comp=np.full(J_comp, e(0.1)),
                b_comp=np.zeros(J_comp), c_comp=np.full(J_comp, e(2.0)), d_comp=np.full(J_comp, e(1.6)), t=t,
                diag=yerr ** 2, y=np.sin(t))


# one width per padded bucket of the wide kernels (9..16, 17..32, 33..64: the walk), odd with a real term; N = 8192
OUTPUT_CHECK_WIDTHS = [(1, 6), (1, 12), (1, 31)]


def output_check_cases():
    """``{name: (generator, kwargs)}``: every family at every width bucket (F1 at every eps, F3 with and without a gap)."""
    out = {}
    for JR, JC in OUTPUT_CHECK_WIDTHS:
        w = JR + 2 * JC
        base = dict(J_real=JR, J_comp=JC, N=8192)
        for eps in (1e-9, 1e-6, 1e-3):
            out["F1 eps=%g w%d" % (eps, w)] = (family_near_identical_ladder, dict(base, eps=eps))
        out["F2 w%d" % w] = (family_harmonic_grid, base)
        out["F3 w%d" % w] = (family_uniform_cadence, base)
        out["F3 gap w%d" % w] = (family_uniform_cadence, dict(base, gap=0.5))
        out["F4 w%d" % w] = (family_tiny_term, base)
        out["F5 w%d" % w] = (family_mixed, base)
    out["F0 w16"] = (family_reference_benchmark, dict(J_real=2, J_comp=7, N=8192))
    return out


# per padded bucket and entry point of tests/test_gpu_output_check.py, the case the output check settles (level 1) that
# the sequential recurrence settles without it (level 2): the route exercised.  Calibrated on an MI355X.  At widths
# 13 .. 16 the families F1, F3, F4 and F5 stay at an output mismatch of 1e-10 .. 3e-9 over the four attempts and go to
# the sequential recurrence; the harmonic grid (with a right-hand side) and the reference benchmark's own kernel are the
# cases there the check settles.
OUTPUT_CHECK_SETTLED = {
    ("9..16", "hint"): "F2 w13", ("9..16", "plan"): "F2 w13", ("9..16", "nohint"): "F0 w16",
    ("17..32", "hint"): "F3 w25", ("17..32", "plan"): "F3 w25", ("17..32", "nohint"): "F3 w25",
    ("33..64", "hint"): "F1 eps=0.001 w63", ("33..64", "plan"): "F1 eps=0.001 w63", ("33..64", "nohint"): "F1 eps=0.001 w63",
}


def output_check_bucket(J):
    """The padded width bucket of the wide kernels a width J falls in."""
    return "9..16" if J <= 16 else ("17..32" if J <= 32 else "33..64")


_TRUTH = {}


def output_check_case(name):
    gen, kw = output_check_cases()[name]
    return gen(**kw)


def output_check_truth(name):
    """The binary128 recurrence of a case (oracle.ref.quad_factor_solve: W, D, x = K^-1 y, log det, y^T K^-1 y), computed
    once per session."""
    if name not in _TRUTH:
        from oracle import ref
        c = output_check_case(name)
        _TRUTH[name] = ref.quad_factor_solve(0.0, *coeffs_of(c), c["t"], c["diag"], c["y"])
    return _TRUTH[name]


# ---- adversarial families of the reverse-mode gradient (csrc/clr_grad_core.h: states rebuilt backwards between stored
# ones, certified by their drift) -- ONE problem each, widths 1..8 (the narrow plan), dict as above.  Every one stays on
# the fast-trig path (max d x max t < 1e9), so that the chunked gradient routes, not the sequential fallback, take it.
GRAD_FAMILY_SHAPE = (2, 3)


def _grad_family(a_real, c_real, a_comp, b_comp, c_comp, d_comp, t, rng, y=None):
    out = _family(a_real, c_real, a_comp, b_comp, c_comp, d_comp, t, rng)
    if y is not None:
        out["y"] = y
    return out


def grad_family_fast_decay(N, J_real=2, J_comp=3, seed=0):
    """G1: one real term with c dt up to ~5 per sample (it forgets between samples: the backward rebuild of its state
    amplifies rounding by exp(c dt) per step) beside slow real and complex terms (c dt ~ 1e-3) at unit mean cadence."""
    rng = np.random.RandomState(seed)
    t = np.cumsum(rng.uniform(0.05, 1.95, N))
    c_real = np.full(J_real, 1e-3)
    c_real[0] = 2.6
    return _grad_family(np.full(J_real, 1.0), c_real, np.full(J_comp, 0.3), np.zeros(J_comp), np.full(J_comp, 2e-3),
                        0.7 + 0.1 * np.arange(J_comp), t, rng, y=rng.randn(N))


def grad_family_long_gap(N, J_real=2, J_comp=3, seed=0, gap_cadences=1000.0, at=0.37):
    """G2: the benchmark's cadence with ONE gap of ``gap_cadences`` mean spacings at ``at`` of the series -- inside a
    chunk for any chunk count that does not put a boundary exactly there.  Decay rates chosen so that the gap takes the
    state down by exp(-2) .. exp(-20), not to nothing (over one cadence, by 2 % at most)."""
    rng = np.random.RandomState(seed)
    dt = rng.uniform(0.5, 1.5, N) / N
    k = int(at * N)
    dt[k] = gap_cadences / N
    t = np.cumsum(dt)
    c = np.geomspace(2.0, 20.0, J_real + J_comp) / dt[k]
    return _grad_family(np.full(J_real, 1.0), c[:J_real], np.full(J_comp, 0.2), np.zeros(J_comp), c[J_real:],
                        1.6 + np.arange(J_comp), t, rng)


def grad_family_bursts(N, J_real=2, J_comp=3, seed=0, burst=64, spacing=1e-3, gap=5.0):
    """G3: bursts of ``burst`` samples ``spacing`` apart, ``gap`` between bursts: within a burst nothing decays, across
    a gap the fast terms forget (c gap ~ 10) and the slow ones do not (c gap ~ 0.05)."""
    rng = np.random.RandomState(seed)
    nb = (N + burst - 1) // burst
    starts = np.cumsum(np.full(nb, gap))
    t = (starts[:, None] + spacing * np.cumsum(rng.uniform(0.5, 1.5, (nb, burst)), axis=1)).reshape(-1)[:N]
    c_real = np.full(J_real, 0.01)
    c_real[0] = 2.0
    c_comp = np.full(J_comp, 0.01)
    c_comp[0] = 2.0
    return _grad_family(np.full(J_real, 1.0), c_real, np.full(J_comp, 0.3), np.zeros(J_comp), c_comp,
                        0.5 + np.arange(J_comp), t, rng)


def grad_family_tiny_term(N, J_real=2, J_comp=3, seed=0, tiny=1e-8):
    """G4: the last complex term at amplitude ``tiny`` of the largest: its c and d partials scale with its amplitude,
    ~1e-8 of the largest partial -- a bar relative to the largest partial cannot see them."""
    rng = np.random.RandomState(seed)
    a = np.full(J_comp, 0.5)
    a[-1] = tiny * 1.0
    b = np.zeros(J_comp)
    b[-1] = 0.5 * tiny
    t = np.sort(rng.uniform(0, 0.8 * N, N))
    return _grad_family(np.full(J_real, 1.0), np.full(J_real, 0.05), a, b, np.full(J_comp, 0.3),
                        0.9 + 0.2 * np.arange(J_comp), t, rng, y=rng.randn(N))


def grad_family_large_phase(N, J_real=2, J_comp=3, seed=0, phase=1e6):
    """G5: d t up to ``phase`` (~1e6: the tangent of every phase carries a factor t, d' t ~ t) while max d x max t stays
    far below the fast-trig limit 1e9."""
    rng = np.random.RandomState(seed)
    t = np.sort(rng.uniform(0, 0.8 * N, N))
    d = (phase / t[-1]) * (1.0 - 0.1 * np.arange(J_comp))
    return _grad_family(np.full(J_real, 1.0), np.full(J_real, 0.1), np.full(J_comp, 0.5), np.zeros(J_comp),
                        np.full(J_comp, 0.5), d, t, rng, y=rng.randn(N))


GRAD_FAMILIES = {"G1 fast decay": grad_family_fast_decay, "G2 long gap": grad_family_long_gap,
                 "G3 bursts": grad_family_bursts, "G4 tiny term": grad_family_tiny_term,
                 "G5 large phase": grad_family_large_phase}
