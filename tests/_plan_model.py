# -*- coding: utf-8 -*-
"""A model of a ``BatchedGP`` plan's state for random walks over its public calls (tests/test_plan_walk_cpu.py checks the
generator and this model, tests/test_gpu_plan_walk.py runs the walks on the device).  Pure Python and NumPy: nothing is
imported from ``celerite_amd`` (the one thing a walk needs from it, a ``terms`` kernel, comes through ``kernel_factory``,
which the GPU test sets).

A plan keeps much that is derived from its inputs -- three chunk-interleaved copies of the series, the residual beside the
caller's ``y``, the variances beside the caller's ``diag``, padded tails, a factor in two layouts, the consumers' cached
factor state -- and csrc/api_internal.h's cause functions decide what a replaced input leaves stale.  ``PlanState`` says
what state a plan SHOULD be in after a sequence of calls, ``fresh(state)`` builds a plan directly at it, and after every
step of a walk the reused plan must give the fresh plan's bits.

Operations.  One class per kind (``KINDS``): ``legal(state)``, ``apply(state) -> state``, ``call(plan)`` and
``expect(state)`` -- ``"ok"``, ``"refuses:<fragment of the message>"`` or ``"undefined"``.  An operation prints as
``(name, k)``; every array it passes is derived from the family, the walk's seed and ``k``, so ``replay(family, seed,
[(name, k), ...])`` rebuilds a failing walk as a fixed regression test.

History dependences ``fresh()`` pins (neither plan may depend on an "auto" decision that remembers what came before):
  * small mode and warm start are set explicitly, off or forced with a fixed warm-up: the automatic small mode stays out of
    a plan that has EVER called a pipeline setter (``pipeline_pinned``, api_batch.hip: ``if (nchunk > 0) h->pipeline_pinned
    = true`` and its twins in set_layout / set_summarize_mode / set_prefix_mode), and the automatic warm start adapts its
    warm-ups to the fallbacks of earlier evaluations (``warm_boost`` / ``warm_clean``, api_internal.h);
  * chunks, layout, summarize mode, rescue mode, factor layout, exact, gradient mode and prefix mode are set explicitly
    too, on both plans, the reused one being ``fresh(first state)``;
  * the factor in HBM belongs to the materialising run that wrote it and to the settings that run was made under: a
    settings operation after the run leaves the factor the old run's (by design: ``clr_batch_set_exact`` and
    ``scan_reader_changed`` touch no factor flag), where a fresh plan would materialise under the new settings.  The model
    marks such a factor ``f_settings`` and the consumers are not legal until the next materialising run.

  * ``fit_mean_weights`` forms ``MeanFit.loglike`` from the log determinant of the evaluation in force
    (celerite_amd/batch.py: ``fit = _mean_fit(w, cov, gram, quad, ld, st, self.results()[1], self.N)``), and a plain
    evaluation's differs from the materialising run's in the last bits: the walks' ``fit_mean_weights`` runs a plain
    evaluation first, on both plans.

  * ``results()`` returns the evaluation in force, and which call ran it is history: the model keeps ``evaluated`` -- the
    last call that ran an evaluation (evaluate, materialize, enqueue, the coefficient and parameter gradients, the
    information matrix, kernel_params, fit_mean_weights' plain evaluation) with the state it ran in -- and ``Results`` is
    drawn only while input setters or ``set_chunks`` alone came since.  The gradient of a one-chunk plan of widths 33..64
    runs no evaluation (``gradient_evaluates``): ``results()`` behind it is the earlier evaluation's.

``"undefined"`` today (the documentation says "materialise again", the code does not refuse; called, not compared -- a
finding for a later issue):
  * every consumer of a REFERENCE-layout factor after the series, the coefficients or the variances (noise basis, noise
    weights) were replaced: ``require_factor`` refuses only a lean factor (``factor_is_lean && factor_inputs_changed``);
  * ``grad_mean_weights`` and ``fit_mean_weights`` on such a factor likewise (they go through ``batch_solve_impl``).
``grad_noise_weights`` does refuse it (``variance_changed``) and is modelled as a refusal.
"""
import numpy as np

from _cases import coeffs_of, synthetic
from _noise_cases import host_diag, noise_basis, noise_weights
from _amplitude_cases import amplitudes, band_basis, host_scale, host_series, log_sum, smooth_basis

kernel_factory = None     # set by the GPU test: (J_real, J_comp) -> a ``celerite_amd.terms`` kernel of that shape

MEAN_K, NOISE_K, AMP_K, M_POINTS = 2, 3, 3, 7
ZERO_PROBLEM = 2          # ``amplitudes_zero``: the problem whose scale is zero on one band (every family has B >= 3)


def make_kernel(terms, JR, JC):
    """The walks' kernel of shape (JR, JC) from the ``terms`` module handed in (``celerite_amd.terms``)."""
    k = None
    for j in range(JR):
        t = terms.RealTerm(1.0 - 0.1 * j, 0.1 + 0.2 * j)
        k = t if k is None else k + t
    for j in range(JC):
        t = terms.ComplexTerm(0.1 - 0.02 * j, 2.0 + 0.05 * j, 1.6 - 0.06 * j)
        k = t if k is None else k + t
    return k

# ---- the families ---------------------------------------------------------------------------------------------------
# B, N, (J_real, J_comp), the series' family and time scale; the settings a walk starts from and moves between; whether
# the route materialises, which consumers its plans carry, the sets of per-problem lengths; ``ill``: the family's
# near-singular problem, which the oracle anchor holds as tests/test_gpu_batch.py holds it (test_gpu_plan_walk._anchor)
NARROW_CONSUMERS = ("solve", "dot_L", "predict_solve", "predict_recurrence", "one_step_ahead", "forecast", "predict_terms",
                    "predict_cov", "leave_one_out", "inverse_diagonal", "fit_mean_weights")
WIDE_CONSUMERS = ("solve", "dot_L", "predict_solve", "one_step_ahead", "leave_one_out", "inverse_diagonal", "fit_mean_weights")


def _family(B, N, JR, JC, data="bench", tscale=1.0, small=0, warm=(0, 0), chunks=(7, 4), layouts=("staged", "interleaved"),
            summarize=(0,), mat=True, consumers=NARROW_CONSUMERS, lengths=None, flayouts=("reference", "lean"), sharded=False,
            tweak=None, ill=None):
    return dict(B=B, N=N, JR=JR, JC=JC, data=data, tscale=tscale, small=small, warm=warm, chunks=chunks, layouts=layouts,
                summarize=summarize, mat=mat, consumers=consumers, lengths=lengths, flayouts=flayouts, sharded=sharded,
                tweak=tweak, ill=ill)


def _near_singular(case):
    case["diag"][3] = 1e-14        # (test_gpu_plan_reuse._one_launch: left pending by the one-launch kernel)


def _slow_term(case):
    case["c_real"][3, 0] = 1e-4    # (test_gpu_plan_reuse._warm: does not forget over the warm-up, falls back to the scan)


FAMILIES = {
    "narrow": _family(5, 601, 2, 1, summarize=(0, -1), lengths=((601, 300, 600, 512, 77), (130, 601, 513, 511, 400))),
    "role split 8": _family(3, 720, 2, 3, tscale=0.03, chunks=(5, 3), layouts=("staged",), summarize=(1, 2, 0)),
    "role split 7": _family(3, 717, 1, 3, tscale=0.03, chunks=(5, 3), layouts=("staged",), summarize=(2, 1, 0)),
    "warm": _family(5, 1536, 2, 2, data="accuracy", warm=(1, 128), chunks=(3, 6), layouts=("staged",), mat=False,
                    consumers=(), flayouts=("reference",), tweak=_slow_term),
    "one launch": _family(5, 1000, 2, 1, small=1, chunks=(8, 5), layouts=("staged", "interleaved"), mat=False, consumers=(),
                          flayouts=("reference",), tweak=_near_singular, ill=3),
    "lengths": _family(5, 1000, 2, 3, chunks=(24, 9), summarize=(-1,), mat=False, consumers=(),
                       lengths=((1000, 512, 999, 700, 641), (300, 1000, 513, 511, 77)), flayouts=("reference",)),
    "wide": _family(3, 600, 1, 10, chunks=(5, 3), layouts=("staged",), consumers=WIDE_CONSUMERS, flayouts=("reference",)),
    "sharded": _family(5, 601, 2, 1, layouts=("staged",), consumers=("solve",), flayouts=("reference",), sharded=True),
    # width 35 below auto_chunks' 128 samples per chunk: ONE chunk, so the plan gradient is the sequential tangent kernel on
    # the resident series with no evaluation in front (api_grad.hip: seq_all)
    "wide 64 one chunk": _family(3, 120, 1, 17, chunks=(1,), layouts=("staged",), mat=False, consumers=(),
                                 flayouts=("reference",)),
}


def gradient_evaluates(fam):
    """Whether ``grad_log_likelihood`` runs an evaluation of its own in the family: not on a one-chunk plan of widths
    33..64, whose gradient leaves the results of the evaluation in force as they are."""
    c = FAMILIES[fam]
    return not (c["JR"] + 2 * c["JC"] > 32 and c["chunks"] == (1,))


# ---- the arrays of a state: functions of (family, seed, k) ----------------------------------------------------------
_CACHE = {}


def _cached(fn):
    def wrapper(*key):
        full = (fn.__name__,) + key
        if full not in _CACHE:
            out = fn(*key)
            for a in (out if isinstance(out, tuple) else (out,)):
                if isinstance(a, np.ndarray):
                    a.flags.writeable = False
            _CACHE[full] = out
        return _CACHE[full]
    return wrapper


@_cached
def _base(fam, seed):
    c = FAMILIES[fam]
    case = synthetic(c["B"], c["N"], c["JR"], c["JC"], c["data"], seed=7000 + 13 * seed)
    case["t"] = case["t"] * c["tscale"]
    if c["tweak"]:
        c["tweak"](case)
    return case


@_cached
def series(fam, seed, k):
    """``(t, diag, y)``, each (B, N): variant ``k`` of the walk's series (0: the family's own)."""
    case = _base(fam, seed)
    if k == 0:
        return case["t"], case["diag"], case["y"]
    rng = np.random.RandomState(100 * seed + k)
    return (case["t"] * (1.0 - 0.01 * (k % 5)), case["diag"] * (1.0 + 0.02 * (k % 7)),
            case["y"] + 0.1 * rng.randn(*case["y"].shape))


@_cached
def draw(fam, seed, k, variant):
    """Coefficient tables of draw ``k`` and its jitter; ``variant``: "draw", "bzero" (every b_comp exactly 0) or "fast"
    (the complex terms' decay rates four times larger: across lazy_eligible's bound 2^-7 on the role-split families)."""
    case = _base(fam, seed)
    rng = np.random.RandomState(500 * seed + k)
    tabs = [np.array(x, copy=True) for x in coeffs_of(case)]
    if k:
        tabs = [x * np.exp(0.05 * rng.randn(*x.shape)) for x in tabs]
    if variant == "bzero":
        tabs[3] = np.zeros_like(tabs[3])
    if variant == "fast":
        tabs[4] = tabs[4] * 4.0
    return tuple(tabs) + (0.0 if k % 2 == 0 else 0.01,)


@_cached
def kernel_params(fam, seed, k):
    c = FAMILIES[fam]
    p0 = kernel_factory(c["JR"], c["JC"]).get_parameter_vector()
    rng = np.random.RandomState(900 * seed + k)
    return p0[None, :] + 0.05 * np.clip(rng.randn(c["B"], len(p0)), -3, 3)


@_cached
def mean_basis(fam, k):
    N = FAMILIES[fam]["N"]
    x = np.linspace(-1.0, 1.0, N)
    return np.stack([np.ones(N), x]) if k % 2 == 0 else np.stack([x, np.sin(3.0 * x)])


@_cached
def mean_basis_at_points(fam, k):
    x = np.linspace(-1.1, 1.1, M_POINTS)
    return np.stack([np.ones(M_POINTS), x]) if k % 2 == 0 else np.stack([x, np.sin(3.0 * x)])


@_cached
def mean_weights(fam, seed, k):
    B = FAMILIES[fam]["B"]
    return np.zeros((B, MEAN_K)) if k == 0 else np.random.RandomState(300 * seed + k).uniform(-0.5, 0.5, (B, MEAN_K))


@_cached
def mean_values(fam, seed, k):
    return np.random.RandomState(400 * seed + k).uniform(-0.7, 0.7, FAMILIES[fam]["B"])


@_cached
def psi(fam, seed, per, k):
    """(K, N) or (B, K, N); bounded by the smallest variant of the diagonal, so that every variance stays positive."""
    diag = _base(fam, seed)["diag"]
    return noise_basis(np.broadcast_to(diag.min(axis=0), diag.shape), NOISE_K, per, seed=10 * seed + k)


@_cached
def psi_nan_tails(fam, seed, k):
    """The per-problem basis with NaN past the longest length a problem has in any of the family's sets: accepted only
    while lengths are in force, and never looked at there (apply_noise pads the variances' tail behind the forming pass)."""
    out = np.array(psi(fam, seed, True, k), copy=True)
    for b, n in enumerate(np.max(FAMILIES[fam]["lengths"], axis=0)):
        out[b, :, n:] = np.nan
    return out


def psi_of(state):
    kind, k = state.psi
    return psi_nan_tails(state.fam, state.seed, k) if kind == "nan" else psi(state.fam, state.seed, kind == "per", k)


@_cached
def psi_weights(fam, seed, k):
    B = FAMILIES[fam]["B"]
    return np.zeros((B, NOISE_K)) if k == 0 else noise_weights(B, NOISE_K, seed=20 * seed + k)


@_cached
def gamma(fam, seed, kind, k):
    """The amplitude basis, (K, N) or (B, K, N): band indicators for an even ``k``, the non-indicator basis for an odd one;
    ``kind`` "nan": per problem, NaN past the longest length a problem has in any of the family's sets (psi_nan_tails)."""
    c = FAMILIES[fam]
    per = kind != "shared"
    out = (band_basis if k % 2 == 0 else smooth_basis)(c["B"], c["N"], AMP_K, per, seed=10 * seed + k)
    if kind == "nan":
        out = np.array(out, copy=True)
        for b, n in enumerate(np.max(c["lengths"], axis=0)):
            out[b, :, n:] = np.nan
    return out


def gamma_of(state):
    return gamma(state.fam, state.seed, *state.gam)


@_cached
def amplitude_values(fam, seed, k, zero_band):
    """Amplitudes ``k`` (B, K); ``zero_band`` >= 0: problem ZERO_PROBLEM's amplitude of that band is zero, ``AMP_K``: all of
    its amplitudes are."""
    a = amplitudes(FAMILIES[fam]["B"], AMP_K, seed=30 * seed + k)
    if zero_band >= 0:
        a[ZERO_PROBLEM, zero_band if zero_band < AMP_K else slice(None)] = 0.0
    return a


def amplitudes_of(state):
    """The amplitudes in force.  The deliberate zero: on an indicator basis the band of problem ZERO_PROBLEM's first sample,
    which is inside every length -- a zero amplitude IS a zero scale on the band's samples; on the non-indicator basis, where
    one zero amplitude leaves a small scale and no zero, all of the problem's amplitudes."""
    band = -1
    if state.amp_zero:
        G = gamma_of(state)
        band = int(np.argmax((G[ZERO_PROBLEM] if G.ndim == 3 else G)[:, 0])) if state.gam[1] % 2 == 0 else AMP_K
    return amplitude_values(state.fam, state.seed, state.amp, band)


@_cached
def points(fam, seed):
    t = _base(fam, seed)["t"]
    lo, hi = t.min(), t.max()
    pad = 0.05 * (hi - lo)
    rng = np.random.RandomState(600 + seed)
    return np.sort(np.concatenate([[lo - pad, t[0, 0], t[0, 100], hi + pad], rng.uniform(lo, hi, M_POINTS - 4)]))


@_cached
def rhs(fam, seed):
    c = FAMILIES[fam]
    return np.random.RandomState(700 + seed).randn(c["B"], c["N"])


# ---- the state ------------------------------------------------------------------------------------------------------
class PlanState(object):
    """What a plan should hold.  Every field is a small immutable value; the arrays follow from them (``arrays``)."""

    def __init__(self, fam, seed, layout=None, summarize=None):
        c = FAMILIES[fam]
        self.fam, self.seed = fam, seed
        # the series: variant, which arrays the caller passes shared, the lengths (an index into the family's sets)
        self.ser, self.y_shared, self.d_shared, self.lengths = 0, False, False, None
        # the mean: None, ("const", k) one value, ("per", k) one per problem; or a basis with weights
        self.mean, self.phi, self.mw = None, None, 0
        # the noise model: None or ("shared" | "per", k), and its weights
        self.psi, self.nw = None, 0
        # the coefficients: ("draw" | "bzero" | "fast", k) tables with their jitter, or ("kernel", k) parameter rows
        self.coef = ("draw", 0)
        # the amplitude model: the basis, None or ("shared" | "per" | "nan", k); the amplitudes in force, None or an index,
        # and whether problem ZERO_PROBLEM carries a zero scale
        self.gam, self.amp, self.amp_zero = None, None, False
        # whether a kernel has ever been handed to the plan (``kernel_params``): grad_parameters / information_parameters
        self.kernel_seen = False
        # the evaluation in force: ``(kind, k, the state it ran in)`` of the last operation that ran one (None: none yet), and
        # whether only input setters or set_chunks came since (``results`` is drawn while they did)
        self.evaluated, self.results_kept = None, False
        # the settings
        self.chunks, self.layout = c["chunks"][0], layout or c["layouts"][0]
        self.summarize = c["summarize"][0] if summarize is None else summarize
        self.small, self.warm, self.rescue, self.flayout, self.exact = c["small"], c["warm"], 0, c["flayouts"][0], False
        self.grad_mode, self.prefix_mode = "reverse", "multilevel"
        # the factor in HBM: the step of the materialising run it belongs to (None: none), whether it is lean, and what
        # changed since: series / coefficients / variances (f_inputs), the variances (f_var), a setting (f_settings)
        self.factor, self.f_lean, self.f_inputs, self.f_var, self.f_settings = None, False, False, False, False
        self.step = 0

    def copy(self):
        n = PlanState.__new__(PlanState)
        n.__dict__.update(self.__dict__)
        return n

    @property
    def cfg(self):
        return FAMILIES[self.fam]

    @property
    def ragged(self):
        return self.lengths is not None

    @property
    def kernel_in_force(self):
        """The coefficients in force were formed from kernel parameters (the C side's ``kp_in_force``)."""
        return self.coef[0] == "kernel"

    def gam_class(self):
        """None, "nan" (NaN past the lengths) or "set"."""
        return None if self.gam is None else ("nan" if self.gam[0] == "nan" else "set")

    def lens(self):
        return None if self.lengths is None else self.cfg["lengths"][self.lengths]

    def factor_state(self):
        """"none", "ok", "lean stale", "stale" (reference layout, inputs replaced) or "settings"."""
        if self.factor is None:
            return "none"
        if self.f_inputs:
            return "lean stale" if self.f_lean else "stale"
        return "settings" if self.f_settings else "ok"


def arrays(state):
    """``(t, diag, y, lengths)`` as the caller passes them to ``set_series``: shared arrays are problem 0's row; with
    lengths the tails are NaN (never read)."""
    t, diag, y = series(state.fam, state.seed, state.ser)
    lens = state.lens()
    if lens is not None:
        t, diag, y = t.copy(), diag.copy(), y.copy()
        for b, n in enumerate(lens):
            t[b, n:], diag[b, n:], y[b, n:] = np.nan, np.nan, np.nan
    return t, (diag[0] if state.d_shared else diag), (y[0] if state.y_shared else y), lens


def host_model(w, Phi):
    """tests/test_gpu_batch_linear_mean.py's statement of the linear mean: the products summed in order."""
    B, K = w.shape
    P = np.broadcast_to(Phi, (B, K, Phi.shape[-1]))
    m = w[:, 0, None] * P[:, 0]
    for k in range(1, K):
        m = m + w[:, k, None] * P[:, k]
    return m


def effective(state):
    """``(t, variances, residual, lengths, L)`` as NumPy forms them -- ``_noise_cases.host_diag`` and
    test_gpu_batch_linear_mean's ``y - host_model(w, Phi)``, and with amplitudes in force ``_amplitude_cases.host_series`` of
    the two on ``host_scale``: ``r / s`` and ``d / (s * s)`` -- each a list of B rows truncated to the problem's length;
    ``L[B]``: ``_amplitude_cases.log_sum`` of the scale over each length (zeros without amplitudes).  A problem with a zero
    scale has non-finite rows and a non-finite ``L``: the library refuses it."""
    c = state.cfg
    B, N = c["B"], c["N"]
    t, diag, y = series(state.fam, state.seed, state.ser)
    diag = np.broadcast_to(diag[0], (B, N)) if state.d_shared else diag
    y = np.broadcast_to(y[0], (B, N)) if state.y_shared else y
    if state.psi is not None:
        diag = host_diag(diag, psi_weights(state.fam, state.seed, state.nw), psi_of(state))
    if state.mean is not None:
        mu = mean_values(state.fam, state.seed, state.mean[1])
        y = y - (mu[:, None] if state.mean[0] == "per" else mu[0])
    elif state.phi is not None:
        y = y - host_model(mean_weights(state.fam, state.seed, state.mw), mean_basis(state.fam, state.phi))
    lens = state.lens() or (N,) * B
    L = np.zeros(B)
    if state.amp is not None:
        s = host_scale(amplitudes_of(state), gamma_of(state))
        with np.errstate(divide="ignore", invalid="ignore"):
            y, diag = host_series(y, diag, s)
            L = log_sum(s, lens)[0]
    return ([t[b, :n] for b, n in enumerate(lens)], [diag[b, :n] for b, n in enumerate(lens)],
            [y[b, :n] for b, n in enumerate(lens)], lens, L)


# ---- a plan built directly at a state -------------------------------------------------------------------------------
def _set_coefficients(plan, state):
    kind, k = state.coef
    if kind == "kernel":
        c = state.cfg
        plan.set_kernel(kernel_factory(c["JR"], c["JC"]))
        plan.evaluate_parameters(kernel_params(state.fam, state.seed, k))
    else:
        tabs = draw(state.fam, state.seed, k, kind)
        plan.set_coefficients(*tabs[:6], jitter=tabs[6])


def host_coefficients(state):
    """The coefficient tables of a state formed on the host, ``(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)`` --
    for kernel parameters by the ``terms`` kernel itself, problem by problem: what the oracle is given, independent of the
    plan's own kernel program."""
    kind, k = state.coef
    if kind != "kernel":
        return draw(state.fam, state.seed, k, kind)
    c = state.cfg
    kernel = kernel_factory(c["JR"], c["JC"])
    rows = []
    for p in kernel_params(state.fam, state.seed, k):
        kernel.set_parameter_vector(p)
        rows.append([np.array(x, dtype=np.float64) for x in kernel.get_all_coefficients()])
    return tuple(np.stack([row[i] for row in rows]) for i in range(6)) + (0.0,)


def _mean_value(state):
    mu = mean_values(state.fam, state.seed, state.mean[1])
    return mu if state.mean[0] == "per" else float(mu[0])


def fresh(state, cls):
    """A plan straight at ``state``, in the canonical order: every setting, the bases, the series, the constant mean and
    the weights (the amplitudes last of them), the coefficients or the kernel.  ``cls(B, N, J_real, J_comp)`` creates it; a setter the class does not
    have (a sharded plan's layout, small mode, factor layout, ...) is skipped."""
    c = state.cfg
    plan = cls(c["B"], c["N"], c["JR"], c["JC"])
    try:
        for name, args in (("set_small_mode", (state.small,)), ("set_warm_start", state.warm if state.warm[0] else (0,)),
                           ("set_chunks", (state.chunks,)), ("set_layout", (state.layout,)),
                           ("set_summarize_mode", (state.summarize,)), ("set_rescue", (state.rescue,)),
                           ("set_factor_layout", (state.flayout,)), ("set_exact", (state.exact,)),
                           ("set_grad_mode", (state.grad_mode,)), ("set_prefix_mode", (state.prefix_mode,))):
            if hasattr(plan, name):
                getattr(plan, name)(*args)
        if state.phi is not None:
            plan.set_mean_basis(mean_basis(state.fam, state.phi))
        if state.psi is not None and state.psi[0] != "nan":
            plan.set_noise_basis(psi_of(state))
        if state.gam is not None and state.gam[0] != "nan":
            plan.set_amplitude_basis(gamma_of(state))
        t, diag, y, lens = arrays(state)
        plan.set_series(t, diag, y, lengths=lens)
        if state.psi is not None and state.psi[0] == "nan":      # (accepted only with the lengths in force)
            plan.set_noise_basis(psi_of(state))
        if state.gam is not None and state.gam[0] == "nan":
            plan.set_amplitude_basis(gamma_of(state))
        if state.mean is not None:
            plan.set_mean(_mean_value(state))
        if state.phi is not None:
            plan.set_mean_weights(mean_weights(state.fam, state.seed, state.mw))
        if state.psi is not None:
            plan.set_noise_weights(psi_weights(state.fam, state.seed, state.nw))
        if state.amp is not None:
            plan.set_amplitudes(amplitudes_of(state))
        _set_coefficients(plan, state)
    except Exception:
        plan.close()
        raise
    return plan


# ---- the operations -------------------------------------------------------------------------------------------------
RAGGED = "per-problem lengths"


class Op(object):
    kind = None
    observes = None      # "eval", "mat", "grad", "info" or "consumer": the class of an observation
    settings = False     # a settings operation: the family's route assertion follows it
    ks = (0,)            # the values of k under which legality, expectation or the abstract state after the call differ
    input_setter = False # series, means, noise, amplitudes, coefficients: settles an evaluation in flight "on ITS series"

    def __init__(self, k=0):
        self.k = int(k)

    def __repr__(self):
        return "(%r, %d)" % (self.kind, self.k)

    def legal(self, s):
        return True

    def expect(self, s):
        return "ok"

    def apply(self, s):
        """The state after the call (a refused or undefined call leaves the model's state as it was)."""
        n = s.copy()
        e = self.expect(s)
        if e == "ok":
            self.change(n)
        # the evaluation in force and whether ``results`` still returns it: a refused call leaves the plan as it was
        if self.evaluates(s):
            n.evaluated, n.results_kept = (self.kind, self.k, s), True
        elif (e == "ok" and not (self.input_setter or self.keeps_results)) or e == "undefined":
            n.results_kept = False
        n.step = s.step + 1
        return n

    keeps_results = False   # neither an evaluation nor a setter, and the results in HBM stay the evaluation's

    def evaluates(self, s):
        """Whether the call runs an evaluation whose results ``results()`` then returns."""
        return False

    def change(self, n):
        pass

    def call(self, plan):
        raise NotImplementedError


def _series_changed(n, ragged_before):
    if n.ragged != ragged_before:
        n.factor = None                       # (set_series_impl: factor_dropped when the kind of plan changes)
    n.f_inputs = n.f_var = True               # (series_replaced; the variances are the new series')


class _SetSeries(Op):
    """``set_series``; the subclasses say what changes.  Called with the arrays of the state after the change."""
    input_setter = True

    def change(self, n):
        ragged = n.ragged
        self.move(n)
        _series_changed(n, ragged)

    def call(self, plan):
        t, diag, y, lens = arrays(self.apply_to)
        plan.set_series(t, diag, y, lengths=lens)


class SeriesNew(_SetSeries):
    kind = "series_new"              # new values at the same strides (and the same lengths)

    def move(self, n):
        n.ser = 1 + self.k % 9 if 1 + self.k % 9 != n.ser else 1 + (self.k + 1) % 9


class SeriesYStride(_SetSeries):
    kind = "series_y_stride"         # y shared <-> per problem, everything else as it was

    def legal(self, s):
        return not s.ragged

    def move(self, n):
        n.y_shared = not n.y_shared


class SeriesDStride(_SetSeries):
    kind = "series_d_stride"         # diag shared <-> per problem

    def legal(self, s):
        return not s.ragged

    def move(self, n):
        n.d_shared = not n.d_shared


class SeriesLengths(_SetSeries):
    kind = "series_lengths"          # per-problem arrays with lengths= (refused on the routes that do not carry them)

    def legal(self, s):
        return not s.cfg["sharded"] and (s.cfg["lengths"] is not None or self.expect(s) != "ok")

    def expect(self, s):
        c = s.cfg
        if c["JR"] + 2 * c["JC"] > 8:
            return "refuses:per-problem lengths cover narrow plans"
        if s.warm[0] == 1 or s.small == 1 or s.summarize > 0:
            return "refuses:do not carry per-problem lengths"
        return "ok"

    def move(self, n):
        sets = n.cfg["lengths"]
        n.lengths = self.k % len(sets) if n.lengths != self.k % len(sets) else (self.k + 1) % len(sets)
        n.y_shared = n.d_shared = False
        n.ser = 1 + self.k % 9

    def call(self, plan):
        s = self.apply_to
        if s.lengths is None:                                   # a refused call: any lengths below N
            t, diag, y = series(s.fam, s.seed, s.ser)
            N = s.cfg["N"]
            plan.set_series(t, diag, y, lengths=[N - 1 - b for b in range(s.cfg["B"])])
        else:
            _SetSeries.call(self, plan)


class SeriesNoLengths(_SetSeries):
    kind = "series_no_lengths"       # the lengths cleared: a uniform plan again

    def legal(self, s):
        return s.ragged and (s.psi is None or s.psi[0] != "nan") and (s.gam is None or s.gam[0] != "nan")

    def move(self, n):
        n.lengths = None
        n.ser = 1 + self.k % 9


class _Mean(Op):
    input_setter, ks = True, (0, 1)


class MeanConst(_Mean):
    kind = "mean_const"

    def legal(self, s):
        return s.phi is None and s.mean != ("const", self.k % 4)

    def expect(self, s):
        return "ok" if s.gam is None else "refuses:an amplitude basis is set"

    def change(self, n):
        n.mean = ("const", self.k % 4)

    def call(self, plan):      # (the value of the call, not of the state behind it: a refused call leaves no mean there)
        plan.set_mean(float(mean_values(self.before.fam, self.before.seed, self.k % 4)[0]))


class MeanPer(_Mean):
    kind = "mean_per"

    def legal(self, s):
        return s.phi is None and s.mean != ("per", self.k % 4)

    def expect(self, s):
        return "ok" if s.gam is None else "refuses:an amplitude basis is set"

    def change(self, n):
        n.mean = ("per", self.k % 4)

    def call(self, plan):
        plan.set_mean(mean_values(self.before.fam, self.before.seed, self.k % 4))


class MeanNone(_Mean):
    kind = "mean_none"

    def legal(self, s):
        return s.mean is not None

    def change(self, n):
        n.mean = None

    def call(self, plan):
        plan.set_mean(None)


class MeanBasis(_Mean):
    kind = "mean_basis"              # a new basis starts from zero weights

    def legal(self, s):
        return s.mean is None

    def change(self, n):
        n.phi, n.mw = self.k % 2, 0

    def call(self, plan):
        plan.set_mean_basis(mean_basis(self.apply_to.fam, self.apply_to.phi))


class MeanBasisNone(_Mean):
    kind = "mean_basis_none"

    def legal(self, s):
        return s.phi is not None

    def change(self, n):
        n.phi, n.mw = None, 0

    def call(self, plan):
        plan.set_mean_basis(None)


class MeanWeights(_Mean):
    kind = "mean_weights"

    def legal(self, s):
        return s.phi is not None

    def change(self, n):
        n.mw = 1 + self.k % 6 if 1 + self.k % 6 != n.mw else 1 + (self.k + 1) % 6

    def call(self, plan):
        s = self.apply_to
        plan.set_mean_weights(mean_weights(s.fam, s.seed, s.mw))


def _variance_changed(n):
    n.f_inputs = n.f_var = True       # (variance_replaced)


class _NoiseBasis(Op):
    per, input_setter = None, True

    def change(self, n):
        n.psi, n.nw = (self.per, self.k % 3), 0
        _variance_changed(n)

    def call(self, plan):
        plan.set_noise_basis(psi_of(self.apply_to))


class NoiseBasisShared(_NoiseBasis):
    kind, per = "noise_basis_shared", "shared"


class NoiseBasisPer(_NoiseBasis):
    kind, per = "noise_basis_per", "per"


class NoiseBasisNanTails(_NoiseBasis):
    kind, per = "noise_basis_nan_tails", "nan"    # NaN past the lengths: legal only while lengths are in force

    def legal(self, s):
        return s.ragged


class NoiseBasisNone(Op):
    kind, input_setter = "noise_basis_none", True

    def legal(self, s):
        return s.psi is not None

    def change(self, n):
        n.psi, n.nw = None, 0
        _variance_changed(n)

    def call(self, plan):
        plan.set_noise_basis(None)


class NoiseWeights(Op):
    kind, input_setter = "noise_weights", True

    def legal(self, s):
        return s.psi is not None

    def change(self, n):
        n.nw = 1 + self.k % 6 if 1 + self.k % 6 != n.nw else 1 + (self.k + 1) % 6
        _variance_changed(n)

    def call(self, plan):
        s = self.apply_to
        plan.set_noise_weights(psi_weights(s.fam, s.seed, s.nw))


class NoiseWeightsZero(Op):
    kind, input_setter = "noise_weights_zero", True

    def legal(self, s):
        return s.psi is not None and s.nw != 0

    def change(self, n):
        n.nw = 0
        _variance_changed(n)

    def call(self, plan):
        plan.set_noise_weights(np.zeros((self.apply_to.cfg["B"], NOISE_K)))


class NoiseWeightsSame(Op):
    input_setter = True
    kind = "noise_weights_same"      # the weights already in force: clr_batch_set_noise_weights' early return, nothing changes

    def legal(self, s):
        return s.psi is not None

    def call(self, plan):
        s = self.apply_to
        plan.set_noise_weights(psi_weights(s.fam, s.seed, s.nw).copy())


class _AmplitudeBasis(Op):
    """``set_amplitude_basis``: a new basis drops the amplitudes in force -- the plan reads the plain series again."""
    per, input_setter = None, True

    def expect(self, s):
        return "ok" if s.mean is None else "refuses:a constant mean is in force"

    def change(self, n):
        if n.amp is not None:
            _variance_changed(n)      # (amplitudes_dropped: the residual and the variances formed again)
        n.gam, n.amp, n.amp_zero = (self.per, self.k % 4), None, False

    def call(self, plan):      # (the basis of the call: a refused call leaves none in the state behind it)
        plan.set_amplitude_basis(gamma(self.before.fam, self.before.seed, self.per, self.k % 4))


class AmplitudeBasisShared(_AmplitudeBasis):
    kind, per = "amplitude_basis_shared", "shared"


class AmplitudeBasisPer(_AmplitudeBasis):
    kind, per = "amplitude_basis_per", "per"


class AmplitudeBasisNanTails(_AmplitudeBasis):
    kind, per = "amplitude_basis_nan_tails", "nan"    # NaN past the lengths: legal only while lengths are in force

    def legal(self, s):
        return s.ragged


class AmplitudeBasisNone(Op):
    kind, input_setter = "amplitude_basis_none", True

    def legal(self, s):
        return s.gam is not None

    def change(self, n):
        if n.amp is not None:
            _variance_changed(n)
        n.gam, n.amp, n.amp_zero = None, None, False

    def call(self, plan):
        plan.set_amplitude_basis(None)


class Amplitudes(Op):
    kind, input_setter, zero = "amplitudes", True, False

    def legal(self, s):
        return s.gam is not None

    def change(self, n):
        n.amp = 1 + self.k % 6 if 1 + self.k % 6 != n.amp else 1 + (self.k + 1) % 6
        n.amp_zero = self.zero
        _variance_changed(n)

    def call(self, plan):
        plan.set_amplitudes(amplitudes_of(self.apply_to))


class AmplitudesZero(Amplitudes):
    kind, zero = "amplitudes_zero", True     # problem ZERO_PROBLEM gets one zero band inside its length: NaN, CLR_INVALID_ARGUMENT


class AmplitudesSame(Op):
    kind, input_setter = "amplitudes_same", True   # the amplitudes already in force: clr_batch_set_amplitudes' early return

    def legal(self, s):
        return s.amp is not None

    def call(self, plan):
        plan.set_amplitudes(amplitudes_of(self.apply_to).copy())


class _Coefficients(Op):
    variant, input_setter, ks = None, True, (0, 1)

    def legal(self, s):
        return s.coef != (self.variant, self.k % 8)

    def change(self, n):
        n.coef = (self.variant, self.k % 8)
        n.f_inputs = True             # (coefficients_replaced)

    def call(self, plan):
        _set_coefficients(plan, self.apply_to)


class CoefDraw(_Coefficients):
    kind, variant = "coef_draw", "draw"


class CoefBZero(_Coefficients):
    kind, variant = "coef_bzero", "bzero"


class CoefFast(_Coefficients):
    kind, variant = "coef_fast", "fast"


class KernelParams(_Coefficients):
    kind, variant = "kernel_params", "kernel"     # set_kernel and evaluate_parameters: the coefficients formed on the device

    def change(self, n):
        _Coefficients.change(self, n)
        n.kernel_seen = True

    def evaluates(self, s):
        return True


class _Setting(Op):
    settings, ks = True, (0, 1, 2)
    field = options = method = None

    def value(self, s):
        opts = s.cfg[self.options] if isinstance(self.options, str) else self.options
        return opts[self.k % len(opts)]

    def legal(self, s):
        opts = s.cfg[self.options] if isinstance(self.options, str) else self.options
        return len(opts) > 1 or self.same_allowed

    same_allowed = False

    def change(self, n):
        setattr(n, self.field, self.value(n))
        n.f_settings = True

    def call(self, plan):
        getattr(plan, self.method)(self.value(self.apply_to))


class SetChunks(_Setting):
    kind, field, options, method, same_allowed = "set_chunks", "chunks", "chunks", "set_chunks", True
    keeps_results = True              # (tests/test_gpu_batch.py: the results of the evaluation in force stay readable)

    def change(self, n):
        _Setting.change(self, n)
        n.factor = None               # (chunking_replaced: factor_dropped, whatever the count)


class SetLayout(_Setting):
    kind, field, options, method = "set_layout", "layout", "layouts", "set_layout"

    def legal(self, s):
        return not s.cfg["sharded"] and _Setting.legal(self, s)


class SetSummarize(_Setting):
    kind, field, options, method, same_allowed = "set_summarize_mode", "summarize", "summarize", "set_summarize_mode", True

    def value(self, s):
        opts = s.cfg["summarize"]
        if s.cfg["lengths"] is not None:
            opts = (-1, 0, 1)         # (the lengths family: mode 1 is refused while lengths are in force)
        return opts[self.k % len(opts)]

    def expect(self, s):
        return "refuses:the forced role-split summarize" if s.ragged and self.value(s) > 0 else "ok"


class SetFactorLayout(_Setting):
    kind, field, options, method = "set_factor_layout", "flayout", "flayouts", "set_factor_layout"

    def legal(self, s):
        return not s.cfg["sharded"] and _Setting.legal(self, s)

    def change(self, n):
        if self.value(n) != n.flayout:
            n.factor = None           # (factor_dropped when the layout changes; the same layout changes nothing)
            n.flayout = self.value(n)


class SetRescue(_Setting):
    kind, field, options, method, same_allowed = "set_rescue", "rescue", (0, 1), "set_rescue", True


class SetExact(_Setting):
    kind, field, options, method = "set_exact", "exact", (False, True), "set_exact"

    def legal(self, s):
        return not s.cfg["sharded"]


class Enqueue(Op):
    kind = "enqueue"                 # an evaluation left in flight: the next operation settles it first

    def evaluates(self, s):
        return True

    def call(self, plan):
        plan.enqueue()


class Evaluate(Op):
    kind, observes = "evaluate", "eval"

    def evaluates(self, s):
        return True

    def call(self, plan):
        return plan.log_likelihood()


class Materialize(Op):
    kind, observes = "materialize", "mat"

    def legal(self, s):
        return s.cfg["mat"] or s.ragged

    def expect(self, s):
        return "refuses:a materialising run" if s.ragged else "ok"

    def change(self, n):
        n.factor, n.f_lean = n.step, n.flayout == "lean"
        n.f_inputs = n.f_var = n.f_settings = False      # (factor_written)

    def evaluates(self, s):
        return self.expect(s) == "ok"

    def call(self, plan):
        return plan.materialize() if hasattr(plan, "materialize") else plan.log_likelihood(True)


class Gradient(Op):
    kind, observes = "grad_log_likelihood", "grad"

    keeps_results = True     # (where it runs no evaluation -- gradient_evaluates -- it leaves the one in force as it is)

    def legal(self, s):
        return s.cfg["JR"] + 2 * s.cfg["JC"] <= 8 or not s.ragged

    def evaluates(self, s):
        return gradient_evaluates(s.fam)

    def call(self, plan):
        return plan.grad_log_likelihood()


class Results(Op):
    """``plan.results()`` with no evaluation of its own: what a fresh plan at the state of the evaluation in force returns
    from ``results()`` directly behind the same call (``reference``), whatever input setter or ``set_chunks`` came since
    -- the calls that reach amplitude_snapshot, pin_results and warm_resolve."""
    kind, observes, keeps_results = "results", "eval", True

    def legal(self, s):
        return s.evaluated is not None and s.results_kept

    def call(self, plan):
        return plan.results()

    def reference(self, make):
        """The expected arrays: ``make(state)`` builds a fresh plan (the caller closes it)."""
        kind, k, at = self.before.evaluated
        other = make(at)
        ev = bind(KINDS[kind](k), at)
        if ev.kind == "consumer" and ev.expected == "ok":
            other.log_likelihood(True)
        try:
            ev.call(other)
        except (RuntimeError, ValueError):
            assert ev.expected != "ok", (kind, k)
        return other.results()


def _width(s):
    return s.cfg["JR"] + 2 * s.cfg["JC"]


NOT_FROM_PARAMETERS = "refuses:the coefficients in force were not formed from parameters"


def _information_expect(s, mean_partial):
    if _width(s) > 8:
        return "refuses:narrow plans (widths 1..8)"
    if mean_partial and s.phi is not None:
        return "refuses:a linear mean is in force"
    if mean_partial and s.amp is not None:
        return "refuses:amplitudes are in force"
    return "ok"


class Information(Op):
    kind, observes, ks = "information", "info", (0, 1)     # k chooses mean_partial; the factor in HBM stays as it was

    def expect(self, s):
        return _information_expect(s, self.k % 2 == 1)

    def evaluates(self, s):
        return self.expect(s) == "ok"

    def call(self, plan):
        return plan.information(mean_partial=self.k % 2 == 1)


class GradParameters(Op):
    kind, observes, keeps_results = "grad_parameters", "grad", True

    def legal(self, s):
        return s.kernel_seen and Gradient(self.k).legal(s)

    def expect(self, s):
        return "ok" if s.kernel_in_force else NOT_FROM_PARAMETERS

    def evaluates(self, s):
        return self.expect(s) == "ok" and gradient_evaluates(s.fam)

    def call(self, plan):
        return plan.grad_parameters()


class InformationParameters(Op):
    kind, observes, ks = "information_parameters", "info", (0, 1)

    def legal(self, s):
        return s.kernel_seen

    def expect(self, s):
        return _information_expect(s, self.k % 2 == 1) if s.kernel_in_force else NOT_FROM_PARAMETERS

    def evaluates(self, s):
        return self.expect(s) == "ok"

    def call(self, plan):
        return plan.information_parameters(mean_partial=self.k % 2 == 1)


def _factor_expect(s, entry=""):
    if s.ragged:
        return "refuses:" + RAGGED
    f = s.factor_state()
    if f == "none":
        return "refuses:no materialising run"
    if f == "lean stale":
        return "refuses:materialise again"
    return {"ok": "ok", "stale": "undefined", "settings": "undefined"}[f]


class GradMeanWeights(Op):
    kind, observes = "grad_mean_weights", "grad"

    def legal(self, s):
        return s.phi is not None and (s.cfg["mat"] or s.ragged) and s.factor_state() != "settings"

    def expect(self, s):
        return _factor_expect(s)

    def call(self, plan):
        return plan.grad_mean_weights()


class GradNoiseWeights(Op):
    kind, observes = "grad_noise_weights", "grad"

    def legal(self, s):
        return s.psi is not None and (s.cfg["mat"] or s.ragged) and s.factor_state() != "settings"

    def expect(self, s):
        e = _factor_expect(s)
        if e in ("ok", "undefined") and s.f_var:
            return "refuses:materialise again"          # (variance_changed)
        return e

    def call(self, plan):
        return plan.grad_noise_weights()


class GradAmplitudes(Op):
    kind, observes = "grad_amplitudes", "grad"

    def legal(self, s):
        return s.amp is not None and (s.cfg["mat"] or s.ragged) and s.factor_state() != "settings"

    def expect(self, s):
        e = _factor_expect(s)
        if e in ("ok", "undefined") and s.f_var:
            return "refuses:materialise again"          # (variance_changed)
        return e

    def call(self, plan):
        return plan.grad_amplitudes()


class Consumer(Op):
    ks = (0, 6, 10)                              # (fit_mean_weights, the consumer that evaluates: the wide and the narrow list's)
    kind, observes = "consumer", "consumer"      # k chooses one of the family's consumers; points and right-hand sides fixed per walk

    def name(self, s):
        names = s.cfg["consumers"] or NARROW_CONSUMERS
        if s.phi is None:
            names = [x for x in names if x != "fit_mean_weights"] or ["solve"]
        return names[self.k % len(names)]

    def legal(self, s):
        return (bool(s.cfg["consumers"]) or s.ragged) and s.factor_state() != "settings"

    def expect(self, s):
        if self.name(s) == "fit_mean_weights" and s.phi is not None and s.amp is not None:
            return "refuses:amplitudes are in force"    # (before the factor is looked at)
        return _factor_expect(s)

    def evaluates(self, s):
        return self.name(s) == "fit_mean_weights" and s.phi is not None     # (its plain evaluation runs whatever follows)

    def call(self, plan):
        s = self.before
        name, xs, z = self.name(s), points(s.fam, s.seed), rhs(s.fam, s.seed)
        basis = mean_basis_at_points(s.fam, s.phi) if s.phi is not None else None
        if name == "solve":
            return plan.solve() if self.k % 2 == 0 else plan.solve(z)
        if name == "dot_L":
            return plan.dot_L(z)
        if name in ("predict_solve", "predict_recurrence"):
            return plan.predict(xs, return_var=True, mean_basis=basis, method=name[8:])
        if name == "forecast":
            return plan.forecast(xs, return_var=True, mean_basis=basis)
        if name == "predict_terms":
            return plan.predict_terms(xs, return_var=True)
        if name == "predict_cov":
            return plan.predict_cov(xs)
        if name == "fit_mean_weights":
            plan.log_likelihood()        # (MeanFit.loglike takes log det K from the evaluation in force: see the module docstring)
        return getattr(plan, name)()     # one_step_ahead, leave_one_out, inverse_diagonal, fit_mean_weights


OPS = [SeriesNew, SeriesYStride, SeriesDStride, SeriesLengths, SeriesNoLengths, MeanConst, MeanPer, MeanNone, MeanBasis,
       MeanBasisNone, MeanWeights, NoiseBasisShared, NoiseBasisPer, NoiseBasisNanTails, NoiseBasisNone, NoiseWeights, NoiseWeightsZero,
       NoiseWeightsSame, AmplitudeBasisShared, AmplitudeBasisPer, AmplitudeBasisNanTails, AmplitudeBasisNone, Amplitudes,
       AmplitudesSame, AmplitudesZero, CoefDraw, CoefBZero, CoefFast, KernelParams, SetChunks, SetLayout, SetSummarize,
       SetFactorLayout, SetRescue, SetExact, Enqueue, Evaluate, Results, Materialize, Gradient, GradMeanWeights,
       GradNoiseWeights, GradAmplitudes, GradParameters, Information, InformationParameters, Consumer]
KINDS = {op.kind: op for op in OPS}
OBSERVATION_CLASSES = ("eval", "mat", "grad", "info", "consumer")


def flatten(result):
    """The arrays of an observation's result, in order (tuples and named tuples opened, ``None`` fields dropped)."""
    if result is None:
        return []
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in flatten(r)]
    return [np.asarray(result)]


# ---- walks ----------------------------------------------------------------------------------------------------------
def initial(fam, seed):
    c = FAMILIES[fam]
    return PlanState(fam, seed, layout=c["layouts"][seed % len(c["layouts"])])


def bind(op, state):
    """``op`` ready to be called on a plan in ``state``: its arrays are those of the state its ``apply`` leads to."""
    op.before = state
    op.expected = op.expect(state)
    op.apply_to = op.apply(state)
    return op


def label(op):
    """The kind, marked when the call is an expected refusal or undefined."""
    return op.kind if op.expected == "ok" else op.kind + "!"


def replay(fam, seed, sequence):
    """``[(name, k), ...]`` -> bound operations from the family's first state; an illegal step is an error."""
    state, ops = initial(fam, seed), []
    for name, k in sequence:
        op = KINDS[name](k)
        assert op.legal(state), (fam, seed, len(ops), name, k)
        ops.append(bind(op, state))
        state = op.apply_to
    return ops


def final_state(fam, seed, ops):
    return ops[-1].apply_to if ops else initial(fam, seed)


def _candidates(state, k):
    return [bind(cls(k), state) for cls in OPS if cls(k).legal(state)]


def _abstract(s):
    """What the legality and the expectation of every kind depend on (besides the family)."""
    return (s.factor_state(), s.f_var, s.phi is None, s.psi and s.psi[0], s.mean is None, s.ragged, s.nw == 0, s.summarize > 0,
            s.flayout, s.gam_class(), s.amp is None, s.kernel_seen, s.kernel_in_force,
            s.evaluated is not None and s.results_kept)


_REACHABLE, _GRAPH = {}, {}


def _graph(fam):
    """The family's graph over the abstract state, from its first state: ``edges[key] = [(kind, key behind the call), ...]`` of
    the calls that are legal and compared there (every value of k that matters: ``Op.ks``), in the order of ``OPS``."""
    if fam not in _GRAPH:
        first = initial(fam, 0)
        edges, frontier = {_abstract(first): None}, [first]
        while frontier:
            nxt = []
            for st in frontier:
                out = []
                for cls in OPS:
                    for k in cls.ks:
                        op = cls(k)
                        if not op.legal(st) or op.expect(st) != "ok":
                            continue
                        after = op.apply(st)
                        key = _abstract(after)
                        if key not in edges:      # (what can follow is a function of the abstract state: explored once)
                            edges[key] = None
                            nxt.append(after)
                        if (op.kind, key) not in out:
                            out.append((op.kind, key))
                edges[_abstract(st)] = out
            frontier = nxt
        _GRAPH[fam] = edges, dict((key, set(kind for kind, _ in out)) for key, out in edges.items())
    return _GRAPH[fam]


def reachable_pairs(fam):
    """Every ordered pair (kind_i, kind_j) that can legally be adjacent in the family, both calls compared: a breadth-first
    search from the family's first state over the abstract state, not over what the walks happened to visit."""
    if fam not in _REACHABLE:
        edges, ok = _graph(fam)
        _REACHABLE[fam] = set((kind, then) for out in edges.values() for kind, key in out for then in ok[key])
    return _REACHABLE[fam]


def _path_to(state, target, then, depth=4):
    """The shortest sequence of kinds, each an "ok" call, from ``state`` to a call of kind ``target`` after which a call of
    kind ``then`` is legal and compared: a search of the family's graph, not of states."""
    edges, ok = _graph(state.fam)
    start = _abstract(state)
    seen, frontier = {start}, [(start, [])]
    for _ in range(depth):
        nxt = []
        for at, path in frontier:
            for kind, key in edges.get(at) or ():
                if kind == target and then in ok[key]:
                    return path + [kind]
                if key not in seen:
                    seen.add(key)
                    nxt.append((key, path + [kind]))
        frontier = nxt
    return None


_RARE = ("consumer", "grad_mean_weights", "grad_noise_weights", "grad_amplitudes", "materialize", "results", "grad_parameters",
         "information_parameters")


def _walk_one(fam, seed, steps, covered, possible):
    """One walk; ``covered``: the pairs (label, kind) the walks of the earlier seeds visited, ``possible``: the pairs they
    found legal, both extended in place.  Each step prefers an operation that visits a new pair now (those that need a
    factor first); with none at hand it heads for a pair left to visit, by the shortest sequence of calls that makes it
    legal.  Expected refusals and undefined calls stay below a fifth of the steps."""
    rng = np.random.RandomState(1000 * (sorted(FAMILIES).index(fam) + 1) + seed)
    state, ops, prev, quiet, plan = initial(fam, seed), [], "start", 0, []
    for i in range(steps):
        k = int(rng.randint(0, 1000))
        cands = []
        for cls in OPS:
            op = cls(k)
            if op.legal(state):
                op.before, op.expected = state, op.expect(state)
                cands.append(op)
                if op.expected == "ok":
                    possible.add((prev, op.kind))
        last = i == steps - 1
        if i % 10 == 9:            # every tenth call is an ``evaluate``: the one the GPU test holds to the oracle
            cands = [op for op in cands if op.kind == "evaluate"]
        if last:
            cands = [op for op in cands if op.observes and op.expected == "ok"]
        if 5 * (quiet + 1) > (i + 1) or i >= steps - 2:
            cands = [op for op in cands if op.expected == "ok"]
        if prev.endswith("!"):     # the plan is as it was after a refusal: a compared observation follows
            cands = [op for op in cands if op.observes and op.expected == "ok"]
        pool = [op for op in cands if (prev, label(op)) not in covered]
        rare = [op for op in pool if op.kind in _RARE and op.expected == "ok"]
        if rare:
            pool, plan = rare, []
        elif pool:
            plan = []
        elif not last:
            if not plan:
                left = sorted(p for p in possible - covered if not p[0].endswith("!") and p[0] != "start")
                at = int(rng.randint(0, len(left))) if left else 0
                for a, b in (left[at:] + left[:at])[:6]:
                    plan = _path_to(state, a, b) or []
                    if plan:
                        break
            if plan:
                pool = [op for op in cands if op.kind == plan[0] and op.expected == "ok"]
                plan = plan[1:] if pool else []
        pool = pool or cands
        op = bind(pool[int(rng.randint(0, len(pool)))], state)
        ops.append(op)
        covered.add((prev, label(op)))
        quiet += op.expected != "ok"
        prev, state = label(op), op.apply_to
    return ops


# Steps per walk and walks per family: the smallest counts at which the walks meet tests/test_plan_walk_cpu.py's coverage
# conditions (1100 to 2000 pairs of kinds per family); more seeds, not longer walks.  LITERAL: further sequences per family,
# ``(seed, [(name, k), ...])``, run and counted like the walks -- regressions, and pairs the generator does not reach.
STEPS = 80
SEEDS = {"narrow": 58, "role split 8": 45, "role split 7": 45, "warm": 30, "one launch": 31, "lengths": 45, "wide": 39,
         "sharded": 40, "wide 64 one chunk": 28}
LITERAL = {
    "narrow": [
        # the residual and the variances both pending, then the caller's stride changes (y, then diag) under both bases
        (0, [("mean_basis", 0), ("noise_basis_shared", 0), ("evaluate", 0), ("mean_weights", 1), ("noise_weights", 1),
             ("series_y_stride", 0), ("evaluate", 0), ("noise_weights", 2), ("mean_weights", 2), ("series_d_stride", 0),
             ("evaluate", 0), ("grad_log_likelihood", 0)]),
        # weights changed while the scan reads no copy (staged), evaluations in between, then the layout makes it read one
        (0, [("noise_basis_per", 0), ("mean_basis", 0), ("evaluate", 0), ("noise_weights", 1), ("mean_weights", 1),
             ("evaluate", 0), ("evaluate", 0), ("set_layout", 1), ("evaluate", 0), ("materialize", 0)]),
        # a lean factor, the variances changed (refused), materialised again, consumers that form the cached factor state
        (2, [("set_factor_layout", 1), ("noise_basis_per", 1), ("materialize", 0), ("consumer", 8), ("noise_weights", 3),
             ("consumer", 0), ("materialize", 0), ("consumer", 8), ("consumer", 3), ("consumer", 0)]),
        # lengths set and cleared around a factor: set_series_impl drops the factor whenever the kind of plan changes
        (3, [("materialize", 0), ("consumer", 0), ("series_lengths", 0), ("consumer", 0), ("evaluate", 0), ("materialize", 0),
             ("grad_log_likelihood", 0), ("series_no_lengths", 0), ("consumer", 0), ("evaluate", 0), ("materialize", 0),
             ("consumer", 0), ("consumer", 8)]),
        # amplitudes arriving and leaving with no other transform, under a mean basis, under both, under a noise basis (the
        # first to arrive moves the caller's array aside, the last to leave moves it back); then the other order: the mean
        # and the noise basis arrive while amplitudes are in force and are removed while they stay
        (1, [("amplitude_basis_shared", 0), ("amplitudes", 1), ("evaluate", 0), ("amplitude_basis_none", 0), ("evaluate", 0),
             ("mean_basis", 0), ("mean_weights", 1), ("amplitude_basis_per", 1), ("amplitudes", 2), ("evaluate", 0),
             ("amplitude_basis_none", 0), ("evaluate", 0), ("noise_basis_per", 0), ("noise_weights", 1),
             ("amplitude_basis_shared", 2), ("amplitudes", 3), ("evaluate", 0), ("amplitude_basis_none", 0), ("evaluate", 0),
             ("mean_basis_none", 0), ("amplitude_basis_per", 3), ("amplitudes", 4), ("evaluate", 0), ("amplitude_basis_none", 0),
             ("evaluate", 0), ("noise_basis_none", 0), ("amplitude_basis_shared", 0), ("amplitudes", 5), ("mean_basis", 1),
             ("mean_weights", 2), ("evaluate", 0), ("consumer", 10), ("results", 0), ("noise_basis_shared", 1), ("noise_weights", 2), ("evaluate", 0),
             ("mean_basis_none", 0), ("evaluate", 0), ("noise_basis_none", 0), ("evaluate", 0), ("materialize", 0),
             ("grad_amplitudes", 0)]),
        # results() behind every kind of setter while the evaluation in force is one with amplitudes: its log term is
        # snapshotted before the forming pass overwrites it (amp_eval, amplitude_snapshot)
        (2, [("amplitude_basis_per", 0), ("amplitudes", 1), ("evaluate", 0), ("results", 0), ("amplitudes", 2), ("results", 0),
             ("evaluate", 0), ("series_new", 0), ("results", 0), ("evaluate", 0), ("amplitude_basis_none", 0), ("results", 0),
             ("evaluate", 0), ("noise_basis_shared", 0), ("amplitude_basis_shared", 1), ("amplitudes", 3), ("enqueue", 0),
             ("noise_weights", 1), ("results", 0), ("evaluate", 0), ("coef_draw", 1), ("set_chunks", 1), ("results", 0),
             ("evaluate", 0)]),
        # a zero scale on one problem and new amplitudes directly behind it (the flags clear again); the caller's strides of y
        # and of diag changed, lengths set and cleared, all with amplitudes in force
        (3, [("noise_basis_shared", 0), ("amplitude_basis_shared", 2), ("amplitudes", 1), ("evaluate", 0), ("amplitudes_zero", 0),
             ("evaluate", 0), ("amplitudes_zero", 1), ("amplitudes", 3), ("evaluate", 0), ("series_y_stride", 0), ("evaluate", 0), ("series_d_stride", 0),
             ("evaluate", 0), ("amplitudes_same", 0), ("series_lengths", 0), ("evaluate", 0), ("information", 0),
             ("series_no_lengths", 0), ("evaluate", 0), ("grad_log_likelihood", 0), ("results", 0)]),
        # information_parameters behind tables that replaced what the parameters formed: refused as grad_parameters is
        (0, [("kernel_params", 1), ("information_parameters", 0), ("grad_parameters", 0), ("coef_draw", 1),
             ("information_parameters", 0), ("evaluate", 0), ("grad_parameters", 0), ("evaluate", 0), ("kernel_params", 2),
             ("information_parameters", 1), ("results", 0)]),
    ],
    "role split 8": [
        # the same through the summarize mode: single wave (no copy read) -> role split
        (0, [("noise_basis_per", 0), ("set_summarize_mode", 2), ("evaluate", 0), ("noise_weights", 1), ("evaluate", 0),
             ("set_summarize_mode", 0), ("evaluate", 0)]),
    ],
    "lengths": [
        # a noise basis removed while lengths are in force, the lengths cleared around it
        (0, [("noise_basis_per", 0), ("noise_weights", 1), ("series_lengths", 0), ("evaluate", 0), ("noise_basis_none", 0),
             ("evaluate", 0), ("noise_basis_shared", 1), ("noise_weights", 2), ("series_no_lengths", 0), ("evaluate", 0),
             ("grad_log_likelihood", 0)]),
        # a basis with NaN past the lengths: the padded tail of the variances must be restored behind every forming pass
        (1, [("series_lengths", 0), ("noise_basis_nan_tails", 0), ("evaluate", 0), ("noise_weights", 1), ("evaluate", 0),
             ("grad_log_likelihood", 0), ("series_lengths", 1), ("noise_weights", 2), ("evaluate", 0)]),
        # an amplitude basis with NaN past the lengths, amplitudes in force while the lengths change and are cleared
        (2, [("series_lengths", 0), ("amplitude_basis_nan_tails", 0), ("amplitudes", 1), ("evaluate", 0), ("series_lengths", 1),
             ("results", 0), ("evaluate", 0), ("amplitude_basis_per", 1), ("amplitudes", 2), ("series_no_lengths", 0),
             ("evaluate", 0), ("grad_log_likelihood", 0)]),
    ],
    "wide 64 one chunk": [
        # the gradient of a one-chunk plan of widths 33..64 runs no evaluation: results() behind it is the evaluation in
        # force with ITS amplitudes' log term, not the one of the amplitudes set since ...
        (0, [("amplitude_basis_shared", 0), ("amplitudes", 1), ("evaluate", 0), ("amplitudes", 2), ("grad_log_likelihood", 0),
             ("results", 0), ("evaluate", 0)]),
        # ... nor no log term at all when the basis was removed in between
        (0, [("amplitude_basis_shared", 0), ("amplitudes", 1), ("evaluate", 0), ("amplitude_basis_none", 0),
             ("grad_log_likelihood", 0), ("results", 0), ("evaluate", 0)]),
    ],
}

_WALKS = {}


def walk(fam, seed, steps, cache=True):
    """The operations of walk ``seed`` of a family, deterministic.  The walks of one family share the pairs they have
    visited: walk ``seed`` is drawn after the walks 0 .. seed - 1 of the same length, towards what those left out."""
    walks, covered, possible = _WALKS.get((fam, steps), ([], set(), set())) if cache else ([], set(), set())
    possible |= reachable_pairs(fam)
    while len(walks) <= seed:
        walks.append(_walk_one(fam, len(walks), steps, covered, possible))
    if cache:
        _WALKS[(fam, steps)] = (walks, covered, possible)
    return walks[seed]


def printable(ops):
    return "[" + ", ".join(repr(op) for op in ops) + "]"
