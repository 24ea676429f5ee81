# -*- coding: utf-8 -*-
"""Cases, binary128 truths and the yardstick of the narrow plan's log-likelihood routes
(tests/test_gpu_loglike_truth.py on the device, tests/test_loglike_truth_cpu.py for the reference side alone).

Every case is registered under a key in ``CASES``; ``reference(key)`` runs the double oracle
(oracle.ref.batch_log_likelihood, the sequential recurrence) and the same recurrence in binary128
(oracle.ref.quad_factor_solve) on it ONCE per session.  Nothing here needs a device.

The yardstick is the double oracle's own distance from the truth, per quantity (log det, quadratic form):

    e_ref = |X_oracle - X_128| / |X_128|,        e_dev = |X_device - X_128| / |X_128|

    benign / structured families:  Y   = max(worst e_ref over the case's problems, sqrt(N) 2^-53)
    adversarial:                   Y_b = max(e_ref of problem b, median e_ref over the judged problems, sqrt(N) 2^-53)

(sqrt(N) 2^-53: the random-walk growth of N roundings -- a lucky oracle does not set a bar of 1e-16) and a route's bar
is ``factor x Y``, factor 30 unless the route documents its own, never above the suite's REL = 1e-10 outside the
adversarial family.  A problem is judged when the oracle's status is OK, the device's status equals it and the truth is
finite and non-zero; every other problem is compared on its status only.
"""
import numpy as np

from _cases import (GRAD_FAMILIES, adversarial, coeffs_of, family_harmonic_grid, family_mixed,
                    family_near_identical_ladder, family_reference_benchmark, family_tiny_term, family_uniform_cadence,
                    synthetic, within)

FACTOR = 30.0        # tests/test_gpu_grad_truth.py, _judge_against_twin: 30 x the double twin's worst distance
# The quadratic form on the routes that settle a problem from SCANNED chunk start states (the scan pipeline at levels 0 and
# 1, the one-launch kernel): on the dense families that do not forget (synthetic bench, F0, F1, F5: y = sin t, the
# quadratic form ~1e-6 of sum y^2 / sigma^2) its distance follows the number of composed chunk elements, not the
# oracle's -- measured on one problem ((6, 0), N = 6000): 2.0e-15 in one chunk (the device's sequential recurrence),
# 7.8e-16 in 2, 5e-14 in 8, 8.6e-14 in 64, 5.2e-13 in 250; the same with every summarize kernel and every prefix mode
# (4e-14 .. 1e-13), and the same when the chunks are replayed exactly from the scanned start states (level 1), whose f
# part is 1.3e-12 (relative to its largest entry) from the long-double recurrence there against 6e-15 on the accuracy
# family: the composition of the chunk elements (the prefix) carries it, not the correction or the finalize.  Log det
# stays inside 30 x Y.  Measured worst e_dev / Y of the quadratic form: 74 (scan pipeline, single wave, N = 3000 in 100
# chunks), 70 with the lazy role split, 56 on the one-launch kernel; the factor is 1.6 x the former.  It holds for those
# families alone (quad_factor_of); every other family, the adversarial one included, and every other route keep 30.
QUAD_FACTOR_CHUNKED = 120.0
DENSE_F = ("F0", "F1", "F5")


def quad_factor_of(key):
    """QUAD_FACTOR_CHUNKED on the dense families that do not forget -- the squeezed synthetic bench family, F0, F1, F5 --
    and 30 like everything else (``None``) on every other case."""
    dense = (key[0] == "syn" and key[1] == "bench") or key[0] == "syn b=0" or (key[0] == "F" and key[1][:2] in DENSE_F)
    return QUAD_FACTOR_CHUNKED if dense else None


REL = 1e-10          # the bar of tests/test_gpu_batch.py: no bar outside the adversarial family is looser
B_BENIGN = 5
ADV_B, ADV_N, ADV_SEED = 32, 2000, 3
ADV_MIN_JUDGED = 8

SPLIT_SHAPES = [(2, 3), (0, 4), (4, 2), (6, 1), (8, 0), (1, 3), (3, 2), (7, 0)]
SMALL_SHAPES = [(1, 0), (2, 0), (3, 0), (4, 0), (0, 1), (1, 1), (2, 1), (0, 2)]
# (N, nchunk) of test_role_split_summarize_kernels: a ragged last chunk, lanes past the last chunk, more chunks than a
# wave has lanes, a short series -- and the synthetic families run at each
SIZES = [(6000, 64), (4099, 37), (3000, 100), (700, 9)]
SIZE_FAMILIES = {N: ("bench", "accuracy") for N, _ in SIZES}
LAZY_C_LIMIT = 2.0 ** -7     # csrc/api_internal.h, lazy_eligible: cmax dxmax
LAZY_D_LIMIT = 2.0 ** -5     #                                     dmax dxmax
EXP_TINY_LIMIT = 2.0 ** -10  # csrc/clr_core.h, features_phi_distinct
EXP_SMALL_LIMIT = 2.0 ** -7

F_FAMILIES = {
    "F0 reference benchmark": lambda JR, JC, N: family_reference_benchmark(JR, JC, N),
    "F1 ladder eps=1e-6": lambda JR, JC, N: family_near_identical_ladder(JR, JC, N, eps=1e-6),
    "F1 ladder eps=1e-3": lambda JR, JC, N: family_near_identical_ladder(JR, JC, N, eps=1e-3),
    "F2 harmonic grid": lambda JR, JC, N: family_harmonic_grid(JR, JC, N),
    "F3 uniform cadence": lambda JR, JC, N: family_uniform_cadence(JR, JC, N),
    "F3 uniform cadence, gap": lambda JR, JC, N: family_uniform_cadence(JR, JC, N, gap=0.5),
    "F4 tiny term": lambda JR, JC, N: family_tiny_term(JR, JC, N),
    "F5 mixed": lambda JR, JC, N: family_mixed(JR, JC, N),
}
F_SHAPES = [(2, 3), (0, 4), (1, 3)]        # routes 1 and 2 (the last one: width 7)
F_SMALL_SHAPES = [(2, 1), (0, 2)]          # the one-launch route
STRUCT_N = 4099
EVERY_STEP_D_N, EVERY_STEP_D_CHUNKS = 700, 4


def _one(c):
    """A one-problem family as a batch of one."""
    return {k: np.asarray(v)[None] for k, v in c.items()}


def _syn(family, JR, JC, N, b_frac=0.3, B=B_BENIGN, seed=None):
    case = synthetic(B, N, JR, JC, family, seed=JR + 7 * JC + N if seed is None else seed, b_frac=b_frac)
    if family == "bench":  # sort(U(0, 1)) at N ~ 5e3 has gaps up to ~2e-3: squeeze the time axis into the lazy regime
        case["t"] = case["t"] * (0.2 * min(1.0, N / 4099.0))  # (the largest gap grows as log N / N: short series further)
    return case


def host_bounds(case):
    """cmax, dmax, dxmax as BatchedGP.selection_bounds() reports them, from the inputs."""
    cs = [np.abs(case[k]).max() for k in ("c_real", "c_comp") if case[k].size]
    dmax = np.abs(case["d_comp"]).max() if case["d_comp"].size else 0.0
    return max(cs), dmax, np.max(np.diff(case["t"], axis=-1))


def _lazy_edge(which, frac, JR, JC):
    """A dense case whose time axis is scaled so that cmax dxmax (``which`` = "c") or dmax dxmax ("d") sits at ``frac``
    of the lazy regime's limit; the other product stays inside the regime ("d": the complex decay rates are taken down
    by 20 and b_comp with them, or c dx would leave first)."""
    case = _syn("bench", JR, JC, 4099, seed=77 + JR + 7 * JC)
    if which == "d":
        case["c_comp"] = case["c_comp"] * 0.05
        case["b_comp"] = case["b_comp"] * 0.05     # (|b d| <= a c: still positive definite)
    cmax, dmax, dxmax = host_bounds(case)
    scale = frac * (LAZY_C_LIMIT / cmax if which == "c" else LAZY_D_LIMIT / dmax) / dxmax
    case["t"] = case["t"] * scale
    return case


def _lazy_edge_every_step(which, JR, JC):
    """EVERY step at 0.9 .. 0.999 of the lazy regime's limit on c dx ("c") or d dx ("d"): the decay factored out of the
    state reaches its smallest value in every renormalisation window (Psi ~ e^-0.47 over 64 steps), every rotation
    between two anchors is the largest the short Taylor series takes.  ("d": the decay rates are taken down so that c dx
    stays inside the regime, b_comp with them; N = 700 in 4 chunks of 175 steps: a truncated rotation series leads
    the phase by the same amount in every 64-step window, a relative effect that does not depend on N, while the
    yardstick's floor sqrt(N) 2^-53 falls with N -- one missing term of the sine, 6e-15 rad per step, measured 0.6 of the
    bar at N = 4099 and 0.33 at N = 32768; the shortest series that still has whole windows inside a chunk shows most.)"""
    N = STRUCT_N if which == "c" else EVERY_STEP_D_N
    case = _syn("bench", JR, JC, N, seed=83 + JR + 7 * JC)
    if which == "d":
        case["c_comp"] = case["c_comp"] * 0.05
        case["b_comp"] = case["b_comp"] * 0.05
        case["c_real"] = case["c_real"] * 0.25
    cmax, dmax, _ = host_bounds(case)
    rng = np.random.RandomState(11 + JR + JC)
    dx = rng.uniform(0.9, 0.999, case["t"].shape) * (LAZY_C_LIMIT / cmax if which == "c" else LAZY_D_LIMIT / dmax)
    case["t"] = np.cumsum(dx, axis=1)
    case["y"] = np.sin(case["t"])
    return case


def _exp_regime(which, JR, JC):
    """c dx just below 2^-10 at every step ("tiny"), just below 2^-7 ("small"), or just below 2^-10 with ONE step at
    1.5 x 2^-10 and ONE at 1.5 x 2^-7, each inside a chunk of the 37-chunk plan ("gaps": at that step exactly one lane
    of the wave is above the threshold, and the whole wave changes its polynomial)."""
    N = STRUCT_N
    case = _syn("bench", JR, JC, N, seed=91 + JR + 7 * JC)
    cmax = host_bounds(case)[0]
    rng = np.random.RandomState(5 + JR + JC)
    limit = EXP_SMALL_LIMIT if which == "small" else EXP_TINY_LIMIT
    dx = rng.uniform(0.9, 0.999, case["t"].shape) * limit / cmax
    if which == "gaps":
        dx[:, 1000] = 1.5 * EXP_TINY_LIMIT / cmax
        dx[:, 3001] = 1.5 * EXP_SMALL_LIMIT / cmax
    case["t"] = np.cumsum(dx, axis=1)
    case["y"] = np.sin(40.0 * case["t"])
    return case


def _warm(seed, B, N, JR, JC, mixed):
    case = synthetic(B, N, JR, JC, "accuracy", seed=seed)
    if mixed:  # test_warm_start_mixed_batch_and_indefinite_neighbours
        case["c_real"][3, 0] = 1e-4          # remembers for ~1e4 time units: not eligible
        case["c_real"][6, 1] = 3e-4
        case["a_real"][8, 0] = -40.0         # indefinite
        case["diag"][8] = 1e-3
    return case


RAGGED_N = 4099


def ragged_lengths(B=7, N=RAGGED_N):
    """Spread over [N / 2, N], one problem at N / 10 and one at N."""
    n = np.linspace(N // 2, N - 1, B - 2).astype(int) + np.array([0, 1, 0, 1, 0])
    return np.concatenate([n, [N // 10, N]]).astype(np.int64)


CASES = {}   # key -> (builder, kind); kind: "benign" (yardstick capped in the CPU companion), "G5", "adversarial"


def _register():
    from _cases import ALL_WIDTH_SHAPES
    for JR, JC in ALL_WIDTH_SHAPES:
        for N, _ in SIZES:
            for fam in SIZE_FAMILIES[N]:
                CASES[("syn", fam, JR, JC, N)] = (lambda fam=fam, JR=JR, JC=JC, N=N: _syn(fam, JR, JC, N), "benign")
        CASES[("adv", JR, JC)] = (lambda JR=JR, JC=JC: adversarial(ADV_B, ADV_N, JR, JC, seed=ADV_SEED), "adversarial")
    for JR, JC in SPLIT_SHAPES:
        if JC:
            for N, _ in SIZES:
                CASES[("syn b=0", JR, JC, N)] = (lambda JR=JR, JC=JC, N=N: _syn("bench", JR, JC, N, b_frac=0.0), "benign")
    for name in sorted(GRAD_FAMILIES):
        CASES[("G", name)] = (lambda name=name: _one(GRAD_FAMILIES[name](STRUCT_N, 2, 3)),
                              "G5" if name.startswith("G5") else "benign")
    for name in sorted(F_FAMILIES):
        for JR, JC in F_SHAPES + F_SMALL_SHAPES:
            CASES[("F", name, JR, JC)] = (lambda name=name, JR=JR, JC=JC: _one(F_FAMILIES[name](JR, JC, STRUCT_N)), "benign")
    for JR, JC in [(2, 3), (0, 4)]:
        for which in "cd":
            for frac in (0.95, 1.05):
                CASES[("lazy edge", which, frac, JR, JC)] = (lambda w=which, f=frac, JR=JR, JC=JC: _lazy_edge(w, f, JR, JC), "benign")
            CASES[("lazy edge, every step", which, JR, JC)] = (lambda w=which, JR=JR, JC=JC: _lazy_edge_every_step(w, JR, JC), "benign")
    for JR, JC in [(3, 0), (1, 2)]:
        for which in ("tiny", "small", "gaps"):
            CASES[("exp", which, JR, JC)] = (lambda w=which, JR=JR, JC=JC: _exp_regime(w, JR, JC), "benign")
    for JR, JC in SMALL_SHAPES:
        for N in (512, 32768) if (JR, JC) in [(4, 0), (0, 2)] else (512,):
            for fam in ("bench", "accuracy"):
                CASES[("syn", fam, JR, JC, N)] = (lambda fam=fam, JR=JR, JC=JC, N=N: _syn(fam, JR, JC, N), "benign")
    CASES[("warm", "all")] = (lambda: _warm(77, 9, 12000, 2, 3, False), "benign")
    CASES[("warm", "mixed")] = (lambda: _warm(5, 10, 16000, 2, 2, True), "benign")
    CASES[("route 1",)] = (lambda: _syn("bench", 2, 3, 6000, B=8, seed=515), "benign")
    for JR, JC in [(2, 3), (1, 0), (0, 4)]:
        CASES[("ragged", JR, JC)] = (lambda JR=JR, JC=JC: _syn("bench", JR, JC, RAGGED_N, B=7, seed=33 + JR + JC), "benign")


_register()
# the warm-start batch with an indefinite problem: every OTHER problem is judged
NOT_ALL_JUDGED = {("warm", "mixed"): 9}

_CASE_CACHE = {}
_REFS = {}


def case_of(key):
    if key not in _CASE_CACHE:
        _CASE_CACHE[key] = CASES[key][0]()
    return _CASE_CACHE[key]


class Reference(object):
    """Oracle and truth of one case: ``ll0, ld0, q0, s0`` (double oracle), ``ld128, q128`` (NaN where the binary128
    recurrence meets a non-positive pivot), ``e_ref[2, B]`` (log det, quadratic form), ``judgeable[B]``, ``n[B]``."""

    def __init__(self, case, kind, lengths=None):
        from oracle import ref
        t = case["t"]
        B, N = t.shape
        self.kind = kind
        self.n = np.full(B, N) if lengths is None else np.asarray(lengths)
        self.ll0, self.ld0, self.q0 = np.empty(B), np.empty(B), np.empty(B)
        self.s0 = np.empty(B, dtype=np.int32)
        self.ld128, self.q128 = np.full(B, np.nan), np.full(B, np.nan)
        if lengths is None:
            self.ll0, self.ld0, self.q0, self.s0 = ref.batch_log_likelihood(0.0, *coeffs_of(case), t, case["diag"], case["y"])
        for b in range(B):
            n = int(self.n[b])
            co = coeffs_of(case, b)
            if lengths is not None:
                l, d, q, s = ref.batch_log_likelihood(0.0, *[c[None] for c in co], t[b:b + 1, :n], case["diag"][b:b + 1, :n],
                                                      case["y"][b:b + 1, :n])
                self.ll0[b], self.ld0[b], self.q0[b], self.s0[b] = l[0], d[0], q[0], s[0]
            try:
                _, _, _, self.ld128[b], self.q128[b] = ref.quad_factor_solve(0.0, *co, t[b, :n], case["diag"][b, :n],
                                                                             case["y"][b, :n], want_factor=False)
            except ref.RefLinAlgError:
                pass
        x128 = np.stack([self.ld128, self.q128])
        self.judgeable = (self.s0 == 0) & np.all(np.isfinite(x128) & (x128 != 0.0), axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            self.e_ref = np.abs(np.stack([self.ld0, self.q0]) - x128) / np.abs(x128)

    def floor(self):
        return np.sqrt(self.n) * 2.0 ** -53

    def yardstick(self, judged=None):
        """``Y[2, B]`` over the problems ``judged`` (default: every judgeable one)."""
        judged = self.judgeable if judged is None else judged
        e = self.e_ref[:, judged]
        if self.kind == "adversarial":
            Y = np.maximum(self.e_ref, np.median(e, axis=1)[:, None])
        else:
            Y = np.broadcast_to(np.max(e, axis=1)[:, None], self.e_ref.shape)
        return np.maximum(Y, self.floor()[None, :])


def reference(key):
    """(``("ragged", ...)``: truth and oracle on each problem's own truncated series.)"""
    if key not in _REFS:
        _REFS[key] = Reference(case_of(key), CASES[key][1], ragged_lengths() if key[0] == "ragged" else None)
    return _REFS[key]


LARGE_T_JITTER = 0.03
_LARGE_T = {}


def large_t_case():
    """test_library_trig_fallback_at_large_t_against_binary128: a series offset to t ~ 3e8."""
    case = synthetic(2, 4000, 2, 3, "accuracy", seed=8)
    case["t"] = case["t"] + 3e8
    return case


def large_t_reference():
    """``(truth[B], twin[B])`` of the log-likelihood at t ~ 3e8: quad_factor_solve forms the phases in binary128, which
    is another problem there; the truth takes each phase as fl(d t), as the device does (oracle.ref.quad_grad,
    ``phase_in_double``), its double twin beside it (one direction each: only the values are used)."""
    if not _LARGE_T:
        from oracle import ref
        from _cases import NO_GENERAL
        case = large_t_case()
        one = np.eye(1 + 2 * 2 + 4 * 3)[:1]
        v = [[fn(LARGE_T_JITTER, *coeffs_of(case, b), *NO_GENERAL, case["t"][b], case["y"][b], case["diag"][b],
                 directions=one, phase_in_double=True)[0] for b in range(2)] for fn in (ref.quad_grad, ref.double_grad)]
        _LARGE_T["v"] = (np.array(v[0]), np.array(v[1]))
    return _LARGE_T["v"]


def must_judge(key, r, subset=None):
    """How many problems a case has to judge: 8 of an adversarial batch, all of every other (``subset``: of those)."""
    if r.kind == "adversarial":
        return ADV_MIN_JUDGED
    B = len(r.s0) if subset is None else int(np.sum(subset))
    return NOT_ALL_JUDGED.get(key, B) if subset is None else B


def judge(route, key, out, ctx=None, subset=None, factor=FACTOR, quad_factor=None, levels=None):
    """Device ``out = (ll, ld, q, st)`` of case ``key`` against the truth.  Status words equal the oracle's on every
    problem; ``loglike`` is the combination of the two quantities; each judged problem's e_dev within ``factor x Y`` per
    quantity (``quad_factor``: the route's own factor for the quadratic form of the problems it settled from scanned
    chunk start states, levels 0 and 1 -- see QUAD_FACTOR_CHUNKED).  ``subset``: the problems this route settled (the
    others are judged by the caller under their own route).  Returns the judged mask."""
    r = reference(key)
    ll, ld, q, st = out
    ctx = (key, ctx)
    assert np.array_equal(st, r.s0), (route, ctx, st, r.s0)
    assert np.all(np.isneginf(ll[r.s0 != 0])), (route, ctx)
    judged = r.judgeable & (st == r.s0)
    if subset is not None:
        judged &= subset
    assert judged.sum() >= must_judge(key, r, subset), (route, ctx, int(judged.sum()))
    combo = -0.5 * (q + ld + r.n * np.log(2 * np.pi))
    assert np.allclose(ll[judged], combo[judged], rtol=1e-14, atol=0), (route, ctx)
    lv = np.zeros(len(st), dtype=int) if levels is None else np.asarray(levels)
    factors = np.full((2, len(st)), float(factor))
    if quad_factor is not None:
        factors[1, lv < 2] = quad_factor
    Y = r.yardstick(judged)
    bar = factors * Y
    if r.kind != "adversarial":
        bar = np.minimum(bar, REL)
    x128 = np.stack([r.ld128, r.q128])
    with np.errstate(invalid="ignore", divide="ignore"):
        e_dev = np.abs(np.stack([ld, q]) - x128) / np.abs(x128)
    family = key[0] if key[0] not in ("syn", "syn b=0") else "synthetic"
    for i, quantity in enumerate(("log det", "quadratic form")):
        ratio = e_dev[i, judged] / bar[i, judged]
        w = int(np.argmax(ratio))
        print("%s | %s %s: %s worst e_dev %.2e (e_ref %.2e, Y %.2e, bar %.2e, ratio %.3f, e_dev / Y %.1f)%s" %
              (route, key, ctx[1], quantity, e_dev[i, judged][w], r.e_ref[i, judged][w], Y[i, judged][w], bar[i, judged][w],
               ratio[w], e_dev[i, judged][w] / Y[i, judged][w], "" if levels is None else " level %d" % lv[judged][w]))
        print("    e_dev %s\n    e_ref %s" % (np.array2string(e_dev[i, judged], precision=1, max_line_width=200),
                                              np.array2string(r.e_ref[i, judged], precision=1, max_line_width=200)))
        for k in np.unique(lv[judged]):  # (the level each judged problem took is part of the line's name)
            m = lv[judged] == k
            w = int(np.argmax(np.where(m, ratio, -1.0)))
            within("%s%s, %s: %s e_dev / (%g x Y)" % (route, "" if levels is None else ", level %d" % k, family, quantity,
                                                      factors[i, judged][w]), ratio[w], 1.0,
                   (ctx, e_dev[i, judged][w], r.e_ref[i, judged][w], bar[i, judged][w]))
    return judged
