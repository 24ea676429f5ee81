# -*- coding: utf-8 -*-
"""Batched log-likelihoods: B independent (time series x hyper-parameter draw)
problems per call -- the data-parallel axis the reference does not have.

One evaluation of problem ``p`` is exactly ``GP.compute`` + ``GP.log_likelihood``
of the reference (celerite/celerite.py:103-219):
``-0.5 (r^T K_p^-1 r + log det K_p + N log 2 pi)``, with ``quiet=True``
semantics for matrices that are not positive definite (``status[p] == 2`` and
``-inf``).  The arithmetic runs as the chunked-scan HIP kernels of
``csrc/clr_core.h`` through ``clr_batch_*`` in ``include/celerite_hip.h``; this
file is plumbing (ctypes).  There is no CPU fallback: without an MI355X every
call raises ``RuntimeError``.
"""
import collections
import ctypes as C
import os

import numpy as np

__all__ = ["BatchedGP", "ShardedBatchedGP", "shard_bounds", "batch_log_likelihood", "batch_grad_log_likelihood",
           "kernel_coefficient_table", "kernel_coefficient_jacobian_table", "chain_gradient", "compile_kernel",
           "CompiledKernel", "MeanFit", "OneStepAhead", "gram_solve", "LIB_PATH"]

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libcelerite_hip.so")

CLR_OK, CLR_NOT_POSITIVE_DEFINITE = 0, 2
CLR_DIMENSION_MISMATCH, CLR_INVALID_ARGUMENT = 1, 6

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lib = None


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libcelerite_hip.so is not built: run `make` at the repository "
                          "root; there is no pure-Python fallback")
    lib = C.CDLL(LIB_PATH)
    lib.clr_last_error.restype = C.c_char_p
    lib.clr_status_string.restype = C.c_char_p
    lib.clr_status_string.argtypes = [C.c_int]
    lib.clr_version.restype = C.c_char_p
    lib.clr_batch_create.restype = C.c_void_p
    lib.clr_batch_create.argtypes = [C.c_int] * 5
    lib.clr_batch_destroy.argtypes = [C.c_void_p]
    lib.clr_batch_set_series.argtypes = [C.c_void_p, _dp, C.c_long, _dp, C.c_long, _dp, C.c_long]
    lib.clr_batch_set_coefficients.argtypes = [C.c_void_p] + [_dp] * 7
    lib.clr_batch_set_chunks.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_get_chunks.argtypes = [C.c_void_p, _ip, _ip]
    lib.clr_batch_enqueue.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_synchronize.argtypes = [C.c_void_p]
    lib.clr_batch_get_results.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    lib.clr_batch_get_factor.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    lib.clr_batch_run_timed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp]
    lib.clr_batch_set_layout.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_set_summarize_mode.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_get_summarize_kernel.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_get_split_variant.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_fp32_probe.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.clr_batch_set_profiling.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_get_profile.argtypes = [C.c_void_p, _dp, _ip]
    lib.clr_batch_set_prefix_mode.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_set_general.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp, C.c_long, _dp, C.c_long]
    lib.clr_batch_set_warm_start.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.clr_batch_get_warm_start.argtypes = [C.c_void_p] + [_ip] * 7
    lib.clr_batch_set_prefix_plan.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.clr_batch_grad.argtypes = [C.c_void_p, _dp, _dp, _ip]
    lib.clr_batch_get_grad_fallbacks.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_set_grad_mode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double]
    lib.clr_batch_get_grad_info.argtypes = [C.c_void_p, _ip, _ip, _dp]
    lib.clr_batch_get_prefix_plan.argtypes = [C.c_void_p, _ip, _ip, _ip]
    lib.clr_batch_debug_get_starts.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_debug_compose_check.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    lib.clr_batch_get_selection_bounds.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
    lib.clr_batch_set_selection_bounds.argtypes = [C.c_void_p] + [C.c_double] * 4
    lib.clr_sharded_get_summarize_kernel.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_set_exact.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_get_exact_count.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_get_exact_flags.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_get_conditioning.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.clr_batch_get_conditioning_chunkwise.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_get_measured_error.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_set_certificate.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.clr_batch_set_certificate_gamma.argtypes = [C.c_void_p, C.c_double, C.c_double]
    lib.clr_shard_bounds.argtypes = [C.c_int, C.c_int, C.c_int, _ip, _ip]
    lib.clr_sharded_create.restype = C.c_void_p
    lib.clr_sharded_create.argtypes = [C.c_int] * 4 + [_ip, C.c_int]
    lib.clr_sharded_destroy.argtypes = [C.c_void_p]
    lib.clr_sharded_last_error.restype = C.c_char_p
    lib.clr_sharded_num_shards.argtypes = [C.c_void_p]
    lib.clr_sharded_get_shard.argtypes = [C.c_void_p, C.c_int, _ip, _ip, _ip]
    lib.clr_sharded_set_chunks.argtypes = [C.c_void_p, C.c_int]
    lib.clr_sharded_get_chunks.argtypes = [C.c_void_p, C.c_int, _ip, _ip]
    lib.clr_sharded_set_summarize_mode.argtypes = [C.c_void_p, C.c_int]
    lib.clr_sharded_set_series.argtypes = [C.c_void_p, _dp, C.c_long, _dp, C.c_long, _dp, C.c_long]
    lib.clr_sharded_set_coefficients.argtypes = [C.c_void_p] + [_dp] * 7
    lib.clr_sharded_enqueue.argtypes = [C.c_void_p]
    lib.clr_sharded_synchronize.argtypes = [C.c_void_p]
    lib.clr_sharded_get_results.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    lib.clr_sharded_evaluate.argtypes = [C.c_void_p] + [_dp] * 7 + [_dp, _dp, _dp, _ip]
    lib.clr_sharded_run_timed.argtypes = [C.c_void_p, C.c_int, _dp]
    lib.clr_batch_set_mean.argtypes = [C.c_void_p, _dp, C.c_long]
    lib.clr_batch_evaluate_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_long] + [C.c_void_p] * 11
    lib.clr_batch_grad_mean.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    lib.clr_sharded_set_mean.argtypes = [C.c_void_p, _dp, C.c_long]
    lib.clr_sharded_evaluate_mean.argtypes = [C.c_void_p, _dp, C.c_long] + [_dp] * 10 + [_ip]
    lib.clr_sharded_grad_mean.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    lib.clr_batch_set_mean_basis.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long]
    lib.clr_batch_set_mean_weights.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_grad_mean_weights.argtypes = [C.c_void_p, _dp, _ip]
    lib.clr_batch_get_mean_project_ms.argtypes = [C.c_void_p, _dp]
    lib.clr_sharded_set_mean_basis.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long]
    lib.clr_sharded_set_mean_weights.argtypes = [C.c_void_p, _dp]
    lib.clr_sharded_grad_mean_weights.argtypes = [C.c_void_p, _dp, _ip]
    lib.clr_batch_fit_mean_weights.argtypes = [C.c_void_p, C.c_double] + [_dp] * 5 + [_ip]
    lib.clr_batch_set_noise_basis.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long]
    lib.clr_batch_set_noise_weights.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_grad_noise_weights.argtypes = [C.c_void_p, _dp, _ip]
    lib.clr_batch_get_noise_project_ms.argtypes = [C.c_void_p, _dp]
    lib.clr_sharded_set_noise_basis.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long]
    lib.clr_sharded_set_noise_weights.argtypes = [C.c_void_p, _dp]
    lib.clr_sharded_grad_noise_weights.argtypes = [C.c_void_p, _dp, _ip]
    lib.clr_sharded_get_noise_project_ms.argtypes = [C.c_void_p, _dp]
    for pre in ("clr_batch", "clr_sharded"):
        getattr(lib, pre + "_set_amplitude_basis").argtypes = [C.c_void_p, C.c_int, _dp, C.c_long]
        getattr(lib, pre + "_set_amplitudes").argtypes = [C.c_void_p, _dp]
        getattr(lib, pre + "_get_log_amplitude_sum").argtypes = [C.c_void_p, _dp]
        getattr(lib, pre + "_grad_amplitudes").argtypes = [C.c_void_p, _dp, _ip]
        getattr(lib, pre + "_get_amplitude_project_ms").argtypes = [C.c_void_p, _dp]
    lib.clr_sharded_fit_mean_weights.argtypes = [C.c_void_p, C.c_double] + [_dp] * 5 + [_ip]
    lib.clr_batch_set_mean_fit_tile.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_get_mean_fit_ms.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.clr_batch_leave_one_out.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    lib.clr_sharded_leave_one_out.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
    lib.clr_batch_get_leave_one_out_ms.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.clr_batch_one_step_ahead.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _ip]
    lib.clr_sharded_one_step_ahead.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _ip]
    lib.clr_batch_forecast.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp, _dp]
    lib.clr_sharded_forecast.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp, _dp]
    for pre in ("clr_batch", "clr_sharded"):
        getattr(lib, pre + "_periodogram").argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, C.c_double, C.c_int, C.c_double,
                                                       _dp, _dp, _dp, _dp, _ip]
        getattr(lib, pre + "_set_periodogram_tile").argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_get_periodogram_ms.argtypes = [C.c_void_p, _dp]
    lib.clr_sharded_get_periodogram_ms.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_debug_get_periodogram_block.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_predict_terms.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, C.c_int, C.c_void_p, _dp, _dp]
    lib.clr_sharded_predict_terms.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, C.c_int, C.c_void_p, _dp, _dp]
    lib.clr_batch_predict_cov.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
    lib.clr_sharded_predict_cov.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
    lib.clr_batch_sample_conditional.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, C.c_int, _dp, C.c_double, C.c_double, _dp, _ip]
    lib.clr_sharded_sample_conditional.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, C.c_int, _dp, C.c_double, C.c_double, _dp, _ip]
    lib.clr_batch_set_conditional_tile.argtypes = [C.c_void_p, C.c_int]
    lib.clr_sharded_set_conditional_tile.argtypes = [C.c_void_p, C.c_int]
    lib.clr_batch_information.argtypes = [C.c_void_p, C.c_int, _dp, _ip]
    lib.clr_sharded_information.argtypes = [C.c_void_p, C.c_int, _dp, _ip]
    lib.clr_batch_set_information_tile.argtypes = [C.c_void_p, C.c_int]
    lib.clr_sharded_set_information_tile.argtypes = [C.c_void_p, C.c_int]
    lib.clr_gram_solve.argtypes = [C.c_int, C.c_int, _dp, _dp, C.c_double] + [_dp] * 4 + [_ip]
    lib.clr_kernel_create.argtypes = [C.c_int, _ip, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    lib.clr_kernel_destroy.argtypes = [C.c_void_p]
    lib.clr_kernel_destroy.restype = None
    lib.clr_kernel_coefficients.argtypes = [C.c_void_p, C.c_int] + [_dp] * 8 + [_ip]
    lib.clr_kernel_jacobian.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _ip]
    lib.clr_batch_set_kernel.argtypes = [C.c_void_p, C.c_void_p]
    lib.clr_batch_set_parameters.argtypes = [C.c_void_p, _dp]
    lib.clr_batch_get_parameter_status.argtypes = [C.c_void_p, _ip]
    lib.clr_batch_evaluate_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long] + [C.c_void_p] * 4
    lib.clr_batch_grad_params.argtypes = [C.c_void_p, _dp, _dp, _ip, C.c_int]
    lib.clr_batch_get_coefficients.argtypes = [C.c_void_p] + [_dp] * 7
    lib.clr_sharded_set_kernel.argtypes = [C.c_void_p, C.c_void_p]
    lib.clr_sharded_evaluate_params.argtypes = [C.c_void_p, _dp, _dp, C.c_long, _dp, _dp, _dp, _ip]
    lib.clr_sharded_grad_params.argtypes = [C.c_void_p, _dp, _dp, _ip, C.c_int]
    lib.clr_sharded_get_coefficients.argtypes = [C.c_void_p] + [_dp] * 7
    lib.clr_device_info.argtypes = [C.c_char_p, C.c_size_t, _ip, C.POINTER(C.c_size_t)]
    lib.clr_set_device.argtypes = [C.c_int]
    _lib = lib
    return lib


def _check(status):
    if status == CLR_OK:
        return
    lib = _load()
    msg = lib.clr_status_string(status).decode()
    detail = lib.clr_last_error().decode()
    raise RuntimeError(msg + (": " + detail if detail else ""))


def set_option(key, value=None):
    """A tuning / cross-check switch of the library (``clr_set_option``, include/celerite_hip.h lists the keys);
    ``value=None`` removes it.  Environment variables of the same names count only under ``CLR_ALLOW_ENV=1``."""
    lib = _load()
    lib.clr_set_option.argtypes = [C.c_char_p, C.c_char_p]
    _check(lib.clr_set_option(key.encode(), None if value is None else str(value).encode()))


def get_option(key):
    lib = _load()
    lib.clr_get_option.argtypes = [C.c_char_p]
    lib.clr_get_option.restype = C.c_char_p
    v = lib.clr_get_option(key.encode())
    return None if v is None else v.decode()


class option(object):
    """``with batch.option("CLR_GRAD_SEQUENTIAL", 1): ...`` -- the switch is removed (or restored) on exit."""

    def __init__(self, key, value="1"):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = get_option(self.key)
        set_option(self.key, self.value)
        return self

    def __exit__(self, *exc):
        set_option(self.key, self.old)
        return False


def device_count():
    return int(_load().clr_device_count())


def measure_fp64(waves_per_simd=2, iters=20000, device=None):
    """``(tflops, clock_mhz, cycles_per_fma)``: the fp64 FMA rate the device's vector ALUs sustain under full load, the
    shader clock during it and the SIMD cycles per issued FMA (``clr_device_measure_fp64``; a roofline measurement).
    ``device``: the calling thread's current device is switched to it first (default: left as it is)."""
    lib = _load()
    if device is not None:
        _check(lib.clr_set_device(int(device)))
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    lib.clr_device_measure_fp64.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 3
    _check(lib.clr_device_measure_fp64(int(waves_per_simd), int(iters), C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def device_synchronize():
    _check(_load().clr_device_synchronize())


def device_info():
    lib = _load()
    name = C.create_string_buffer(256)
    cus = C.c_int()
    mem = C.c_size_t()
    _check(lib.clr_device_info(name, 256, C.byref(cus), C.byref(mem)))
    return dict(name=name.value.decode(), compute_units=cus.value, hbm_bytes=mem.value)


def device_memory():
    """``(free_bytes, total_bytes)`` of the current device's HBM (``clr_device_memory``)."""
    f, t = C.c_size_t(), C.c_size_t()
    _check(_load().clr_device_memory(C.byref(f), C.byref(t)))
    return f.value, t.value


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _mean_arg(mu, B):
    """``(array, stride)`` of a constant mean for ``clr_*_set_mean``: a scalar (stride 0), ``(B,)`` (stride 1) or
    ``None`` (no mean)."""
    if mu is None:
        return None, 0
    m = np.asarray(mu, dtype=np.float64)
    if m.ndim == 0:
        return np.ascontiguousarray(m.reshape(1)), 0
    if m.shape != (B,):
        raise ValueError("dimension mismatch")
    return np.ascontiguousarray(m), 1


def _lengths_arg(lengths, B, N):
    """Per-problem series lengths for ``clr_*_set_series_ragged``: ``None`` (every problem has ``N`` samples) or ``B``
    integers in ``[1, N]``, returned as a contiguous ``int32`` array.  Checked without a device: a wrong shape is
    ``ValueError("dimension mismatch")``, a non-integral or out-of-range entry a ``ValueError`` that names it."""
    if lengths is None:
        return None
    a = np.asarray(lengths)
    if a.shape != (B,):
        raise ValueError("dimension mismatch")
    if a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError("lengths must be integers")
    if np.issubdtype(a.dtype, np.floating):
        if not np.all(np.isfinite(a)) or np.any(a != np.floor(a)):
            raise ValueError("lengths must be integers")
    bad = np.flatnonzero((a < 1) | (a > N))
    if bad.size:
        raise ValueError("length %s of problem %d is outside [1, N = %d]" % (a[bad[0]], bad[0], N))
    return np.ascontiguousarray(a, dtype=np.int32)


MAX_MEAN_BASIS = 16      # CLR_MAX_MEAN_BASIS of include/celerite_hip.h


def _basis_arg(Phi, B, N):
    """``(array, stride, K)`` of a linear mean's basis for ``clr_*_set_mean_basis``: ``(K, N)`` shared by all problems
    (stride 0) or ``(B, K, N)`` (stride ``K * N``), ``1 <= K <= MAX_MEAN_BASIS``; ``None``: ``(None, 0, 0)`` (no linear
    mean)."""
    if Phi is None:
        return None, 0, 0
    a = np.ascontiguousarray(Phi, dtype=np.float64)
    if a.ndim == 2 and a.shape[1] == N:
        stride = 0
    elif a.ndim == 3 and a.shape[0] == B and a.shape[2] == N:
        stride = a.shape[1] * N
    else:
        raise ValueError("dimension mismatch")
    K = a.shape[-2]
    if not 1 <= K <= MAX_MEAN_BASIS:
        raise ValueError("dimension mismatch: a linear mean has 1..%d basis functions" % MAX_MEAN_BASIS)
    return a, stride, K


def _weights_arg(w, B, K):
    """The weights of a linear mean as a contiguous ``(B, K)`` array: ``(B, K)``, or ``(K,)`` for all problems."""
    a = np.asarray(w, dtype=np.float64)
    if K < 1 or a.shape not in ((K,), (B, K)):
        raise ValueError("dimension mismatch")
    return np.ascontiguousarray(np.broadcast_to(a, (B, K)))


MAX_NOISE_BASIS = 16     # CLR_MAX_NOISE_BASIS of include/celerite_hip.h


def _noise_basis_arg(Psi, B, N, lengths=None):
    """:func:`_basis_arg` for a linear noise model's basis (``clr_*_set_noise_basis``; the same shapes and limit), with
    the entries checked: all finite -- with per-problem ``lengths`` in force, within each problem's length (of a shared
    basis: the longest problem's), for the rest of a row is never looked at."""
    a, stride, K = _basis_arg(Psi, B, N)
    if a is None:
        return a, stride, K
    if lengths is None:
        ok = np.all(np.isfinite(a))
    else:
        lens = np.asarray(lengths)
        live = np.arange(N) < (lens[:, None, None] if a.ndim == 3 else lens.max())
        ok = np.all(np.isfinite(a) | ~live)
    if not ok:
        raise ValueError("a non-finite noise basis entry")
    return a, stride, K


def _noise_weights_arg(s, B, K):
    """:func:`_weights_arg` for the weights of a linear noise model, which must be finite."""
    if K < 1:
        raise ValueError("dimension mismatch: no noise basis is set (set_noise_basis)")
    a = _weights_arg(s, B, K)
    if not np.all(np.isfinite(a)):
        raise ValueError("a non-finite noise weight")
    return a


MAX_AMPLITUDE_BASIS = 16     # CLR_MAX_AMPLITUDE_BASIS of include/celerite_hip.h


def _amplitude_basis_arg(Gamma, B, N, lengths=None):
    """:func:`_noise_basis_arg` for the basis of a per-sample amplitude model (``clr_*_set_amplitude_basis``): the same
    shapes, the limit ``MAX_AMPLITUDE_BASIS``, and the same rule for the entries -- all finite, with per-problem
    ``lengths`` in force within each problem's length (of a shared basis: the longest problem's)."""
    try:
        return _noise_basis_arg(Gamma, B, N, lengths)
    except ValueError as e:
        raise ValueError(str(e).replace("noise basis", "amplitude basis").replace("a linear mean", "an amplitude model"))


def _amplitudes_arg(a, B, K):
    """:func:`_weights_arg` for the amplitudes of an amplitude model, which must be finite."""
    if K < 1:
        raise ValueError("dimension mismatch: no amplitude basis is set (set_amplitude_basis)")
    a = _weights_arg(a, B, K)
    if not np.all(np.isfinite(a)):
        raise ValueError("a non-finite amplitude")
    return a


MeanFit = collections.namedtuple("MeanFit", ["weights", "covariance", "gram", "quad", "logdet_gram", "loglike",
                                             "loglike_marginal", "status"])
MeanFit.__doc__ = """The generalised-least-squares fit of a linear mean's weights (``fit_mean_weights``): ``weights[B, K]``,
their ``covariance[B, K, K]`` = ``G^-1``, the bordered Gram matrix ``gram[B, K + 1, K + 1]`` = ``[[G, d], [d^T, q]]``, the
profiled quadratic form ``quad[B]``, ``logdet_gram[B]`` = ``log det G``, the profiled log-likelihood ``loglike[B]``, the
log-likelihood marginalised over the weights under a flat prior ``loglike_marginal[B]``, and ``status[B]``."""


def _check_min_pivot(min_pivot):
    p = float(min_pivot)
    if not (np.isfinite(p) and 0.0 <= p < 1.0):
        raise ValueError("min_pivot must be finite and lie in [0, 1)")
    return p


def gram_solve(gram, w0=None, min_pivot=1e-10):
    """The small solve of :meth:`BatchedGP.fit_mean_weights` on the host (``clr_gram_solve``; no GPU): from bordered Gram
    matrices ``gram[n, K + 1, K + 1]`` = ``[[G, d], [d^T, q]]`` and the weights ``w0[n, K]`` the residual was formed at
    (``None``: zeros), ``(weights, covariance, quad, logdet_gram, status)`` -- the routine the device runs per problem,
    the same bits."""
    g = np.ascontiguousarray(gram, dtype=np.float64)
    if g.ndim == 2:
        g = g[None]
    if g.ndim != 3 or g.shape[1] != g.shape[2] or not 2 <= g.shape[1] <= MAX_MEAN_BASIS + 1:
        raise ValueError("dimension mismatch")
    n, K = g.shape[0], g.shape[1] - 1
    p = _check_min_pivot(min_pivot)
    w = np.zeros((n, K)) if w0 is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w0, dtype=np.float64), (n, K)))
    w_hat, cov, quad, ld = np.empty((n, K)), np.empty((n, K, K)), np.empty(n), np.empty(n)
    st = np.empty(n, dtype=np.int32)
    _check(_load().clr_gram_solve(n, K, _ptr(g), _ptr(w), p, _ptr(w_hat), _ptr(cov), _ptr(quad), _ptr(ld),
                                  st.ctypes.data_as(_ip)))
    return w_hat, cov, quad, ld, st


def _mean_fit(w_hat, cov, gram, quad, ld_gram, status, logdet_K, N):
    """The :class:`MeanFit` of the library's outputs and ``log det K`` of the evaluation in force:
    ``loglike = -1/2 (quad + log det K + N log 2 pi)``, ``loglike_marginal = loglike - 1/2 log det G + 1/2 K log 2 pi``
    (refused problems: NaN, through their NaN ``quad``)."""
    K = w_hat.shape[1]
    log2pi = np.log(2.0 * np.pi)
    ll = -0.5 * (quad + logdet_K + N * log2pi)
    return MeanFit(w_hat, cov, gram, quad, ld_gram, ll, ll - 0.5 * ld_gram + 0.5 * K * log2pi, status)


LeaveOneOut = collections.namedtuple("LeaveOneOut", ["residual", "variance", "logpdf", "kinv_diag", "alpha", "status"])
LeaveOneOut.__doc__ = """The leave-one-out predictive distribution of every sample (``leave_one_out``): ``residual[B, N]`` =
``y_n - mu_-n`` = ``alpha_n / c_n``, ``variance[B, N]`` = ``sigma^2_-n`` = ``1 / c_n``, ``logpdf[B]`` = ``sum_n log p(y_n |
y_-n)``, ``kinv_diag[B, N]`` = ``c`` = ``diag(K^-1)``, ``alpha[B, N]`` = ``K^-1 r`` and ``status[B]``."""


def _loo_args(c, alpha, logpdf, st):
    """The four output pointers of ``clr_*_leave_one_out``: ``None`` stays a null pointer (not asked for)."""
    return [None if a is None else _ptr(a) for a in (c, alpha, logpdf)] + [None if st is None else st.ctypes.data_as(_ip)]


def _predict_method(method):
    """The ``method`` argument of ``predict``: checked before anything touches the device."""
    if method not in ("solve", "recurrence"):
        raise ValueError("predict: method is 'solve' or 'recurrence', not %r" % (method,))


def leave_one_out_from(kinv_diag, alpha):
    """``(residual, variance, logpdf)`` of the leave-one-out predictive distribution from ``c = diag(K^-1)`` and
    ``alpha = K^-1 r``, both ``(N,)`` or ``(B, N)`` (no GPU):

        ``residual_n = y_n - mu_-n = alpha_n / c_n``, ``variance_n = sigma^2_-n = 1 / c_n``,
        ``logpdf = sum_n -1/2 log(2 pi / c_n) - 1/2 alpha_n^2 / c_n``.

    The sum runs in the order of the device's reduction (``clr_batch_leave_one_out``): 256 partial sums over the samples
    ``i, i + 256, ...`` in order, then a tree over the 256 -- host and device agree to the rounding of ``log``."""
    c = np.asarray(kinv_diag, dtype=np.float64)
    a = np.asarray(alpha, dtype=np.float64)
    if c.shape != a.shape or c.ndim not in (1, 2) or c.shape[-1] < 1:
        raise ValueError("dimension mismatch")
    single = c.ndim == 1
    c2, a2 = np.atleast_2d(c), np.atleast_2d(a)
    B, N = c2.shape
    terms = -0.5 * np.log(6.283185307179586 / c2) - 0.5 * a2 * a2 / c2
    rows = (N + 255) // 256
    padded = np.zeros((B, rows * 256))
    padded[:, :N] = terms
    padded = padded.reshape(B, rows, 256)
    part = np.zeros((B, 256))
    for r in range(rows):
        part = part + padded[:, r, :]
    w = 128
    while w > 0:
        part[:, :w] = part[:, :w] + part[:, w:2 * w]
        w >>= 1
    logpdf = part[:, 0].copy()
    residual, variance = a / c, 1.0 / c
    return (residual, variance, logpdf[0]) if single else (residual, variance, logpdf)


class OneStepAhead(collections.namedtuple("OneStepAhead", ["innovation", "variance", "status"])):
    """The one-step-ahead residuals of every sample (``one_step_ahead``): ``innovation[B, N]`` (``[B, nrhs, N]`` for a 3-D
    ``b``) = ``z = L^-1 b`` with ``K = L diag(D) L^T``, ``variance[B, N]`` = ``D`` and ``status[B]``.  For the residual
    ``r``: ``E[y_n | y_<n] = y_n - z_n`` with variance ``D_n``.  Rows of problems whose status is not 0 are NaN."""
    __slots__ = ()

    def _var(self):
        return self.variance if self.innovation.ndim == 2 else self.variance[:, None, :]

    @property
    def standardized(self):
        """``innovation / sqrt(variance)``: white and standard normal under the model."""
        return self.innovation / np.sqrt(self._var())

    @property
    def log_density(self):
        """``-1/2 (log(2 pi variance) + innovation^2 / variance)`` per sample: ``log p(y_n | y_<n)``; its sum over n is
        the log-likelihood."""
        v = self._var()
        return -0.5 * (np.log(2.0 * np.pi * v) + self.innovation * self.innovation / v)


def _one_step_ahead(plan, name, check, b):
    """``one_step_ahead`` of both plan classes: the arguments are checked before the library is touched."""
    if b is None:
        nrhs, shape, bp = 1, (plan.B, plan.N), None
    else:
        b = _f64(b)
        if b.ndim not in (2, 3) or b.shape[0] != plan.B or b.shape[-1] != plan.N:
            raise ValueError("dimension mismatch")
        nrhs, shape, bp = (1 if b.ndim == 2 else b.shape[1]), b.shape, _ptr(b)
    z, D, st = np.empty(shape), np.empty((plan.B, plan.N)), np.empty(plan.B, dtype=np.int32)
    check(getattr(_load(), name)(plan._h, int(nrhs), bp, _ptr(z), _ptr(D), st.ctypes.data_as(_ip)))
    return OneStepAhead(z, D, st)


class Periodogram(collections.namedtuple("Periodogram", ["power", "coef", "cov", "status", "gram"])):
    """The periodogram under a plan's covariance (``periodogram``): per problem and trial frequency ``power[B, F]``, the
    gain in maximised log-likelihood of the sinusoid; ``coef[B, F, K]`` the fitted amplitudes of ``(cos, sin)`` --
    ``(1, cos, sin)`` with the offset --; ``cov[B, F, K, K]`` their covariance ``G^-1``; ``status[B, F]``; ``gram[B, F, K + 1,
    K + 1]`` = ``[[G, d], [d^T, q]]`` with ``return_gram=True``, else ``None``.  Refused entries are NaN."""
    __slots__ = ()

    @property
    def amplitude(self):
        """``hypot`` of the (cos, sin) coefficients: the amplitude of ``A cos(w tau) + B sin(w tau)``."""
        return np.hypot(self.coef[..., -2], self.coef[..., -1])

    @property
    def phase(self):
        """``phi`` of ``amplitude * cos(w tau + phi)`` = ``A cos(w tau) + B sin(w tau)``: ``arctan2(-B, A)``."""
        return np.arctan2(-self.coef[..., -1], self.coef[..., -2])


def _periodogram_args(B, omega, offset, t_ref, min_pivot):
    """The arguments of ``periodogram`` of both plan classes, checked before the library is touched:
    ``(omega, stride, F, t_ref, min_pivot, K)``."""
    omega = _f64(omega)
    if omega.ndim == 1:
        stride = 0
    elif omega.ndim == 2 and omega.shape[0] == B:
        stride = omega.shape[1]
    else:
        raise ValueError("dimension mismatch")
    if not np.all(np.isfinite(omega)):
        raise ValueError("the frequencies must be finite")
    t_ref = float(t_ref)
    if not np.isfinite(t_ref):
        raise ValueError("t_ref must be finite")
    return omega, stride, omega.shape[-1], t_ref, _check_min_pivot(min_pivot), (3 if offset else 2)


def _periodogram(plan, name, check, omega, offset, t_ref, min_pivot, return_gram):
    """``periodogram`` of both plan classes."""
    omega, stride, F, t_ref, p, K = _periodogram_args(plan.B, omega, offset, t_ref, min_pivot)
    B = plan.B
    power, coef, cov = np.empty((B, F)), np.empty((B, F, K)), np.empty((B, F, K, K))
    gram = np.empty((B, F, K + 1, K + 1)) if return_gram else None
    st = np.empty((B, F), dtype=np.int32)
    check(getattr(_load(), name)(plan._h, int(F), _ptr(omega), stride, t_ref, 1 if offset else 0, p, _ptr(power), _ptr(coef),
                                 _ptr(cov), None if gram is None else _ptr(gram), st.ctypes.data_as(_ip)))
    return Periodogram(power, coef, cov, st, gram)


def _forecast(plan, name, check, xs, return_var, mean_basis):
    """``forecast`` of both plan classes: the arguments are checked before the library is touched."""
    xs = _f64(xs)
    if xs.ndim == 1:
        stride = 0
    elif xs.ndim == 2 and xs.shape[0] == plan.B:
        stride = xs.shape[1]
    else:
        raise ValueError("dimension mismatch")
    M = xs.shape[-1]
    model = _linear_mean_at(plan, mean_basis, M)
    mean = np.empty((plan.B, M))
    var = np.empty((plan.B, M)) if return_var else None
    check(getattr(_load(), name)(plan._h, int(M), _ptr(xs), stride, _ptr(mean), None if var is None else _ptr(var)))
    if model is not None:
        mean = model + mean
    return (mean, var) if return_var else mean


def _term_groups(groups, T):
    """``groups`` of ``predict_terms`` as a ``(G, T)`` array of 0 / 1 bytes: ``None`` -- one group per coefficient term
    --, a sequence of sequences of term indices, or a ``(G, T)`` boolean array."""
    if groups is None:
        return np.ascontiguousarray(np.eye(T, dtype=np.uint8))
    if isinstance(groups, np.ndarray) and groups.dtype == np.bool_:
        if groups.ndim != 2 or groups.shape[0] < 1 or groups.shape[1] != T:
            raise ValueError("groups as a boolean array is (G, %d) with G >= 1: one column per coefficient term" % T)
        return np.ascontiguousarray(groups, dtype=np.uint8)
    try:
        rows = [list(g) for g in groups]
    except TypeError:
        raise ValueError("groups is None, a sequence of sequences of term indices, or a (G, T) boolean array")
    if not rows:
        raise ValueError("groups is empty: at least one group (an empty group is fine)")
    out = np.zeros((len(rows), T), dtype=np.uint8)
    for g, row in enumerate(rows):
        for k in row:
            if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
                raise ValueError("group %d: term indices are integers (a boolean mask goes in as a (G, T) boolean array)" % g)
            if not 0 <= k < T:
                raise ValueError("group %d: term index %d out of range (the kernel has %d coefficient terms)" % (g, k, T))
            if out[g, k]:
                raise ValueError("group %d: term index %d is repeated" % (g, k))
            out[g, k] = 1
    return out


def _predict_terms(plan, name, check, xs, groups, return_var):
    """``predict_terms`` of both plan classes: the arguments are checked before the library is touched."""
    xs = _f64(xs)
    if xs.ndim == 1:
        stride = 0
    elif xs.ndim == 2 and xs.shape[0] == plan.B:
        stride = xs.shape[1]
    else:
        raise ValueError("dimension mismatch")
    M = xs.shape[-1]
    masks = _term_groups(groups, plan.J_real + plan.J_comp)
    G = masks.shape[0]
    mean = np.empty((plan.B, G, M))
    var = np.empty((plan.B, G, M)) if return_var else None
    check(getattr(_load(), name)(plan._h, int(M), _ptr(xs), stride, int(G), masks.ctypes.data_as(C.c_void_p), _ptr(mean),
                                 None if var is None else _ptr(var)))
    return (mean, var) if return_var else mean


def _points_arg(plan, xs):
    xs = _f64(xs)
    if xs.ndim == 1:
        return xs, 0
    if xs.ndim == 2 and xs.shape[0] == plan.B:
        return xs, xs.shape[1]
    raise ValueError("dimension mismatch")


def _predict_cov(plan, name, check, xs):
    """``predict_cov`` of both plan classes: the arguments are checked before the library is touched."""
    xs, stride = _points_arg(plan, xs)
    M = xs.shape[-1]
    cov = np.empty((plan.B, M, M))
    check(getattr(_load(), name)(plan._h, int(M), _ptr(xs), stride, _ptr(cov)))
    return cov


def _predict_any_order(plan, xs, mean_basis):
    """``plan.predict(xs, mean_basis=mean_basis)`` for points in any order: ``predict`` walks its points as the reference
    does, ascending, so unsorted ones go in sorted (ties in the given order) and the means come back in the caller's order."""
    if xs.shape[-1] < 2 or not np.any(np.diff(xs, axis=-1) < 0):
        return plan.predict(xs, mean_basis=mean_basis)
    order = np.argsort(xs, axis=-1, kind="stable")
    basis = None
    if mean_basis is not None:
        a = _f64(mean_basis)
        if xs.ndim == 1:
            basis = np.ascontiguousarray(a[..., order])
        else:
            a = np.broadcast_to(a, (plan.B,) + a.shape[-2:]) if a.ndim in (2, 3) else a
            basis = np.ascontiguousarray(np.take_along_axis(a, order[:, None, :], axis=-1))
    got = plan.predict(np.ascontiguousarray(np.take_along_axis(xs, order, axis=-1)), mean_basis=basis)
    mean = np.empty_like(got)
    np.put_along_axis(mean, np.broadcast_to(order, got.shape), got, axis=-1)
    return mean


def _sample_conditional(plan, name, check, xs, size, regularize, min_pivot, mean_basis, random, normals, return_status):
    """``sample_conditional`` of both plan classes: the arguments are checked before the library is touched."""
    xs, stride = _points_arg(plan, xs)
    M = xs.shape[-1]
    if size is not None and (isinstance(size, (bool, np.bool_)) or int(size) != size or int(size) < 1):
        raise ValueError("size is None or an integer >= 1")
    n = 1 if size is None else int(size)
    p = _check_min_pivot(min_pivot)
    reg = float(regularize)
    if not (np.isfinite(reg) and reg >= 0.0):
        raise ValueError("regularize must be finite and not negative")
    if normals is not None:
        z = _f64(normals)
        if z.shape != ((plan.B, M) if size is None else (plan.B, n, M)):
            raise ValueError("dimension mismatch")
    else:
        rng = np.random if random is None else random
        z = _f64(rng.standard_normal((plan.B, M) if size is None else (plan.B, n, M)))
    _linear_mean_at(plan, mean_basis, M)      # (its checks, before the device works)
    draws = np.empty((plan.B, n, M))
    st = np.empty(plan.B, dtype=np.int32)
    check(getattr(_load(), name)(plan._h, int(M), _ptr(xs), stride, n, _ptr(z), reg, p, _ptr(draws), st.ctypes.data_as(_ip)))
    out = _predict_any_order(plan, xs, mean_basis)[:, None, :] + draws
    if size is None:
        out = out[:, 0, :]
    return (out, st) if return_status else out


def _exclusive_means(mean, mean_weights):
    if mean is not None and mean_weights is not None:
        raise ValueError("mean and mean_weights are mutually exclusive: a plan has a constant mean or a linear one")


def _linear_mean_at(plan, mean_basis, M):
    """``sum_k w[b, k] basis_k`` at ``M`` prediction points, ``(B, M)``, added up in the order of the device's residual
    (``k = 0, 1, ...``); ``None`` when the plan has no linear mean."""
    K = getattr(plan, "_mean_K", 0)
    if not K:
        if mean_basis is not None:
            raise ValueError("mean_basis without a linear mean (set_mean_basis)")
        return None
    if mean_basis is None:
        raise ValueError("a linear mean is in force: predict needs mean_basis, the basis at the prediction points")
    a, _, Kb = _basis_arg(mean_basis, plan.B, M)
    if Kb != K:
        raise ValueError("dimension mismatch")
    a = np.broadcast_to(a, (plan.B, K, M))
    w = plan._mean_w
    m = w[:, 0, None] * a[:, 0]
    for k in range(1, K):
        m = m + w[:, k, None] * a[:, k]
    return m


class BatchedGP(object):
    """Device-resident plan for B problems of N samples and a fixed kernel shape.

    Args:
        B, N: batch size and samples per series.
        J_real, J_comp: number of real / complex celerite terms
            (width ``J = J_real + 2 J_comp``: 1..8 run the chunked scan with one lane
            per (problem, chunk), 9..64 one wave per (problem, chunk)).
        device: GPU index (one process per GPU; shard the batch across ranks).
    """

    def __init__(self, B, N, J_real, J_comp, device=0):
        lib = _load()
        self.B, self.N, self.J_real, self.J_comp = int(B), int(N), int(J_real), int(J_comp)
        self.J = self.J_real + 2 * self.J_comp
        self._h = lib.clr_batch_create(self.B, self.N, self.J_real, self.J_comp, int(device))
        if not self._h:
            raise RuntimeError("clr_batch_create failed: " + lib.clr_last_error().decode())
        self._h = C.c_void_p(self._h)
        self._evaluate_fn = None
        self._mean_K, self._mean_w = 0, None

    def close(self):
        if getattr(self, "_h", None):
            _load().clr_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- inputs -------------------------------------------------------------
    def set_series(self, t, diag, y, lengths=None):
        """``t``, ``diag`` (= yerr**2), ``y``: each ``(B, N)`` or ``(N,)`` for one
        series shared by all problems.  ``t`` must be sorted along the last axis
        (checked: GP.compute does the same, celerite.py:126-129).  A mean set by
        :meth:`set_mean` stays in force and is subtracted from the new ``y`` on
        the device; without one ``y`` is taken as it is (mean zero).

        ``lengths`` (``(B,)`` integers in ``[1, N]``; ``clr_batch_set_series_ragged``): problem ``b`` is the first
        ``lengths[b]`` samples of its rows, which must then be ``(B, N)`` each.  The rest of a row is never read -- it
        may be NaN or unsorted -- and every result is that of the problem's own samples.  Narrow plans (widths 1..8)
        evaluate and differentiate such a batch; the materialised factor and its consumers (:meth:`solve`,
        :meth:`predict`, ...) refuse it.  Without ``lengths`` the plan is uniform again."""
        lens = _lengths_arg(lengths, self.B, self.N)
        arrs, strides = [], []
        for a in (t, diag, y):
            a = _f64(a)
            if a.shape == (self.N,):
                strides.append(0)
            elif a.shape == (self.B, self.N):
                strides.append(self.N)
            else:
                raise ValueError("dimension mismatch")
            arrs.append(a)
        self._series_lengths = lens      # (set_noise_basis: the part of a row its finiteness check covers)
        lib = _load()
        if lens is None:
            _check(lib.clr_batch_set_series(self._h, _ptr(arrs[0]), strides[0], _ptr(arrs[1]),
                                            strides[1], _ptr(arrs[2]), strides[2]))
        else:
            lib.clr_batch_set_series_ragged.argtypes = [C.c_void_p, _dp, C.c_long, _dp, C.c_long, _dp, C.c_long, _ip]
            _check(lib.clr_batch_set_series_ragged(self._h, _ptr(arrs[0]), strides[0], _ptr(arrs[1]), strides[1],
                                                   _ptr(arrs[2]), strides[2], lens.ctypes.data_as(_ip)))
        # sortedness from the device-side scan of the uploaded t (np.diff over 0.8 GB of times costs more than the
        # whole transfer): an unsorted batch is dropped again
        dtmin = C.c_double()
        lib.clr_batch_get_series_order.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _check(lib.clr_batch_get_series_order(self._h, C.byref(dtmin)))
        if dtmin.value < 0.0:
            lib.clr_batch_clear_series.argtypes = [C.c_void_p]
            _check(lib.clr_batch_clear_series(self._h))
            raise ValueError("the input coordinates must be sorted")

    @property
    def lengths(self):
        """The series lengths in force, ``(B,)`` (``N`` for every problem of a uniform plan; a series must be set)."""
        out = np.empty(self.B, dtype=np.int32)
        lib = _load()
        lib.clr_batch_get_lengths.argtypes = [C.c_void_p, _ip]
        _check(lib.clr_batch_get_lengths(self._h, out.ctypes.data_as(_ip)))
        out.flags.writeable = False
        return out

    def set_mean(self, mu):
        """A constant mean per problem (``clr_batch_set_mean``): a scalar for all problems, ``(B,)``, or ``None`` to
        remove it.  Every route that reads ``y`` -- the evaluation, :meth:`solve` of ``None``, :meth:`predict`, the
        gradient -- then sees the residual ``y - mu_b``, formed on the device from the uploaded ``y``."""
        m, stride = _mean_arg(mu, self.B)
        _check(_load().clr_batch_set_mean(self._h, None if m is None else _ptr(m), stride))

    def set_mean_basis(self, Phi):
        """A mean that is linear in its parameters, ``mean_b(t_n) = sum_k w[b, k] Phi_k(t_n)``
        (``clr_batch_set_mean_basis``): ``Phi`` is the basis at the plan's times, ``(K, N)`` for all problems or
        ``(B, K, N)``, ``K <= 16`` -- a polynomial trend, per-instrument offsets, a sinusoid of fixed period, a transit
        template.  It is uploaded once and stays on the device; the weights start at zero.  ``None`` removes the linear
        mean.  Not together with :meth:`set_mean` (a constant is the basis function 1)."""
        a, stride, K = _basis_arg(Phi, self.B, self.N)
        self._set_mean_basis(K, a, stride)
        self._mean_K, self._mean_w = K, (np.zeros((self.B, K)) if K else None)

    def _set_mean_basis(self, K, a, stride):
        _check(_load().clr_batch_set_mean_basis(self._h, K, None if a is None else _ptr(a), stride))

    def set_mean_weights(self, w):
        """The weights of the linear mean, ``(B, K)`` or ``(K,)`` for all problems (``clr_batch_set_mean_weights``):
        every route that reads ``y`` then sees ``y - sum_k w[b, k] Phi_k``, formed on the device from the uploaded ``y``
        -- B x K numbers go up per optimiser step, not a new ``y``.  The factor of a materialising run stays valid."""
        a = _weights_arg(w, self.B, self._mean_K)
        self._set_mean_weights(a)
        self._mean_w = a

    def _set_mean_weights(self, a):
        _check(_load().clr_batch_set_mean_weights(self._h, _ptr(a)))

    def grad_mean_weights(self):
        """``(dw[B, K], status[B])``: ``d loglike_b / d w[b, k] = Phi_k^T K_b^-1 r_b`` at the weights in force, from the
        factor of the last materialising run (``clr_batch_grad_mean_weights``): the batched solve of the residual and
        one projection pass on the device.  A problem whose status is not 0 has a row of zeros."""
        dw, st = np.empty((self.B, self._mean_K)), np.empty(self.B, dtype=np.int32)
        self._grad_mean_weights(dw, st)
        return dw, st

    def _grad_mean_weights(self, dw, st):
        if not self._mean_K:
            raise RuntimeError("no basis is set: call set_mean_basis first")
        _check(_load().clr_batch_grad_mean_weights(self._h, _ptr(dw), st.ctypes.data_as(_ip)))

    def fit_mean_weights(self, apply=False, min_pivot=1e-10):
        """The weights of the linear mean that maximise every problem's log-likelihood at the coefficients in force, as a
        :class:`MeanFit` (``clr_batch_fit_mean_weights``).  The log-likelihood is exactly quadratic in the weights: with
        ``r`` the residual at the weights in force, ``G = Phi^T K^-1 Phi`` and ``d = Phi^T K^-1 r``, the optimum is
        ``w + G^-1 d`` -- one generalised-least-squares solve from the factor of the last materialising run, its right-hand
        sides formed on the device from the resident basis.  No optimiser step over the weights is ever needed, and
        ``covariance`` = ``G^-1`` and the marginal likelihood come with it.  ``min_pivot``: a problem whose scaled Gram
        matrix has a Cholesky pivot below it (a rank-deficient basis) is refused -- status 2, its weights unchanged, NaN
        elsewhere but in ``gram``.  ``apply=True``: :meth:`set_mean_weights` of the result (refused rows keep their
        weights); the next evaluation's ``loglike`` is then ``MeanFit.loglike``."""
        if not self._mean_K:
            raise RuntimeError("no basis is set: call set_mean_basis first")
        p = _check_min_pivot(min_pivot)
        B, K = self.B, self._mean_K
        w, cov, gram = np.empty((B, K)), np.empty((B, K, K)), np.empty((B, K + 1, K + 1))
        quad, ld, st = np.empty(B), np.empty(B), np.empty(B, dtype=np.int32)
        self._fit_mean_weights(p, w, cov, gram, quad, ld, st)
        fit = _mean_fit(w, cov, gram, quad, ld, st, self.results()[1], self.N)
        if apply:
            self.set_mean_weights(w)
        return fit

    def _fit_mean_weights(self, p, w, cov, gram, quad, ld, st):
        _check(_load().clr_batch_fit_mean_weights(self._h, p, _ptr(w), _ptr(cov), _ptr(gram), _ptr(quad), _ptr(ld),
                                                  st.ctypes.data_as(_ip)))

    def set_mean_fit_tile(self, rhs=0):
        """Right-hand sides per tile of :meth:`fit_mean_weights` (``clr_batch_set_mean_fit_tile``); 0: automatic.  The
        results do not depend on it."""
        _check(_load().clr_batch_set_mean_fit_tile(self._h, int(rhs)))

    def mean_fit_ms(self):
        """``(solve_ms, gram_ms, small_ms)``: device time of the three parts of the last :meth:`fit_mean_weights`."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(_load().clr_batch_get_mean_fit_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def mean_project_ms(self):
        """Device time of the projection pass of the last :meth:`grad_mean_weights` (its solve: :meth:`solve_device_ms`)."""
        ms = C.c_double()
        _check(_load().clr_batch_get_mean_project_ms(self._h, C.byref(ms)))
        return ms.value

    def set_noise_basis(self, Psi):
        """A noise model that is linear in its parameters (``clr_batch_set_noise_basis``): the variances every route
        reads become

            ``diag_eff[b, n] = diag[b, n] + sum_k s[b, k] Psi_k[b, n]``

        with the plan's scalar ``jitter`` added on top as before.  ``Psi`` is the basis at the plan's samples, ``(K, N)``
        for all problems or ``(B, K, N)``, ``K <= 16`` -- a jitter per instrument (``diag = sigma^2``, ``Psi_g`` the
        indicator of instrument g, ``s_g`` its jitter squared), an error-bar inflation ``f^2 sigma^2`` (``Psi_0 =
        sigma^2``, ``s_0 = f^2 - 1``), a noise level per observing season.  It is uploaded once and stays on the device;
        the weights start at zero, so the plan is the plain plan until :meth:`set_noise_weights`.  ``None`` removes the
        noise model.  The entries must be finite (with ``lengths=`` in force: within each problem's length) and need be
        nothing else: a variance that comes out non-positive shows in the problem's status."""
        a, stride, K = _noise_basis_arg(Psi, self.B, self.N, getattr(self, "_series_lengths", None))
        self._set_noise_basis(K, a, stride)
        self._noise_K = K

    def _set_noise_basis(self, K, a, stride):
        _check(_load().clr_batch_set_noise_basis(self._h, K, None if a is None else _ptr(a), stride))

    def set_noise_weights(self, s):
        """The weights of the linear noise model, ``(B, K)`` or ``(K,)`` for all problems
        (``clr_batch_set_noise_weights``): every route that reads the diagonal then sees ``diag + (s[b, 0] Psi_0 +
        s[b, 1] Psi_1 + ...)`` -- the bits of that NumPy expression -- formed on the device from the uploaded ``diag``:
        B x K numbers go up per optimiser or sampler step, not a new ``(B, N)`` diagonal through :meth:`set_series`, and
        nothing derived from ``t`` is rebuilt.  The factor of an earlier materialising run is that of the earlier
        variances: materialise again before :meth:`solve`, :meth:`predict`, ... or :meth:`grad_noise_weights`."""
        self._set_noise_weights(_noise_weights_arg(s, self.B, getattr(self, "_noise_K", 0)))

    def _set_noise_weights(self, a):
        _check(_load().clr_batch_set_noise_weights(self._h, _ptr(a)))

    def grad_noise_weights(self):
        """``(ds[B, K], status[B])``: the gradient with respect to the noise weights in force,

            ``d loglike_b / d s[b, k] = 1/2 sum_n Psi_k[b, n] (alpha_n^2 - c_n)``,  ``alpha = K_b^-1 r_b``,  ``c = diag(K_b^-1)``

        (``clr_batch_grad_noise_weights``): :meth:`leave_one_out`'s diagonal recurrence and solve, then one projection
        pass on the device.  It needs a materialising run (``enqueue(materialize=True)``) made AFTER the weights -- and
        the basis and the series -- were set: the factor must be that of the variances in force, and a change of any of
        them since is refused with ``CLR_NOT_COMPUTED`` until the plan is materialised again.  :meth:`leave_one_out`'s
        domain: celerite-only plans of widths 1..64 without ``lengths=``.  A problem whose status is not 0 has a row of
        zeros."""
        K = getattr(self, "_noise_K", 0)
        if not K:
            raise RuntimeError("no noise basis is set: call set_noise_basis first")
        ds, st = np.empty((self.B, K)), np.empty(self.B, dtype=np.int32)
        self._grad_noise_weights(ds, st)
        return ds, st

    def _grad_noise_weights(self, ds, st):
        _check(_load().clr_batch_grad_noise_weights(self._h, _ptr(ds), st.ctypes.data_as(_ip)))

    def noise_project_ms(self):
        """Device time of the projection pass of the last :meth:`grad_noise_weights` (its diagonal and solve:
        :meth:`leave_one_out_ms`)."""
        ms = C.c_double()
        _check(_load().clr_batch_get_noise_project_ms(self._h, C.byref(ms)))
        return ms.value

    def set_amplitude_basis(self, Gamma):
        """A per-sample amplitude model (``clr_batch_set_amplitude_basis``): the same latent process ``f`` seen with
        another amplitude per band,

            ``y_n = s_n f(t_n) + eps_n``,  ``s[b, n] = sum_k a[b, k] Gamma_k[b, n]``

        -- multi-colour photometry of one variable source (``Gamma_k`` the indicator of band k), a radial velocity next
        to an activity indicator, a chromatic amplitude law (``Gamma`` a polynomial in wavelength).  ``Gamma`` is the basis
        at the plan's samples, ``(K, N)`` for all problems or ``(B, K, N)``, ``K <= 16``, uploaded once.  A basis alone
        changes nothing: zero amplitudes are no neutral start, so the plan stays the plain plan until
        :meth:`set_amplitudes`; a new basis drops the amplitudes in force.  ``None`` removes the model and restores the
        plain plan.  The entries must be finite (with ``lengths=`` in force: within each problem's length).  Not together
        with a constant mean (:meth:`set_mean`): a constant in data units is the mean-basis function 1."""
        a, stride, K = _amplitude_basis_arg(Gamma, self.B, self.N, getattr(self, "_series_lengths", None))
        self._set_amplitude_basis(K, a, stride)
        self._amplitude_K = K

    def _set_amplitude_basis(self, K, a, stride):
        _check(_load().clr_batch_set_amplitude_basis(self._h, K, None if a is None else _ptr(a), stride))

    def set_amplitudes(self, a):
        """The amplitudes of the amplitude model, ``(B, K)`` or ``(K,)`` for all problems (``clr_batch_set_amplitudes``).
        With ``S = diag(s)``, ``K_y = S K S + D = S (K + S^-1 D S^-1) S``, so the device rewrites the series every route
        reads -- ``y' = r / s`` and ``d' = d / (s * s)``, ``r`` and ``d`` the residual and the variances in force, the
        bits of those NumPy expressions with ``s = a[:, 0, None] * Gamma[0] + ...`` summed in the order of k -- and
        ``evaluate`` / ``evaluate_parameters`` / ``results`` / the gradient's value report ``logdet = logdet' + (L + L)``,
        ``loglike = loglike' - L``, ``quad = quad'`` with ``L =`` :meth:`log_amplitude_sum`.  B x K numbers go up per step.
        A problem with a zero or non-finite ``s_n`` reports NaN and ``CLR_INVALID_ARGUMENT``.  The factor's consumers run
        on the scaled system: :meth:`predict` and its relatives return the posterior of the LATENT process ``f`` (a band's
        curve is ``a_band * f``), :meth:`solve` is ``K'^-1 b``, :meth:`leave_one_out` is that of the scaled samples.  The
        factor of an earlier materialising run is that of the earlier amplitudes: materialise again before them."""
        self._set_amplitudes(_amplitudes_arg(a, self.B, getattr(self, "_amplitude_K", 0)))

    def _set_amplitudes(self, a):
        _check(_load().clr_batch_set_amplitudes(self._h, _ptr(a)))

    def log_amplitude_sum(self):
        """``L[B] = sum_n log|s[b, n]|`` of the amplitudes in force over each problem's length
        (``clr_batch_get_log_amplitude_sum``); zeros while none are."""
        L = np.empty(self.B)
        self._log_amplitude_sum(L)
        return L

    def _log_amplitude_sum(self, L):
        _check(_load().clr_batch_get_log_amplitude_sum(self._h, _ptr(L)))

    def grad_amplitudes(self):
        """``(da[B, K], status[B])``: the gradient with respect to the amplitudes in force,

            ``d loglike_b / d a[b, k] = sum_n Gamma_k[b, n] (alpha'_n y'_n + d'_n (c'_n - alpha'_n^2) - 1) / s_n``

        with ``alpha' = K'^-1 y'`` and ``c' = diag(K'^-1)`` of the scaled system (``clr_batch_grad_amplitudes``):
        :meth:`grad_noise_weights`' steps and rules -- it needs a materialising run made AFTER the amplitudes, the basis,
        the noise weights and the series were set (``CLR_NOT_COMPUTED`` otherwise), :meth:`leave_one_out`'s domain, and a
        problem whose status is not 0 has a row of zeros."""
        K = getattr(self, "_amplitude_K", 0)
        if not K:
            raise RuntimeError("no amplitude basis is set: call set_amplitude_basis first")
        da, st = np.empty((self.B, K)), np.empty(self.B, dtype=np.int32)
        self._grad_amplitudes(da, st)
        return da, st

    def _grad_amplitudes(self, da, st):
        _check(_load().clr_batch_grad_amplitudes(self._h, _ptr(da), st.ctypes.data_as(_ip)))

    def amplitude_project_ms(self):
        """Device time of the projection pass of the last :meth:`grad_amplitudes` (its diagonal and solve:
        :meth:`leave_one_out_ms`)."""
        ms = C.c_double()
        _check(_load().clr_batch_get_amplitude_project_ms(self._h, C.byref(ms)))
        return ms.value

    def set_coefficients(self, a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter=0.0):
        """Coefficient tables ``(B, J_real)`` / ``(B, J_comp)``; ``jitter`` scalar or ``(B,)``."""
        try:
            blocks = [_f64(a_real, (self.B, self.J_real)), _f64(c_real, (self.B, self.J_real)),
                      _f64(a_comp, (self.B, self.J_comp)), _f64(b_comp, (self.B, self.J_comp)),
                      _f64(c_comp, (self.B, self.J_comp)), _f64(d_comp, (self.B, self.J_comp))]
        except ValueError:
            raise ValueError("dimension mismatch")
        jit = np.ascontiguousarray(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (self.B,)))
        self._last_params = None                           # (tables replace what parameters formed: information_parameters)
        _check(_load().clr_batch_set_coefficients(self._h, _ptr(jit), *[_ptr(b) for b in blocks]))

    def set_general(self, A, U, V):
        """General semiseparable terms (``CholeskySolver.compute``'s ``A, U, V``; cholesky.h:65-72,148-152) for the
        batch: ``A`` ``(B, N)`` or ``(N,)``, ``U`` and ``V`` ``(B, J_general, N)`` or ``(J_general, N)`` (shared by
        all problems).  Empty ``U`` removes them.  Up to a total width of 64 the plan then runs the wave-per-(problem,
        chunk) kernels with the general rows as one more row class, above that the any-width sequential kernel
        (:meth:`set_general_route`)."""
        U, V, A = _f64(U), _f64(V), _f64(A)
        if U.size == 0:
            _check(_load().clr_batch_set_general(self._h, 0, None, 0, None, 0, None, 0))
            return
        if U.shape != V.shape or U.shape[-1] != self.N or U.ndim not in (2, 3):
            raise ValueError("dimension mismatch")
        JG = U.shape[-2]
        if U.ndim == 3 and U.shape[0] != self.B:
            raise ValueError("dimension mismatch")
        if A.shape not in ((self.N,), (self.B, self.N)):
            raise ValueError("dimension mismatch")
        _check(_load().clr_batch_set_general(self._h, JG, _ptr(A), self.N if A.ndim == 2 else 0,
                                             _ptr(U), JG * self.N if U.ndim == 3 else 0,
                                             _ptr(V), JG * self.N if V.ndim == 3 else 0))

    def set_general_route(self, route=-1):
        """Plans with general terms: -1 the wide kernels when the total width allows (default), 1 the any-width
        sequential kernel (one workgroup per problem; the cross-check)."""
        lib = _load()
        lib.clr_batch_set_general_route.argtypes = [C.c_void_p, C.c_int]
        _check(lib.clr_batch_set_general_route(self._h, int(route)))

    # -- tuning -------------------------------------------------------------
    def set_chunks(self, nchunk):
        _check(_load().clr_batch_set_chunks(self._h, int(nchunk)))

    @property
    def chunks(self):
        n, l = C.c_int(), C.c_int()
        _load().clr_batch_get_chunks(self._h, C.byref(n), C.byref(l))
        return n.value, l.value

    # -- evaluation -----------------------------------------------------------
    def enqueue(self, materialize=False):
        _check(_load().clr_batch_enqueue(self._h, int(bool(materialize))))

    def synchronize(self):
        _check(_load().clr_batch_synchronize(self._h))

    def results(self):
        ll = np.empty(self.B)
        ld = np.empty(self.B)
        q = np.empty(self.B)
        st = np.empty(self.B, dtype=np.int32)
        _check(_load().clr_batch_get_results(self._h, _ptr(ll), _ptr(ld), _ptr(q),
                                             st.ctypes.data_as(_ip)))
        return ll, ld, q, st

    def evaluate(self, a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter=0.0, mean=None, mean_weights=None,
                 noise_weights=None):
        """One optimiser / MCMC evaluation in ONE library call (``clr_batch_evaluate``): new coefficient tables in,
        ``(loglike, logdet, quad, status)`` of all B problems out -- ``set_coefficients`` + ``enqueue`` + ``results``
        without two of the three trips through ctypes.  Arrays that already are C-contiguous float64 of the right shape
        are passed as they are.  ``mean`` (a scalar or ``(B,)``): :meth:`set_mean` in the same call
        (``clr_batch_evaluate_mean``); ``None`` leaves the mean in force as it is.  ``mean_weights``:
        :meth:`set_mean_weights` first (a linear mean, :meth:`set_mean_basis`); not together with ``mean``.
        ``noise_weights``: :meth:`set_noise_weights` first (a linear noise model, :meth:`set_noise_basis`)."""
        _exclusive_means(mean, mean_weights)
        if mean_weights is not None:
            self.set_mean_weights(mean_weights)
        if noise_weights is not None:
            self.set_noise_weights(noise_weights)
        B, JR, JC = self.B, self.J_real, self.J_comp
        tabs = []
        for a, w in ((a_real, JR), (c_real, JR), (a_comp, JC), (b_comp, JC), (c_comp, JC), (d_comp, JC)):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == (B, w)):
                try:
                    a = _f64(a, (B, w))
                except ValueError:
                    raise ValueError("dimension mismatch")
            tabs.append(a)
        jit = np.ascontiguousarray(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (B,)))
        ll, ld, q, st = np.empty(B), np.empty(B), np.empty(B), np.empty(B, dtype=np.int32)
        self._last_params = None
        if mean is not None:
            m, stride = _mean_arg(mean, B)
            _check(_load().clr_batch_evaluate_mean(self._h, m.ctypes.data, stride, jit.ctypes.data,
                                                   *([a.ctypes.data for a in tabs] + [ll.ctypes.data, ld.ctypes.data,
                                                                                     q.ctypes.data, st.ctypes.data])))
            return ll, ld, q, st
        fn = self._evaluate_fn
        if fn is None:
            fn = _load().clr_batch_evaluate
            fn.argtypes = [C.c_void_p] * 12      # (plain addresses: ndarray.ctypes.data is cheaper than data_as)
            self._evaluate_fn = fn
        _check(fn(self._h, jit.ctypes.data, *([a.ctypes.data for a in tabs] + [ll.ctypes.data, ld.ctypes.data, q.ctypes.data, st.ctypes.data])))
        return ll, ld, q, st

    # -- evaluation straight from `terms` kernel parameters ----------------------------------------------------------
    def set_kernel(self, kernel):
        """Compile a ``terms`` kernel of built-in terms (:func:`compile_kernel`; or take a :class:`CompiledKernel`) and
        hand the program to the plan (``clr_batch_set_kernel``): :meth:`evaluate_parameters` then needs only the
        parameter vectors per step.  ``ValueError`` when the kernel cannot be compiled or its ``(J_real, J_comp)`` at
        its current parameters is not the plan's."""
        prog = kernel if isinstance(kernel, CompiledKernel) else compile_kernel(kernel)
        if (prog.J_real, prog.J_comp) != (self.J_real, self.J_comp):
            raise ValueError("dimension mismatch: the kernel has (J_real, J_comp) = (%d, %d), the plan (%d, %d)"
                             % (prog.J_real, prog.J_comp, self.J_real, self.J_comp))
        self._set_kernel_handle(prog)
        self._last_params = None                           # (clr_batch_set_kernel: no parameters are in force)
        self.kernel_program = prog
        self.kernel = prog.kernel
        return prog

    def _set_kernel_handle(self, prog):
        _check(_load().clr_batch_set_kernel(self._h, prog._k))

    def _params_arg(self, params):
        prog = getattr(self, "kernel_program", None)
        if prog is None:
            raise RuntimeError("no kernel is set: call set_kernel first")
        p = np.ascontiguousarray(params, dtype=np.float64)
        if p.shape != (self.B, prog.n_params):
            raise ValueError("dimension mismatch")
        return p

    def evaluate_parameters(self, params, mean=None, mean_weights=None, noise_weights=None):
        """One optimiser / MCMC evaluation from kernel parameters (``clr_batch_evaluate_params``): ``params`` is
        ``(B, kernel.vector_size)`` in ``get_parameter_vector()`` order, ``mean``, ``mean_weights`` and
        ``noise_weights`` as in :meth:`evaluate`.  The coefficients are formed on the device and never leave it.  Returns ``(loglike, logdet,
        quad, status)``; a draw the program refuses (an SHO term across Q = 1/2, a non-finite parameter or coefficient)
        has status ``CLR_INVALID_ARGUMENT`` and NaN results, the other problems are not affected."""
        _exclusive_means(mean, mean_weights)
        if mean_weights is not None:
            self.set_mean_weights(mean_weights)
        if noise_weights is not None:
            self.set_noise_weights(noise_weights)
        p = self._params_arg(params)
        ll, ld, q, st = np.empty(self.B), np.empty(self.B), np.empty(self.B), np.empty(self.B, dtype=np.int32)
        m, stride = _mean_arg(mean, self.B)
        self._last_params = None
        _check(_load().clr_batch_evaluate_params(self._h, p.ctypes.data, None if m is None else m.ctypes.data, stride,
                                                 ll.ctypes.data, ld.ctypes.data, q.ctypes.data, st.ctypes.data))
        self._last_params = p                              # (information_parameters: the Jacobian at these rows)
        return ll, ld, q, st

    def grad_parameters(self, mean_partial=False):
        """``(value[B], grad[B, P], status[B])`` at the parameters of the last :meth:`evaluate_parameters`: the
        batched coefficient gradient chained to the kernel's parameters on the device (``clr_batch_grad_params``).
        ``mean_partial=True``: ``grad[B, P + 1]`` with ``d loglike / d mean`` last (the reference's order)."""
        P = self.kernel_program.n_params + (1 if mean_partial else 0)
        value, grad, st = np.empty(self.B), np.empty((self.B, P)), np.empty(self.B, dtype=np.int32)
        _check(_load().clr_batch_grad_params(self._h, _ptr(value), _ptr(grad), st.ctypes.data_as(_ip), int(bool(mean_partial))))
        return value, grad, st

    def coefficients(self):
        """The coefficients in force, read back from the device (``clr_batch_get_coefficients``):
        ``(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)``, the arguments of :meth:`evaluate`."""
        B, JR, JC = self.B, self.J_real, self.J_comp
        out = [np.empty((B, JR)), np.empty((B, JR))] + [np.empty((B, JC)) for _ in range(4)]
        jit = np.empty(B)
        _check(_load().clr_batch_get_coefficients(self._h, _ptr(jit), *[_ptr(a) for a in out]))
        return tuple(out) + (jit,)

    def log_likelihood(self, materialize=False):
        """Evaluate all B problems; returns ``(loglike, logdet, quad, status)``."""
        self.enqueue(materialize)
        return self.results()

    def factor(self, p):
        """``(phi, u, W, D)`` of problem ``p`` after a materialising run, shaped
        like the reference's pickled state (solver.cpp:36-42)."""
        N, J = self.N, self.J
        phi = np.empty((N - 1, J))
        u = np.empty((N - 1, J))
        W = np.empty((N, J))
        D = np.empty(N)
        _check(_load().clr_batch_get_factor(self._h, int(p), _ptr(phi), _ptr(u), _ptr(W), _ptr(D)))
        return phi.T, u.T, W.T, D

    def solve(self, b=None):
        """``K_p^-1 b_p`` for every problem from the factor of the last materialising run (``clr_batch_solve``;
        ``CholeskySolver.solve``, cholesky.h:218-318, for B problems at once).  ``b``: ``(B, N)`` or ``(B, nrhs, N)``;
        ``None``: the plan's own ``y`` less the mean of :meth:`set_mean` (no upload).  Returns an array of the same
        shape."""
        lib = _load()
        lib.clr_batch_solve.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        if b is None:
            x = np.empty((self.B, self.N))
            _check(lib.clr_batch_solve(self._h, 1, None, _ptr(x)))
            return x
        b = _f64(b)
        if b.ndim not in (2, 3) or b.shape[0] != self.B or b.shape[-1] != self.N:
            raise ValueError("dimension mismatch")
        nrhs = 1 if b.ndim == 2 else b.shape[1]
        x = np.empty(b.shape)
        _check(lib.clr_batch_solve(self._h, int(nrhs), _ptr(b), _ptr(x)))
        return x

    def predict(self, xs, return_var=False, mean_basis=None, method="solve"):
        """The conditional mean ``mu_p + K_p(x*, t_p) K_p^-1 (y_p - mu_p)`` of every problem (``mu_p`` the mean of
        :meth:`set_mean`, zero without one; ``GP.predict``, celerite.py:279) at the prediction points ``xs`` --
        ``(M,)`` shared by all problems or ``(B, M)`` -- from the factor of the last materialising run
        (``clr_batch_predict``; ``CholeskySolver.predict``, cholesky.h:599-698, for B problems).  Returns ``(B, M)``.
        With a linear mean in force (:meth:`set_mean_basis`) ``mean_basis`` is required: the basis at ``xs``, ``(K, M)``
        or ``(B, K, M)``; its product with the weights is added to the conditional mean of the residual.
        ``return_var=True``: ``(mu, var)`` with the conditional variance ``k_p(0) - k*^T K_p^-1 k*`` of every point
        (``clr_batch_predict_var``; celerite.py:465-470), both ``(B, M)``: only ``xs`` goes up and ``var`` comes down.
        ``method`` chooses the variance's route and is ignored for the mean: ``"solve"`` (the default) is one forward
        substitution per point, O(M N J) per problem, any width; ``"recurrence"`` (``clr_batch_predict_var_recurrence``,
        narrow plans, widths 1..8) is one forward and one backward matrix recurrence over the series plus O(J^2) per
        point, O((N + M) J^2).  The two agree to rounding (each within 1e-10 k(0) of the reference), not bit for bit.
        Which to choose (``profiles/predict_var_recurrence_timing.txt``, device time): on a narrow plan ``"recurrence"``
        from a handful of points on -- at 256 x 1e4 x width 4 it is the faster one at every measured M >= 1 (0.52 ms
        against 737 ms at M = N = 1e4), at 1024 x 1e5 x width 8 the two tie at M = 1 (6.5 ms) and it wins from M = 4
        on (7.2 ms against 25.9 ms; 21.4 ms at M = 1e4).  ``"solve"`` on wide plans (widths 9..64, which the recurrence
        refuses), for a single point on a long series, and where the phases ``d t`` reach ~1e9: the recurrence evaluates
        a point's features at the absolute phase ``d x`` and carries its rounding (1e-8 k(0) at t ~ 3e8).  Unsorted
        points are sorted on the host (150 ms for 256 x 1e4 points): pass them sorted where that matters."""
        _predict_method(method)
        lib = _load()
        lib.clr_batch_predict.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
        xs = _f64(xs)
        if xs.ndim == 1:
            stride = 0
        elif xs.ndim == 2 and xs.shape[0] == self.B:
            stride = xs.shape[1]
        else:
            raise ValueError("dimension mismatch")
        M = xs.shape[-1]
        model = _linear_mean_at(self, mean_basis, M)
        pred = np.empty((self.B, M))
        _check(lib.clr_batch_predict(self._h, int(M), _ptr(xs), stride, _ptr(pred)))
        if model is not None:
            pred = model + pred
        if not return_var:
            return pred
        entry = lib.clr_batch_predict_var_recurrence if method == "recurrence" else lib.clr_batch_predict_var
        entry.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
        var = np.empty((self.B, M))
        _check(entry(self._h, int(M), _ptr(xs), stride, _ptr(var)))
        return pred, var

    def set_predict_tile(self, points=0):
        """Prediction points per tile of ``predict(xs, return_var=True)`` (``clr_batch_set_predict_tile``); 0:
        automatic.  The results do not depend on it."""
        lib = _load()
        lib.clr_batch_set_predict_tile.argtypes = [C.c_void_p, C.c_int]
        _check(lib.clr_batch_set_predict_tile(self._h, int(points)))

    def one_step_ahead(self, b=None):
        """The one-step-ahead residuals (innovations) of every problem, a :class:`OneStepAhead`
        (``clr_batch_one_step_ahead``), from the factor ``K = L diag(D) L^T`` of the last materialising run:
        ``innovation = L^-1 b``, undivided, ``variance = D``.  ``b``: ``(B, N)`` or ``(B, nrhs, N)``; ``None``: the
        residual in force, ``y`` less the mean of :meth:`set_mean` / :meth:`set_mean_weights` (no upload).  Then
        ``E[y_n | y_<n] = y_n - innovation_n`` with variance ``variance_n`` (``diag_n + jitter`` enters it),
        ``.standardized`` should be white and standard normal, and ``.log_density`` sums to the log-likelihood.  One
        forward chunked scan -- the forward half of :meth:`solve`."""
        return _one_step_ahead(self, "clr_batch_one_step_ahead", _check, b)

    def forecast(self, xs, return_var=False, mean_basis=None):
        """The causal forecast ``p(f(x) | y_n : t_n < x)`` of every problem at the points ``xs`` -- ``(M,)`` shared by
        all problems or ``(B, M)``, sorted or not -- given only the samples STRICTLY before each point
        (``clr_batch_forecast``), from the factor of the last materialising run; narrow plans (widths 1..8).  Returns
        the mean ``(B, M)``, with ``return_var=True`` ``(mean, var)``: the conditional variance of the latent process
        (no jitter, no observational variance), as :meth:`predict`'s.  The mean in force is added at the points as
        :meth:`predict` adds it: a constant mean as is, a linear mean through ``mean_basis`` (required while one is in
        force).  Before the first sample the result is the prior (the mean model, ``k(0)``); at ``x = t_n`` it is the
        one-step-ahead prediction of sample n (:meth:`one_step_ahead`: ``y_n - innovation_n``, ``variance_n - diag_n -
        jitter``).  One forward pass over the series plus O(J^2) per point; tiles follow :meth:`set_predict_tile`."""
        return _forecast(self, "clr_batch_forecast", _check, xs, return_var, mean_basis)

    def periodogram(self, omega, offset=False, t_ref=0.0, min_pivot=1e-10, return_gram=False):
        """The periodogram under the plan's covariance, a :class:`Periodogram` (``clr_batch_periodogram``): at every
        trial angular frequency ``omega`` -- ``(F,)`` shared by all problems or ``(B, F)`` -- the generalised-least-squares
        fit of ``A cos(omega (t - t_ref)) + B sin(omega (t - t_ref))``, plus a constant with ``offset=True``, to the
        residual in force with ``K^-1`` as the metric, from the factor of the last materialising run.  ``power`` is the
        log-likelihood the fit gains over the model without the sinusoid; ``coef`` holds ``(A, B)`` -- ``(offset, A, B)``
        --, ``cov`` their covariance; ``.amplitude`` and ``.phase`` follow from them.  A frequency whose normal matrix
        is not positive definite to ``min_pivot`` (``omega = 0``; with the offset, one far below ``1 / T``) has status
        ``CLR_NOT_POSITIVE_DEFINITE`` and NaN there.  Two forward walks over the series per block of frequencies with
        the columns formed on the fly: nothing is uploaded but ``omega``; narrow plans (widths 1..8), chunked."""
        return _periodogram(self, "clr_batch_periodogram", _check, omega, offset, t_ref, min_pivot, return_gram)

    def set_periodogram_tile(self, frequencies=0):
        """Frequencies per tile of :meth:`periodogram` (``clr_batch_set_periodogram_tile``); 0: automatic.  The results
        do not depend on it."""
        _check(_load().clr_batch_set_periodogram_tile(self._h, int(frequencies)))

    def periodogram_ms(self):
        """Device time of the last :meth:`periodogram`'s kernels, ms."""
        ms = C.c_double(0.0)
        _check(_load().clr_batch_get_periodogram_ms(self._h, C.byref(ms)))
        return ms.value

    def periodogram_block(self):
        """Frequencies one lane of :meth:`periodogram`'s walks carries at this width (a test hook)."""
        n = C.c_int(0)
        _check(_load().clr_batch_debug_get_periodogram_block(self._h, C.byref(n)))
        return n.value

    def predict_terms(self, xs, groups=None, return_var=False):
        """Component separation: the posterior of the process of each GROUP of kernel terms, ``E[f_g(x) | y] = k_g*^T
        K^-1 r`` and with ``return_var=True`` also ``Var[f_g(x) | y] = k_g(0) - k_g*^T K^-1 k_g*``, of every problem at the
        points ``xs`` -- ``(M,)`` shared by all problems or ``(B, M)``, sorted or not -- from the factor of the last
        materialising run (``clr_batch_predict_terms``); narrow plans (widths 1..8, N >= 128).  ``groups``: ``None`` --
        one group per coefficient term, in ``kernel.coefficients`` order (real terms first, then the complex ones) --, a
        sequence of sequences of term indices, or a ``(G, T)`` boolean array; ``CompiledKernel.groups`` is "each summand
        of my kernel".  Returns ``(B, G, M)``, or ``(mean, var)`` of that shape.  ``r`` is the residual in force and NO
        mean is added: the mean belongs to no term.  The group of all terms is :meth:`predict`'s conditional mean of the
        residual and its ``method="recurrence"`` variance; the empty group is exactly 0; the means of disjoint groups
        add up, their variances do not.  One solve plus one forward and one backward pass over the series whatever the
        number of groups, O(G J^2) per point; tiles follow :meth:`set_predict_tile`.  Measured
        (``profiles/predict_terms_timing.txt``, wall time, one group per term): at 1024 x 1e5 x width 8 the means of
        the 5 terms take 20.3 ms at M = 1 and 21.7 ms at M = 100 beside 207 and 242 ms for :meth:`predict` (one launch
        set per problem), with the variances 26.8 and 30.5 ms beside 215 and 249 ms for its ``method="recurrence"``; at
        M = 1e4, where G times the numbers come down and the points go in 5 tiles, 171 ms beside 247 ms and 334 ms
        beside 277 ms.  At 256 x 1e4 x width 4: 1.20 / 1.32 ms beside 19.3 / 19.6 ms at M = 1."""
        return _predict_terms(self, "clr_batch_predict_terms", _check, xs, groups, return_var)

    def predict_cov(self, xs):
        """The posterior covariance of the latent process between the points ``xs`` -- ``(M,)`` shared by all problems or
        ``(B, M)``, sorted or not -- of every problem, ``(B, M, M)`` (``clr_batch_predict_cov``; ``GP.predict(...,
        return_cov=True)``, celerite.py:283-291, for B problems): ``k(x_i - x_j) - k*_i^T K^-1 k*_j`` from the factor of the
        last materialising run -- no jitter, no observational variance, as :meth:`predict`'s variance, which is its
        diagonal.  Full, symmetric to the bit.  No N x M block is solved: one forward and two backward passes over the
        factor, O(J^3) per point and O(J^2) per pair of points (``csrc/clr_bcond_kernels.h``).  Narrow plans (widths
        1..8, N >= 128); problems go through in tiles (:meth:`set_conditional_tile`)."""
        return _predict_cov(self, "clr_batch_predict_cov", _check, xs)

    def sample_conditional(self, xs, size=None, regularize=0.0, min_pivot=1e-10, mean_basis=None, random=None, normals=None,
                           return_status=False):
        """Joint draws of the latent process at the points ``xs`` given the data (``GP.sample_conditional``,
        celerite.py:327-332, for B problems): :meth:`predict`'s conditional mean (``mean_basis`` as there) plus
        ``L diag(d)^1/2 n`` with ``C + regularize I = L diag(d) L^T``, ``C`` the covariance of :meth:`predict_cov`
        (``clr_batch_sample_conditional``).  ``size=None``: ``(B, M)``; else ``(B, size, M)``.  The standard normals
        ``n`` come from ``random`` (default ``np.random``) as in :meth:`sample`, or are ``normals`` of the result's
        shape; ``normals[..., r]`` belongs to point ``xs[..., r]``, the factor is taken in ascending order of the points.
        The factor follows from the celerite recurrence over the points -- O(J^3) per point, O(J^2) per point and draw,
        no M x M matrix.  A pivot within ``min_pivot k(0)`` of zero (1e-10: the bar on a predictive variance) marks a
        point that is a function of the earlier ones -- a repeated point, a point on a sample without noise -- and its
        normal does not enter; a pivot below ``-min_pivot k(0)`` refuses the problem: its rows are NaN and its status
        ``CLR_NOT_POSITIVE_DEFINITE`` (``return_status=True``: ``(draws, status[B])``).  Narrow plans (widths 1..8,
        N >= 128); problems go through in tiles (:meth:`set_conditional_tile`)."""
        return _sample_conditional(self, "clr_batch_sample_conditional", _check, xs, size, regularize, min_pivot, mean_basis,
                                   random, normals, return_status)

    def set_conditional_tile(self, problems=0):
        """Problems per tile of :meth:`predict_cov` and :meth:`sample_conditional` (``clr_batch_set_conditional_tile``);
        0: automatic, as many as fit 1 GiB of device scratch.  The results do not depend on it."""
        _check(_load().clr_batch_set_conditional_tile(self._h, int(problems)))

    def inverse_diagonal(self):
        """``diag(K_p^-1)`` of every problem, ``(B, N)``, from the factor of the last materialising run
        (``clr_batch_leave_one_out``): all N entries by one backward matrix recurrence, O(N J^2) per problem.  With
        ``c = diag(K^-1)``, ``alpha = K^-1 r`` (:meth:`solve`) and ``s_n = diag_eff_n + jitter`` (``diag_eff``: ``diag`` plus the noise model of
        :meth:`set_noise_weights`) the in-sample answer of
        ``GP.predict(y)`` (celerite.py:270-272) is ``mu_n = y_n - s_n alpha_n``, ``var_n = s_n - s_n^2 c_n`` -- no O(N^2)
        work.  Rows of problems whose status is not 0 are NaN."""
        c = np.empty((self.B, self.N))
        self._leave_one_out(c, None, None, None)
        return c

    def leave_one_out(self, arrays=True):
        """The leave-one-out predictive distribution of every sample of every problem, a :class:`LeaveOneOut`
        (``clr_batch_leave_one_out``), from the factor of the last materialising run.  With ``c_n = (K^-1)_nn`` and
        ``alpha = K^-1 r``, ``r = y`` less the mean in force (:meth:`set_mean`, :meth:`set_mean_weights`):

            ``residual_n = y_n - mu_-n = alpha_n / c_n``, ``variance_n = sigma^2_-n = 1 / c_n``,
            ``log p(y_n | y_-n) = -1/2 log(2 pi / c_n) - 1/2 alpha_n^2 / c_n``, ``logpdf = `` their sum over n

        (``residual`` and ``variance`` are formed on the host from the two downloaded arrays; see
        :func:`leave_one_out_from`).  The in-sample ``GP.predict(y)`` (celerite.py:270-272) follows without O(N^2) work:
        ``mu_n = y_n - s_n alpha_n``, ``var_n = s_n - s_n^2 c_n`` with ``s_n = diag_eff_n + jitter`` (``diag_eff``: ``diag`` plus the noise model of
        :meth:`set_noise_weights`).
        ``arrays=False`` downloads ``logpdf[B]`` and ``status[B]`` only -- the step of a leave-one-out cross-validation
        model comparison; the array fields are then ``None``.  Rows of problems whose status is not 0 are NaN."""
        logpdf, st = np.empty(self.B), np.empty(self.B, dtype=np.int32)
        if not arrays:
            self._leave_one_out(None, None, logpdf, st)
            return LeaveOneOut(None, None, logpdf, None, None, st)
        c, alpha = np.empty((self.B, self.N)), np.empty((self.B, self.N))
        self._leave_one_out(c, alpha, logpdf, st)
        return LeaveOneOut(alpha / c, 1.0 / c, logpdf, c, alpha, st)

    def _leave_one_out(self, c, alpha, logpdf, st):
        _check(_load().clr_batch_leave_one_out(self._h, *_loo_args(c, alpha, logpdf, st)))

    def leave_one_out_ms(self):
        """``(diag_ms, solve_ms, reduce_ms)``: device time of the three parts of the last :meth:`leave_one_out` or
        :meth:`inverse_diagonal` (a part that did not run: 0)."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _check(_load().clr_batch_get_leave_one_out_ms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def dot_L(self, z):
        """``L_p z_p`` with ``K_p = L_p L_p^T`` for every problem from the factor of the last materialising run
        (``clr_batch_dot_L``; ``CholeskySolver.dot_L``, cholesky.h:409-431, for B problems at once).  ``z``: ``(B, N)``
        or ``(B, nrhs, N)``; returns an array of the same shape."""
        lib = _load()
        lib.clr_batch_dot_L.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        z = _f64(z)
        if z.ndim not in (2, 3) or z.shape[0] != self.B or z.shape[-1] != self.N:
            raise ValueError("dimension mismatch")
        nrhs = 1 if z.ndim == 2 else z.shape[1]
        y = np.empty(z.shape)
        _check(lib.clr_batch_dot_L(self._h, int(nrhs), _ptr(z), _ptr(y)))
        return y

    def dot(self, z):
        """``K_p z_p`` for every problem at the coefficients in force (``clr_batch_dot``; ``CholeskySolver.dot``,
        cholesky.h:441-596, for B problems at once -- the kernel matrix WITHOUT the observational variance, as
        ``GP.dot``).  ``z``: ``(B, N)`` or ``(B, nrhs, N)``; returns an array of the same shape."""
        lib = _load()
        lib.clr_batch_dot.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        z = _f64(z)
        if z.ndim not in (2, 3) or z.shape[0] != self.B or z.shape[-1] != self.N:
            raise ValueError("dimension mismatch")
        nrhs = 1 if z.ndim == 2 else z.shape[1]
        y = np.empty(z.shape)
        _check(lib.clr_batch_dot(self._h, int(nrhs), _ptr(z), _ptr(y)))
        return y

    def sample(self, size=None, mean=None, random=None):
        """Draws from every problem's prior ``N(mean_p, K_p)`` (``GP.sample``, celerite.py:422-451: ``mean + L n`` with
        standard normal ``n``) from the factor of the last materialising run.  ``size=None``: ``(B, N)``; else
        ``(B, size, N)``.  ``mean``: ``None``, a scalar, ``(N,)`` or ``(B, N)``."""
        rng = np.random if random is None else random
        shape = (self.B, self.N) if size is None else (self.B, int(size), self.N)
        y = self.dot_L(rng.standard_normal(shape))
        if mean is not None:
            m = np.asarray(mean, dtype=float)
            if m.ndim == 2 and size is not None:
                m = m[:, None, :]
            y += m
        return y

    def solve_device_ms(self):
        """Device time of the last :meth:`solve` (its kernels, without the host <-> HBM copies)."""
        lib = _load()
        ms = C.c_double()
        lib.clr_batch_get_solve_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _check(lib.clr_batch_get_solve_ms(self._h, C.byref(ms)))
        return ms.value

    KERNEL_NAMES = ("relayout", "summarize", "prefix", "correct", "replay", "finalize")

    LAYOUTS = {"rowmajor": 0, "interleaved": 1, "staged": 2}

    def set_layout(self, layout="staged"):
        """How the kernels read the series: ``"staged"`` (default: coalesced tiles
        transposed through LDS, no extra pass), ``"interleaved"`` (a cached
        chunk-interleaved copy built by a transpose kernel when the series change)
        or ``"rowmajor"`` (direct, slow; for A/B measurements)."""
        _check(_load().clr_batch_set_layout(self._h, self.LAYOUTS.get(layout, layout)))

    PREFIX_MODES = {"single": 0, "walk": 1, "multilevel": 2}

    def set_prefix_mode(self, mode="multilevel", cooperative=None):
        """Prefix phase (chunk elements -> chunk start states): ``"multilevel"`` (default: groups of
        elements composed in parallel, the composed ones walked, start states fanned out;
        csrc/clr_prefix_kernels.h), ``"walk"`` (16 lanes per problem, chunk after chunk) or ``"single"``
        (one lane: the host-checked form, cross-check).  ``True`` / ``False`` mean walk / single
        (also accepted as the keyword ``cooperative`` of earlier releases)."""
        if cooperative is not None:
            mode = bool(cooperative)
        if isinstance(mode, bool):
            mode = 1 if mode else 0
        _check(_load().clr_batch_set_prefix_mode(self._h, int(self.PREFIX_MODES.get(mode, mode))))

    def set_prefix_plan(self, levels=-1, group=0):
        """Level structure of the multi-level prefix: ``levels`` levels of groups of ``group`` elements
        (``levels < 0``: chosen from the chunk count)."""
        _check(_load().clr_batch_set_prefix_plan(self._h, int(levels), int(group)))

    @property
    def prefix_plan(self):
        """``(levels, group sizes, element counts per level)`` of the prefix phase."""
        lv = C.c_int()
        g = (C.c_int * 3)()
        n = (C.c_int * 4)()
        _check(_load().clr_batch_get_prefix_plan(self._h, C.byref(lv), g, n))
        return lv.value, list(g)[:max(lv.value, 0)], list(n)[:lv.value + 1]

    def debug_starts(self):
        """Chunk start states of the last evaluation, ``(B, nchunk, J (J + 1) / 2 + J)`` (widths 1..8)."""
        out = np.empty((self.B, self.chunks[0], self.J * (self.J + 1) // 2 + self.J))
        _check(_load().clr_batch_debug_get_starts(self._h, _ptr(out)))
        return out

    def compose_check(self, group):
        """Cooperative composition kernel against the single-lane host-checked form on the last
        evaluation's chunk elements, in groups of ``group``: ``(largest relative difference, largest
        magnitude)``."""
        d, m = C.c_double(), C.c_double()
        _check(_load().clr_batch_debug_compose_check(self._h, int(group), C.byref(d), C.byref(m)))
        return d.value, m.value

    def selection_bounds(self):
        """``dict(tmax, dxmax, dmax, cmax, set_series_host_ms)``: what the kernel selection looks at."""
        v = [C.c_double() for _ in range(5)]
        _check(_load().clr_batch_get_selection_bounds(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("tmax", "dxmax", "dmax", "cmax", "set_series_host_ms"), [x.value for x in v]))

    def set_warm_start(self, mode=-1, forced_warmup=0):
        """Warm-started plain recurrence for series that forget their past (``clr_batch_set_warm_start``):
        -1 auto, 0 off, 1 forced with ``forced_warmup`` steps.  Takes effect at the next
        :meth:`set_coefficients`."""
        _check(_load().clr_batch_set_warm_start(self._h, int(mode), int(forced_warmup)))

    def set_small_mode(self, mode=-1):
        """One-launch evaluation of short narrow problems (``clr_batch_set_small_mode``): -1 automatic, 0 off,
        1 whenever supported (widths 1..4, 512 <= N <= 32768)."""
        lib = _load()
        lib.clr_batch_set_small_mode.argtypes = [C.c_void_p, C.c_int]
        _check(lib.clr_batch_set_small_mode(self._h, int(mode)))

    def small_mode_active(self):
        """Whether the next evaluation runs as one launch (series and coefficients must be set)."""
        a = C.c_int()
        lib = _load()
        lib.clr_batch_get_small_mode.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        _check(lib.clr_batch_get_small_mode(self._h, C.byref(a)))
        return bool(a.value)

    def warm_start(self):
        """``dict(active, chunks, chunk_len, warmup_min, warmup_max, settled, fallbacks)``."""
        v = [C.c_int() for _ in range(7)]
        _check(_load().clr_batch_get_warm_start(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("active", "chunks", "chunk_len", "warmup_min", "warmup_max", "settled", "fallbacks"),
                        [x.value for x in v]))

    def grad_log_likelihood(self, mean_partial=False):
        """``(value[B], grad[B, 1 + 2 J_real + 4 J_comp], status[B])`` at the coefficients in force, parallel in n
        (``clr_batch_grad``; the reference's conventions per problem, ``CholeskySolver.grad_log_likelihood``,
        solver.cpp:347-463).  ``mean_partial=True``: ``(value, grad, dmean[B], status)`` with ``dmean = d loglike /
        d mu = 1^T K^-1 (y - mu)`` (``clr_batch_grad_mean``; the last column of :func:`chain_gradient`)."""
        NG = 1 + 2 * self.J_real + 4 * self.J_comp
        value, grad, st = np.empty(self.B), np.empty((self.B, NG)), np.empty(self.B, dtype=np.int32)
        if mean_partial:
            dmean = np.empty(self.B)
            _check(_load().clr_batch_grad_mean(self._h, _ptr(value), _ptr(grad), _ptr(dmean), st.ctypes.data_as(_ip)))
            return value, grad, dmean, st
        _check(_load().clr_batch_grad(self._h, _ptr(value), _ptr(grad), st.ctypes.data_as(_ip)))
        return value, grad, st

    def information(self, mean_partial=False):
        """``(info[B, M, M], status[B])``: the information matrix of every problem at the coefficients and on the series
        in force (``clr_batch_information``; Fisher scoring on the innovations form), ``M = 1 + 2 J_real + 4 J_comp`` in
        the order of :meth:`grad_log_likelihood`'s columns; ``mean_partial=True``: ``M + 1`` with the constant mean
        last.  Symmetric, positive semi-definite; its expectation over data drawn from the model is the Fisher
        information -- it is not the Hessian.  A problem that is not ``CLR_OK`` is all NaN with its status; ``jitter <=
        2.2e-16`` zeroes the jitter row and column.  Narrow plans with celerite terms; the blocks of linear-mean, noise
        and amplitude weights are not covered.  Chain to kernel parameters with :func:`chain_information`."""
        M = 1 + 2 * self.J_real + 4 * self.J_comp + (1 if mean_partial else 0)
        info, st = np.empty((self.B, M, M)), np.empty(self.B, dtype=np.int32)
        self._information(int(bool(mean_partial)), info, st)
        return info, st

    def _information(self, mean_partial, info, st):
        _check(_load().clr_batch_information(self._h, mean_partial, _ptr(info), st.ctypes.data_as(_ip)))

    def set_information_tile(self, problems=0):
        """Problems per tile of :meth:`information` (``clr_batch_set_information_tile``); 0: as many as hold their rows
        in 1 GiB."""
        _check(_load().clr_batch_set_information_tile(self._h, int(problems)))

    def information_device_ms(self):
        """Device time of the last :meth:`information` in ms (``clr_batch_get_information_ms``)."""
        ms = C.c_double()
        lib = _load()
        lib.clr_batch_get_information_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        _check(lib.clr_batch_get_information_ms(self._h, C.byref(ms)))
        return ms.value

    def information_parameters(self, mean_partial=False):
        """``(info[B, P(+1), P(+1)], status[B])`` in the kernel's parameters at the rows of the last
        :meth:`evaluate_parameters`: :func:`chain_information` of :meth:`information` with the program's Jacobian there
        (exact for this form: no second derivative of a coefficient formula enters).  A draw the program refused is NaN.
        Refused wherever :meth:`grad_parameters` is: behind :meth:`set_coefficients`, :meth:`evaluate` or :meth:`set_kernel`
        the coefficients in force are not those parameters' any more, until the next :meth:`evaluate_parameters`."""
        prog, p = getattr(self, "kernel_program", None), getattr(self, "_last_params", None)
        if prog is None or p is None:
            raise RuntimeError("no parameters are in force: the coefficients in force were not formed from parameters "
                               "(call set_kernel and evaluate_parameters first)")
        info, st = self.information(mean_partial)
        jac, jj, _ = prog.jacobian(p, status=True)
        return chain_information(info, jac, jj, mean_partial), st

    def set_grad_mode(self, mode="reverse", stored_state_distance=0, drift_tolerance=0.0):
        """``"reverse"`` (default: one sweep for all partials), ``"forward"`` (one tangent per partial) or
        ``"reverse-direct-riders"`` (reverse mode with the riders accumulated along the trajectory instead of taken
        from the scan's elements; A/B runs); ``clr_batch_set_grad_mode``."""
        _check(_load().clr_batch_set_grad_mode(self._h, {"reverse": 0, "forward": 1, "reverse-direct-riders": 2}[mode], int(stored_state_distance),
                                               float(drift_tolerance)))

    def grad_info(self):
        """``dict(reverse, forward_reruns, drift_max)`` of the last :meth:`grad_log_likelihood`."""
        r, n, d = C.c_int(), C.c_int(), C.c_double()
        _check(_load().clr_batch_get_grad_info(self._h, C.byref(r), C.byref(n), C.byref(d)))
        return {"reverse": bool(r.value), "forward_reruns": n.value, "drift_max": d.value}

    def grad_fallbacks(self):
        """Problems of the last :meth:`grad_log_likelihood` that took the sequential gradient kernel."""
        n = C.c_int()
        _check(_load().clr_batch_get_grad_fallbacks(self._h, C.byref(n)))
        return n.value

    def set_rescue(self, mode=-1):
        """Route-1 problems (ill-conditioned, checked chunked replay) re-planned as a small plan of their own with many
        short chunks (``clr_batch_set_rescue``): -1 automatic (chunks of >= 1024 samples), 0 the inline replay, 1 always."""
        lib = _load()
        lib.clr_batch_set_rescue.argtypes = [C.c_void_p, C.c_int]
        _check(lib.clr_batch_set_rescue(self._h, int(mode)))

    def rescue(self):
        """Of the last fetched evaluation: problems re-planned (negative: replayed inline), running total, the side
        plan's chunking."""
        lib = _load()
        last, total, nc, L = C.c_int(), C.c_long(), C.c_int(), C.c_int()
        lib.clr_batch_get_rescue.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _check(lib.clr_batch_get_rescue(self._h, C.byref(last), C.byref(total), C.byref(nc), C.byref(L)))
        return {"last": last.value, "total": total.value, "chunks": (nc.value, L.value)}

    FACTOR_LAYOUTS = {"reference": 0, "lean": 1}

    def set_factor_layout(self, layout="reference"):
        """What a materialising run keeps in HBM (``clr_batch_set_factor_layout``): ``"reference"`` -- phi, u, W, D,
        ``8 N (3 J + 1)`` bytes per problem -- or ``"lean"`` -- W and D only, ``8 N (J + 1)`` bytes; phi and u are pure
        functions of the times and the coefficients (cholesky.h:127-147) and :meth:`factor` regenerates them."""
        lib = _load()
        lib.clr_batch_set_factor_layout.argtypes = [C.c_void_p, C.c_int]
        _check(lib.clr_batch_set_factor_layout(self._h, self.FACTOR_LAYOUTS.get(layout, layout)))

    def set_factor_refine(self, samples=64):
        """Samples at the head of every chunk a materialising run recomputes from the previous chunk's replayed end
        state (``clr_batch_set_factor_refine``; 0 switches the refinement off)."""
        lib = _load()
        lib.clr_batch_set_factor_refine.argtypes = [C.c_void_p, C.c_int]
        _check(lib.clr_batch_set_factor_refine(self._h, int(samples)))

    def factor_bytes(self):
        """Bytes of factor per problem in HBM under the layout and chunking in force."""
        lib = _load()
        n = C.c_size_t()
        lib.clr_batch_get_factor_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
        _check(lib.clr_batch_get_factor_bytes(self._h, C.byref(n)))
        return int(n.value)

    def set_exact(self, force=True):
        """Replay every problem step by step (the reference's recurrence) instead
        of settling it from the chunk summaries; for A/B runs and cross-checks."""
        _check(_load().clr_batch_set_exact(self._h, int(bool(force))))

    def exact_count(self):
        """Problems of the last (synchronised) run that needed the exact replay."""
        n = C.c_int()
        _check(_load().clr_batch_get_exact_count(self._h, C.byref(n)))
        return n.value

    def exact_flags(self):
        """Boolean mask: which problems of the last run went through the exact recurrence."""
        return self.exact_levels() != 0

    def exact_levels(self):
        """Per problem: 0 settled from the chunk summaries, 1 chunked replay (end states
        consistent with the scan), 2 truly sequential recurrence."""
        f = np.zeros(self.B, dtype=np.int32)
        _check(_load().clr_batch_get_exact_flags(self._h, f.ctypes.data_as(_ip)))
        return f

    def set_certificate(self, max_gamma_over_mu=1e7, max_residual=1e-11, max_gamma=None, max_gamma_error=None):
        """Routing of ill-conditioned problems (``clr_batch_set_certificate``,
        ``clr_batch_set_certificate_gamma``); a bound <= 0 switches that test off.  The two gamma bounds
        (defaults of a new plan: 1e4 and 3e-9) are only touched when one of them is passed."""
        _check(_load().clr_batch_set_certificate(self._h, float(max_gamma_over_mu), float(max_residual)))
        if max_gamma is not None or max_gamma_error is not None:
            _check(_load().clr_batch_set_certificate_gamma(self._h, float(1e4 if max_gamma is None else max_gamma),
                                                           float(3e-9 if max_gamma_error is None else max_gamma_error)))

    def conditioning(self):
        """``(gamma_max, mu_min)`` per problem of the last run: largest ``a_n / D_n`` over the
        zero-start pivots, smallest certificate pivot (see ``clr_batch_get_conditioning``)."""
        g, m, r = np.empty(self.B), np.empty(self.B), np.empty(self.B)
        _check(_load().clr_batch_get_conditioning(self._h, _ptr(g), _ptr(m), _ptr(r)))
        self.last_residual = r
        return g, m

    def measured_error(self):
        """Per problem: the largest measured relative error of the chunks' ``G = (I + P Jm)^-1 P``
        (``clr_batch_get_measured_error``; the routing tests ``gamma_max * eG_max``)."""
        e = np.empty(self.B)
        _check(_load().clr_batch_get_measured_error(self._h, _ptr(e)))
        return e

    def conditioning_chunkwise(self):
        r = np.empty(self.B)
        _check(_load().clr_batch_get_conditioning_chunkwise(self._h, _ptr(r)))
        return r

    def set_summarize_mode(self, mode=-1):
        """summarize kernel of widths 7, 8: 0 single wave, 1 two roles on two waves per
        SIMD, 2 the same with the decay factored out of the state on dense series, -1 auto
        (``clr_batch_set_summarize_mode``; csrc/clr_split_kernels.h)."""
        _check(_load().clr_batch_set_summarize_mode(self._h, int(mode)))

    def summarize_kernel(self):
        """Name of the summarize kernel the next evaluation runs."""
        k = C.c_int()
        _check(_load().clr_batch_get_summarize_kernel(self._h, C.byref(k)))
        return ("single wave", "role split", "role split, lazy decay")[k.value]

    def split_variant(self):
        """The variant of the lazy role-split summarize the next evaluation runs: ``dict(b_zero=...)``, true for the
        kernel without the ``b_comp`` terms, false for the general one and any other kernel
        (``clr_batch_get_split_variant``)."""
        v = C.c_int()
        _check(_load().clr_batch_get_split_variant(self._h, C.byref(v)))
        return dict(b_zero=bool(v.value & 1))

    def fp32_probe(self):
        """``(logdet, quad, ms)`` of the sequential sweep with a float state (widths 9..32;
        a measurement of the fp32 tolerance, ``clr_batch_fp32_probe``)."""
        ld, q = np.empty(self.B), np.empty(self.B)
        ms = C.c_double()
        _check(_load().clr_batch_fp32_probe(self._h, _ptr(ld), _ptr(q), C.byref(ms)))
        return ld, q, ms.value

    def set_profiling(self, on=True):
        """Bracket the kernels of every following :meth:`enqueue` with HIP events; ``on=2`` brackets the
        summarize (dominant) kernel only: two event records per evaluation instead of seven."""
        _check(_load().clr_batch_set_profiling(self._h, 2 if on == 2 else int(bool(on))))

    def profile(self):
        """``({kernel name: summed ms}, evaluations recorded)`` since :meth:`set_profiling`."""
        k = (C.c_double * 6)()
        n = C.c_int()
        _check(_load().clr_batch_get_profile(self._h, k, C.byref(n)))
        return dict(zip(self.KERNEL_NAMES, [k[i] for i in range(6)])), n.value

    def run_timed(self, steps, materialize=False, relayout_each_step=True):
        """``steps`` back-to-back evaluations bracketed by HIP events on the
        plan's stream.  Returns ``(total_ms, {kernel name: summed ms})``."""
        tot = C.c_double()
        k = (C.c_double * 6)()
        _check(_load().clr_batch_run_timed(self._h, int(bool(materialize)), int(steps),
                                           int(bool(relayout_each_step)), C.byref(tot), k))
        return tot.value, dict(zip(self.KERNEL_NAMES, [k[i] for i in range(6)]))


def shard_bounds(total, nshards, shard):
    """``[lo, hi)`` of ``shard`` when ``total`` problems are cut into ``nshards``
    contiguous slices (``clr_shard_bounds``; pure host arithmetic, needs no GPU)."""
    lo, hi = C.c_int(), C.c_int()
    if _load().clr_shard_bounds(int(total), int(nshards), int(shard), C.byref(lo), C.byref(hi)) != CLR_OK:
        raise ValueError("bad shard arguments")
    return lo.value, hi.value


class ShardedBatchedGP(object):
    """The batch axis over several GPUs: ``len(devices)`` contiguous shards, one
    :class:`BatchedGP`-like plan and one host thread per shard, no collective
    (problems are independent: cholesky.h:703-706).  ``devices`` defaults to every
    visible GPU; a device may be listed more than once (shards sharing a GPU), which
    is how the sharding is tested on one GPU.  The kernels are selected once for the whole
    batch (batch-wide maxima of the series and coefficients), so results do not depend on the
    sharding bit for bit when the chunk count is the same (:meth:`set_chunks`; the automatic
    choice looks at the shard size) and the warm-started recurrence is not in play (it adapts per
    plan: see :meth:`set_warm_start`)."""

    def __init__(self, B, N, J_real, J_comp, devices=None):
        lib = _load()
        if devices is None:
            devices = list(range(device_count()))
        devices = [int(d) for d in devices]
        if not devices:
            raise RuntimeError("no gfx950 (MI355X) device is visible; libcelerite_hip has no CPU path")
        self.B, self.N, self.J_real, self.J_comp = int(B), int(N), int(J_real), int(J_comp)
        arr = (C.c_int * len(devices))(*devices)
        h = lib.clr_sharded_create(self.B, self.N, self.J_real, self.J_comp, arr, len(devices))
        if not h:
            raise RuntimeError("clr_sharded_create failed: " + lib.clr_sharded_last_error().decode())
        self._h = C.c_void_p(h)
        self._mean_K, self._mean_w = 0, None

    def _ok(self, status):
        if status != CLR_OK:
            lib = _load()
            raise RuntimeError(lib.clr_status_string(status).decode() + ": " +
                               lib.clr_sharded_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            _load().clr_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def shards(self):
        """``[(device, lo, hi), ...]``"""
        lib = _load()
        out = []
        for s in range(lib.clr_sharded_num_shards(self._h)):
            d, lo, hi = C.c_int(), C.c_int(), C.c_int()
            lib.clr_sharded_get_shard(self._h, s, C.byref(d), C.byref(lo), C.byref(hi))
            out.append((d.value, lo.value, hi.value))
        return out

    def set_chunks(self, nchunk):
        self._ok(_load().clr_sharded_set_chunks(self._h, int(nchunk)))

    def set_summarize_mode(self, mode=-1):
        self._ok(_load().clr_sharded_set_summarize_mode(self._h, int(mode)))

    def set_rescue(self, mode=-1):
        """``clr_batch_set_rescue`` on every shard.  Side plan or inline replay of route-1 problems, and the side plan's
        chunk count, follow their number in the WHOLE batch: bit-identical under any sharding."""
        lib = _load()
        lib.clr_sharded_set_rescue.argtypes = [C.c_void_p, C.c_int]
        self._ok(lib.clr_sharded_set_rescue(self._h, int(mode)))

    def rescued(self):
        """Problems of the last fetched evaluation that took the checked route outside the main pass, over all shards."""
        lib = _load()
        n = C.c_int()
        lib.clr_sharded_get_rescue.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        self._ok(lib.clr_sharded_get_rescue(self._h, C.byref(n)))
        return n.value

    def set_certificate(self, max_gamma_over_mu=1e7, max_residual=1e-11, max_gamma=None, max_gamma_error=None):
        """``BatchedGP.set_certificate`` on every shard (the routing bounds of ill-conditioned problems)."""
        lib = _load()
        lib.clr_sharded_set_certificate.argtypes = [C.c_void_p] + [C.c_double] * 4
        touch = max_gamma is not None or max_gamma_error is not None
        self._ok(lib.clr_sharded_set_certificate(self._h, float(max_gamma_over_mu), float(max_residual),
                                                 float(1e4 if max_gamma is None else max_gamma) if touch else -1.0,
                                                 float(3e-9 if max_gamma_error is None else max_gamma_error) if touch else -1.0))

    def set_warm_start(self, mode=-1, forced_warmup=0):
        """``clr_batch_set_warm_start`` on every shard.  Activation (half of the problems of the WHOLE batch eligible) and
        the adaptation of the warm-up lengths are decided once for the batch: the same route -- the same bits -- under
        any sharding; ``mode=0`` switches the warm start off."""
        lib = _load()
        lib.clr_sharded_set_warm_start.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self._ok(lib.clr_sharded_set_warm_start(self._h, int(mode), int(forced_warmup)))

    def summarize_kernel(self):
        """The summarize kernel ALL shards run (resolved once for the whole batch)."""
        k = C.c_int()
        self._ok(_load().clr_sharded_get_summarize_kernel(self._h, C.byref(k)))
        return ("single wave", "role split", "role split, lazy decay")[k.value] if k.value >= 0 else "shards disagree"

    def set_series(self, t, diag, y, lengths=None):
        """``BatchedGP.set_series`` over the shards; ``lengths`` is ``(B,)`` for the whole batch."""
        lens = _lengths_arg(lengths, self.B, self.N)
        arrs, strides = [], []
        for a in (t, diag, y):
            a = _f64(a)
            if a.shape == (self.N,):
                strides.append(0)
            elif a.shape == (self.B, self.N):
                strides.append(self.N)
            else:
                raise ValueError("dimension mismatch")
            arrs.append(a)
        self._series_lengths = lens      # (set_noise_basis: the part of a row its finiteness check covers)
        lib = _load()
        if lens is None:
            self._ok(lib.clr_sharded_set_series(self._h, _ptr(arrs[0]), strides[0], _ptr(arrs[1]),
                                                strides[1], _ptr(arrs[2]), strides[2]))
        else:
            lib.clr_sharded_set_series_ragged.argtypes = [C.c_void_p, _dp, C.c_long, _dp, C.c_long, _dp, C.c_long, _ip]
            self._ok(lib.clr_sharded_set_series_ragged(self._h, _ptr(arrs[0]), strides[0], _ptr(arrs[1]), strides[1],
                                                       _ptr(arrs[2]), strides[2], lens.ctypes.data_as(_ip)))
        dtmin = C.c_double()
        lib.clr_sharded_get_series_order.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self._ok(lib.clr_sharded_get_series_order(self._h, C.byref(dtmin)))
        if dtmin.value < 0.0:       # (the device-side scans of the shards: see BatchedGP.set_series)
            lib.clr_sharded_clear_series.argtypes = [C.c_void_p]
            self._ok(lib.clr_sharded_clear_series(self._h))
            raise ValueError("the input coordinates must be sorted")

    @property
    def lengths(self):
        """The series lengths in force over the whole batch, ``(B,)``."""
        out = np.empty(self.B, dtype=np.int32)
        lib = _load()
        lib.clr_sharded_get_lengths.argtypes = [C.c_void_p, _ip]
        self._ok(lib.clr_sharded_get_lengths(self._h, out.ctypes.data_as(_ip)))
        out.flags.writeable = False
        return out

    def _coeff_blocks(self, a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter):
        try:
            blocks = [_f64(a_real, (self.B, self.J_real)), _f64(c_real, (self.B, self.J_real)),
                      _f64(a_comp, (self.B, self.J_comp)), _f64(b_comp, (self.B, self.J_comp)),
                      _f64(c_comp, (self.B, self.J_comp)), _f64(d_comp, (self.B, self.J_comp))]
        except ValueError:
            raise ValueError("dimension mismatch")
        jit = np.ascontiguousarray(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (self.B,)))
        return jit, blocks

    def set_coefficients(self, a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter=0.0):
        jit, blocks = self._coeff_blocks(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)
        self._last_params = None
        self._ok(_load().clr_sharded_set_coefficients(self._h, _ptr(jit), *[_ptr(b) for b in blocks]))

    def set_mean(self, mu):
        """A constant mean (a scalar, ``(B,)`` or ``None``), as :meth:`BatchedGP.set_mean`; every shard takes its
        slice (``clr_sharded_set_mean``)."""
        m, stride = _mean_arg(mu, self.B)
        self._ok(_load().clr_sharded_set_mean(self._h, None if m is None else _ptr(m), stride))

    set_mean_basis = BatchedGP.set_mean_basis
    set_mean_weights = BatchedGP.set_mean_weights
    grad_mean_weights = BatchedGP.grad_mean_weights
    fit_mean_weights = BatchedGP.fit_mean_weights
    # (set_mean_fit_tile / mean_fit_ms are BatchedGP's alone: the tile and the three device times belong to one plan's
    #  stream, and the sharded C ABI has no entry point for them -- every shard sizes its tile automatically, which no
    #  result depends on)

    set_noise_basis = BatchedGP.set_noise_basis
    set_noise_weights = BatchedGP.set_noise_weights
    grad_noise_weights = BatchedGP.grad_noise_weights

    def _set_noise_basis(self, K, a, stride):
        self._ok(_load().clr_sharded_set_noise_basis(self._h, K, None if a is None else _ptr(a), stride))

    def _set_noise_weights(self, a):
        self._ok(_load().clr_sharded_set_noise_weights(self._h, _ptr(a)))

    def _grad_noise_weights(self, ds, st):
        self._ok(_load().clr_sharded_grad_noise_weights(self._h, _ptr(ds), st.ctypes.data_as(_ip)))

    def noise_project_ms(self):
        """Device time of the projection pass of the last :meth:`grad_noise_weights`: the largest over the shards, which
        run concurrently (``clr_sharded_get_noise_project_ms``)."""
        ms = C.c_double()
        self._ok(_load().clr_sharded_get_noise_project_ms(self._h, C.byref(ms)))
        return ms.value

    set_amplitude_basis = BatchedGP.set_amplitude_basis
    set_amplitudes = BatchedGP.set_amplitudes
    log_amplitude_sum = BatchedGP.log_amplitude_sum
    grad_amplitudes = BatchedGP.grad_amplitudes

    def _set_amplitude_basis(self, K, a, stride):
        self._ok(_load().clr_sharded_set_amplitude_basis(self._h, K, None if a is None else _ptr(a), stride))

    def _set_amplitudes(self, a):
        self._ok(_load().clr_sharded_set_amplitudes(self._h, _ptr(a)))

    def _log_amplitude_sum(self, L):
        self._ok(_load().clr_sharded_get_log_amplitude_sum(self._h, _ptr(L)))

    def _grad_amplitudes(self, da, st):
        self._ok(_load().clr_sharded_grad_amplitudes(self._h, _ptr(da), st.ctypes.data_as(_ip)))

    def amplitude_project_ms(self):
        """Device time of the projection pass of the last :meth:`grad_amplitudes`: the largest over the shards, which
        run concurrently (``clr_sharded_get_amplitude_project_ms``)."""
        ms = C.c_double()
        self._ok(_load().clr_sharded_get_amplitude_project_ms(self._h, C.byref(ms)))
        return ms.value

    def _fit_mean_weights(self, p, w, cov, gram, quad, ld, st):
        self._ok(_load().clr_sharded_fit_mean_weights(self._h, p, _ptr(w), _ptr(cov), _ptr(gram), _ptr(quad), _ptr(ld),
                                                      st.ctypes.data_as(_ip)))

    def _set_mean_basis(self, K, a, stride):
        self._ok(_load().clr_sharded_set_mean_basis(self._h, K, None if a is None else _ptr(a), stride))

    def _set_mean_weights(self, a):
        self._ok(_load().clr_sharded_set_mean_weights(self._h, _ptr(a)))

    def _grad_mean_weights(self, dw, st):
        if not self._mean_K:
            raise RuntimeError("no basis is set: call set_mean_basis first")
        self._ok(_load().clr_sharded_grad_mean_weights(self._h, _ptr(dw), st.ctypes.data_as(_ip)))

    def grad_log_likelihood(self, mean_partial=False):
        """``(value[B], grad[B, 1 + 2 J_real + 4 J_comp], status[B])`` at the coefficients in force: every shard's
        plan gradient concurrently (``clr_sharded_grad``).  ``mean_partial=True``: ``(value, grad, dmean, status)``
        as :meth:`BatchedGP.grad_log_likelihood` (``clr_sharded_grad_mean``)."""
        NG = 1 + 2 * self.J_real + 4 * self.J_comp
        value, grad, st = np.empty(self.B), np.empty((self.B, NG)), np.empty(self.B, dtype=np.int32)
        lib = _load()
        if mean_partial:
            dmean = np.empty(self.B)
            self._ok(lib.clr_sharded_grad_mean(self._h, _ptr(value), _ptr(grad), _ptr(dmean), st.ctypes.data_as(_ip)))
            return value, grad, dmean, st
        lib.clr_sharded_grad.argtypes = [C.c_void_p, _dp, _dp, _ip]
        self._ok(lib.clr_sharded_grad(self._h, _ptr(value), _ptr(grad), st.ctypes.data_as(_ip)))
        return value, grad, st

    information = BatchedGP.information
    information_parameters = BatchedGP.information_parameters

    def _information(self, mean_partial, info, st):
        self._ok(_load().clr_sharded_information(self._h, mean_partial, _ptr(info), st.ctypes.data_as(_ip)))

    def set_information_tile(self, problems=0):
        """:meth:`BatchedGP.set_information_tile` on every shard."""
        self._ok(_load().clr_sharded_set_information_tile(self._h, int(problems)))

    def enqueue(self):
        self._ok(_load().clr_sharded_enqueue(self._h))

    def synchronize(self):
        self._ok(_load().clr_sharded_synchronize(self._h))

    def _out(self):
        return np.empty(self.B), np.empty(self.B), np.empty(self.B), np.empty(self.B, dtype=np.int32)

    def results(self):
        ll, ld, q, st = self._out()
        self._ok(_load().clr_sharded_get_results(self._h, _ptr(ll), _ptr(ld), _ptr(q), st.ctypes.data_as(_ip)))
        return ll, ld, q, st

    def log_likelihood(self):
        """Evaluate all B problems with the coefficients set last; returns ``(loglike, logdet, quad,
        status)`` (as :meth:`BatchedGP.log_likelihood`)."""
        self.enqueue()
        return self.results()

    def evaluate(self, a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter=0.0, mean=None, mean_weights=None,
                 noise_weights=None):
        """One optimiser / MCMC evaluation: new coefficients in, ``(loglike, logdet,
        quad, status)`` of all B problems out.  ``mean``, ``mean_weights``, ``noise_weights``: as
        :meth:`BatchedGP.evaluate` (``clr_sharded_evaluate_mean``; :meth:`set_mean_weights` / :meth:`set_noise_weights`
        first)."""
        _exclusive_means(mean, mean_weights)
        if mean_weights is not None:
            self.set_mean_weights(mean_weights)
        if noise_weights is not None:
            self.set_noise_weights(noise_weights)
        jit, blocks = self._coeff_blocks(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)
        ll, ld, q, st = self._out()
        self._last_params = None
        if mean is not None:
            m, stride = _mean_arg(mean, self.B)
            self._ok(_load().clr_sharded_evaluate_mean(self._h, _ptr(m), stride, _ptr(jit), *(
                [_ptr(b) for b in blocks] + [_ptr(ll), _ptr(ld), _ptr(q), st.ctypes.data_as(_ip)])))
            return ll, ld, q, st
        self._ok(_load().clr_sharded_evaluate(self._h, _ptr(jit), *([_ptr(b) for b in blocks] +
                                              [_ptr(ll), _ptr(ld), _ptr(q), st.ctypes.data_as(_ip)])))
        return ll, ld, q, st

    set_kernel = BatchedGP.set_kernel
    _params_arg = BatchedGP._params_arg

    def _set_kernel_handle(self, prog):
        self._ok(_load().clr_sharded_set_kernel(self._h, prog._k))

    def evaluate_parameters(self, params, mean=None, mean_weights=None, noise_weights=None):
        """:meth:`BatchedGP.evaluate_parameters` over the shards (``clr_sharded_evaluate_params``): every shard forms the
        coefficients of its slice of ``params`` on its own device."""
        _exclusive_means(mean, mean_weights)
        if mean_weights is not None:
            self.set_mean_weights(mean_weights)
        if noise_weights is not None:
            self.set_noise_weights(noise_weights)
        p = self._params_arg(params)
        ll, ld, q, st = self._out()
        m, stride = _mean_arg(mean, self.B)
        self._last_params = None
        self._ok(_load().clr_sharded_evaluate_params(self._h, _ptr(p), None if m is None else _ptr(m), stride,
                                                     _ptr(ll), _ptr(ld), _ptr(q), st.ctypes.data_as(_ip)))
        self._last_params = p
        return ll, ld, q, st

    def grad_parameters(self, mean_partial=False):
        """:meth:`BatchedGP.grad_parameters` over the shards (``clr_sharded_grad_params``)."""
        P = self.kernel_program.n_params + (1 if mean_partial else 0)
        value, grad, st = np.empty(self.B), np.empty((self.B, P)), np.empty(self.B, dtype=np.int32)
        self._ok(_load().clr_sharded_grad_params(self._h, _ptr(value), _ptr(grad), st.ctypes.data_as(_ip), int(bool(mean_partial))))
        return value, grad, st

    def coefficients(self):
        """The coefficients in force on every shard (``clr_sharded_get_coefficients``), as :meth:`BatchedGP.coefficients`."""
        B, JR, JC = self.B, self.J_real, self.J_comp
        out = [np.empty((B, JR)), np.empty((B, JR))] + [np.empty((B, JC)) for _ in range(4)]
        jit = np.empty(B)
        self._ok(_load().clr_sharded_get_coefficients(self._h, _ptr(jit), *[_ptr(a) for a in out]))
        return tuple(out) + (jit,)

    def materialize(self):
        """A materialising evaluation on every shard (``clr_sharded_materialize``): ``(loglike, logdet, quad, status)``
        as :meth:`log_likelihood`, and every shard's factor left in its HBM for :meth:`solve`, :meth:`dot_L`,
        :meth:`sample` and :meth:`predict`."""
        ll, ld, q, st = self._out()
        lib = _load()
        lib.clr_sharded_materialize.argtypes = [C.c_void_p, _dp, _dp, _dp, _ip]
        self._ok(lib.clr_sharded_materialize(self._h, _ptr(ll), _ptr(ld), _ptr(q), st.ctypes.data_as(_ip)))
        return ll, ld, q, st

    def _rhs(self, b):
        b = _f64(b)
        if b.ndim not in (2, 3) or b.shape[0] != self.B or b.shape[-1] != self.N:
            raise ValueError("dimension mismatch")
        return b, (1 if b.ndim == 2 else b.shape[1])

    def solve(self, b=None):
        """``K_p^-1 b_p`` for every problem (as :meth:`BatchedGP.solve`), every shard on its slice."""
        lib = _load()
        lib.clr_sharded_solve.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        if b is None:
            x = np.empty((self.B, self.N))
            self._ok(lib.clr_sharded_solve(self._h, 1, None, _ptr(x)))
            return x
        b, nrhs = self._rhs(b)
        x = np.empty(b.shape)
        self._ok(lib.clr_sharded_solve(self._h, int(nrhs), _ptr(b), _ptr(x)))
        return x

    def dot_L(self, z):
        """``L_p z_p`` for every problem (as :meth:`BatchedGP.dot_L`), every shard on its slice."""
        lib = _load()
        lib.clr_sharded_dot_L.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        z, nrhs = self._rhs(z)
        y = np.empty(z.shape)
        self._ok(lib.clr_sharded_dot_L(self._h, int(nrhs), _ptr(z), _ptr(y)))
        return y

    sample = BatchedGP.sample

    def dot(self, z):
        """``K_p z_p`` for every problem (as :meth:`BatchedGP.dot`), every shard on its slice."""
        lib = _load()
        lib.clr_sharded_dot.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
        z, nrhs = self._rhs(z)
        y = np.empty(z.shape)
        self._ok(lib.clr_sharded_dot(self._h, int(nrhs), _ptr(z), _ptr(y)))
        return y

    def predict(self, xs, return_var=False, mean_basis=None, method="solve"):
        """The conditional mean of every problem at ``xs`` (``(M,)`` shared or ``(B, M)``) and, with ``return_var=True``,
        the conditional variance beside it, as :meth:`BatchedGP.predict` (``mean_basis``: the linear mean's basis at
        ``xs``, required while one is in force; ``method``: the variance's route, ``"solve"`` or ``"recurrence"``)."""
        _predict_method(method)
        lib = _load()
        lib.clr_sharded_predict.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
        xs = _f64(xs)
        if xs.ndim == 1:
            stride = 0
        elif xs.ndim == 2 and xs.shape[0] == self.B:
            stride = xs.shape[1]
        else:
            raise ValueError("dimension mismatch")
        M = xs.shape[-1]
        model = _linear_mean_at(self, mean_basis, M)
        pred = np.empty((self.B, M))
        self._ok(lib.clr_sharded_predict(self._h, int(M), _ptr(xs), stride, _ptr(pred)))
        if model is not None:
            pred = model + pred
        if not return_var:
            return pred
        entry = lib.clr_sharded_predict_var_recurrence if method == "recurrence" else lib.clr_sharded_predict_var
        entry.argtypes = [C.c_void_p, C.c_int, _dp, C.c_long, _dp]
        var = np.empty((self.B, M))
        self._ok(entry(self._h, int(M), _ptr(xs), stride, _ptr(var)))
        return pred, var

    def one_step_ahead(self, b=None):
        """The one-step-ahead residuals of every problem (as :meth:`BatchedGP.one_step_ahead`), every shard on its slice."""
        return _one_step_ahead(self, "clr_sharded_one_step_ahead", lambda st: self._ok(st), b)

    def forecast(self, xs, return_var=False, mean_basis=None):
        """The causal forecast of every problem at ``xs`` (as :meth:`BatchedGP.forecast`), every shard on its slice."""
        return _forecast(self, "clr_sharded_forecast", lambda st: self._ok(st), xs, return_var, mean_basis)

    def periodogram(self, omega, offset=False, t_ref=0.0, min_pivot=1e-10, return_gram=False):
        """The periodogram under the plan's covariance (as :meth:`BatchedGP.periodogram`), every shard on its slice: the
        unsharded plan's bits."""
        return _periodogram(self, "clr_sharded_periodogram", lambda st: self._ok(st), omega, offset, t_ref, min_pivot, return_gram)

    def set_periodogram_tile(self, frequencies=0):
        """Frequencies per tile of :meth:`periodogram` on every shard."""
        self._ok(_load().clr_sharded_set_periodogram_tile(self._h, int(frequencies)))

    def periodogram_ms(self):
        """Device time of the last :meth:`periodogram`'s kernels: the largest over the shards, which run concurrently."""
        ms = C.c_double(0.0)
        self._ok(_load().clr_sharded_get_periodogram_ms(self._h, C.byref(ms)))
        return ms.value

    def predict_terms(self, xs, groups=None, return_var=False):
        """The posterior of each group of kernel terms at ``xs`` (as :meth:`BatchedGP.predict_terms`), every shard on
        its slice."""
        return _predict_terms(self, "clr_sharded_predict_terms", lambda st: self._ok(st), xs, groups, return_var)

    def predict_cov(self, xs):
        """The posterior covariance between the points ``xs`` of every problem (as :meth:`BatchedGP.predict_cov`), every
        shard on its slice."""
        return _predict_cov(self, "clr_sharded_predict_cov", lambda st: self._ok(st), xs)

    def sample_conditional(self, xs, size=None, regularize=0.0, min_pivot=1e-10, mean_basis=None, random=None, normals=None,
                           return_status=False):
        """Joint draws at the points ``xs`` given the data (as :meth:`BatchedGP.sample_conditional`), every shard on its
        slice."""
        return _sample_conditional(self, "clr_sharded_sample_conditional", lambda st: self._ok(st), xs, size, regularize,
                                   min_pivot, mean_basis, random, normals, return_status)

    def set_conditional_tile(self, problems=0):
        """Problems per tile of :meth:`predict_cov` and :meth:`sample_conditional` on every shard."""
        self._ok(_load().clr_sharded_set_conditional_tile(self._h, int(problems)))

    inverse_diagonal = BatchedGP.inverse_diagonal
    leave_one_out = BatchedGP.leave_one_out

    def _leave_one_out(self, c, alpha, logpdf, st):
        self._ok(_load().clr_sharded_leave_one_out(self._h, *_loo_args(c, alpha, logpdf, st)))

    def run_timed(self, steps):
        """``steps`` evaluations on every shard concurrently; per-shard HIP-event ms."""
        n = _load().clr_sharded_num_shards(self._h)
        ms = np.zeros(n)
        self._ok(_load().clr_sharded_run_timed(self._h, int(steps), _ptr(ms)))
        return ms


def batch_log_likelihood(a_real, c_real, a_comp, b_comp, c_comp, d_comp, t, diag, y,
                         jitter=0.0, device=0, nchunk=0):
    """One-shot batched evaluation; see :class:`BatchedGP`."""
    a_real = np.atleast_2d(_f64(a_real))
    B, J_real = a_real.shape
    a_comp = _f64(a_comp).reshape(B, -1)
    N = np.asarray(t).shape[-1]
    plan = BatchedGP(B, N, J_real, a_comp.shape[1], device=device)
    try:
        if nchunk:
            plan.set_chunks(nchunk)
        plan.set_series(t, diag, y)
        plan.set_coefficients(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)
        return plan.log_likelihood()
    finally:
        plan.close()


def batch_grad_log_likelihood(a_real, c_real, a_comp, b_comp, c_comp, d_comp, t, diag, y, jitter=0.0, device=0):
    """Value and coefficient gradient of B problems at once (``clr_batch_grad_log_likelihood``): returns
    ``(value[B], grad[B, 1 + 2 J_real + 4 J_comp], status[B])`` with the reference's conventions per
    problem (``CholeskySolver.grad_log_likelihood``, solver.cpp:347-463; its ``pi log N`` constant)."""
    lib = _load()
    a_real = np.atleast_2d(_f64(a_real))
    B, JR = a_real.shape
    a_comp = _f64(a_comp).reshape(B, -1)
    JC = a_comp.shape[1]
    blocks = [a_real, _f64(c_real, (B, JR)), a_comp, _f64(b_comp, (B, JC)), _f64(c_comp, (B, JC)), _f64(d_comp, (B, JC))]
    N = np.asarray(t).shape[-1]
    arrs, strides = [], []
    for a in (t, diag, y):
        a = _f64(a)
        strides.append(0 if a.shape == (N,) else N)
        if a.shape not in ((N,), (B, N)):
            raise ValueError("dimension mismatch")
        arrs.append(a)
    jit = np.ascontiguousarray(np.broadcast_to(np.asarray(jitter, dtype=np.float64), (B,)))
    NG = 1 + 2 * JR + 4 * JC
    value, grad, st = np.empty(B), np.empty((B, NG)), np.empty(B, dtype=np.int32)
    lib.clr_batch_grad_log_likelihood.argtypes = ([C.c_int] * 4 + [_dp] * 7 + [_dp, C.c_long] * 3 +
                                                  [_dp, _dp, _ip, C.c_int])
    _check(lib.clr_batch_grad_log_likelihood(B, N, JR, JC, _ptr(jit), *[_ptr(b) for b in blocks],
                                             _ptr(arrs[0]), strides[0], _ptr(arrs[1]), strides[1],
                                             _ptr(arrs[2]), strides[2], _ptr(value), _ptr(grad),
                                             st.ctypes.data_as(_ip), int(device)))
    return value, grad, st


# ---- a `terms` kernel as a program (include/celerite_hip.h, "kernel programs") -------------------------------------
_KP_REAL, _KP_COMPLEX, _KP_COMPLEX_B0, _KP_SHO_OVER, _KP_SHO_UNDER, _KP_MATERN32, _KP_JITTER = 1, 2, 3, 4, 5, 6, 7
_KP_MUL_RR, _KP_MUL_RC, _KP_MUL_CC = 8, 9, 10


class CompiledKernel(object):
    """A ``terms`` kernel compiled by :func:`compile_kernel`: the program (``ops``, ``consts``), its input size
    ``n_params`` (= ``kernel.vector_size`` at compile time) and output shape ``(J_real, J_comp)``, evaluated through
    ``clr_kernel_coefficients`` / ``clr_kernel_jacobian`` on the host -- no GPU needed -- and by the plans on the device.
    ``groups``: one tuple of coefficient-term indices (``kernel.coefficients`` order: real terms first, then the complex
    ones) per top-level summand of the tree -- a kernel that is no sum is one group, a ``JitterTerm`` summand gives
    ``()``, an overdamped ``SHOTerm`` its two real terms, a product all the terms it expands to --, ready for
    ``plan.predict_terms(xs, groups=compiled.groups)``."""

    def __init__(self, kernel, ops, consts, n_params, J_real, J_comp, groups=None):
        self.kernel = kernel
        # one tuple of coefficient-term indices per top-level summand of the tree (predict_terms' `groups`)
        self.groups = tuple(tuple(int(k) for k in g) for g in groups) if groups is not None else None
        self.ops = np.ascontiguousarray(ops, dtype=np.int32)
        self.consts = np.ascontiguousarray(consts, dtype=np.float64)
        self.n_params, self.J_real, self.J_comp = int(n_params), int(J_real), int(J_comp)
        self._k = _create_kernel(self.ops, self.consts, self.n_params, self.J_real, self.J_comp)

    def close(self):
        if getattr(self, "_k", None):
            _load().clr_kernel_destroy(self._k)
            self._k = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _params(self, parameter_vectors):
        p = np.ascontiguousarray(np.atleast_2d(parameter_vectors), dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.n_params:
            raise ValueError("dimension mismatch")
        return p

    def coefficients(self, parameter_vectors, status=False):
        """``(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)`` of the draws ``(B, n_params)``.  A draw the
        program refuses raises ``ValueError`` -- or, with ``status=True``, is a row of NaN and the per-draw status array
        is returned as an eighth element."""
        p = self._params(parameter_vectors)
        B, JR, JC = p.shape[0], self.J_real, self.J_comp
        out = [np.empty((B, JR)), np.empty((B, JR))] + [np.empty((B, JC)) for _ in range(4)] + [np.empty(B)]
        st = np.zeros(B, dtype=np.int32)
        _check(_load().clr_kernel_coefficients(self._k, B, _ptr(p), *([_ptr(a) for a in out] + [st.ctypes.data_as(_ip)])))
        if status:
            return tuple(out) + (st,)
        if st.any():
            raise ValueError("the draws do not share one (J_real, J_comp) shape, or are not finite")
        return tuple(out)

    def jacobian(self, parameter_vectors, status=False):
        """``(jac[B, P, 2 J_real + 4 J_comp], jitter_jac[B, P])`` of the draws, as
        :func:`kernel_coefficient_jacobian_table` lays them out."""
        p = self._params(parameter_vectors)
        B, P, NC = p.shape[0], self.n_params, 2 * self.J_real + 4 * self.J_comp
        jac, jj = np.empty((B, P, NC)), np.empty((B, P))
        st = np.zeros(B, dtype=np.int32)
        _check(_load().clr_kernel_jacobian(self._k, B, _ptr(p), _ptr(jac), _ptr(jj), st.ctypes.data_as(_ip)))
        if status:
            return jac, jj, st
        if st.any():
            raise ValueError("the draws do not share one (J_real, J_comp) shape, or are not finite")
        return jac, jj


def _create_kernel(ops, consts, n_params, J_real, J_comp):
    """``clr_kernel_create``: the handle, or ``RuntimeError`` (``CLR_INVALID_ARGUMENT``) for a malformed program."""
    lib = _load()
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    consts = np.ascontiguousarray(consts, dtype=np.float64)
    k = C.c_void_p()
    _check(lib.clr_kernel_create(len(ops), ops.ctypes.data_as(_ip), len(consts), _ptr(consts), int(n_params),
                                 int(J_real), int(J_comp), C.byref(k)))
    return k


def compile_kernel(kernel):
    """Compile a ``terms`` tree of built-in terms -- ``RealTerm``, ``ComplexTerm``, ``SHOTerm``, ``Matern32Term``,
    ``JitterTerm``, sums and products of them, nested in any way -- into a :class:`CompiledKernel`.

    The program's input is the kernel's unfrozen parameter vector (``get_parameter_vector()`` order); frozen
    parameters are baked in with their current value, and every ``SHOTerm`` is fixed in the regime (Q below or not
    below 1/2) of its current value, which fixes ``(J_real, J_comp)``.  The output order is that of
    ``kernel.coefficients``.  A term whose class overrides the coefficient formulas, or a user-defined term, cannot be
    compiled: ``ValueError`` naming it."""
    from . import terms

    full = np.asarray(kernel.get_parameter_vector(include_frozen=True), dtype=np.float64)
    mask = np.asarray(kernel.unfrozen_mask, dtype=bool)
    unfrozen_index = np.cumsum(mask) - 1
    ops, consts = [], []
    count = {"r": 0, "c": 0, "tr": 0, "tc": 0}
    summands = []                                          # (real ids, complex ids) per top-level summand

    def const(x):
        consts.append(float(x))
        return len(consts) - 1

    def ref(i):
        return int(unfrozen_index[i]) if mask[i] else -(const(full[i]) + 1)

    def dst(kind, top):
        key = kind if top else "t" + kind
        count[key] += 1
        return count[key] - 1 if top else -count[key]

    def cannot(term):
        raise ValueError("cannot compile %s %r: only the built-in terms with their own coefficient formulas"
                         % (type(term).__name__, term))

    def emit(term, at, top):
        """instructions of `term` (its parameters at `at` in the full vector); returns its (real, complex) term ids"""
        if isinstance(term, terms.TermSum):
            if not term._formulas_are(terms.TermSum):
                cannot(term)
            reals, comps = [], []
            for sub in term.terms:
                r, c = emit(sub, at, top)
                if term is kernel:
                    summands.append((r, c))
                reals += r
                comps += c
                at += sub.full_size
            return reals, comps
        if isinstance(term, terms.TermProduct):
            if not term._formulas_are(terms.TermProduct):
                cannot(term)
            k1, k2 = term.models["k1"], term.models["k2"]
            r1, c1 = emit(k1, at, False)
            r2, c2 = emit(k2, at + k1.full_size, False)
            tmp = lambda ids: [-(i + 1) for i in ids]      # (a temporary's index as a product reads it)
            r1, c1, r2, c2 = tmp(r1), tmp(c1), tmp(r2), tmp(c2)
            reals, comps = [], []
            for x in r1:
                for y in r2:
                    reals.append(dst("r", top))
                    ops.extend([_KP_MUL_RR, reals[-1], x, y])
            for rs, cs in ((r1, c2), (r2, c1)):
                for x in rs:
                    for y in cs:
                        comps.append(dst("c", top))
                        ops.extend([_KP_MUL_RC, comps[-1], x, y])
            for x in c1:
                for y in c2:
                    dm, dp = dst("c", top), dst("c", top)
                    comps += [dm, dp]
                    ops.extend([_KP_MUL_CC, dm, dp, x, y])
            return reals, comps
        if isinstance(term, terms.JitterTerm) and term._formulas_are(terms.JitterTerm):
            ops.extend([_KP_JITTER, ref(at)])
            return [], []
        if isinstance(term, terms.RealTerm) and term._formulas_are(terms.RealTerm):
            d = dst("r", top)
            ops.extend([_KP_REAL, d, ref(at), ref(at + 1)])
            return [d], []
        if isinstance(term, terms.ComplexTerm) and term._formulas_are(terms.ComplexTerm):
            d = dst("c", top)
            if term.fit_b:
                ops.extend([_KP_COMPLEX, d] + [ref(at + i) for i in range(4)])
            else:
                ops.extend([_KP_COMPLEX_B0, d] + [ref(at + i) for i in range(3)])
            return [], [d]
        if isinstance(term, terms.SHOTerm) and term._formulas_are(terms.SHOTerm):
            if np.exp(full[at + 1]) < 0.5:
                d0, d1 = dst("r", top), dst("r", top)
                ops.extend([_KP_SHO_OVER, d0, d1] + [ref(at + i) for i in range(3)])
                return [d0, d1], []
            d = dst("c", top)
            ops.extend([_KP_SHO_UNDER, d] + [ref(at + i) for i in range(3)])
            return [], [d]
        if isinstance(term, terms.Matern32Term) and term._formulas_are(terms.Matern32Term):
            d = dst("c", top)
            ops.extend([_KP_MATERN32, d, ref(at), ref(at + 1), const(term.eps)])
            return [], [d]
        cannot(term)

    whole = emit(kernel, 0, True)
    if not isinstance(kernel, terms.TermSum):
        summands.append(whole)
    if max(count["tr"], count["tc"]) > 16:
        raise ValueError("cannot compile %r: more than 16 factor terms of one kind inside products" % (kernel,))
    groups = [list(r) + [count["r"] + k for k in c] for r, c in summands]
    return CompiledKernel(kernel, ops, consts, int(mask.sum()), count["r"], count["c"], groups)


def _compiled_for(kernel, compiled):
    """The program behind the ``compiled=`` switch of the two table functions: None for the Python loop."""
    if compiled is False:
        return None
    if isinstance(compiled, CompiledKernel):
        return compiled
    try:
        return compile_kernel(kernel)
    except ValueError:
        if compiled is None:
            return None
        raise


def kernel_coefficient_table(kernel, parameter_vectors, compiled=False):
    """Coefficient tables for many hyper-parameter draws of one ``terms.Term``.

    ``parameter_vectors``: ``(B, kernel.vector_size)``.  Returns
    ``(a_real, c_real, a_comp, b_comp, c_comp, d_comp, jitter)`` ready for
    :meth:`BatchedGP.set_coefficients`.  The kernel's parameters are restored.
    Every draw must give the same number of real / complex terms.

    ``compiled``: ``False`` (default) the Python loop over the draws; ``True`` the compiled program
    (:func:`compile_kernel`, evaluated by ``clr_kernel_coefficients`` -- equal to the loop up to the last bits of
    ``exp``); ``None`` the program when the kernel can be compiled, the loop otherwise.  The program's shape is the one
    of the kernel's CURRENT parameters; draws of another shape raise ``ValueError`` either way.
    """
    prog = _compiled_for(kernel, compiled)
    if prog is not None:
        return prog.coefficients(parameter_vectors)
    saved = kernel.get_parameter_vector()
    rows, jit = [], []
    try:
        for p in np.atleast_2d(parameter_vectors):
            kernel.set_parameter_vector(p)
            rows.append([np.array(b, dtype=np.float64) for b in kernel.coefficients])
            jit.append(float(kernel.jitter))
    finally:
        kernel.set_parameter_vector(saved)
    shapes = set(tuple(len(b) for b in r) for r in rows)
    if len(shapes) != 1:
        raise ValueError("the draws do not share one (J_real, J_comp) shape")
    blocks = [np.array([r[i] for r in rows]).reshape(len(rows), -1) for i in range(6)]
    return tuple(blocks) + (np.array(jit),)


def kernel_coefficient_jacobian_table(kernel, parameter_vectors, compiled=False):
    """The chain rule's other half for :func:`kernel_coefficient_table`: for every draw the Jacobian of the
    coefficients with respect to the kernel's (unfrozen) parameters.

    Returns ``(jac, jitter_jac)``: ``jac[b, p, c]`` = d coefficient ``c`` / d parameter ``p`` with the coefficients
    in the order of the batched gradient's columns 1.. (``a_real, c_real, a_comp, b_comp, c_comp, d_comp``, each
    block contiguous: ``Term.get_coeffs_jacobian``, terms.py:206-215) and ``jitter_jac[b, p]`` = d jitter / d
    parameter (``get_jitter_jacobian``, :197-204).  Built-in terms need no autograd (their formulas are evaluated
    on dual numbers, ``terms._dual_coefficients``).  ``compiled``: as in :func:`kernel_coefficient_table`
    (``clr_kernel_jacobian``: the same formulas on duals)."""
    prog = _compiled_for(kernel, compiled)
    if prog is not None:
        return prog.jacobian(parameter_vectors)
    saved = kernel.get_parameter_vector()
    jac, jit = [], []
    try:
        for p in np.atleast_2d(parameter_vectors):
            kernel.set_parameter_vector(p)
            if kernel._has_coeffs:
                jac.append(np.asarray(kernel.get_coeffs_jacobian(), dtype=np.float64))
            else:
                jac.append(np.zeros((len(p), 0)))
            jit.append(np.asarray(kernel.get_jitter_jacobian(), dtype=np.float64) if kernel._has_jitter
                       else np.zeros(len(p)))
    finally:
        kernel.set_parameter_vector(saved)
    return np.array(jac), np.array(jit)


def chain_gradient(grad, jac, jitter_jac, dmean=None):
    """``d loglike / d parameters`` of every draw, ``[B, P]``, from the batched coefficient gradient ``grad``
    (``[B, 1 + 2 J_real + 4 J_comp]``: column 0 the jitter partial, as ``BatchedGP.grad_log_likelihood`` returns
    it) and the tables of :func:`kernel_coefficient_jacobian_table` (what ``GP.grad_log_likelihood`` does for one
    problem, celerite.py:286-305).  ``dmean`` (``[B]``, ``grad_log_likelihood(mean_partial=True)``): appended as the
    last column, the reference's order -- the kernel's parameters, then the constant mean's (celerite.py:224-227);
    ``[B, P + 1]``."""
    grad = np.asarray(grad, dtype=np.float64)
    full = np.einsum("bpc,bc->bp", jac, grad[:, 1:]) + jitter_jac * grad[:, :1]
    if dmean is None:
        return full
    dmean = np.asarray(dmean, dtype=np.float64).reshape(-1, 1)
    if dmean.shape[0] != full.shape[0]:
        raise ValueError("dimension mismatch")
    return np.concatenate([full, dmean], axis=1)


def chain_information(info, jac, jitter_jac, mean_partial=False):
    """The information matrix in the kernel's parameters, ``[B, P, P]``, from the batched coefficient matrix ``info``
    (``[B, M, M]``, ``BatchedGP.information``) and the tables of :func:`kernel_coefficient_jacobian_table`: the bilinear
    twin of :func:`chain_gradient` -- per draw ``T = [jitter_jac | jac]`` (``[P, M]``) and ``T info T^T``.
    ``mean_partial=True``: ``info`` is ``[B, M + 1, M + 1]`` with the constant mean last, which passes through;
    ``[B, P + 1, P + 1]``."""
    info = np.asarray(info, dtype=np.float64)
    jac = np.asarray(jac, dtype=np.float64)
    jitter_jac = np.asarray(jitter_jac, dtype=np.float64)
    extra = 1 if mean_partial else 0
    if (info.ndim != 3 or jac.ndim != 3 or jitter_jac.shape != jac.shape[:2] or info.shape[0] != jac.shape[0]
            or info.shape[1] != info.shape[2] or info.shape[1] != 1 + jac.shape[2] + extra):
        raise ValueError("dimension mismatch")
    B, P = jac.shape[:2]
    T = np.zeros((B, P + extra, info.shape[1]))
    T[:, :P, 0] = jitter_jac
    T[:, :P, 1:1 + jac.shape[2]] = jac
    if mean_partial:
        T[:, P, -1] = 1.0
    return np.einsum("bpi,bij,bqj->bpq", T, info, T)
