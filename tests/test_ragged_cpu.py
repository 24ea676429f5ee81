# -*- coding: utf-8 -*-
"""No GPU: per-problem series lengths on batched plans (``clr_batch_set_series_ragged``) -- the host-side validation of
the ``lengths`` argument, and the new entries of the C ABI (declared in the header, exported by the library, reachable
from the Python classes)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from celerite_amd import batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["clr_batch_set_series_ragged", "clr_batch_get_lengths", "clr_sharded_set_series_ragged", "clr_sharded_get_lengths"]


def test_lengths_arg_accepts_what_the_interface_promises():
    assert batch._lengths_arg(None, 4, 10) is None
    for given in ([1, 10, 5, 9], (1, 10, 5, 9), np.array([1, 10, 5, 9], dtype=np.int64), np.array([1, 10, 5, 9], dtype=np.uint8),
                  np.array([1.0, 10.0, 5.0, 9.0])):
        out = batch._lengths_arg(given, 4, 10)
        assert out.dtype == np.int32 and out.flags.c_contiguous and out.tolist() == [1, 10, 5, 9]
    # a strided view comes back contiguous; the bounds themselves are lengths
    assert batch._lengths_arg(np.arange(1, 9)[::2], 4, 10).tolist() == [1, 3, 5, 7]
    assert batch._lengths_arg([1], 1, 1).tolist() == [1]
    assert batch._lengths_arg(np.full(3, 7), 3, 7).tolist() == [7, 7, 7]


@pytest.mark.parametrize("given", [[1, 2, 3], [1, 2, 3, 4, 5], 3, [[1, 2], [3, 4]], np.ones((4, 1), dtype=int), []])
def test_lengths_arg_refuses_a_wrong_shape(given):
    with pytest.raises(ValueError, match="dimension mismatch"):
        batch._lengths_arg(given, 4, 10)


@pytest.mark.parametrize("given,what", [([0, 1, 2, 3], r"length 0 of problem 0 is outside \[1, N = 10\]"),
                                        ([1, 2, 3, 11], r"length 11 of problem 3 is outside \[1, N = 10\]"),
                                        ([1, -5, 3, 4], r"length -5 of problem 1"),
                                        ([1, 2, 2 ** 40, 4], r"problem 2 is outside"),
                                        ([1.5, 2, 3, 4], "must be integers"),
                                        ([np.nan, 2, 3, 4], "must be integers"),
                                        ([np.inf, 2, 3, 4], "must be integers"),
                                        ([True, True, True, True], "must be integers"),
                                        (["1", "2", "3", "4"], "must be integers"),
                                        ([1 + 0j, 2, 3, 4], "must be integers")])
def test_lengths_arg_refuses_what_is_not_a_length(given, what):
    with pytest.raises(ValueError, match=what):
        batch._lengths_arg(given, 4, 10)


def test_new_entries_are_declared_and_exported():
    import __graft_entry__ as entry

    declared = entry.declared_symbols()
    lib = ctypes.CDLL(batch.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(lib, s), s
    header = open(os.path.join(ROOT, "include", "celerite_hip.h")).read()
    # the ragged entries take the series as clr_*_set_series does, then the lengths
    for kind in ("batch", "sharded"):
        m = re.search(r"int clr_%s_set_series_ragged\((.*?)\);" % kind, header, flags=re.S)
        assert m and re.sub(r"\s+", " ", m.group(1)).endswith("const double* y, long y_stride, const int* lengths")
        assert re.search(r"int clr_%s_get_lengths\(const clr_%s\* h, int\* lengths\);" % (kind, kind), header)


def test_python_interface_has_lengths():
    for cls in (batch.BatchedGP, batch.ShardedBatchedGP):
        sig = inspect.signature(cls.set_series)
        assert list(sig.parameters) == ["self", "t", "diag", "y", "lengths"] and sig.parameters["lengths"].default is None
        assert isinstance(cls.lengths, property) and cls.lengths.fset is None
