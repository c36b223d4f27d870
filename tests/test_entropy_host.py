"""Entropy / mutual information without a GPU: the C ABI's argument checks and texts, BN_ERR_NO_DEVICE
for valid input, the numpy restatement of transinformation.hpp against hand values, and the C++14
drop-in (include/bayesian/evaluation/transinformation.hpp) compiling over include/compat."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp", "test_evaluation.cpp")
LIBDIR = os.path.join(ROOT, "bayesiannetwork_amd")


def np_entropy(pats, counts, variables):
    """H = -sum (c/N) log2(c/N) over the non-zero cells of the joint table of `variables` (duplicates
    collapse), fp64 -- transinformation.hpp:35-39."""
    vs = sorted(set(int(v) for v in np.atleast_1d(variables)))
    counts = np.asarray(counts, np.uint64)
    if not vs:
        return 0.0
    sub = np.asarray(pats)[:, vs].astype(np.int64)
    if np.prod((sub.max(axis=0) + 1).astype(float)) < 2.0 ** 62:
        key = np.zeros(len(counts), np.int64)
        for j in range(sub.shape[1]):
            key = key * (int(sub[:, j].max()) + 1) + sub[:, j]
        _, inv = np.unique(key, return_inverse=True)
    else:
        _, inv = np.unique(sub, axis=0, return_inverse=True)
    cells = np.zeros(int(inv.max()) + 1, np.uint64)
    np.add.at(cells, inv.ravel(), counts)
    cells = cells[cells > 0]
    p = cells.astype(np.float64) / float(int(counts.sum(dtype=np.uint64)))
    return float(-(p * np.log2(p)).sum())


def build_cpp(tmp_path):
    exe = str(tmp_path / "test_evaluation")
    cmd = ["g++", "-std=c++14", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "include", "compat"),
           CPP, "-L", LIBDIR, "-lbn_mi355x", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _create(lib, P, n, pats, counts, k, device=0):
    h = ctypes.c_void_p()
    rc = lib.bn_info_create(P, n, pats, counts, k, device, ctypes.byref(h))
    return rc, lib.bn_last_error().decode(), h


def test_argument_errors_and_texts(bnlib):
    from bayesiannetwork_amd import _lib
    u8 = lambda a: a.ctypes.data_as(_lib.u8p)                              # noqa: E731
    u64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))     # noqa: E731
    i32 = lambda a: a.ctypes.data_as(_lib.i32p)                            # noqa: E731
    pats, cnt, k = np.zeros((4, 2), np.uint8), np.ones(4, np.uint64), np.array([2, 3], np.int32)
    cases = [
        ((4, 2, None, u64(cnt), i32(k)), "bad pattern table"),
        ((4, 2, u8(pats), None, i32(k)), "bad pattern table"),
        ((4, 2, u8(pats), u64(cnt), None), "null arity array"),
        ((4, 0, u8(pats), u64(cnt), i32(k)), "n_vars must be in 1..2^23"),
        ((-1, 2, u8(pats), u64(cnt), i32(k)), "n_patterns < 0"),
        ((4, 2, u8(pats), u64(cnt), i32(np.array([2, 0], np.int32))), "arity must be in 1..255"),
        ((4, 2, u8(pats), u64(cnt), i32(np.array([256, 2], np.int32))), "arity must be in 1..255"),
        ((4, 2, u8(pats), u64(np.zeros(4, np.uint64)), i32(k)), "empty sample table"),
        ((0, 2, None, None, i32(k)), "empty sample table"),
        ((2, 2, u8(pats), u64(np.array([1 << 63, 1 << 63], np.uint64)), i32(k)), "does not fit in 64 bits"),
    ]
    for args, text in cases:
        rc, msg, h = _create(bnlib, *args)
        assert rc == _lib.BN_ERR_ARG and text in msg, (text, rc, msg)
        assert not h.value
    assert bnlib.bn_info_create(4, 2, u8(pats), u64(cnt), i32(k), 0, None) == _lib.BN_ERR_ARG
    for fn, args in (("bn_info_entropy", (None, 1, i32(k), 0, None)), ("bn_info_pair_entropies", (None, 1, None, None, None, None)),
                     ("bn_info_pair_counts", (None, 1, i32(k), None))):
        assert getattr(bnlib, fn)(*args) == _lib.BN_ERR_ARG
    bnlib.bn_info_destroy(None)


def test_valid_input_without_device(bnlib):
    """Valid arguments on a box with no GPU: BN_ERR_NO_DEVICE (checked after the arguments)."""
    from bayesiannetwork_amd import _lib
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is visible here; the no-device answer is checked on CPU-only boxes")
    pats, cnt, k = np.zeros((4, 2), np.uint8), np.ones(4, np.uint64), np.array([2, 3], np.int32)
    rc, msg, h = _create(bnlib, 4, 2, pats.ctypes.data_as(_lib.u8p), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                         k.ctypes.data_as(_lib.i32p))
    assert rc == _lib.BN_ERR_NO_DEVICE, (rc, msg)
    assert not h.value


def test_restatement_hand_values():
    # two uniform independent bits: H(x, y) = 2, MI = 0
    pats = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], np.uint8)
    c = np.full(4, 5, np.uint64)
    assert np_entropy(pats, c, [0]) == 1.0 and np_entropy(pats, c, [0, 1]) == 2.0
    assert np_entropy(pats, c, [0]) + np_entropy(pats, c, [1]) - np_entropy(pats, c, [0, 1]) == 0.0
    # MI(x, x) = H(x): the duplicate collapses
    pats2 = np.array([[0, 2], [1, 0], [1, 1], [2, 1]], np.uint8)
    c2 = np.array([1, 2, 3, 4], np.uint64)
    hx = np_entropy(pats2, c2, [0])
    assert np_entropy(pats2, c2, [0, 0]) == hx and hx + hx - np_entropy(pats2, c2, [0, 0]) == hx
    assert abs(hx - -(0.1 * np.log2(0.1) + 0.5 * np.log2(0.5) + 0.4 * np.log2(0.4))) < 1e-15
    # an arity-1 column: 0, and it adds nothing to a joint entropy
    pats3 = np.array([[0, 1], [0, 0]], np.uint8)
    assert np_entropy(pats3, np.array([3, 1], np.uint64), [0]) == 0.0
    assert np_entropy(pats3, np.array([3, 1], np.uint64), [0, 1]) == np_entropy(pats3, np.array([3, 1], np.uint64), [1])
    # a listed pattern with occurrence 0 contributes nothing
    assert np_entropy(pats, np.array([5, 5, 0, 0], np.uint64), [0, 1]) == 1.0


def test_cpp_evaluation_compiles_and_empty_sampler(bnlib, tmp_path):
    """transinformation.hpp compiles with g++ -std=c++14 over include/compat; an empty sampler gives 0.0
    without touching the GPU (the reference's value)."""
    exe = build_cpp(tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "evaluation empty ok" in p.stdout
