"""Host side of the retrieval search (no GPU): the univl_sim_topk entry points are declared, exported and bound, the descriptor
mirrors the C struct, the workspace formula of the header is the one the library evaluates, and rank positions taken from counts
are the reference's `ind`."""
import ctypes as C
import os
import re

import numpy as np

from univl_amd import _lib, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sim_topk_is_declared_exported_and_bound():
    """The pattern of tests/test_caption_eval_cpu.py::test_beam_captions_is_declared_exported_and_bound."""
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
    declared = set(re.findall(r"\b(univl_[a-z0-9_]+)\s*\(", header))
    for name in ("univl_sim_topk", "univl_sim_topk_workspace"):
        assert name in declared and name in _lib.EXPORTED and hasattr(L, name)
    assert declared == set(_lib.EXPORTED)
    m = re.search(r"int\s+univl_sim_topk\s*\(([^;]*)\)\s*;", header)
    assert m, "declaration not found"
    params = [p.strip() for p in m.group(1).split(",")]
    fn = L.univl_sim_topk
    assert fn.restype is C.c_int32 and len(fn.argtypes) == len(params) == 2
    for p, t in zip(params, fn.argtypes):
        assert (t is C.c_void_p) == ("*" in p or "hipStream_t" in p), (p, t)
    m = re.search(r"int64_t\s+univl_sim_topk_workspace\s*\(([^;]*)\)\s*;", header)
    params = [p.strip() for p in m.group(1).split(",")]
    fn = L.univl_sim_topk_workspace
    assert fn.restype is C.c_int64 and len(fn.argtypes) == len(params) == 4
    assert all(t is C.c_int32 and p.startswith("int32_t ") for p, t in zip(params, fn.argtypes))


def test_sim_topk_struct_mirrors_the_header():
    L = _lib.lib()
    assert _lib._STRUCTS[9] is _lib.SimTopk and L.univl_struct_size(9) == C.sizeof(_lib.SimTopk)
    header = open(os.path.join(ROOT, "include", "univl_hip.h")).read()
    body = re.search(r"typedef struct UnivlSimTopk \{(.*?)\} UnivlSimTopk;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [f.strip().lstrip("*").strip() for f in decl.split(" ", 2 if decl.startswith("const") else 1)[-1].split(",")]
    assert fields == [f for f, _ in _lib.SimTopk._fields_]
    assert int(re.search(r"#define UNIVL_TOPK_MAX (\d+)", header).group(1)) == _lib.TOPK_MAX == 64
    assert int(re.search(r"#define UNIVL_TOPK_SLICES_MAX (\d+)", header).group(1)) == _lib.TOPK_SLICES_MAX


def test_workspace_formula_of_the_header():
    """Nq * S * (8 k + 8) with S as the header derives it; forced slice counts are capped at the tile count; bad arguments < 0."""
    L = _lib.lib()

    def want(Nq, Ng, k, slices):
        T = -(-Ng // 128)
        QT = -(-Nq // (16 if Nq <= 16 else 32))
        w = slices if slices else -(-256 // QT)
        w = min(w, _lib.TOPK_SLICES_MAX, T)
        S = -(-T // -(-T // w))
        return Nq * S * (8 * k + 8)
    for Nq in (1, 16, 17, 33, 1024, 100000):
        for Ng in (1, 128, 129, 4099, 10 ** 6):
            for k in (0, 1, 10, 64):
                for slices in (0, 1, 7, 256):
                    assert L.univl_sim_topk_workspace(Nq, Ng, k, slices) == want(Nq, Ng, k, slices), (Nq, Ng, k, slices)
    for bad in ((0, 5, 1, 0), (5, 0, 1, 0), (5, 5, -1, 0), (5, 5, 65, 0), (5, 5, 1, 257), (5, 5, 1, -1)):
        assert L.univl_sim_topk_workspace(*bad) < 0, bad
        assert b"univl_sim_topk_workspace" in L.univl_last_error()


def test_rank_positions_from_counts_is_the_reference_ind():
    """A hand-made matrix with ties on and off the diagonal: the counts per row, fed to rank_positions as a (gt, eq) tuple, give the
    `ind` the reference's row sort gives (metrics.py:9-14), and compute_metrics on the tuple the reference's numbers."""
    x = np.array([[3., 3., 1., 0., 3.],
                  [5., 2., 2., 2., 1.],
                  [0., 1., 9., 1., 1.],
                  [4., 4., 4., 4., 4.],
                  [7., 6., 5., 4., 3.]], dtype=np.float32)
    d = np.diag(x)
    gt = (x > d[:, None]).sum(1).astype(np.int32)
    eq = (x == d[:, None]).sum(1).astype(np.int32)
    assert eq.tolist() == [3, 3, 1, 5, 1]
    sx = np.sort(-x, axis=1)                                   # the reference's arithmetic
    ind = np.where((sx - (-d)[:, None]) == 0)[1]
    got = metrics.rank_positions((gt, eq))
    assert got.dtype == np.int64 and np.array_equal(got, ind)
    assert np.array_equal(metrics.positions_from_counts(gt, eq), ind)
    m = metrics.compute_metrics((gt, eq))
    assert m == {"R1": float(np.sum(ind == 0)) / len(ind), "R5": float(np.sum(ind < 5)) / len(ind),
                 "R10": float(np.sum(ind < 10)) / len(ind), "MR": np.median(ind) + 1}
    # no ties: the counts themselves
    assert np.array_equal(metrics.rank_positions((np.array([2, 0, 1]), np.array([1, 1, 1]))), np.array([2, 0, 1]))
