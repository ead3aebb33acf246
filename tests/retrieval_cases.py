"""What the retrieval test modules share (test_retrieve_gpu, test_qbnorm_gpu, test_moment_gpu and the two *_cpu modules): the padded
operand view, the exact-arithmetic integer gallery, the synthetic batches of the small model, the deterministic-mode fixture and the
header's struct parser.  A plain module beside moment_ref.py and qbnorm_ref.py; importing it needs no GPU."""
import os
import re

import pytest
import torch

from univl_amd import _lib

DEV = "cuda"
H = 768
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "univl_hip.h")).read()


def padded(x, ld):
    """x as a [rows, 768] device view with row stride ld."""
    buf = torch.full((x.shape[0], ld), 77.0, dtype=torch.float32)         # the padding must never enter a score
    buf[:, :H] = x
    return buf.to(DEV)[:, :H]


def int_gallery(Nq, Ng):
    """Integer queries and gallery in [-8, 8] (every partial sum is an integer below 2^24, exact in fp32 in any order); rows j = 5, 9,
    13, ... duplicate row j % 3; targets sit on duplicated rows where there are any.  (q, g, targets, the int64 scores)."""
    gen = torch.Generator().manual_seed(1000 * Nq + Ng)
    q = torch.randint(-8, 9, (Nq, H), generator=gen).float()
    g = torch.randint(-8, 9, (Ng, H), generator=gen).float()
    for j in range(5, Ng, 4):
        g[j] = g[j % 3]
    tgt = torch.tensor([(5 + 4 * i) % Ng if Ng > 5 else i % Ng for i in range(Nq)], dtype=torch.int32)
    return q, g, tgt, (q.to(torch.int64) @ g.to(torch.int64).t()).numpy()


def batches(cfg, sizes, seed):
    import univl_oracle as O
    out = []
    for n, b in enumerate(sizes):
        bt = O.synthetic_batch(cfg, b, seed=seed + n)
        out.append({k: bt[k].to(DEV) for k in ("input_ids", "attention_mask", "token_type_ids", "video", "video_mask")})
    return out


@pytest.fixture
def deterministic_models():
    """Models built inside the test run in deterministic mode (the mode of tests/test_model_gpu.py); restored afterwards."""
    import univl_amd
    was = univl_amd.deterministic()
    univl_amd.set_deterministic(True)
    yield
    univl_amd.set_deterministic(was)


def header_fields(struct):
    """The (name, ctypes kind) list of a descriptor struct as include/univl_hip.h declares it."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    kinds = {"int32_t": _lib.i32, "int64_t": _lib.i64, "float": _lib.f32, "ptr": _lib.vp}
    want = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const\s+)?(\w+)\s*(\*?)\s*(.*)", decl)
        for nm in m.group(4).split(","):
            want.append((nm.strip(), kinds["ptr" if m.group(3) else m.group(2)]))
    return want
