"""Case tables, fp64 / fp32 references and deliberately wrong references for the plain GEMM entry points (csrc/gemm.hip).
Shared by test_gemm_host.py (CPU: the comparator bites at every case) and test_gemm_gpu.py (the kernels against fp64).

Every case is held in LOGICAL form, whatever the entry point's memory layout:

    C[M][N] (+)= act(A[M][K] . B[N][K]^T + bias[N]) + residual[M][N]

NN stores B as [K][N] and TN stores both operands K-major; the GPU test lays the same values out accordingly."""
import collections

import torch

from util import rand

Case = collections.namedtuple("Case", "kind m n k variant kvalid batch")
Case.__str__ = lambda c: (f"{c.kind}-M{c.m}-N{c.n}-K{c.k}-{c.variant}" + (f"-kv{c.kvalid}" if c.kvalid else "")
                          + (f"-b{c.batch}" if c.batch > 1 else ""))

# NT variants: which epilogue arguments a case passes ("aslice": a is a column slice of a wider matrix, lda > K)
_HAS_BIAS = {"bias", "bias_relu", "all"}
_HAS_ACT = {"bias_relu", "all"}
_HAS_RES = {"res", "all"}
_HAS_ACC = {"acc", "all", "kvacc"}


def _nt(m, n, k, variant):
    return Case("nt", m, n, k, variant, 0, 1)


# igemm_launch: N <= 32 -> 256x32 tile, N <= 64 -> 128x64, else 128x128; < 1024 rows the fp32 pipe, from 1024 rows the wide tile takes
# the bf16 three-piece split.  M on either side of one and eight tile heights, N on either side of every tile width, K of 1, 3 and 16 steps (the sets
# test_gemm_host.test_tables_cover_the_required_values pins); each N class on both sides of 1024 rows; every variant on
# every tile.  The last case crosses 16384 rows, where the K-step changes from 32 to 16.
NT_CASES = [_nt(*c) for c in (
    (1, 4, 32, "plain"), (7, 15, 96, "bias"), (127, 32, 512, "bias_relu"), (128, 36, 32, "res"), (129, 64, 96, "acc"),
    (1023, 68, 512, "all"), (7, 128, 32, "aslice"), (127, 132, 96, "plain"), (128, 252, 512, "bias"), (129, 4, 96, "all"),
    (1023, 15, 32, "aslice"), (1, 64, 512, "all"), (7, 36, 512, "aslice"), (1023, 32, 96, "res"), (1, 252, 96, "bias_relu"),
    (129, 132, 32, "res"), (128, 128, 96, "acc"), (1023, 252, 32, "plain"),
    (1024, 4, 512, "bias"), (1030, 15, 96, "bias_relu"), (1024, 32, 32, "acc"), (1030, 36, 96, "bias"), (1024, 64, 512, "bias_relu"),
    (1030, 64, 32, "plain"), (1024, 68, 96, "plain"), (1030, 128, 512, "all"), (1024, 132, 32, "bias_relu"), (1030, 252, 96, "res"),
    (1024, 252, 512, "acc"), (1030, 132, 512, "aslice"), (1024, 36, 512, "all"), (1030, 32, 512, "all"),
    (16400, 32, 32, "bias"),
)]

# NN: the N <= 64 tile and the wide one, both sides of 1024 rows (the wide tile takes the split pipe from 1024 rows), kvalid < K,
# accumulate, b as a column slice (ldb > N).  "kvacc": kvalid, accumulate and the slice together.
NN_CASES = [Case("nn", m, n, k, v, kv, 1) for m, n, k, kv, v in (
    (7, 4, 64, 0, "plain"), (1030, 4, 32, 0, "plain"), (129, 64, 96, 70, "plain"), (1024, 64, 64, 0, "acc"), (127, 68, 32, 0, "bslice"),
    (1030, 68, 96, 0, "acc"), (1023, 256, 64, 33, "plain"), (1024, 256, 128, 0, "bslice"), (1500, 256, 512, 500, "kvacc"),
)]

# TN (tn_gemm_batched): one case per (tm, tn) of the nine tiles at K = 40 (tail of 8 behind one 32-chunk), the K list at M = N = 128
# (masked tail on either side of a chunk; the 128x128 tile takes the split pipe from K = 1024), accumulate, column slices.
TN_CASES = ([Case("tn", m, n, 40, "plain", 0, 1) for m in (4, 64, 132) for n in (4, 64, 132)]
            + [Case("tn", 128, 128, k, "plain", 0, 1) for k in (1, 31, 32, 33, 1000, 1024, 1056)]
            + [Case("tn", 64, 132, 33, "acc", 0, 1), Case("tn", 128, 128, 1056, "acc", 0, 1),
               Case("tn", 132, 64, 1000, "slices", 0, 1), Case("tn", 128, 132, 1024, "slices", 0, 1)])

# NT batched: A and B as strided selections pairs[:, 0] / pairs[:, 1] of one (batch, 2, M, K) tensor
NTB_CASES = [Case("ntb", m, m, 64, "plain", 0, b) for b in (1, 3) for m in (25, 169)]

ALL_CASES = NT_CASES + NN_CASES + TN_CASES + NTB_CASES


# inputs redrawn where torch's CPU fp32 product came out unusually coarse (6.5 units of 2**-24), which would have made that case's
# tolerance the loosest of the table
_RESEED = {"nt-M1030-N15-K96-bias_relu": 6000}


def seed_of(case):
    return 1000 + 10 * ALL_CASES.index(case) + _RESEED.get(str(case), 0)


def make_inputs(case):
    """fp32 CPU operands of a case in logical form: a (batch, M, K), b (batch, N, K), then bias (N) / residual (M, N) / c_old (M, N)
    or None.  NN with kvalid: K is the valid length (the padding up to the kernel's K is the GPU test's business)."""
    s = seed_of(case)
    k = case.kvalid or case.k
    x = {"a": rand(case.batch, case.m, k, seed=s), "b": rand(case.batch, case.n, k, seed=s + 1),
         "bias": rand(case.n, seed=s + 2) if case.variant in _HAS_BIAS else None,
         "res": rand(case.m, case.n, seed=s + 3) if case.variant in _HAS_RES else None,
         "c_old": rand(case.m, case.n, seed=s + 4) if case.variant in _HAS_ACC else None,
         "act": case.variant in _HAS_ACT}
    return x


def evaluate(x, dtype, wrong=None):
    """The case in ``dtype`` on the CPU.  ``wrong`` names one of the deliberately wrong evaluations (None if it does not apply)."""
    a, b = x["a"].clone(), x["b"]
    if wrong == "a16":          # A rounded to 16 significant bits: the lowest of the three bf16 pieces lost
        a = ((a.view(torch.int32) + 0x80) & ~0xFF).view(torch.float32)
    if wrong == "elem":         # one element of A's last row and last K column
        a[:, -1, -1] = 0
    out = torch.matmul(a.to(dtype), b.to(dtype).transpose(1, 2))
    if x["bias"] is not None:
        bias = x["bias"].to(dtype).clone()
        if wrong == "bias":
            bias[-1] = 0
        out = out + bias
    elif wrong == "bias":
        return None
    if x["act"]:
        if wrong != "act":
            out = torch.relu(out)       # ACT_LEAKY through dcn_gemm_nt: the slope is fixed at 0
    elif wrong == "act":
        return None
    if x["res"] is not None:
        out = out + x["res"].to(dtype)
    if x["c_old"] is not None:
        if wrong != "acc":
            out = out + x["c_old"].to(dtype)
    elif wrong == "acc":
        return None
    return out


def scale64(x):
    """|A| . |B|^T + |bias| + |residual| + |C_old| in fp64: what an element's rounding errors are proportional to"""
    s = torch.matmul(x["a"].double().abs(), x["b"].double().abs().transpose(1, 2))
    for k in ("bias", "res", "c_old"):
        if x[k] is not None:
            s = s + x[k].double().abs()
    return s


WRONG = ("a16", "elem", "bias", "acc", "act")
