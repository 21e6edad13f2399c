"""BiCGStab (KSPBCGS) restated in numpy -- the reference of test_cpu_bcgs.py
and test_gpu_bcgs.py (a helper, not a test).

van der Vorst's method in PETSc's arrangement, left preconditioning (B: the
identity or Jacobi's 1/diag, zero diagonal entries use 1), preconditioned
norm, KSPConvergedDefault.  The MatMult is OracleMat.mult (the bit-exact
MatMult_SeqAIJ restatement); the dot product is a parameter so the CPU tests
can show that the cases' iteration counts do not hang on the summation order.
"""
import math

import numpy as np

RTOL, ATOL, ITS, BREAKDOWN, DIV_ITS, DTOL, NANORINF = 2, 3, 4, -5, -3, -4, -9


def dot_np(a, b):
    return float(np.dot(a, b))


def dot_fsum(a, b):
    return math.fsum((a * b).tolist())


def dot_reversed(a, b):
    s = 0.0
    for t in (a * b)[::-1].tolist():
        s += t
    return s


DOTS = {"np.dot": dot_np, "fsum": dot_fsum, "reversed": dot_reversed}


def bcgs_ref(O, b, pc="jacobi", x0=None, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000, norm="default",
             dot=dot_np):
    """Returns dict(its, reason, x, history, ttol)."""
    if norm not in ("default", "preconditioned", "none"):
        raise ValueError("BiCGStab with left preconditioning supports the preconditioned norm only")
    b = np.asarray(b, np.float64)
    n = b.size
    if pc == "jacobi":
        d = O.diagonal()
        B = np.where(d == 0.0, 1.0, 1.0 / np.where(d == 0.0, 1.0, d))
    else:
        B = None
    papply = (lambda r: r * B) if B is not None else (lambda r: r.copy())
    st = {"rnorm0": 0.0, "ttol": 0.0}

    def converged(k, rnorm, guess_zero=True, snorm=0.0):
        if norm == "none":
            return ITS if k >= max_it else 0
        if k == 0:
            if not guess_zero:
                st["rnorm0"] = rnorm if snorm == 0.0 else snorm
            else:
                st["rnorm0"] = rnorm
            st["ttol"] = max(rtol * st["rnorm0"], atol)
        if math.isnan(rnorm) or math.isinf(rnorm):
            return NANORINF
        if rnorm <= st["ttol"]:
            return ATOL if rnorm < atol else RTOL
        if rnorm >= dtol * st["rnorm0"]:
            return DTOL
        return 0

    def out(its, reason, x, hist):
        return dict(its=its, reason=reason, x=x, history=np.array(hist), ttol=st["ttol"])

    with np.errstate(all="ignore"):
        if x0 is None:
            x = np.zeros(n)
            R = papply(b)
            snorm = 0.0
        else:
            x = np.array(x0, np.float64)
            R = papply(b - O.mult(x))
            Bb = papply(b)
            snorm = math.sqrt(dot(Bb, Bb))
        dp = math.sqrt(dot(R, R))
        its = 0
        hist = [dp]
        reason = converged(0, dp, x0 is None, snorm)
        if reason:
            return out(its, reason, x, hist)
        RP = R.copy()
        rhoold = alphaold = omegaold = 1.0
        P = np.zeros(n)
        V = np.zeros(n)
        for _ in range(max_it):
            rho = dot(RP, R)
            if rho == 0.0:
                return out(its, BREAKDOWN, x, hist)
            beta = (rho / rhoold) * (alphaold / omegaold)
            P = R + beta * (P - omegaold * V)
            V = papply(O.mult(P))
            d1 = dot(V, RP)
            if d1 == 0.0:
                return out(its, BREAKDOWN, x, hist)
            alpha = rho / d1
            S = R - alpha * V
            T = papply(O.mult(S))
            d1 = dot(S, T)
            d2 = dot(T, T)
            if d2 == 0.0:
                x = x + alpha * P
                its += 1
                hist.append(0.0)
                return out(its, RTOL if dot(S, S) == 0.0 else BREAKDOWN, x, hist)
            omega = d1 / d2
            x = x + (alpha * P + omega * S)
            R = S - omega * T
            dp = math.sqrt(dot(R, R))
            rhoold, alphaold, omegaold = rho, alpha, omega
            its += 1
            hist.append(dp)
            reason = converged(its, dp)
            if reason:
                return out(its, reason, x, hist)
        return out(its, ITS if norm == "none" else DIV_ITS, x, hist)


# ------------------------------------------------------------------ the tests' systems
def random_csr(N, k, seed):
    """Rows of k random columns (the diagonal included, no repeats, ascending),
    negative off-diagonal values, a dominant diagonal: the nonsymmetric family
    of test_gpu_cb.py's _random_csr."""
    rng = np.random.default_rng(seed)
    ip = [0]
    cols, vals = [], []
    for r in range(N):
        c = sorted(set(rng.integers(0, N, size=k - 1).tolist()) | {r})
        v = -rng.random(len(c))
        for j, cc in enumerate(c):
            if cc == r:
                v[j] = 1.0 + np.abs(v).sum()
        cols += c
        vals += v.tolist()
        ip.append(len(cols))
    return np.array(ip, np.int64), np.array(cols, np.int32), np.array(vals)


# name -> (builder of (indptr, cols, vals), right-hand side: a seed of
# default_rng(seed).random(M), or None for the library's hash).  BiCGStab on
# the convection-diffusion stencil is sensitive to the order of its sums (rho
# = RP . R cancels more every iteration): run to rtol 1e-5 with np.dot, fsum
# and a reversed sum, 16^3 (31 its) gives histories that differ by 8e-6 and x
# by 2e-11, 24 x 20 x 12 (35 / 36 its) by 2e-4 and 6e-10, whatever the
# right-hand side -- no summation order can then match another to the GPU
# tests' 1e-8 / 1e-10.  So those two shapes are compared over their first 12
# iterations (TRUNCATED; orders agree to 1e-12 there), and the solves run to
# convergence use the shapes and seeds that meet test_cpu_bcgs.py's conditions.
SYSTEMS = {
    "convdiff8": (lambda oracle: oracle.stencil("convdiff3d", 8), 4),
    "convdiff10": (lambda oracle: oracle.stencil("convdiff3d", 10), 1),
    "convdiff13x10x9": (lambda oracle: oracle.stencil("convdiff3d", 13, 10, 9), 3),
    "random4099": (lambda oracle: random_csr(4099, 7, 11), 4),
    "convdiff16": (lambda oracle: oracle.stencil("convdiff3d", 16), None),
    "convdiff24x20x12": (lambda oracle: oracle.stencil("convdiff3d", 24, 20, 12), None),
}
CONVERGED = ("convdiff8", "convdiff10", "convdiff13x10x9", "random4099")
TRUNCATED = ("convdiff16", "convdiff24x20x12")
TRUNCATED_ITS = 12
_CACHE = {}


def system(oracle, name):
    """(indptr, cols, vals, b, OracleMat) of a named system, built once."""
    if name not in _CACHE:
        build, seed = SYSTEMS[name]
        ip, c, v = build(oracle)
        M = ip.size - 1
        b = oracle.rhs_hash(0, M) if seed is None else np.random.default_rng(seed).random(M)
        _CACHE[name] = (ip, c, v, b, oracle.OracleMat.from_csr(M, M, ip, c, v))
    return _CACHE[name]


def x_true(n):
    """The solution of the nonzero-guess cases (b = A x_true)."""
    return np.random.default_rng(1).standard_normal(n)


_REF = {}


def reference(oracle, name, pc, **kw):
    """bcgs_ref with np.dot on a named system, computed once per argument set
    (callers must not modify the result)."""
    key = (name, pc, tuple(sorted(kw.items())))
    if key not in _REF:
        O, b = system(oracle, name)[4], system(oracle, name)[3]
        _REF[key] = bcgs_ref(O, b, pc=pc, **kw)
    return _REF[key]
